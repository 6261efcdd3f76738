// performFFT / detectTransient: the exports of the reference's codec/analysis/transient.js (:17-55), same signatures and return
// types, computed on the device in the reference's arithmetic (c1_perform_fft, c1_detect_transients).  The encoder detects
// transients inside its own kernels at the codec's band sizes and never comes through here; these exist for code that imports
// the module, e.g. a block selector with per-band thresholds.  Inputs are typed arrays or plain Arrays, read as doubles.
// Deviations (INTEGRATION.md section 2): an fftSize that is not a power of two 1 .. 2^22 is a RangeError, and performFFT also
// takes a plain Array (the reference calls samples.subarray).
import { native, context } from '../native.js'

const doubles = (x) => (x instanceof Float64Array ? x : Float64Array.from(x))

// (cos, sin)(-2 pi / stride) for stride = 2 .. n from THIS engine's Math.cos / Math.sin, as FFT.fft computes them (fft.js:37-39)
function twiddles(n) {
  const w = []
  for (let stride = 2; stride <= n; stride <<= 1) {
    const angle = (-2 * Math.PI) / stride
    w.push(Math.cos(angle), Math.sin(angle))
  }
  return Float64Array.from(w)
}

export function performFFT(samples, fftSize) {
  if (!Number.isInteger(fftSize) || fftSize < 1 || fftSize > 1 << 22 || (fftSize & (fftSize - 1)) !== 0) {
    throw new RangeError(`performFFT: fftSize ${fftSize} is not a power of two 1 .. 2^22`)
  }
  const copyLen = Math.min(samples.length, fftSize)
  const head = typeof samples.subarray === 'function' ? samples.subarray(0, copyLen) : Array.prototype.slice.call(samples, 0, copyLen)
  return native().performFFT(context(), doubles(head), fftSize, twiddles(fftSize))
}

// the transient score of transient.js:189-226 (NaN when prevCoeffs is falsy): what detectTransient compares with its threshold
export function transientScore(currentCoeffs, prevCoeffs) {
  if (!prevCoeffs) return NaN
  return native().detectTransient(context(), doubles(currentCoeffs), doubles(prevCoeffs), 0)[1]
}

export function detectTransient(currentCoeffs, prevCoeffs, threshold) {
  if (!prevCoeffs) return false // :46
  return native().detectTransient(context(), doubles(currentCoeffs), doubles(prevCoeffs), Number(threshold))[0]
}
