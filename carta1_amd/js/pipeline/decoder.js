// decode(bufferPool) -> frame closure (codec/pipeline/decoder.js:408-411): dequantization, IMDCT with
// overlap-add and QMF synthesis run as one HIP kernel; decoder state lives in the pool's native stream.
import { BufferPool } from '../core/buffers.js'
import { SPECS_PER_BFU } from '../core/constants.js'
import { native, context, checkPrecision, decodeContext } from '../native.js'
import { throwError } from '../utils.js'

// A sound unit (Uint8Array) is decoded from its bytes; a frameData object from its fields as they stand, without
// serializeFrame, so that fields no unit can carry (an nBfu outside BFU_AMOUNTS, a band mode of 1, mantissas beyond their word
// length) decode as the reference decodes them.  Both kinds continue the same native stream.
// options: { precision: 'exact' (default) | 'binary32' } (native.js).  The pool's native stream lives on the context of the
// precision it was created with; a closure of the other precision on the same pool moves it -- the pool's state is read from
// the stream and a new stream on the other context continues from it -- so the audio goes on without a seam.
export function decode(bufferPool = new BufferPool(), options = {}) {
  const precision = checkPrecision(options)
  if (!bufferPool) throwError('imdctStage: bufferPool is required')
  return (frameData) => {
    const addon = native()
    if (bufferPool.decoderStream && bufferPool.decoderPrecision !== precision) {
      bufferPool.pendingDecoderState = addon.decStreamGetState(bufferPool.decoderStream, 1)
      bufferPool.decoderStream = null
    }
    if (!bufferPool.decoderStream) {
      bufferPool.decoderStream = addon.decStreamCreate(decodeContext(precision), 1)
      bufferPool.decoderPrecision = precision
      if (bufferPool.pendingDecoderState) { // a state set before the stream existed (BufferPool.setDecoderState)
        addon.decStreamSetState(bufferPool.decoderStream, 1, bufferPool.pendingDecoderState)
        bufferPool.pendingDecoderState = null
      }
    }
    if (frameData instanceof Uint8Array) return addon.decStreamPush(bufferPool.decoderStream, frameData, 1)[0]
    const f = frameFields(frameData)
    return addon.decStreamPushFields(bufferPool.decoderStream, f.nbfu, f.modes, f.sfi, f.wl, f.q, 1)[0]
  }
}

// dequantizationStage(), imdctStage(context) and qmfSynthesisStage(context): the three stages decode() composes, exported on
// their own as the reference does (codec/pipeline/decoder.js:52, :116, :349), with its call and return shapes.  The frame
// fields go to the device as they are, without serializeFrame: any nBfu 0..52, any int32 mantissa, any band mode.  The
// stateful stages keep the previous frame's input in the pool and the device rebuilds imdctOverlap / qmfDelays from it
// (include/carta1_hip.h states those histories): bit-identical to carrying the reference's buffers along.
const isLong = (mode) => (mode === 0 ? 0 : 1)            // a band is long only when its mode is exactly 0 (decoder.js:82)

// frameData -> the native frame fields (Int32Array nbfu[1], modes[3], sfi[52], wl[52], q[512]): what the reference's
// dequantizationStage reads of it (decoder.js:63-95) and nothing else -- BFUs at or above nBfu and the mantissas of BFUs with
// word length 0 stay zero.  Indices the device cannot name are left for the native call to reject.
function frameFields(frameData) {
  const { nBfu, scaleFactorIndices, wordLengthIndices, quantizedCoefficients, blockModes } = frameData
  const sfi = new Int32Array(52), wl = new Int32Array(52), q = new Int32Array(512)
  for (let b = 0, at = 0; b < 52; at += SPECS_PER_BFU[b], b++) {
    if (!(b < nBfu)) continue
    sfi[b] = scaleFactorIndices[b]
    wl[b] = wordLengthIndices[b]
    if (wl[b] === 0) continue
    const src = quantizedCoefficients[b], n = Math.min(src.length, SPECS_PER_BFU[b])
    for (let i = 0; i < n; i++) q[at + i] = src[i]               // ToInt32 on the store, as Int32Array.from converts
  }
  return { nbfu: Int32Array.of(nBfu), modes: Int32Array.from(blockModes, isLong), sfi, wl, q }
}

export function dequantizationStage() {
  return (frameData) => {
    const f = frameFields(frameData)
    const coefficients = native().dequantizeFrames(context(), f.nbfu, f.modes, f.sfi, f.wl, f.q)
    return { coefficients, blockModes: frameData.blockModes }
  }
}

export function imdctStage(stageContext) {
  const bufferPool = (stageContext && stageContext.bufferPool) || throwError('imdctStage: bufferPool is required')
  return (input) => {
    const { coefficients, blockModes } = input
    const prev = bufferPool.imdctPrevious
    const coefs = new Float32Array((prev ? 2 : 1) * 512), modes = new Int32Array((prev ? 2 : 1) * 3)
    if (prev) { coefs.set(prev.coefficients, 0); modes.set(prev.modes, 0) }
    const cur = Float32Array.from(coefficients), curModes = Int32Array.from(blockModes, isLong)
    coefs.set(cur, prev ? 512 : 0)
    modes.set(curModes, prev ? 3 : 0)
    const bands = native().imdct(context(), coefs, prev ? 1 : 0, modes)
    bufferPool.imdctPrevious = { coefficients: cur, modes: curModes }
    return [bands.slice(0, 128), bands.slice(128, 256), bands.slice(256, 512)]
  }
}

export function qmfSynthesisStage(stageContext) {
  const bufferPool = (stageContext && stageContext.bufferPool) || throwError('qmfSynthesisStage: bufferPool is required')
  return (bands) => {
    if (bands[0].length !== 128 || bands[1].length !== 128 || bands[2].length !== 256) {
      throwError('qmfSynthesisStage: expected bands of 128, 128 and 256 samples')
    }
    const prev = bufferPool.synthesisPreviousBands
    const all = new Float32Array((prev ? 2 : 1) * 512)
    const at = prev ? 512 : 0
    if (prev) all.set(prev, 0)
    all.set(bands[0], at); all.set(bands[1], at + 128); all.set(bands[2], at + 256)
    bufferPool.synthesisPreviousBands = all.slice(at, at + 512)
    return native().qmfSynthesis(context(), all, prev ? 1 : 0)
  }
}
