// quantize / dequantize: the reference's single-BFU functions (codec/coding/quantization.js:34-78), same signatures, computed
// on the device in the reference's arithmetic (c1_quantize / c1_dequantize).  The encoder itself quantizes inside its packing
// kernel and never comes through here; these exist for code that imports the names.
import { native, context } from '../native.js'

// Every int32 bitsPerSample has the reference's meaning on the device (c1_quantize); scaleFactorIndex outside 0..63 is refused
// there.  Non-integers are refused here: `| 0` would change what the reference computes with them.
function checkArgs(name, scaleFactorIndex, bitsPerSample) {
  if (!Number.isInteger(scaleFactorIndex) || scaleFactorIndex < 0 || scaleFactorIndex > 63) {
    throw new RangeError(`${name}: scaleFactorIndex ${scaleFactorIndex} outside SCALE_FACTORS (0..63)`)
  }
  if (!Number.isInteger(bitsPerSample) || (bitsPerSample | 0) !== bitsPerSample) {
    throw new RangeError(`${name}: bitsPerSample ${bitsPerSample} is not an int32`)
  }
}

export function quantize(coefficients, scaleFactorIndex, bitsPerSample) {
  checkArgs('quantize', scaleFactorIndex, bitsPerSample)
  const x = coefficients instanceof Float32Array ? coefficients : Float32Array.from(coefficients)
  return native().quantize(context(), x, scaleFactorIndex, bitsPerSample)
}

export function dequantize(quantized, scaleFactorIndex, bitsPerSample) {
  checkArgs('dequantize', scaleFactorIndex, bitsPerSample)
  const q = quantized instanceof Int32Array ? quantized : Int32Array.from(quantized)
  return native().dequantize(context(), q, scaleFactorIndex, bitsPerSample)
}
