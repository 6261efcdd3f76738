// decode(bufferPool) -> frame closure (codec/pipeline/decoder.js:408-411): dequantization, IMDCT with
// overlap-add and QMF synthesis run as one HIP kernel; decoder state lives in the pool's native stream.
import { BufferPool } from '../core/buffers.js'
import { SOUND_UNIT_SIZE, SPECS_PER_BFU } from '../core/constants.js'
import { serializeFrame } from '../io/serialization.js'
import { native, context } from '../native.js'
import { throwError } from '../utils.js'

export function decode(bufferPool = new BufferPool()) {
  if (!bufferPool) throwError('imdctStage: bufferPool is required')
  return (frameData) => {
    const addon = native()
    if (!bufferPool.decoderStream) bufferPool.decoderStream = addon.decStreamCreate(context(), 1)
    let unit
    if (frameData instanceof Uint8Array) unit = frameData
    else if (!frameData.nBfu) {
      // the reference's padding frame (processor.js:300-308): no BFUs -> all-zero spectrum
      unit = new Uint8Array(SOUND_UNIT_SIZE)
      unit[0] = 0xac
    } else unit = serializeFrame(frameData)
    return addon.decStreamPush(bufferPool.decoderStream, unit, 1)[0]
  }
}

// dequantizationStage(), imdctStage(context) and qmfSynthesisStage(context): the three stages decode() composes, exported on
// their own as the reference does (codec/pipeline/decoder.js:52, :116, :349), with its call and return shapes.  The frame
// fields go to the device as they are, without serializeFrame: any nBfu 0..52, any int32 mantissa, any band mode.  The
// stateful stages keep the previous frame's input in the pool and the device rebuilds imdctOverlap / qmfDelays from it
// (include/carta1_hip.h states those histories): bit-identical to carrying the reference's buffers along.
const isLong = (mode) => (mode === 0 ? 0 : 1)            // a band is long only when its mode is exactly 0 (decoder.js:82)

export function dequantizationStage() {
  return (frameData) => {
    const { nBfu, scaleFactorIndices, wordLengthIndices, quantizedCoefficients, blockModes } = frameData
    const sfi = new Int32Array(52), wl = new Int32Array(52), q = new Int32Array(512)
    for (let b = 0, at = 0; b < 52; at += SPECS_PER_BFU[b], b++) {
      if (b >= nBfu) continue
      sfi[b] = scaleFactorIndices[b]
      wl[b] = wordLengthIndices[b]
      if (wl[b] !== 0) q.set(Int32Array.from(quantizedCoefficients[b].slice(0, SPECS_PER_BFU[b])), at)
    }
    const modes = Int32Array.from(blockModes, isLong)
    const coefficients = native().dequantizeFrames(context(), Int32Array.of(nBfu), modes, sfi, wl, q)
    return { coefficients, blockModes }
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
