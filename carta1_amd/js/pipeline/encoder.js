// encode(options, bufferPool) -> frame closure, the reference's public encoder entry point
// (codec/pipeline/encoder.js:438-450).  The four stages the reference composes there -- QMF analysis,
// block selection, MDCT, RDO quantization -- run as HIP kernels; the per-stream state the reference
// keeps in the BufferPool lives in a native stream handle owned by the pool.  The closure returns the
// same fields object: { nBfu, scaleFactorIndices, wordLengthIndices, quantizedCoefficients, blockModes }.
import { EncoderOptions } from '../core/options.js'
import { BufferPool } from '../core/buffers.js'
import { SAMPLES_PER_FRAME, SCALE_FACTORS, SPECS_PER_BFU } from '../core/constants.js'
import { deserializeFrame } from '../io/serialization.js'
import { native, context, checkScaleFactorOffsets, checkMasking, modeCandidateBytes } from '../native.js'
import { throwError } from '../utils.js'

// measured (not in the reference; optional, read per call as `options` is): { measuredAllocation: true, scaleFactorOffsets,
// masking } allocates the frame's word lengths -- with scaleFactorOffsets its scale-factor indices too, with masking under a
// masking threshold -- by the measured coding error, as encodeAeaPcm's options of the same names do (include/carta1_hip.h,
// c1_enc_stream_push_measured).  measuredModeCandidates (with measuredAllocation: true only; scaleFactorOffsets combines with it,
// masking does not: encodeAeaPcm's TypeErrors) chooses the frame's block modes among 1 to 8 mode bytes or triples by the measured
// allocation's final error under each (c1_enc_stream_push_measured_modes); the fields' blockModes are then the unit's, whatever
// options.fixedBlockModes says.  Neither keeps any state, so frames with and without them may alternate on one pool.  Without the
// object, or with measuredAllocation falsy, the closure is the reference's, byte for byte; scaleFactorOffsets, masking or
// measuredModeCandidates without measuredAllocation: true is encodeAeaPcm's TypeError.  modeSearchMasking (true | { floor, spread };
// with measuredAllocation: true and measuredModeCandidates only, else encodeAeaPcm's TypeError naming what is missing) weighs that
// search with one masking threshold per unit, from the all-long spectrum (c1_enc_stream_push_measured_modes_masked).
function measuredArguments(measured) {
  if (measured === undefined || measured === null) return null
  const { measuredAllocation, measuredModeCandidates, modeSearchMasking, scaleFactorOffsets, masking } = measured
  if (measuredAllocation !== undefined && measuredAllocation !== null && typeof measuredAllocation !== 'boolean') {
    throw new TypeError(`measuredAllocation must be a boolean, got ${measuredAllocation}`)
  }
  const haveMasking = masking !== undefined && masking !== null && masking !== false
  const haveCandidates = measuredModeCandidates !== undefined && measuredModeCandidates !== null
  let candidates = null
  if (haveCandidates) {
    if (!measuredAllocation) throw new TypeError('measuredModeCandidates needs measuredAllocation: true; blockModeCandidates is the search under the reference\'s allocation')
    if (haveMasking) throw new TypeError('measuredModeCandidates and masking are mutually exclusive: thresholds of different block modes are not comparable')
    const n = measuredModeCandidates.length
    if (!(Array.isArray(measuredModeCandidates) || measuredModeCandidates instanceof Uint8Array) || n < 1 || n > 8) {
      throw new RangeError(`measuredModeCandidates must hold 1 to 8 mode bytes, got ${n}`)
    }
    candidates = modeCandidateBytes(measuredModeCandidates)
  }
  const haveSearchMasking = modeSearchMasking !== undefined && modeSearchMasking !== null && modeSearchMasking !== false
  if (haveSearchMasking) {
    if (!measuredAllocation) throw new TypeError('modeSearchMasking needs measuredAllocation: true and measuredModeCandidates: it weighs the measured block-mode search')
    if (!haveCandidates) throw new TypeError('modeSearchMasking needs measuredModeCandidates: it weighs the measured block-mode search; masking weighs the allocation under given modes')
  }
  const haveOffsets = scaleFactorOffsets !== undefined && scaleFactorOffsets !== null
  if (haveOffsets && !measuredAllocation) throw new TypeError('scaleFactorOffsets needs measuredAllocation: true; no other path chooses scale factors')
  if (haveMasking && !measuredAllocation) throw new TypeError('masking needs measuredAllocation: true; no other path weighs its errors')
  if (!measuredAllocation) return null
  return { candidates, offsets: haveOffsets ? checkScaleFactorOffsets(scaleFactorOffsets) : null, tables: haveMasking ? checkMasking(masking) : { floor: null, spread: null }, searchTables: haveSearchMasking ? checkMasking(modeSearchMasking) : null }
}

export function encode(options = new EncoderOptions(), bufferPool = new BufferPool(), measured = undefined) {
  if (!bufferPool) throwError('qmfAnalysisStage: bufferPool is required')
  if (!options) throwError('blockSelectorStage: options is required')
  return (pcmSamples) => {
    if (!(pcmSamples instanceof Float32Array) || pcmSamples.length !== SAMPLES_PER_FRAME) {
      throwError(`encode: expected a Float32Array of ${SAMPLES_PER_FRAME} samples`)
    }
    const how = measuredArguments(measured)   // before anything changes: a TypeError leaves the pool as it was
    const addon = native()
    // options are read per call, as the reference's stages do (encoder.js:131,381); a change goes on with the same stream
    // from the next frame, detection history included (include/carta1_hip.h, c1_enc_stream_set_options)
    const packed = options.toNative()
    const key = packed.join(',')
    if (!bufferPool.encoderStream) {
      bufferPool.encoderStream = addon.encStreamCreate(context(), 1, packed)
      bufferPool.encoderOptionsKey = key
      if (bufferPool.pendingEncoderState) { // a state set before the stream existed (BufferPool.setEncoderState)
        addon.encStreamSetState(bufferPool.encoderStream, 1, bufferPool.pendingEncoderState)
        bufferPool.pendingEncoderState = null
      }
    } else if (bufferPool.encoderOptionsKey !== key) {
      addon.encStreamSetOptions(bufferPool.encoderStream, packed)
      bufferPool.encoderOptionsKey = key
    }
    const searched = how !== null && how.candidates !== null
    const unit = searched && how.searchTables
      ? addon.encStreamPushMeasuredModesMasked(bufferPool.encoderStream, [pcmSamples], how.candidates, how.offsets, how.searchTables.floor, how.searchTables.spread)
      : searched
        ? addon.encStreamPushMeasuredModes(bufferPool.encoderStream, [pcmSamples], how.candidates, how.offsets)
        : how
          ? addon.encStreamPushMeasured(bufferPool.encoderStream, [pcmSamples], how.offsets, how.tables.floor, how.tables.spread)
          : addon.encStreamPush(bufferPool.encoderStream, [pcmSamples])
    const fields = deserializeFrame(unit)
    // same array, as encoder.js:131-132; modes the candidates chose are the unit's own
    if (options.fixedBlockModes && !searched) fields.blockModes = options.fixedBlockModes
    return fields
  }
}

// qmfAnalysisStage(context) and mdctStage(context): the two pipeline stages the reference also exports on their own
// (codec/pipeline/encoder.js:57-96, :170-349; codec/index.js:30-31), with the reference's call shapes.  Their state -- the QMF
// delay lines, the MDCT overlap -- is a bounded function of the previous frame (SURVEY.md 5.1), so the pool keeps that frame's
// input and the device rebuilds the state from it: bit-identical to carrying the reference's buffers along.
export function qmfAnalysisStage(stageContext) {
  const bufferPool = (stageContext && stageContext.bufferPool) || throwError('qmfAnalysisStage: bufferPool is required')
  return (pcmSamples) => {
    if (!(pcmSamples instanceof Float32Array) || pcmSamples.length !== SAMPLES_PER_FRAME) {
      throwError(`qmfAnalysisStage: expected a Float32Array of ${SAMPLES_PER_FRAME} samples`)
    }
    const prev = bufferPool.qmfHistory
    const pcm = new Float32Array((prev ? 2 : 1) * SAMPLES_PER_FRAME)
    if (prev) pcm.set(prev, 0)
    pcm.set(pcmSamples, prev ? SAMPLES_PER_FRAME : 0)
    const bands = native().qmfAnalysis(context(), pcm, prev ? 1 : 0)
    bufferPool.qmfHistory = pcmSamples.slice()
    return { bands: [bands.slice(0, 128), bands.slice(128, 256), bands.slice(256, 512)] }
  }
}

export function mdctStage(stageContext) {
  const bufferPool = (stageContext && stageContext.bufferPool) || throwError('mdctStage: bufferPool is required')
  return (input) => {
    const { bands, blockModes, originalFrame } = input
    const prev = bufferPool.mdctPreviousBands
    const all = new Float32Array((prev ? 2 : 1) * 512)
    const at = prev ? 512 : 0
    if (prev) all.set(prev, 0)
    all.set(bands[0], at); all.set(bands[1], at + 128); all.set(bands[2], at + 256)
    bufferPool.mdctPreviousBands = all.slice(at, at + 512)   // the samples as they came in: the next frame's overlap is made of them
    const [coefficients, windowed] = native().mdctFromBands(context(), all, prev ? 1 : 0, Int32Array.from(blockModes))
    // the reference windows the band arrays it was given in place and hands the same arrays on (encoder.js:244,292,314)
    bands[0].set(windowed.subarray(0, 128)); bands[1].set(windowed.subarray(128, 256)); bands[2].set(windowed.subarray(256, 512))
    return { bands, coefficients, blockModes, originalFrame }
  }
}

// blockSelectorStage(context) and quantizationStage(context): the other two stages encode() composes (codec/pipeline/encoder.js:111,
// :365), with the reference's call and return shapes, so that pipe(context, qmfAnalysisStage, blockSelectorStage, mdctStage,
// quantizationStage) is encode() again.  The detection history the reference keeps -- transientDetection, performFFT's
// magnitudes of the last frame detection ran on -- is a function of that frame's bands: the pool keeps a copy of them and the
// device rebuilds the magnitudes (include/carta1_hip.h, c1_select_block_modes).
export function blockSelectorStage(stageContext) {
  const bufferPool = (stageContext && stageContext.bufferPool) || throwError('blockSelectorStage: bufferPool is required')
  const options = (stageContext && stageContext.options) || throwError('blockSelectorStage: options is required')
  return (input) => {
    const { bands } = input
    if (options.fixedBlockModes) return { bands, blockModes: options.fixedBlockModes }   // the history stays as it is (:130-132)
    const prev = bufferPool.transientBands
    const all = new Float32Array((prev ? 2 : 1) * 512)
    const at = prev ? 512 : 0
    if (prev) all.set(prev, 0)
    all.set(bands[0], at); all.set(bands[1], at + 128); all.set(bands[2], at + 256)
    const modes = native().selectBlockModes(context(), all, prev ? 1 : 0, options.transientThresholdLow)
    // a copy: mdctStage windows the band arrays in place right after this stage
    bufferPool.transientBands = all.slice(at, at + 512)
    return { bands, blockModes: Array.from(modes) }
  }
}

// allocationBias's table (bitallocation.js:46-61) in the packed options the addon reads; threshold and modes are not read
function quantizationOptions(options) {
  if (typeof options.toNative === 'function') return options.toNative()
  const out = new Float64Array(68)
  const bias = options.allocationBias === undefined ? 1 : options.allocationBias
  for (let i = 0; i < 64; i++) out[i] = bias === 1 ? SCALE_FACTORS[i] : Math.pow(SCALE_FACTORS[i], bias)
  out[64] = 1
  out[65] = out[66] = out[67] = -1
  return out
}

export function quantizationStage(stageContext) {
  const options = (stageContext && stageContext.options) || throwError('quantizationStage: options is required')
  return (input) => {
    const { coefficients, blockModes } = input
    const coefs = coefficients instanceof Float32Array ? coefficients : Float32Array.from(coefficients)
    const f = native().quantizeFrames(context(), coefs, Int32Array.from(blockModes), quantizationOptions(options))
    const nBfu = f.nbfu[0]
    const quantizedCoefficients = []
    for (let b = 0, at = 0; b < nBfu; at += SPECS_PER_BFU[b], b++) quantizedCoefficients.push(f.quantized.slice(at, at + SPECS_PER_BFU[b]))
    return {
      nBfu,
      scaleFactorIndices: f.sfi.slice(0, nBfu),
      wordLengthIndices: f.wl.slice(0, nBfu),
      quantizedCoefficients,
      blockModes,
    }
  }
}
