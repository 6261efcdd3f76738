// AudioProcessor + encodeAeaPcm / decodeAeaPcm: the stream/file level API of the reference
// (codec/io/processor.js:37-671), with the per-frame hot loop (processor.js:119-136, :193-237)
// replaced by ONE batched native call per buffer; encodeAeaPcmMany / decodeAeaPcmMany do that for many buffers at once.
// The WAV helpers createWavBlob and assemblePcmFrames are host code with the reference's call shapes.
import { EncoderOptions } from '../core/options.js'
import { BufferPool } from '../core/buffers.js'
import { SAMPLES_PER_FRAME, AEA_HEADER_SIZE, SOUND_UNIT_SIZE, SAMPLE_RATE } from '../core/constants.js'
import { encode } from '../pipeline/encoder.js'
import { decode } from '../pipeline/decoder.js'
import { serializeFrame, deserializeFrame, AeaFile } from './serialization.js'
import { native, context, checkPrecision, decodeContext, encodeBatchModes, encodeBatchBiases, encodeBestBias, encodeBestModes, encodeMeasured, encodeMeasuredModes, encodeMeasuredModesMasked, encodeSignalsMeasured, checkScaleFactorOffsets, checkMasking } from '../native.js'
import { biasedTable } from '../coding/bitallocation.js'

function padChannels(channels) {
  const longest = Math.max(...channels.map((c) => c.length))
  const frames = Math.ceil(longest / SAMPLES_PER_FRAME)
  return {
    frames,
    padded: channels.map((c) => {
      if (c.length === frames * SAMPLES_PER_FRAME) return c
      const p = new Float32Array(frames * SAMPLES_PER_FRAME) // zero padding: processor.js:246-279
      p.set(c)
      return p
    }),
  }
}

export async function encodeAeaPcm(channels, options = {}) {
  checkChannels(channels)
  // options.devices (not in the reference): device indices to shard the frame batch over, e.g. [0, 1, 2, 3]; contiguous
  // frame ranges, one context and host thread per entry, no collective -- same bytes as one device
  // options.blockModes (not in the reference): a Uint8Array of frames * channels mode bytes (m0 | m1 << 2 | m2 << 4, frame-major,
  // channels interleaved), frames = ceil(length / 512): every frame is encoded as the reference encodes it with fixedBlockModes
  // set to that frame's modes before the call; the detector does not run and devices is not used
  // options.allocationBiases (not in the reference): a Float64Array of frames (every channel of a frame takes the frame's) or
  // frames * channels values (frame-major, channels interleaved): every frame is encoded as the reference encodes it with
  // allocationBias set to that value before the call.  Each value is range-checked as allocationBias is; at most 8 distinct
  // values per call (RangeError), their tables from this engine's Math.pow.  Combines with blockModes; devices is not used
  // options.allocationBiasCandidates (not in the reference): an array of 1 to 8 distinct allocationBias values: every sound unit
  // is encoded under the candidate that leaves the least coding error, the sum over its 512 MDCT coefficients of the squared
  // difference between the coefficient and what the decoder dequantizes (c1_encode_best_bias_batch).  Each value is
  // range-checked as allocationBias is, their tables from this engine's Math.pow.  Combines with blockModes; mutually
  // exclusive with allocationBiases (TypeError); devices is not used
  // options.blockModeCandidates (not in the reference): an array or Uint8Array of 1 to 8 distinct mode bytes (or triples [low,
  // mid, high]): every sound unit is encoded under the candidate that leaves the least coding error, the squared differences
  // weighted by the transform's scaling so that long and short blocks compare as their PCM error does
  // (c1_encode_best_modes_batch).  The detector does not run; mutually exclusive with blockModes and with
  // allocationBiasCandidates (TypeError), and allocationBiases and devices are not used
  // options.measuredAllocation (not in the reference): true allocates every sound unit's word lengths by the measured coding
  // error instead of the reference's model of it, and keeps the reference's allocation where that codes better
  // (c1_encode_measured_batch).  The units are not the reference encoder's, but decode() reads them.  Alone or with blockModes;
  // mutually exclusive with allocationBiases, allocationBiasCandidates and blockModeCandidates (TypeError); devices is not used
  // options.scaleFactorOffsets (with measuredAllocation: true only, else TypeError): 1 to 8 distinct integers within -8 .. 8, the
  // first 0 (SCALE_FACTOR_OFFSETS is the suggested set).  The measured allocation then also chooses every BFU's scale-factor
  // index among findScaleFactor's plus each offset by the same error (c1_encode_measured_sf_batch)
  // options.masking (with measuredAllocation: true only, else TypeError): true (the packaged tables, MASKING_DEFAULT) or { floor,
  // spread } as for encodeMeasured.  The measured allocation then minimises every BFU's error divided by a masking threshold
  // computed from the unit's own spectrum and these tables (c1_encode_measured_masked_batch)
  // options.measuredModeCandidates (with measuredAllocation: true only, else TypeError): an array or Uint8Array of 1 to 8 distinct
  // mode bytes (or triples) as for blockModeCandidates: every sound unit is encoded under the candidate whose measured allocation
  // leaves the least error (c1_encode_measured_modes_batch).  scaleFactorOffsets combines with it; mutually exclusive with
  // blockModes, blockModeCandidates and masking (TypeError naming both).  The dearest encode of all: one greedy allocation per
  // unit and candidate
  // options.modeSearchMasking (with measuredAllocation: true and measuredModeCandidates only, else TypeError naming what is missing):
  // true or { floor, spread } as for masking.  The search then weighs every candidate's errors with ONE masking threshold per unit
  // and BFU, from the unit's all-long spectrum (c1_encode_measured_modes_masked_batch).  `masking` keeps meaning "thresholds from
  // the unit's own modes" and stays mutually exclusive with measuredModeCandidates
  const { title = 'encoded by carta1', devices, blockModes, allocationBiases, allocationBiasCandidates, blockModeCandidates, measuredAllocation, measuredModeCandidates, modeSearchMasking, scaleFactorOffsets, masking, ...encoderValues } = options
  const encoderOptions = new EncoderOptions(encoderValues)
  const { frames, padded } = padChannels(channels)
  const haveCandidates = allocationBiasCandidates !== undefined && allocationBiasCandidates !== null
  if (haveCandidates && allocationBiases !== undefined && allocationBiases !== null) {
    throw new TypeError('allocationBiases and allocationBiasCandidates are mutually exclusive: give the bias of every frame, or the candidates to choose among')
  }
  const haveModeCandidates = blockModeCandidates !== undefined && blockModeCandidates !== null
  if (haveModeCandidates && blockModes !== undefined && blockModes !== null) {
    throw new TypeError('blockModes and blockModeCandidates are mutually exclusive: give the modes of every frame, or the candidates to choose among')
  }
  if (haveModeCandidates && haveCandidates) {
    throw new TypeError('blockModeCandidates and allocationBiasCandidates are mutually exclusive: one search per call')
  }
  if (haveModeCandidates && allocationBiases !== undefined && allocationBiases !== null) {
    throw new TypeError('blockModeCandidates and allocationBiases are mutually exclusive: the candidates are measured under one allocationBias')
  }
  if (haveModeCandidates) {
    const n = blockModeCandidates.length
    if (!(Array.isArray(blockModeCandidates) || blockModeCandidates instanceof Uint8Array) || n < 1 || n > 8) {
      throw new RangeError(`blockModeCandidates must hold 1 to 8 mode bytes, got ${n}`)
    }
  }
  if (measuredAllocation !== undefined && measuredAllocation !== null && typeof measuredAllocation !== 'boolean') {
    throw new TypeError(`measuredAllocation must be a boolean, got ${measuredAllocation}`)
  }
  const haveMeasuredModes = measuredModeCandidates !== undefined && measuredModeCandidates !== null
  if (haveMeasuredModes) {
    if (!measuredAllocation) throw new TypeError('measuredModeCandidates needs measuredAllocation: true; blockModeCandidates is the search under the reference\'s allocation')
    for (const [name, value, why] of [['blockModes', blockModes, 'give the modes of every frame, or the candidates to choose among'],
      ['blockModeCandidates', blockModeCandidates, 'one search per call'],
      ['masking', masking === false ? null : masking, 'thresholds of different block modes are not comparable']]) {
      if (value !== undefined && value !== null) throw new TypeError(`measuredModeCandidates and ${name} are mutually exclusive: ${why}`)
    }
    const n = measuredModeCandidates.length
    if (!(Array.isArray(measuredModeCandidates) || measuredModeCandidates instanceof Uint8Array) || n < 1 || n > 8) {
      throw new RangeError(`measuredModeCandidates must hold 1 to 8 mode bytes, got ${n}`)
    }
  }
  const haveSearchMasking = modeSearchMasking !== undefined && modeSearchMasking !== null && modeSearchMasking !== false
  if (haveSearchMasking) {
    if (!measuredAllocation) throw new TypeError('modeSearchMasking needs measuredAllocation: true and measuredModeCandidates: it weighs the measured block-mode search')
    if (!haveMeasuredModes) throw new TypeError('modeSearchMasking needs measuredModeCandidates: it weighs the measured block-mode search; masking weighs the allocation under given modes')
    checkMasking(modeSearchMasking)
  }
  if (measuredAllocation) {
    for (const [name, value] of [['allocationBiases', allocationBiases], ['allocationBiasCandidates', allocationBiasCandidates], ['blockModeCandidates', blockModeCandidates]]) {
      if (value !== undefined && value !== null) {
        throw new TypeError(`measuredAllocation and ${name} are mutually exclusive: the measured allocation replaces the search over the reference's options`)
      }
    }
  }
  const haveOffsets = scaleFactorOffsets !== undefined && scaleFactorOffsets !== null
  if (haveOffsets) {
    if (!measuredAllocation) throw new TypeError('scaleFactorOffsets needs measuredAllocation: true; no other path chooses scale factors')
    checkScaleFactorOffsets(scaleFactorOffsets)
  }
  const haveMasking = masking !== undefined && masking !== null && masking !== false
  if (haveMasking) {
    if (!measuredAllocation) throw new TypeError('masking needs measuredAllocation: true; no other path weighs its errors')
    checkMasking(masking)
  }
  let candidates = null
  if (haveCandidates) {
    const values = Array.from(allocationBiasCandidates)
    if (!(Array.isArray(allocationBiasCandidates) || allocationBiasCandidates instanceof Float64Array) || values.length < 1 || values.length > 8) {
      throw new RangeError(`allocationBiasCandidates must hold 1 to 8 values, got ${values.length}`)
    }
    const probe = new EncoderOptions(encoderValues)
    for (const b of values) {
      if (typeof b !== 'number' || Number.isNaN(b)) throw new Error(`Value for allocationBias must be a number, got ${b}`)
      probe.setValue('allocationBias', b)
    }
    if (new Set(values).size !== values.length) throw new RangeError('allocationBiasCandidates must be distinct')
    const base = encoderOptions.toNative()
    candidates = new Float64Array(68 * values.length)
    values.forEach((b, k) => {
      candidates.set(base, 68 * k)
      candidates.set(biasedTable(b), 68 * k)
    })
  }
  let palette = null
  let biasIndex = null
  if (allocationBiases !== undefined && allocationBiases !== null) {
    const units = frames * channels.length
    if (!(allocationBiases instanceof Float64Array) || (allocationBiases.length !== frames && allocationBiases.length !== units)) {
      throw new TypeError(`allocationBiases must be a Float64Array of frames = ${frames} or frames * channels = ${units} values`)
    }
    const probe = new EncoderOptions(encoderValues)
    for (const b of allocationBiases) {
      if (Number.isNaN(b)) throw new Error('Value for allocationBias must be a number, got NaN')
      probe.setValue('allocationBias', b)
    }
    const values = Array.from(new Set(allocationBiases)).sort((x, y) => x - y)
    if (values.length > 8) throw new RangeError(`at most 8 distinct allocation biases per call, got ${values.length}`)
    const slot = new Map(values.map((v, k) => [v, k]))
    const perFrame = allocationBiases.length === frames && channels.length > 1
    biasIndex = Uint8Array.from({ length: units }, (_, u) => slot.get(allocationBiases[perFrame ? Math.floor(u / channels.length) : u]))
    const base = encoderOptions.toNative()
    palette = new Float64Array(68 * Math.max(values.length, 1))
    for (let k = 0; k < Math.max(values.length, 1); k++) {
      palette.set(base, 68 * k)
      if (k < values.length) palette.set(biasedTable(values[k]), 68 * k)
    }
  }
  if (blockModes !== undefined && blockModes !== null &&
      (!(blockModes instanceof Uint8Array) || blockModes.length !== frames * channels.length)) {
    throw new TypeError(`blockModes must be a Uint8Array of frames * channels = ${frames * channels.length} mode bytes`)
  }
  const unitCount = frames * channels.length
  const image = new Uint8Array(AEA_HEADER_SIZE + unitCount * SOUND_UNIT_SIZE)
  image.set(AeaFile.createHeader(title, unitCount, channels.length), 0) // frameCount counts units: processor.js:320-325
  if (frames > 0 && haveMeasuredModes && haveSearchMasking) {
    image.set(encodeMeasuredModesMasked(padded, encoderOptions.toNative(), measuredModeCandidates, haveOffsets ? scaleFactorOffsets : null, modeSearchMasking).units, AEA_HEADER_SIZE)
  } else if (frames > 0 && haveMeasuredModes) {
    image.set(encodeMeasuredModes(padded, encoderOptions.toNative(), measuredModeCandidates, haveOffsets ? scaleFactorOffsets : null).units, AEA_HEADER_SIZE)
  } else if (frames > 0 && measuredAllocation) {
    image.set(encodeMeasured(padded, encoderOptions.toNative(), blockModes || null, haveOffsets ? scaleFactorOffsets : null, haveMasking ? masking : null).units, AEA_HEADER_SIZE)
  } else if (frames > 0 && haveModeCandidates) {
    image.set(encodeBestModes(padded, encoderOptions.toNative(), blockModeCandidates).units, AEA_HEADER_SIZE)
  } else if (frames > 0 && candidates) {
    image.set(encodeBestBias(padded, candidates, blockModes || null).units, AEA_HEADER_SIZE)
  } else if (frames > 0 && palette) {
    image.set(encodeBatchBiases(padded, biasIndex, palette, blockModes || null), AEA_HEADER_SIZE)
  } else if (frames > 0 && blockModes) {
    image.set(encodeBatchModes(padded, blockModes, encoderOptions.toNative()), AEA_HEADER_SIZE)
  } else if (frames > 0) {
    const where = Array.isArray(devices) && devices.length ? devices : context()
    const units = await native().encodeBatchAsync(where, padded, 0, encoderOptions.toNative())
    image.set(units, AEA_HEADER_SIZE)
  }
  return image
}

// options: { devices, precision: 'exact' (default) | 'binary32' } (native.js); the multi-device decode is the exact one only
export async function decodeAeaPcm(input, options = {}) {
  const precision = checkPrecision(options)
  const multi = Array.isArray(options.devices) && options.devices.length
  if (multi && precision !== 'exact') throw new TypeError("precision: 'binary32' cannot be combined with devices")
  let bytes
  if (input instanceof Uint8Array) bytes = input
  else if (input instanceof ArrayBuffer) bytes = new Uint8Array(input)
  else if (typeof Blob !== 'undefined' && input instanceof Blob) bytes = new Uint8Array(await input.arrayBuffer())
  else throw new TypeError('ATRAC1 decoding requires AEA bytes or a Blob')
  const { info, units } = AudioProcessor.parseAea(bytes)
  const nch = info.channelCount
  if (nch !== 1 && nch !== 2) throw new Error(`Unsupported channel count: ${nch}`)
  let body = units
  const count = units.length / SOUND_UNIT_SIZE
  if (nch === 2 && count % 2 === 1) {
    // trailing lone left unit is paired with the reference's dummy frame (processor.js:222-232)
    body = new Uint8Array(units.length + SOUND_UNIT_SIZE)
    body.set(units)
    body[units.length] = 0xac
  }
  if (body.length === 0) return nch === 1 ? [new Float32Array(0)] : [new Float32Array(0), new Float32Array(0)]
  const where = multi ? options.devices : decodeContext(precision)
  return native().decodeBatchAsync(where, body, nch, 0)
}

function checkChannels(channels) {
  if (!Array.isArray(channels) || (channels.length !== 1 && channels.length !== 2) ||
      channels.some((channel) => !(channel instanceof Float32Array))) {
    throw new TypeError('ATRAC1 encoding requires one or two Float32 channels')
  }
}

// ---- many items in one native call: the host part (layout only) ----
// items, each [L] or [L, R] -> one padded mono signal per channel in item order, the frame offsets of the concatenation
// (Float64Array, n + 1 entries) and the channel count of every item
export function itemsToSignals(items) {
  if (!Array.isArray(items)) throw new TypeError('items must be an array of [L] or [L, R]')
  const signals = []
  const counts = []
  for (const channels of items) {
    checkChannels(channels)
    signals.push(...padChannels(channels).padded)
    counts.push(channels.length)
  }
  const frameOffsets = new Float64Array(signals.length + 1)
  signals.forEach((s, i) => { frameOffsets[i + 1] = frameOffsets[i] + s.length / SAMPLES_PER_FRAME })
  return { signals, counts, frameOffsets }
}

function concatSignals(signals, frameOffsets) {
  const pcm = new Float32Array(frameOffsets[signals.length] * SAMPLES_PER_FRAME)
  signals.forEach((s, i) => pcm.set(s, frameOffsets[i] * SAMPLES_PER_FRAME))
  return pcm
}

// the units of item k's channels (signal-major in `units`) -> one AEA body, interleaved L, R
export function interleaveItemUnits(units, frameOffsets, first, channelCount) {
  const frames = frameOffsets[first + 1] - frameOffsets[first]
  const body = new Uint8Array(frames * channelCount * SOUND_UNIT_SIZE)
  for (let c = 0; c < channelCount; c++) {
    const from = frameOffsets[first + c] * SOUND_UNIT_SIZE
    for (let f = 0; f < frames; f++) {
      body.set(units.subarray(from + f * SOUND_UNIT_SIZE, from + (f + 1) * SOUND_UNIT_SIZE), (f * channelCount + c) * SOUND_UNIT_SIZE)
    }
  }
  return body
}

// the inverse for one item: an AEA body interleaved L, R -> one run of units per channel, written into `units` from unit `at`
export function deinterleaveItemUnits(body, channelCount, units, at) {
  const frames = body.length / SOUND_UNIT_SIZE / channelCount
  for (let c = 0; c < channelCount; c++) {
    for (let f = 0; f < frames; f++) {
      const from = (f * channelCount + c) * SOUND_UNIT_SIZE
      units.set(body.subarray(from, from + SOUND_UNIT_SIZE), (at + c * frames + f) * SOUND_UNIT_SIZE)
    }
  }
  return frames
}

// one AEA image -> { nch, body }: whole units only, a lone trailing left unit paired with the dummy right unit
function imageBody(input) {
  if (!(input instanceof Uint8Array) && !(input instanceof ArrayBuffer)) throw new TypeError('ATRAC1 decoding requires AEA bytes')
  const { info, units } = AudioProcessor.parseAea(input instanceof Uint8Array ? input : new Uint8Array(input))
  const nch = info.channelCount
  if (nch !== 1 && nch !== 2) throw new Error(`Unsupported channel count: ${nch}`)
  if (nch === 2 && (units.length / SOUND_UNIT_SIZE) % 2 === 1) {
    const body = new Uint8Array(units.length + SOUND_UNIT_SIZE)
    body.set(units)
    body[units.length] = 0xac
    return { nch, body }
  }
  return { nch, body: units }
}

// encodeAeaPcm for many items at once: every channel of every item is one signal of ONE native call (c1_encode_signals).
// options.title: one string, or one per item.  Each image is byte for byte what encodeAeaPcm returns for that item alone.
// options.measuredAllocation: true, with scaleFactorOffsets and masking as for encodeAeaPcm (they need it, TypeError): the
// measured allocation of every item in the same one call (c1_encode_signals_measured).  blockModes, measuredModeCandidates and
// the candidate searches of encodeAeaPcm are not supported for many items (TypeError)
export async function encodeAeaPcmMany(items, options = {}) {
  const { title = 'encoded by carta1', measuredAllocation, scaleFactorOffsets, masking, ...encoderValues } = options
  for (const name of ['blockModes', 'measuredModeCandidates', 'blockModeCandidates', 'allocationBiases', 'allocationBiasCandidates']) {
    if (encoderValues[name] !== undefined && encoderValues[name] !== null) {
      throw new TypeError(`${name} is not supported by encodeAeaPcmMany: encode the items one by one with encodeAeaPcm`)
    }
  }
  if (measuredAllocation !== undefined && measuredAllocation !== null && typeof measuredAllocation !== 'boolean') {
    throw new TypeError(`measuredAllocation must be a boolean, got ${measuredAllocation}`)
  }
  const haveOffsets = scaleFactorOffsets !== undefined && scaleFactorOffsets !== null
  if (haveOffsets) {
    if (!measuredAllocation) throw new TypeError('scaleFactorOffsets needs measuredAllocation: true; no other path chooses scale factors')
    checkScaleFactorOffsets(scaleFactorOffsets)
  }
  const haveMasking = masking !== undefined && masking !== null && masking !== false
  if (haveMasking) {
    if (!measuredAllocation) throw new TypeError('masking needs measuredAllocation: true; no other path weighs its errors')
    checkMasking(masking)
  }
  const { signals, counts, frameOffsets } = itemsToSignals(items)
  const titles = Array.isArray(title) ? title : items.map(() => title)
  if (titles.length !== items.length || titles.some((t) => typeof t !== 'string')) {
    throw new TypeError('options.title must be a string or one string per item')
  }
  const encoderOptions = new EncoderOptions(encoderValues)
  const total = frameOffsets[signals.length]
  let units = new Uint8Array(0)
  if (total > 0 && measuredAllocation) {
    units = encodeSignalsMeasured(concatSignals(signals, frameOffsets), frameOffsets, encoderOptions.toNative(), haveOffsets ? scaleFactorOffsets : null, haveMasking ? masking : null)
  } else if (total > 0) {
    units = native().encodeSignals(context(), concatSignals(signals, frameOffsets), frameOffsets, encoderOptions.toNative())
  }
  let first = 0
  return counts.map((nch, k) => {
    const body = interleaveItemUnits(units, frameOffsets, first, nch)
    first += nch
    const image = new Uint8Array(AEA_HEADER_SIZE + body.length)
    image.set(AeaFile.createHeader(titles[k], body.length / SOUND_UNIT_SIZE, nch), 0)
    image.set(body, AEA_HEADER_SIZE)
    return image
  })
}

// decodeAeaPcm for many AEA images (Uint8Array or ArrayBuffer) at once -> per image an array of Float32Array, one per channel.
// options: { precision: 'exact' (default) | 'binary32' } (native.js)
export async function decodeAeaPcmMany(images, options = {}) {
  const precision = checkPrecision(options)
  if (!Array.isArray(images)) throw new TypeError('images must be an array of AEA byte images')
  const parsed = images.map(imageBody)
  const frameOffsets = new Float64Array(parsed.reduce((n, p) => n + p.nch, 0) + 1)
  let k = 0
  for (const { nch, body } of parsed) {
    for (let c = 0; c < nch; c++, k++) frameOffsets[k + 1] = frameOffsets[k] + body.length / SOUND_UNIT_SIZE / nch
  }
  const total = frameOffsets[k]
  const units = new Uint8Array(total * SOUND_UNIT_SIZE)
  k = 0
  for (const { nch, body } of parsed) {
    deinterleaveItemUnits(body, nch, units, frameOffsets[k])
    k += nch
  }
  const pcm = total > 0 ? native().decodeSignals(decodeContext(precision), units, frameOffsets) : new Float32Array(0)
  k = 0
  return parsed.map(({ nch }) => {
    const out = []
    for (let c = 0; c < nch; c++, k++) out.push(pcm.slice(frameOffsets[k] * SAMPLES_PER_FRAME, frameOffsets[k + 1] * SAMPLES_PER_FRAME))
    return out
  })
}

// WAV body (interleaved little-endian integer PCM: Int16Array, or a Uint8Array with bits = 16, 24 or 32) -> AEA image.
// What the reference's CLI does with WavReader + encodeStream (bin/cli.js:367-404, processor.js:246-276) as one
// native call: the integer samples cross PCIe and are converted on the device.
export function encodeWavPcm(wavBody, options = {}) {
  const { title = 'encoded by carta1', channelCount = 1, bits = 16, ...encoderValues } = options
  if (!(wavBody instanceof Int16Array) && !(wavBody instanceof Uint8Array)) {
    throw new TypeError('ATRAC1 WAV encoding requires an Int16Array or a Uint8Array of sample bytes')
  }
  if (channelCount !== 1 && channelCount !== 2) throw new TypeError('ATRAC1 encoding requires one or two channels')
  const encoderOptions = new EncoderOptions(encoderValues)
  const units = native().encodeWavBatch(context(), wavBody, wavBody instanceof Int16Array ? 16 : bits, channelCount, encoderOptions.toNative())
  const image = new Uint8Array(AEA_HEADER_SIZE + units.length)
  image.set(AeaFile.createHeader(title, units.length / SOUND_UNIT_SIZE, channelCount), 0)
  image.set(units, AEA_HEADER_SIZE)
  return image
}

// AEA image -> { channelCount, samples: Int16Array (interleaved) }: decode + the 16-bit conversion of createWavBlob
// (processor.js:349-447) on the device.  options: { precision: 'exact' (default) | 'binary32' } (native.js)
export function decodeAeaToWav16(bytes, options = {}) {
  const precision = checkPrecision(options)
  if (!(bytes instanceof Uint8Array)) throw new TypeError('ATRAC1 decoding requires AEA bytes')
  const { info, units } = AudioProcessor.parseAea(bytes)
  const nch = info.channelCount
  if (nch !== 1 && nch !== 2) throw new Error(`Unsupported channel count: ${nch}`)
  // a stereo image that ends on a lone left unit: the reference pairs it with a dummy right unit (processor.js:222-232)
  let whole = units
  const rest = units.length % (nch * SOUND_UNIT_SIZE)
  if (rest >= SOUND_UNIT_SIZE) {
    whole = new Uint8Array(units.length - rest + nch * SOUND_UNIT_SIZE)
    whole.set(units.subarray(0, units.length - rest + SOUND_UNIT_SIZE))
    whole[units.length - rest + SOUND_UNIT_SIZE] = 0xac            // the dummy unit's two header bytes, zeros after
  } else if (rest) {
    whole = units.subarray(0, units.length - rest)
  }
  return { channelCount: nch, samples: whole.length ? native().decodeWav16Batch(decodeContext(precision), whole, nch) : new Int16Array(0) }
}

export class AudioProcessor {
  static encodeAeaPcm(channels, options = {}) { return encodeAeaPcm(channels, options) }
  static decodeAeaPcm(input, options = {}) { return decodeAeaPcm(input, options) }

  // PCM frames -> a 16-bit PCM WAV file (the reference's createWavBlob, processor.js:349-447, returns a Blob; createWavBytes
  // returns the same bytes as a Uint8Array so this also runs where Blob does not exist).  pcmFrames: mono frames (or one
  // Float32Array), or [left, right] pairs; the shorter side of a pair is zero filled.  Samples are clipped to [-1, 1] and
  // scaled by 0x7fff (>= 0) or 0x8000 (< 0), then truncated as DataView.setInt16 truncates.
  static createWavBlob(pcmFrames, channelCount = 1, sampleRate = SAMPLE_RATE) {
    const bytes = AudioProcessor.createWavBytes(pcmFrames, channelCount, sampleRate)
    if (typeof Blob === 'undefined') throw new Error('Blob is not available in this runtime; use createWavBytes')
    return new Blob([bytes], { type: 'audio/wav' })
  }

  static createWavBytes(pcmFrames, channelCount = 1, sampleRate = SAMPLE_RATE) {
    if (channelCount !== 1 && channelCount !== 2) throw new Error(`Unsupported channel count: ${channelCount}`)
    const pcm = AudioProcessor.assemblePcmFrames(Array.isArray(pcmFrames) ? pcmFrames : [pcmFrames], channelCount)
    const dataBytes = pcm.length * 2
    const view = new DataView(new ArrayBuffer(44 + dataBytes))
    const tag = (at, text) => { for (let i = 0; i < 4; i++) view.setUint8(at + i, text.charCodeAt(i)) }
    tag(0, 'RIFF'); view.setUint32(4, 36 + dataBytes, true); tag(8, 'WAVE')
    tag(12, 'fmt '); view.setUint32(16, 16, true); view.setUint16(20, 1, true); view.setUint16(22, channelCount, true)
    view.setUint32(24, sampleRate, true); view.setUint32(28, sampleRate * channelCount * 2, true)
    view.setUint16(32, channelCount * 2, true); view.setUint16(34, 16, true)
    tag(36, 'data'); view.setUint32(40, dataBytes, true)
    for (let i = 0; i < pcm.length; i++) {
      const x = Math.max(-1, Math.min(1, pcm[i]))
      view.setInt16(44 + 2 * i, x < 0 ? x * 0x8000 : x * 0x7fff, true)
    }
    return new Uint8Array(view.buffer)
  }

  // PCM frames -> one continuous Float32Array (the reference's assemblePcmFrames, processor.js:545-579): mono frames back to
  // back, or [left, right] pairs interleaved sample by sample, the shorter side of a pair zero filled
  static assemblePcmFrames(pcmFrames, channelCount) {
    if (channelCount === 1) {
      const pcm = new Float32Array(pcmFrames.reduce((n, f) => n + f.length, 0))
      let at = 0
      for (const f of pcmFrames) { pcm.set(f, at); at += f.length }
      return pcm
    }
    if (channelCount !== 2) throw new Error(`Unsupported channel count: ${channelCount}`)
    const lengths = pcmFrames.map(([l, r]) => Math.max(l.length, r.length))
    const pcm = new Float32Array(2 * lengths.reduce((n, m) => n + m, 0))
    let at = 0
    pcmFrames.forEach(([l, r], k) => {
      for (let j = 0; j < l.length; j++) pcm[at + 2 * j] = l[j]
      for (let j = 0; j < r.length; j++) pcm[at + 2 * j + 1] = r[j]
      at += 2 * lengths[k]
    })
    return pcm
  }

  // Streams of frames in, frame fields out: one closure per channel, as processor.js:69-136.
  // options.batchFrames (default 1 = a result after every frame, like the reference): with N > 1 the frames are
  // collected and handed to the device N at a time (one native stream for all channels); same fields, N times fewer
  // device round trips.  The encoder options are read as each frame is collected, as the reference's closures read them
  // per frame: the frames collected under other options are pushed first, and the stream goes on under the new ones.
  static async *encodeStream(audioFrames, options = {}) {
    const { channelCount = 1, onProgress, encoderOptions, batchFrames = 1 } = options
    if (channelCount !== 1 && channelCount !== 2) throw new Error(`Unsupported channel count: ${channelCount}`)
    const opts = encoderOptions || new EncoderOptions()
    let frameIndex = 0
    if (batchFrames > 1) {
      const addon = native()
      const first = opts.toNative()
      let key = first.join(',')
      const stream = addon.encStreamCreate(context(), channelCount, first)
      let pending = 0
      let buffers = null
      const modes = []   // options.fixedBlockModes as each pending frame was collected
      const flush = function* () {
        const units = addon.encStreamPush(stream, buffers.map((b) => b.subarray(0, pending * SAMPLES_PER_FRAME)))
        const frameModes = modes.splice(0, pending)
        pending = 0
        for (let f = 0; f < frameModes.length; f++) {
          for (let c = 0; c < channelCount; c++) {
            const at = (f * channelCount + c) * SOUND_UNIT_SIZE
            const fields = deserializeFrame(units.subarray(at, at + SOUND_UNIT_SIZE))
            if (frameModes[f]) fields.blockModes = frameModes[f]
            yield fields
          }
          if (onProgress) onProgress(frameIndex++)
        }
      }
      for await (const frame of audioFrames) {
        const parts = channelCount === 1 ? [frame] : frame
        if (!buffers) buffers = parts.map(() => new Float32Array(batchFrames * SAMPLES_PER_FRAME))
        for (let c = 0; c < channelCount; c++) {
          if (!(parts[c] instanceof Float32Array) || parts[c].length !== SAMPLES_PER_FRAME) {
            throw new Error(`encode: expected a Float32Array of ${SAMPLES_PER_FRAME} samples`)
          }
        }
        const now = opts.toNative()
        const nowKey = now.join(',')
        if (nowKey !== key) {
          if (pending) yield* flush()
          addon.encStreamSetOptions(stream, now)
          key = nowKey
        }
        modes.push(opts.fixedBlockModes)
        for (let c = 0; c < channelCount; c++) buffers[c].set(parts[c], pending * SAMPLES_PER_FRAME)
        if (++pending === batchFrames) yield* flush()
      }
      if (pending) yield* flush()
      return
    }
    const encoders = []
    for (let c = 0; c < channelCount; c++) encoders.push(encode(opts, new BufferPool()))
    for await (const frame of audioFrames) {
      const parts = channelCount === 1 ? [frame] : frame
      for (let c = 0; c < channelCount; c++) yield encoders[c](parts[c])
      if (onProgress) onProgress(frameIndex++)
    }
  }

  static async *decodeStream(encodedFrames, options = {}) {
    const { channelCount = 1, onProgress } = options
    const precision = checkPrecision(options)
    if (channelCount !== 1 && channelCount !== 2) throw new Error(`Unsupported channel count: ${channelCount}`)
    const decoders = []
    for (let c = 0; c < channelCount; c++) decoders.push(decode(new BufferPool(), { precision }))
    let frameIndex = 0
    let pending = []
    for await (const frame of encodedFrames) {
      pending.push(frame)
      if (pending.length < channelCount) continue
      const out = pending.map((f, c) => decoders[c](f))
      pending = []
      yield channelCount === 1 ? out[0] : out
      if (onProgress) onProgress(frameIndex++)
    }
    if (pending.length === 1 && channelCount === 2) {
      yield [decoders[0](pending[0]), decoders[1](AudioProcessor._createDummyFrame())]
      if (onProgress) onProgress(frameIndex++)
    }
  }

  static *frameBufferToFrames(buffers, frameSize = SAMPLES_PER_FRAME) {
    if (buffers.length !== 1 && buffers.length !== 2) throw new Error(`Unsupported channel count: ${buffers.length}`)
    const longest = Math.max(...buffers.map((b) => b.length))
    for (let at = 0; at < longest; at += frameSize) {
      const frames = buffers.map((b) => {
        const f = new Float32Array(frameSize)
        if (at < b.length) f.set(b.subarray(at, Math.min(at + frameSize, b.length)))
        return f
      })
      yield buffers.length === 1 ? frames[0] : frames
    }
  }

  static async collectFrames(frameStream) {
    const frames = []
    for await (const frame of frameStream) frames.push(frame)
    return frames
  }

  static _createDummyFrame() {
    return { nBfu: 0, blockModes: [0, 0, 0], scaleFactorIndices: new Int32Array(0), wordLengthIndices: new Int32Array(0), quantizedCoefficients: [] }
  }

  // AEA image from a stream of frame fields (createAeaBlob of the reference returns a Blob; a
  // Uint8Array is returned here so this also runs where Blob does not exist).
  static async createAeaBytes(encodedFrames, options = {}) {
    const { title = 'encoded by atrac1.js', channelCount = 1 } = options
    const units = []
    for await (const frame of encodedFrames) units.push(serializeFrame(frame))
    const image = new Uint8Array(AEA_HEADER_SIZE + units.length * SOUND_UNIT_SIZE)
    image.set(AeaFile.createHeader(title, units.length, channelCount), 0)
    units.forEach((u, i) => image.set(u, AEA_HEADER_SIZE + i * SOUND_UNIT_SIZE))
    return image
  }

  static async createAeaBlob(encodedFrames, options = {}) {
    const bytes = await AudioProcessor.createAeaBytes(encodedFrames, options)
    if (typeof Blob === 'undefined') throw new Error('Blob is not available in this runtime; use createAeaBytes')
    return new Blob([bytes], { type: 'application/octet-stream' })
  }

  static parseAea(bytes) {
    const info = AeaFile.parseHeader(bytes.subarray(0, AEA_HEADER_SIZE))
    const whole = Math.floor((bytes.length - AEA_HEADER_SIZE) / SOUND_UNIT_SIZE) // a partial trailing unit is dropped
    return { info, units: bytes.subarray(AEA_HEADER_SIZE, AEA_HEADER_SIZE + whole * SOUND_UNIT_SIZE) }
  }

  static async parseAeaBlob(blob) {
    const { info, units } = AudioProcessor.parseAea(new Uint8Array(await blob.arrayBuffer()))
    const frameData = []
    for (let at = 0; at < units.length; at += SOUND_UNIT_SIZE) frameData.push(units.slice(at, at + SOUND_UNIT_SIZE))
    return { info, frameData }
  }

  static *deserializedFrameStream(frameData) {
    for (const frame of frameData) yield deserializeFrame(frame)
  }
}
