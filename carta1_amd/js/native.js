// Loads the N-API addon (addon/carta1_napi.node -> lib/libcarta1_hip.so) and owns the default device
// context.  There is no JavaScript fallback for the hot path: if the addon or a HIP device is missing,
// the first call throws the library's error.
import fs from 'fs'
import { createRequire } from 'module'
import { buildNativeTables } from './core/constants.js'

const require = createRequire(import.meta.url)
let addon = null
let defaultCtx = null
let binary32Ctx = null

export function native() {
  if (!addon) {
    try {
      addon = require('./addon/carta1_napi.node')
    } catch (e) {
      throw new Error(`carta1-amd: native addon not built (${e.message}); run \`make -C carta1_amd/js/addon\` -- there is no CPU fallback`)
    }
    addon.setTables(buildNativeTables())
  }
  return addon
}

export function context(device = 0) {
  if (device !== 0) return native().ctxCreate(device)
  if (!defaultCtx) defaultCtx = native().ctxCreate(0)
  return defaultCtx
}

// The decode option { precision: 'exact' | 'binary32' } of decode(), decodeAeaPcm, decodeAeaPcmMany, decodeAeaToWav16 and
// AudioProcessor.decodeStream.  'exact' (default): bit-identical to the reference.  'binary32': every decode entry in binary32
// (c1_ctx_set_decode_model, C1_DECODE_BINARY32): the PCM differs from the reference's by rounding noise, a few 2^-24 of the
// signal.  Anything else is a TypeError naming the option, raised before any native call.
export const DECODE_EXACT = 0, DECODE_BINARY32_BULK = 1, DECODE_BINARY32 = 2
export function checkPrecision(options) {
  if (options === null || typeof options !== 'object') throw new TypeError('options must be an object { precision }')
  const precision = options.precision === undefined ? 'exact' : options.precision
  if (precision !== 'exact' && precision !== 'binary32') throw new TypeError(`precision must be 'exact' or 'binary32', got ${String(precision)}`)
  return precision
}

// The context decode calls of the given precision run on.  The shared default context is never switched: binary32 decodes have
// a default context of their own, created at the first use, whose decode model is C1_DECODE_BINARY32.
export function decodeContext(precision = 'exact') {
  if (precision !== 'binary32') return context()
  if (!binary32Ctx) {
    const ctx = native().ctxCreate(0)
    native().ctxSetDecodeModel(ctx, DECODE_BINARY32)
    binary32Ctx = ctx
  }
  return binary32Ctx
}

export function deviceCount() {
  return native().deviceCount()
}

// Float32Array in page-locked host memory: PCM placed there is uploaded at the pinned PCIe rate and large batches
// are streamed (upload, kernels and download of consecutive chunks overlap).  Garbage collected like any array.
export function allocPinnedFloat32Array(length) {
  return new Float32Array(native().allocPinned(length * 4))
}

// c1_encode_modes_batch on the default context: encode() with the block modes of every frame given.  channels: one or two
// Float32Arrays of (haloFrames + frames) * 512 samples; modes: Uint8Array of frames * channels bytes m0 | m1 << 2 | m2 << 4
// (frame-major, channels interleaved; low and mid field 0 or 2, high field 0 or 3); nativeOptions: EncoderOptions.toNative(),
// of which only the allocation bias is used.  Returns the units, frames * channels * 212 bytes.
export function encodeBatchModes(channels, modes, nativeOptions, haloFrames = 0, ctx = context()) {
  return native().encodeBatchModes(ctx, channels, haloFrames, nativeOptions, modes)
}

// c1_encode_biases_batch on the default context: encode() with the allocation bias of every frame and channel taken from a
// palette.  nativePalette: Float64Array(68 * n), n = 1 .. 8 results of EncoderOptions.toNative() one after the other; index:
// Uint8Array of frames * channels palette indices (frame-major, channels interleaved); modes: null (detection or fixed modes as
// the palette's entries say, which must then agree) or mode bytes as for encodeBatchModes.  Returns the units.
export function encodeBatchBiases(channels, index, nativePalette, modes = null, haloFrames = 0, ctx = context()) {
  return native().encodeBatchBiases(ctx, channels, haloFrames, nativePalette, index, modes)
}

// c1_encode_best_bias_batch on the default context: encode() with the allocation bias of every sound unit chosen among the
// option sets by least coding error -- the sum over the unit's 512 MDCT coefficients of (c - d)^2, d what the decoder's
// dequantizationStage makes of the unit.  optionSets: 1 .. 8 results of EncoderOptions.toNative() (an array of them, or one
// Float64Array(68 * n)); modes: null (detection or fixed modes as the sets say, which must then agree) or mode bytes as for
// encodeBatchModes.  Returns { units, choice: Uint8Array(frames * channels) indexing optionSets, distortion:
// Float64Array(frames * channels * n) unit-major, energy: Float64Array(frames * channels) }.
export function encodeBestBias(channels, optionSets, modes = null, haloFrames = 0, ctx = context()) {
  let palette = optionSets
  if (Array.isArray(optionSets)) {
    palette = new Float64Array(68 * optionSets.length)
    optionSets.forEach((set, k) => {
      if (!(set instanceof Float64Array) || set.length !== 68) throw new TypeError('optionSets: results of EncoderOptions.toNative()')
      palette.set(set, 68 * k)
    })
  }
  return native().encodeBestBias(ctx, channels, haloFrames, palette, modes)
}

// c1_encode_best_modes_batch on the default context: encode() with the block modes of every sound unit chosen among the
// candidates by least coding error -- the sum over the unit's 512 MDCT coefficients of W * (c - d)^2, d what the decoder's
// dequantizationStage makes of the unit and W the transform's scaling (1 long, 1/4 low or mid short, 1/2 high short).
// nativeOptions: EncoderOptions.toNative(), of which only the allocation bias is used; candidates: 1 .. 8 distinct mode bytes
// as for encodeBatchModes (a Uint8Array or an array; an entry may be a triple [low, mid, high]).  Returns { units, choice:
// Uint8Array(frames * channels) indexing candidates, modes: Uint8Array(frames * channels) the chosen bytes, distortion and
// energy: Float64Array(frames * channels * n) unit-major }.
export function encodeBestModes(channels, nativeOptions, candidates, haloFrames = 0, ctx = context()) {
  const bytes = Uint8Array.from(Array.from(candidates), (c) => {
    if (Array.isArray(c)) {
      if (c.length !== 3 || c.some((m) => !Number.isInteger(m) || m < 0 || m > 3)) throw new TypeError('candidates: a triple holds three block modes 0..3')
      return c[0] | (c[1] << 2) | (c[2] << 4)
    }
    if (!Number.isInteger(c) || c < 0 || c > 255) throw new TypeError('candidates: mode bytes 0..255 or triples [low, mid, high]')
    return c
  })
  return native().encodeBestModes(ctx, channels, haloFrames, nativeOptions, bytes)
}

// c1_encode_measured_batch on the default context: encode() with the word lengths of every sound unit allocated by the
// measured coding error instead of the reference's model of it (opt-in: the units are not the reference encoder's, but ordinary
// sound units with its block modes and scale factors that decode() reads).  nativeOptions: EncoderOptions.toNative(); modes:
// null (detection or fixed modes as the options say) or mode bytes as for encodeBatchModes.  Returns { units, taken:
// Uint8Array(frames * channels), 1 where the greedy allocation coded with less error than the reference's record and was packed,
// 0 where the unit is byte for byte the plain encode's, distortion: Float64Array(frames * channels * 2), per unit the reference
// record's weighted error and the greedy allocation's, energy: Float64Array(frames * channels) }.
// scaleFactorOffsets (c1_encode_measured_sf_batch): null, or 1 .. 8 distinct integers within -8 .. 8, the first 0, e.g.
// SCALE_FACTOR_OFFSETS.  Every BFU's scale-factor index is then chosen, per word length, among findScaleFactor's plus each
// offset by the same error; a taken unit carries the chosen indices, and the result gains shifts: Int8Array(frames * channels *
// 52), the offset written per BFU and 0 where none was.  A list that breaks these rules is a TypeError naming the option.
// (A number in the place of scaleFactorOffsets is taken as haloFrames, as the function's earlier form had it.)
export const SCALE_FACTOR_OFFSETS = Object.freeze([0, -1, 1, -2, -3])

export function checkScaleFactorOffsets(scaleFactorOffsets) {
  const list = scaleFactorOffsets !== null && typeof scaleFactorOffsets === 'object' && typeof scaleFactorOffsets.length === 'number' ? Array.from(scaleFactorOffsets) : null
  if (!list) throw new TypeError('scaleFactorOffsets must be an array of integers')
  if (list.length < 1 || list.length > 8) throw new TypeError(`scaleFactorOffsets must hold 1 to 8 offsets, got ${list.length}`)
  list.forEach((v, k) => {
    if (!Number.isInteger(v) || v < -8 || v > 8) throw new TypeError(`scaleFactorOffsets[${k}] = ${v} is not an integer within -8..8`)
    if (list.indexOf(v) !== k) throw new TypeError(`scaleFactorOffsets[${k}] = ${v} is given twice`)
  })
  if (list[0] !== 0) throw new TypeError(`scaleFactorOffsets[0] must be 0, the reference's own index, got ${list[0]}`)
  return Int8Array.from(list)
}

// masking (c1_encode_measured_masked_batch): null, true (MASKING_DEFAULT, the packaged tables of carta1_amd/masking_default.json,
// which both hosts read so that they feed identical bits) or { floor, spread }: floor 52 finite numbers within [1e-60, 1e60],
// spread null or 52 * 52 finite numbers within [0, 1e60], row-major (or 52 rows of 52), spread[52 b + c] = masker c onto maskee b.
// Every BFU's error is then divided by a masking threshold computed per unit from the unit's own spectrum and these tables;
// distortion and energy are the weighted ones, and the result gains weights: Float64Array(frames * channels * 52), the reciprocal
// threshold of every BFU.  Without offsets the offsets are [0].  Tables that break the rules are a TypeError naming the option.
// (A number in the place of masking is taken as haloFrames, as the function's earlier form had it.)
let maskingDefault = null
function packagedMasking() {
  if (!maskingDefault) {
    const raw = JSON.parse(fs.readFileSync(new URL('../masking_default.json', import.meta.url), 'utf8'))
    const value = (h) => new DataView(Uint8Array.from(h.match(/../g), (x) => parseInt(x, 16)).buffer).getFloat64(0, false)
    maskingDefault = Object.freeze({ floor: Float64Array.from(raw.floor_f64, value), spread: Float64Array.from(raw.spread_f64.flat(), value) })
  }
  return maskingDefault
}
export const MASKING_DEFAULT = Object.freeze({
  get floor() { return packagedMasking().floor },
  get spread() { return packagedMasking().spread },
})

export function checkMasking(masking) {
  if (masking === true) return packagedMasking()
  if (masking === null || typeof masking !== 'object' || masking.floor === undefined) throw new TypeError('masking must be true or { floor, spread }')
  const numbers = (x) => (x !== null && typeof x === 'object' && typeof x.length === 'number' ? Array.from(x).flatMap((v) => (v !== null && typeof v === 'object' ? Array.from(v) : [v])) : null)
  const floor = numbers(masking.floor)
  const spread = masking.spread === null || masking.spread === undefined ? null : numbers(masking.spread)
  if (!floor || floor.length !== 52) throw new TypeError('masking.floor must hold 52 numbers')
  if (masking.spread !== null && masking.spread !== undefined && (!spread || spread.length !== 52 * 52)) throw new TypeError('masking.spread must be null or hold 52 * 52 numbers')
  floor.forEach((v, b) => {
    if (typeof v !== 'number' || !(v >= 1e-60 && v <= 1e60)) throw new TypeError(`masking.floor[${b}] = ${v} is outside [1e-60, 1e60]`)
  })
  if (spread) {
    spread.forEach((v, i) => {
      if (typeof v !== 'number' || !(v >= 0 && v <= 1e60)) throw new TypeError(`masking.spread[${i}] = ${v} is outside [0, 1e60]`)
    })
  }
  return { floor: Float64Array.from(floor), spread: spread ? Float64Array.from(spread) : null }
}

export function encodeMeasured(channels, nativeOptions, modes = null, scaleFactorOffsets = null, masking = null, haloFrames = 0, ctx = context()) {
  if (typeof scaleFactorOffsets === 'number') return encodeMeasured(channels, nativeOptions, modes, null, null, scaleFactorOffsets, masking || context())
  if (typeof masking === 'number') return encodeMeasured(channels, nativeOptions, modes, scaleFactorOffsets, null, masking, haloFrames || context())
  if (masking !== null && masking !== undefined) {
    const tables = checkMasking(masking)
    const offsets = scaleFactorOffsets === null || scaleFactorOffsets === undefined ? Int8Array.of(0) : checkScaleFactorOffsets(scaleFactorOffsets)
    return native().encodeMeasuredMasked(ctx, channels, haloFrames, nativeOptions, modes, offsets, tables.floor, tables.spread)
  }
  if (scaleFactorOffsets === null || scaleFactorOffsets === undefined) return native().encodeMeasured(ctx, channels, haloFrames, nativeOptions, modes)
  return native().encodeMeasuredSf(ctx, channels, haloFrames, nativeOptions, modes, checkScaleFactorOffsets(scaleFactorOffsets))
}

// c1_encode_signals_measured on the default context: encodeMeasured for n independent mono signals of any lengths in one call,
// every signal from a fresh pool.  pcm: the signals' whole frames back to back; frameOffsets: Float64Array of n + 1 whole numbers,
// signal i owns frames [frameOffsets[i], frameOffsets[i + 1]).  scaleFactorOffsets and masking as for encodeMeasured (with masking
// and no offsets the offsets are [0]).  Returns the units, Uint8Array(frames * 212): signal i's are what encodeMeasured gives for
// it alone.
export function encodeSignalsMeasured(pcm, frameOffsets, nativeOptions, scaleFactorOffsets = null, masking = null, ctx = context()) {
  const offsets = scaleFactorOffsets === null || scaleFactorOffsets === undefined ? null : checkScaleFactorOffsets(scaleFactorOffsets)
  const tables = masking === null || masking === undefined ? null : checkMasking(masking)
  return native().encodeSignalsMeasured(ctx, pcm, frameOffsets, nativeOptions, offsets, tables ? tables.floor : null, tables ? tables.spread : null)
}

// mode candidates as the mode-search calls take them (a Uint8Array or an array; an entry may be a triple [low, mid, high]) ->
// Uint8Array of mode bytes; the library checks domain, count and repeats
export function modeCandidateBytes(candidates) {
  return Uint8Array.from(Array.from(candidates), (c) => {
    if (Array.isArray(c)) {
      if (c.length !== 3 || c.some((m) => !Number.isInteger(m) || m < 0 || m > 3)) throw new TypeError('candidates: a triple holds three block modes 0..3')
      return c[0] | (c[1] << 2) | (c[2] << 4)
    }
    if (!Number.isInteger(c) || c < 0 || c > 255) throw new TypeError('candidates: mode bytes 0..255 or triples [low, mid, high]')
    return c
  })
}

// c1_encode_signals_measured_modes on the default context: encodeMeasuredModes for n independent mono signals of any lengths in one
// call, every signal from a fresh pool.  pcm and frameOffsets as for encodeSignalsMeasured; candidates and scaleFactorOffsets
// (null: the plain measured allocation) as for encodeMeasuredModes.  Returns the units, Uint8Array(frames * 212): signal i's are
// what encodeMeasuredModes gives for it alone.
export function encodeSignalsMeasuredModes(pcm, frameOffsets, nativeOptions, candidates, scaleFactorOffsets = null, ctx = context()) {
  const bytes = modeCandidateBytes(candidates)
  const offsets = scaleFactorOffsets === null || scaleFactorOffsets === undefined ? null : checkScaleFactorOffsets(scaleFactorOffsets)
  return native().encodeSignalsMeasuredModes(ctx, pcm, frameOffsets, nativeOptions, bytes, offsets)
}

// c1_encode_measured_modes_batch on the default context: encodeMeasured with the block modes of every sound unit chosen among the
// candidates by the final error of the measured allocation under each -- per (unit, candidate) the figures of encodeMeasured under
// that constant byte, the candidate of least T_final = taken ? T(n*) : T_ref wins, the first on a tie.  nativeOptions:
// EncoderOptions.toNative(), of which only the allocation bias is used; candidates: as for encodeBestModes; scaleFactorOffsets:
// null (the plain measured allocation) or as for encodeMeasured.  Returns { units, choice: Uint8Array(frames * channels) indexing
// candidates, modes: the chosen bytes, taken, shifts: Int8Array(frames * channels * 52) (the winner's), distortion:
// Float64Array(frames * channels * n * 2) unit-major (T_ref, T(n*) per candidate), energy: Float64Array(frames * channels * n) };
// units are what encodeMeasured gives under `modes`.  The dearest encode of the library: one greedy allocation per unit and
// candidate.
export function encodeMeasuredModes(channels, nativeOptions, candidates, scaleFactorOffsets = null, haloFrames = 0, ctx = context()) {
  const bytes = Uint8Array.from(Array.from(candidates), (c) => {
    if (Array.isArray(c)) {
      if (c.length !== 3 || c.some((m) => !Number.isInteger(m) || m < 0 || m > 3)) throw new TypeError('candidates: a triple holds three block modes 0..3')
      return c[0] | (c[1] << 2) | (c[2] << 4)
    }
    if (!Number.isInteger(c) || c < 0 || c > 255) throw new TypeError('candidates: mode bytes 0..255 or triples [low, mid, high]')
    return c
  })
  const offsets = scaleFactorOffsets === null || scaleFactorOffsets === undefined ? Int8Array.of(0) : checkScaleFactorOffsets(scaleFactorOffsets)
  return native().encodeMeasuredModes(ctx, channels, haloFrames, nativeOptions, bytes, offsets)
}

// c1_encode_measured_modes_masked_batch on the default context: encodeMeasuredModes with every candidate's errors divided by ONE
// masking threshold per unit and BFU, computed from the unit's all-long spectrum whatever the candidates (the weights
// encodeMeasured reports under all-long modes and the same tables), so that the candidates' weighted T_final are comparable.
// candidates and scaleFactorOffsets as for encodeMeasuredModes; masking: true (MASKING_DEFAULT) or { floor, spread } as for
// encodeMeasured, required.  Returns encodeMeasuredModes' object with the weighted distortion and energy, and weights:
// Float64Array(frames * channels * 52).
export function encodeMeasuredModesMasked(channels, nativeOptions, candidates, scaleFactorOffsets, masking, haloFrames = 0, ctx = context()) {
  const bytes = modeCandidateBytes(candidates)
  const offsets = scaleFactorOffsets === null || scaleFactorOffsets === undefined ? Int8Array.of(0) : checkScaleFactorOffsets(scaleFactorOffsets)
  if (masking === null || masking === undefined) throw new TypeError('encodeMeasuredModesMasked needs masking: true or { floor, spread }')
  const tables = checkMasking(masking)
  return native().encodeMeasuredModesMasked(ctx, channels, haloFrames, nativeOptions, bytes, offsets, tables.floor, tables.spread)
}

// c1_measure_units_batch on the default context: the coding error of sound units that already exist -- any encoder's -- against
// their PCM, scored from the bytes with the yardstick of encodeMeasured.  channels: one or two Float32Arrays of (haloFrames +
// frames) * 512 samples; units: Uint8Array of frames * channels * 212 bytes (frame-major, channels interleaved), every unit's
// block modes as the encoder writes them (low and mid 0 or 2, high 0 or 3).  options: { masking, haloFrames }; masking: null,
// true or { floor, spread } as for encodeMeasured.  Returns { noise, signal: Float64Array(frames * channels * 52), per BFU the
// W-weighted squared error of the dequantized unit against the exact coefficients under the unit's own block modes and the
// W-weighted energy of those, totals: Float64Array(frames * channels * 2), their sums over the BFUs -- weighted by every BFU's
// reciprocal masking threshold when masking is given, and the result then gains weights: Float64Array(frames * channels * 52) }.
// thresholdFrom: 'own' (the default) forms those thresholds from the unit's spectrum under its own block modes; 'long' (needs
// masking) from the frame's all-long spectrum, the one threshold per unit of encodeMeasuredModesMasked under which units coded in
// different modes compare (c1_measure_units_shared_batch).  noise and signal are the same either way.
// Arguments that break these rules are a TypeError naming the argument, raised before any native call.
export function checkMeasuredUnits(channels, units, haloFrames = 0) {
  if (!Array.isArray(channels) || channels.length < 1 || channels.length > 2 || channels.some((c) => !(c instanceof Float32Array))) {
    throw new TypeError('channels must be an array of one or two Float32Array')
  }
  if (!Number.isInteger(haloFrames) || haloFrames < 0 || haloFrames > 2) throw new TypeError(`haloFrames must be 0, 1 or 2, got ${haloFrames}`)
  const samples = channels[0].length
  if (channels.some((c) => c.length !== samples) || samples % 512 || samples / 512 < haloFrames) {
    throw new TypeError('channels must have equal length, a multiple of 512 that covers haloFrames')
  }
  const count = (samples / 512 - haloFrames) * channels.length
  if (!(units instanceof Uint8Array)) throw new TypeError('units must be a Uint8Array')
  if (units.length !== count * 212) throw new TypeError(`units must hold frames * channels = ${count} sound units of 212 bytes, got ${units.length} bytes`)
  for (let u = 0; u < count; u++) {
    const first = units[212 * u]
    const fields = [['low', 2 - ((first >> 6) & 3), 2], ['mid', 2 - ((first >> 4) & 3), 2], ['high', 3 - ((first >> 2) & 3), 3]]
    for (const [name, mode, other] of fields) {
      if (mode !== 0 && mode !== other) {
        const where = channels.length === 2 ? `frame ${u >> 1}, channel ${u & 1}` : `frame ${u}`
        throw new TypeError(`units: ${where}: ${name} block mode of the unit is ${mode}, not 0 or ${other}`)
      }
    }
  }
  return count
}

export function measureUnits(channels, units, options = {}, ctx = context()) {
  if (options === null || typeof options !== 'object') throw new TypeError('options must be an object { masking, haloFrames, thresholdFrom }')
  const haloFrames = options.haloFrames === undefined ? 0 : options.haloFrames
  const thresholdFrom = options.thresholdFrom === undefined ? 'own' : options.thresholdFrom
  if (thresholdFrom !== 'own' && thresholdFrom !== 'long') throw new TypeError(`thresholdFrom must be 'own' or 'long', got ${String(thresholdFrom)}`)
  const noMasking = options.masking === null || options.masking === undefined
  if (thresholdFrom === 'long' && noMasking) throw new TypeError("thresholdFrom 'long' needs masking")
  checkMeasuredUnits(channels, units, haloFrames)
  const tables = noMasking ? null : checkMasking(options.masking)
  const call = thresholdFrom === 'long' ? native().measureUnitsShared : native().measureUnits
  return call(ctx, channels, haloFrames, units, tables ? tables.floor : null, tables ? tables.spread : null)
}

// c1_measure_pcm_batch on the default context: the error of the decoded PCM of sound units against the PCM they were made from,
// per unit and per 32-sample segment.  channels: one or two Float32Arrays of (haloFrames + frames) * 512 samples; units:
// Uint8Array of (haloUnits + frames) * channels * 212 bytes (frame-major, channels interleaved), the unit(s) of frame -1 first
// when haloUnits is 1 (the decoder starts from a fresh pool otherwise); any bytes are units to the decoder.  options:
// { haloFrames: 0 .. 2, haloUnits: 0 or 1 }.  With y the exact decode of the units and x the input PCM_DELAY = 266 samples
// earlier (zero before the history given), returns { noise, signal: Float64Array(frames * channels * 16), the sums of (y - x)^2
// and of x^2 over the samples 32 s .. 32 s + 31 of every unit's frame, totals: Float64Array(frames * channels * 2), their sums
// over the sixteen segments }.  Arguments that break these rules are a TypeError naming the argument, raised before any native call.
export const PCM_DELAY = 266
export function measurePcm(channels, units, options = {}, ctx = context()) {
  if (options === null || typeof options !== 'object') throw new TypeError('options must be an object { haloFrames, haloUnits }')
  const haloFrames = options.haloFrames === undefined ? 0 : options.haloFrames
  const haloUnits = options.haloUnits === undefined ? 0 : options.haloUnits
  if (!Array.isArray(channels) || channels.length < 1 || channels.length > 2 || channels.some((c) => !(c instanceof Float32Array))) {
    throw new TypeError('channels must be an array of one or two Float32Array')
  }
  if (!Number.isInteger(haloFrames) || haloFrames < 0 || haloFrames > 2) throw new TypeError(`haloFrames must be 0, 1 or 2, got ${haloFrames}`)
  if (haloUnits !== 0 && haloUnits !== 1) throw new TypeError(`haloUnits must be 0 or 1, got ${haloUnits}`)
  const samples = channels[0].length
  if (channels.some((c) => c.length !== samples) || samples % 512 || samples / 512 < haloFrames) {
    throw new TypeError('channels must have equal length, a multiple of 512 that covers haloFrames')
  }
  const count = (samples / 512 - haloFrames + haloUnits) * channels.length
  if (!(units instanceof Uint8Array)) throw new TypeError('units must be a Uint8Array')
  if (units.length !== count * 212) {
    throw new TypeError(`units must hold (haloUnits + frames) * channels = ${count} sound units of 212 bytes, got ${units.length} bytes`)
  }
  return native().measurePcm(ctx, channels, haloFrames, units, haloUnits)
}
