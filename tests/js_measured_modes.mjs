// encodeMeasuredModes(channels, options, candidates, scaleFactorOffsets) and encodeAeaPcm(channels, { measuredAllocation: true,
// measuredModeCandidates }) (carta1_amd/js/native.js, io/processor.js -> c1_encode_measured_modes_batch) against what the Python
// host got for the same PCM, candidates and offsets.
// argv[2]: a directory with cand.u8 and, per tag (_1: 24 mono frames, _2: 24 stereo frames) and per suffix ('': no offsets,
// '_s': the suggested offsets), ch0<tag>.f32, ch1_2.f32 (raw float32) and units, choice, modes, taken (.u8), shifts (.i8), dist
// and energy (.f64) <tag><suffix>, written by tests/test_js_measured_modes.py.  Prints ALL OK on success.
import fs from 'fs'
import path from 'path'

import * as api from '../carta1_amd/js/index.js'

const { encodeAeaPcm, encodeMeasuredModes, encodeMeasured, EncoderOptions, SCALE_FACTOR_OFFSETS } = api
const dir = process.argv[2]
const raw = (name) => { const b = fs.readFileSync(path.join(dir, name)); return b.buffer.slice(b.byteOffset, b.byteOffset + b.length) }
const f32 = (name) => new Float32Array(raw(name))
const u8 = (name) => new Uint8Array(fs.readFileSync(path.join(dir, name)))
const file = (name) => fs.readFileSync(path.join(dir, name))
const bytes = (a) => Buffer.from(a.buffer, a.byteOffset, a.byteLength)

// codec/index.js:26-47 of the reference
const REFERENCE_EXPORTS = ['encode', 'decode', 'qmfAnalysisStage', 'mdctStage', 'serializeFrame', 'deserializeFrame', 'AeaFile', 'AudioProcessor',
  'quantize', 'dequantize', 'FFT', 'BufferPool', 'EncoderOptions', 'pipe', 'WORD_LENGTH_BITS', 'SPECS_PER_BFU', 'SCALE_FACTORS', 'BFU_START_LONG',
  'encodeAeaPcm', 'decodeAeaPcm']

let failures = 0
function ok(cond, msg) { if (!cond) { failures++; console.log('FAIL', msg) } }
async function rejects(fn, type, needles, msg) {
  let err = null
  try { await fn() } catch (e) { err = e }
  ok(err instanceof type && needles.every((n) => String(err.message).includes(n)), `${msg}: expected ${type.name} naming ${needles}, got ${err}`)
}

async function main() {
  ok(REFERENCE_EXPORTS.length === 20 && REFERENCE_EXPORTS.every((n) => api[n] !== undefined), 'the twenty reference names are still exported')
  ok(typeof encodeMeasuredModes === 'function', 'encodeMeasuredModes is exported next to encodeMeasured')
  const cand = u8('cand.u8')
  const n = cand.length
  const options = new EncoderOptions().toNative()
  for (const [tag, nch] of [['_1', 1], ['_2', 2]]) {
    const chs = nch === 1 ? [f32('ch0_1.f32')] : [f32('ch0_2.f32'), f32('ch1_2.f32')]
    const units = (chs[0].length / 512) * nch
    for (const [offsets, suffix] of [[null, ''], [SCALE_FACTOR_OFFSETS, '_s']]) {
      const t = `${nch} channel(s)${suffix}`
      const got = encodeMeasuredModes(chs, options, cand, offsets)
      ok(got.units instanceof Uint8Array && got.units.length === units * 212, `${t}: units is one unit per frame and channel`)
      ok(got.choice instanceof Uint8Array && got.modes instanceof Uint8Array && got.taken instanceof Uint8Array, `${t}: choice, modes and taken are bytes`)
      ok(got.shifts instanceof Int8Array && got.shifts.length === units * 52, `${t}: shifts is 52 offsets per unit`)
      ok(got.distortion instanceof Float64Array && got.distortion.length === units * n * 2, `${t}: distortion is units * n * 2 doubles`)
      ok(got.energy instanceof Float64Array && got.energy.length === units * n, `${t}: energy is units * n doubles`)
      for (const [name, ext] of [['units', 'u8'], ['choice', 'u8'], ['modes', 'u8'], ['taken', 'u8'], ['shifts', 'i8']]) {
        ok(bytes(got[name]).equals(file(`${name}${tag}${suffix}.${ext}`)), `${t}: ${name} == the Python result`)
      }
      ok(bytes(got.distortion).equals(file(`dist${tag}${suffix}.f64`)), `${t}: distortion == the Python result, bit for bit`)
      ok(bytes(got.energy).equals(file(`energy${tag}${suffix}.f64`)), `${t}: energy == the Python result, bit for bit`)
      ok(got.modes.every((m, u) => m === cand[got.choice[u]]), `${t}: modes == candidates[choice]`)
      ok(new Set(got.choice).size >= 2, `${t}: more than one candidate wins somewhere`)
      if (offsets === null) ok(got.shifts.every((v) => v === 0), `${t}: no offsets, no shifts`)
      const under = encodeMeasured(chs, options, got.modes, offsets)
      ok(bytes(under.units).equals(bytes(got.units)) && bytes(under.taken).equals(bytes(got.taken)), `${t}: units and taken == encodeMeasured under the chosen modes`)
      const triples = Array.from(cand, (b) => [b & 3, (b >> 2) & 3, (b >> 4) & 3])
      ok(bytes(encodeMeasuredModes(chs, options, triples, offsets).units).equals(bytes(got.units)), `${t}: triples == mode bytes`)

      const extra = offsets === null ? {} : { scaleFactorOffsets: offsets }
      const image = await encodeAeaPcm(chs, { measuredAllocation: true, measuredModeCandidates: Array.from(cand), ...extra })
      ok(image.length === 2048 + units * 212, `${t}: the image has a header and one unit per frame and channel`)
      const plain = await encodeAeaPcm(chs, {})
      ok(bytes(image.subarray(0, 2048)).equals(bytes(plain.subarray(0, 2048))), `${t}: the header is the one encodeAeaPcm writes`)
      ok(bytes(image.subarray(2048)).equals(bytes(got.units)), `${t}: the body is encodeMeasuredModes's units`)
      ok(bytes((await encodeAeaPcm(chs, { measuredAllocation: true, measuredModeCandidates: cand, ...extra })).subarray(2048)).equals(bytes(got.units)),
        `${t}: a Uint8Array of candidates == the array`)
      const given = await encodeAeaPcm(chs, { measuredAllocation: true, blockModes: got.modes, ...extra })
      ok(bytes(given).equals(bytes(image)), `${t}: the image == encodeAeaPcm with the measured allocation under the chosen blockModes`)
    }
  }

  const chs = [f32('ch0_2.f32'), f32('ch1_2.f32')]
  const sched = new Uint8Array((chs[0].length / 512) * 2)
  const on = { measuredAllocation: true, measuredModeCandidates: [0, 58] }
  await rejects(() => encodeAeaPcm(chs, { measuredModeCandidates: [0, 58] }), TypeError, ['measuredModeCandidates', 'measuredAllocation: true'], 'without measuredAllocation')
  await rejects(() => encodeAeaPcm(chs, { measuredAllocation: false, measuredModeCandidates: [0, 58] }), TypeError, ['measuredModeCandidates', 'measuredAllocation: true'], 'measuredAllocation false')
  await rejects(() => encodeAeaPcm(chs, { ...on, blockModes: sched }), TypeError, ['measuredModeCandidates', 'blockModes', 'mutually exclusive'], 'blockModes too')
  await rejects(() => encodeAeaPcm(chs, { ...on, masking: true }), TypeError, ['measuredModeCandidates', 'masking', 'mutually exclusive'], 'masking too')
  await rejects(() => encodeAeaPcm(chs, { ...on, blockModeCandidates: [0, 58] }), TypeError, ['measuredModeCandidates', 'blockModeCandidates', 'mutually exclusive'], 'blockModeCandidates too')
  await rejects(() => encodeAeaPcm(chs, { measuredAllocation: true, blockModeCandidates: [0, 58] }), TypeError,
    ['measuredAllocation', 'blockModeCandidates', 'mutually exclusive'], 'measuredAllocation with blockModeCandidates stays an error')
  await rejects(() => encodeAeaPcm(chs, { ...on, measuredModeCandidates: [] }), RangeError, ['1 to 8'], 'no candidate')
  await rejects(() => encodeAeaPcm(chs, { ...on, measuredModeCandidates: [0, 2, 8, 10, 48, 50, 56, 58, 0] }), RangeError, ['1 to 8'], 'nine candidates')
  await rejects(() => encodeAeaPcm(chs, { ...on, measuredModeCandidates: [0, 58, 0] }), Error, ['candidate 2'], 'a candidate given twice')
  await rejects(() => encodeAeaPcm(chs, { ...on, measuredModeCandidates: [0, 1] }), Error, ['candidate 1', 'low field'], 'a candidate outside the domain')
  await rejects(() => encodeAeaPcm(chs, { ...on, scaleFactorOffsets: [1, 0] }), TypeError, ['scaleFactorOffsets[0]'], 'offsets that do not start with 0')
  await rejects(async () => encodeMeasuredModes(chs, options, [[0, 0]]), TypeError, ['triple'], 'a triple of two')
  await rejects(async () => encodeMeasuredModes(chs, options, [0, 58], [0, 9]), TypeError, ['scaleFactorOffsets[1]'], 'an offset out of range')

  if (failures) { console.log(`${failures} FAILURES`); process.exit(1) }
  console.log('ALL OK')
}

main().catch((e) => { console.log('ERROR', e && e.stack ? e.stack : e); process.exit(1) })
