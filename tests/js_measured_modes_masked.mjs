// encodeMeasuredModesMasked(channels, options, candidates, scaleFactorOffsets, masking), encodeAeaPcm(channels, { measuredAllocation:
// true, measuredModeCandidates, modeSearchMasking }) and the encode(options, bufferPool, measured) frame closure with
// modeSearchMasking (carta1_amd/js/native.js, io/processor.js, pipeline/encoder.js -> c1_encode_measured_modes_masked_batch,
// c1_enc_stream_push_measured_modes_masked) against what the Python host got for the same PCM, candidates, offsets and tables.
// argv[2]: a directory with cand.u8, floor_x.f64, spread_x.f64 and, per tag (_1: 24 mono frames, _2: 24 stereo frames),
// ch0<tag>.f32, ch1_2.f32 (raw float32), stream_units<tag>.u8 and stream_modes<tag>.u8 (a frame per push, the suggested offsets,
// the packaged tables) and, per suffix ('': no offsets, '_s': the suggested offsets, both with the packaged tables; '_x': the
// offsets and the explicit tables), units, choice, modes, taken (.u8), shifts (.i8), dist, energy and weights (.f64)
// <tag><suffix>, written by tests/test_js_measured_modes_masked.py.  Prints ALL OK on success.
import fs from 'fs'
import path from 'path'

import * as api from '../carta1_amd/js/index.js'

const { encode, serializeFrame, BufferPool, encodeAeaPcm, encodeMeasuredModes, encodeMeasuredModesMasked, encodeMeasured, EncoderOptions, SCALE_FACTOR_OFFSETS, MASKING_DEFAULT } = api
const dir = process.argv[2]
const raw = (name) => { const b = fs.readFileSync(path.join(dir, name)); return b.buffer.slice(b.byteOffset, b.byteOffset + b.length) }
const f32 = (name) => new Float32Array(raw(name))
const f64 = (name) => new Float64Array(raw(name))
const u8 = (name) => new Uint8Array(fs.readFileSync(path.join(dir, name)))
const file = (name) => fs.readFileSync(path.join(dir, name))
const bytes = (a) => Buffer.from(a.buffer, a.byteOffset, a.byteLength)

let failures = 0
function ok(cond, msg) { if (!cond) { failures++; console.log('FAIL', msg) } }
async function rejects(fn, type, needles, msg) {
  let err = null
  try { await fn() } catch (e) { err = e }
  ok(err instanceof type && needles.every((n) => String(err.message).includes(n)), `${msg}: expected ${type.name} naming ${needles}, got ${err}`)
}

async function main() {
  ok(typeof encodeMeasuredModesMasked === 'function', 'encodeMeasuredModesMasked is exported next to encodeMeasuredModes')
  const cand = u8('cand.u8')
  const n = cand.length
  const options = new EncoderOptions().toNative()
  const explicit = { floor: f64('floor_x.f64'), spread: f64('spread_x.f64') }
  for (const [tag, nch] of [['_1', 1], ['_2', 2]]) {
    const chs = nch === 1 ? [f32('ch0_1.f32')] : [f32('ch0_2.f32'), f32('ch1_2.f32')]
    const frames = chs[0].length / 512
    const units = frames * nch
    for (const [offsets, masking, suffix] of [[null, true, ''], [SCALE_FACTOR_OFFSETS, true, '_s'], [SCALE_FACTOR_OFFSETS, explicit, '_x']]) {
      const t = `${nch} channel(s)${suffix}`
      const got = encodeMeasuredModesMasked(chs, options, cand, offsets, masking)
      ok(got.units instanceof Uint8Array && got.units.length === units * 212, `${t}: units is one unit per frame and channel`)
      ok(got.shifts instanceof Int8Array && got.shifts.length === units * 52, `${t}: shifts is 52 offsets per unit`)
      ok(got.distortion instanceof Float64Array && got.distortion.length === units * n * 2, `${t}: distortion is units * n * 2 doubles`)
      ok(got.energy instanceof Float64Array && got.energy.length === units * n, `${t}: energy is units * n doubles`)
      ok(got.weights instanceof Float64Array && got.weights.length === units * 52, `${t}: weights is 52 doubles per unit`)
      for (const [name, ext] of [['units', 'u8'], ['choice', 'u8'], ['modes', 'u8'], ['taken', 'u8'], ['shifts', 'i8']]) {
        ok(bytes(got[name]).equals(file(`${name}${tag}${suffix}.${ext}`)), `${t}: ${name} == the Python result`)
      }
      ok(bytes(got.distortion).equals(file(`dist${tag}${suffix}.f64`)), `${t}: distortion == the Python result, bit for bit`)
      ok(bytes(got.energy).equals(file(`energy${tag}${suffix}.f64`)), `${t}: energy == the Python result, bit for bit`)
      ok(bytes(got.weights).equals(file(`weights${tag}${suffix}.f64`)), `${t}: weights == the Python result, bit for bit`)
      ok(got.modes.every((m, u) => m === cand[got.choice[u]]), `${t}: modes == candidates[choice]`)
      ok(!bytes(got.choice).equals(bytes(encodeMeasuredModes(chs, options, cand, offsets).choice)), `${t}: the weights change the choice`)
      // the weights are those of the masked allocation under all-long modes, whatever the candidates
      const long = encodeMeasured(chs, options, new Uint8Array(units), offsets, masking)
      ok(bytes(long.weights).equals(bytes(got.weights)), `${t}: weights == encodeMeasured's under all-long modes`)
      ok(bytes(encodeMeasuredModesMasked(chs, options, [58], offsets, masking).weights).equals(bytes(got.weights)), `${t}: weights do not depend on the candidates`)
      const triples = Array.from(cand, (b) => [b & 3, (b >> 2) & 3, (b >> 4) & 3])
      ok(bytes(encodeMeasuredModesMasked(chs, options, triples, offsets, masking).units).equals(bytes(got.units)), `${t}: triples == mode bytes`)
      if (masking === true) {
        ok(bytes(encodeMeasuredModesMasked(chs, options, cand, offsets, { floor: MASKING_DEFAULT.floor, spread: MASKING_DEFAULT.spread }).units).equals(bytes(got.units)),
          `${t}: true == the packaged tables`)
      }

      const extra = offsets === null ? {} : { scaleFactorOffsets: offsets }
      const image = await encodeAeaPcm(chs, { measuredAllocation: true, measuredModeCandidates: Array.from(cand), modeSearchMasking: masking, ...extra })
      ok(image.length === 2048 + units * 212, `${t}: the image has a header and one unit per frame and channel`)
      const plain = await encodeAeaPcm(chs, {})
      ok(bytes(image.subarray(0, 2048)).equals(bytes(plain.subarray(0, 2048))), `${t}: the header is the one encodeAeaPcm writes`)
      ok(bytes(image.subarray(2048)).equals(bytes(got.units)), `${t}: the body is encodeMeasuredModesMasked's units`)
      const unweighted = await encodeAeaPcm(chs, { measuredAllocation: true, measuredModeCandidates: Array.from(cand), modeSearchMasking: false, ...extra })
      ok(bytes(unweighted.subarray(2048)).equals(bytes(encodeMeasuredModes(chs, options, cand, offsets).units)), `${t}: modeSearchMasking false is the unweighted search`)
    }

    // the frame closure, a pool per channel, against the Python stream pushed a frame at a time
    const want = u8(`stream_units${tag}.u8`)
    const modes = u8(`stream_modes${tag}.u8`)
    const how = { measuredAllocation: true, measuredModeCandidates: Array.from(cand), scaleFactorOffsets: SCALE_FACTOR_OFFSETS, modeSearchMasking: true }
    const encoders = chs.map(() => encode(new EncoderOptions(), new BufferPool(), how))
    const parts = []
    for (let f = 0; f < frames; f++) {
      for (let c = 0; c < nch; c++) {
        const fields = encoders[c](chs[c].slice(f * 512, (f + 1) * 512))
        const byte = fields.blockModes[0] | (fields.blockModes[1] << 2) | (fields.blockModes[2] << 4)
        ok(byte === modes[f * nch + c], `${nch} channel(s), frame ${f}, channel ${c}: blockModes are the unit's`)
        parts.push(Buffer.from(serializeFrame(fields)))
      }
    }
    ok(Buffer.concat(parts).equals(bytes(want)), `${nch} channel(s): the closure's serialised fields == the Python stream's units`)
    ok(bytes(want).equals(file(`units${tag}_s.u8`)), `${nch} channel(s): the stream's units == the whole-buffer call's`)
  }

  const chs = [f32('ch0_2.f32'), f32('ch1_2.f32')]
  const on = { measuredAllocation: true, measuredModeCandidates: [0, 58] }
  await rejects(() => encodeAeaPcm(chs, { modeSearchMasking: true }), TypeError, ['modeSearchMasking', 'measuredAllocation: true', 'measuredModeCandidates'], 'alone')
  await rejects(() => encodeAeaPcm(chs, { measuredModeCandidates: [0, 58], modeSearchMasking: true }), TypeError, ['measuredAllocation: true'], 'without measuredAllocation')
  await rejects(() => encodeAeaPcm(chs, { measuredAllocation: true, modeSearchMasking: true }), TypeError, ['modeSearchMasking', 'measuredModeCandidates'], 'without candidates')
  await rejects(() => encodeAeaPcm(chs, { measuredAllocation: true, masking: true, modeSearchMasking: true }), TypeError, ['modeSearchMasking', 'measuredModeCandidates'], 'with masking, without candidates')
  await rejects(() => encodeAeaPcm(chs, { ...on, modeSearchMasking: { floor: [1, 2] } }), TypeError, ['masking.floor', '52'], 'a short floor')
  await rejects(() => encodeAeaPcm(chs, { ...on, modeSearchMasking: 3 }), TypeError, ['masking must be true or'], 'a number')
  await rejects(() => encodeAeaPcm(chs, { ...on, modeSearchMasking: { floor: new Float64Array(52) } }), TypeError, ['masking.floor[0] = 0'], 'a zero floor')
  // `masking` keeps meaning "thresholds from the unit's own modes": with the candidates it stays the TypeError it was
  await rejects(() => encodeAeaPcm(chs, { ...on, masking: true }), TypeError, ['measuredModeCandidates and masking are mutually exclusive'], 'masking with candidates')
  await rejects(() => encodeAeaPcm(chs, { ...on, masking: true, modeSearchMasking: true }), TypeError, ['measuredModeCandidates and masking are mutually exclusive'], 'both maskings')
  await rejects(async () => encodeMeasuredModesMasked(chs, options, [0, 58], null, null), TypeError, ['needs masking'], 'no tables')
  await rejects(async () => encodeMeasuredModesMasked(chs, options, [0, 58], [0, 9], true), TypeError, ['scaleFactorOffsets[1]'], 'an offset out of range')
  await rejects(async () => encodeMeasuredModesMasked(chs, options, [0, 58, 0], null, true), Error, ['candidate 2'], 'a candidate given twice')
  // the closure: the same TypeErrors, before anything changes
  const pool = new BufferPool()
  const wrong = { measuredAllocation: true, modeSearchMasking: true }
  const enc = encode(new EncoderOptions(), pool, wrong)
  const frame0 = chs[0].slice(0, 512)
  await rejects(async () => enc(frame0), TypeError, ['modeSearchMasking', 'measuredModeCandidates'], 'closure without candidates')
  delete wrong.measuredAllocation
  wrong.measuredModeCandidates = [0, 58]
  await rejects(async () => enc(frame0), TypeError, ['measuredAllocation: true'], 'closure without measuredAllocation')
  Object.assign(wrong, { measuredAllocation: true, masking: true })
  await rejects(async () => enc(frame0), TypeError, ['measuredModeCandidates and masking are mutually exclusive'], 'closure with masking and candidates')
  delete wrong.masking
  Object.assign(wrong, { measuredModeCandidates: Array.from(cand), scaleFactorOffsets: SCALE_FACTOR_OFFSETS })
  ok(Buffer.from(serializeFrame(enc(frame0))).equals(bytes(u8('stream_units_2.u8').subarray(0, 212))), 'after the errors the pool encodes its first frame as a fresh one')

  if (failures) { console.log(`${failures} FAILURES`); process.exit(1) }
  console.log('ALL OK')
}

main().catch((e) => { console.log('ERROR', e && e.stack ? e.stack : e); process.exit(1) })
