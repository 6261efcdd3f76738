// encodeBestModes(channels, options, candidates) and encodeAeaPcm(channels, { blockModeCandidates }) (carta1_amd/js/native.js,
// io/processor.js -> c1_encode_best_modes_batch) against what the Python host got for the same PCM and candidates.
// argv[2]: a directory with ch0.f32, ch1.f32 (raw float32), cand.u8 (the candidates), units.u8, choice.u8, modes.u8, dist.f64,
// energy.f64 and units_const10.u8 (encode_modes under the constant byte 10), written by tests/test_js_best_modes.py.
// Prints ALL OK on success.
import fs from 'fs'
import path from 'path'

import { encodeAeaPcm, encodeBestModes, EncoderOptions } from '../carta1_amd/js/index.js'

const dir = process.argv[2]
const raw = (name) => { const b = fs.readFileSync(path.join(dir, name)); return b.buffer.slice(b.byteOffset, b.byteOffset + b.length) }
const f32 = (name) => new Float32Array(raw(name))
const f64 = (name) => new Float64Array(raw(name))
const u8 = (name) => new Uint8Array(fs.readFileSync(path.join(dir, name)))
const bytes = (a) => Buffer.from(a.buffer, a.byteOffset, a.byteLength)

let failures = 0
function ok(cond, msg) { if (!cond) { failures++; console.log('FAIL', msg) } }
async function rejects(fn, type, needles, msg) {
  let err = null
  try { await fn() } catch (e) { err = e }
  ok(err instanceof type && needles.every((n) => String(err.message).includes(n)), `${msg}: expected ${type.name} naming ${needles}, got ${err}`)
}

async function main() {
  const chs = [f32('ch0.f32'), f32('ch1.f32')]
  const cand = u8('cand.u8')
  const frames = chs[0].length / 512, units = frames * 2, n = cand.length
  const options = new EncoderOptions().toNative()
  const got = encodeBestModes(chs, options, cand)
  ok(got.units instanceof Uint8Array && got.units.length === units * 212, 'units is a Uint8Array of one unit per frame and channel')
  ok(got.choice instanceof Uint8Array && got.choice.length === units, 'choice is one byte per unit')
  ok(got.modes instanceof Uint8Array && got.modes.length === units, 'modes is one byte per unit')
  ok(got.distortion instanceof Float64Array && got.distortion.length === units * n, 'distortion is units * n doubles')
  ok(got.energy instanceof Float64Array && got.energy.length === units * n, 'energy is units * n doubles')
  ok(bytes(got.units).equals(bytes(u8('units.u8'))), 'units == the Python result')
  ok(bytes(got.choice).equals(bytes(u8('choice.u8'))), 'choice == the Python result')
  ok(bytes(got.modes).equals(bytes(u8('modes.u8'))), 'modes == the Python result')
  ok(bytes(got.distortion).equals(bytes(f64('dist.f64'))), 'distortion == the Python result, bit for bit')
  ok(bytes(got.energy).equals(bytes(f64('energy.f64'))), 'energy == the Python result, bit for bit')
  ok(new Set(got.choice).size >= 4, 'at least four candidates win somewhere')
  ok(got.modes.every((m, u) => m === cand[got.choice[u]]), 'modes == candidates[choice]')
  const triples = Array.from(cand, (b) => [b & 3, (b >> 2) & 3, (b >> 4) & 3])
  ok(bytes(encodeBestModes(chs, options, triples).units).equals(bytes(got.units)), 'triples == mode bytes')

  const image = await encodeAeaPcm(chs, { blockModeCandidates: Array.from(cand) })
  ok(image.length === 2048 + units * 212, 'the image has a header and one unit per frame and channel')
  const plain = await encodeAeaPcm(chs, {})
  ok(bytes(image.subarray(0, 2048)).equals(bytes(plain.subarray(0, 2048))), 'the header is the one encodeAeaPcm writes')
  ok(bytes(image.subarray(2048)).equals(bytes(got.units)), 'the body is encodeBestModes\'s units')
  ok(bytes((await encodeAeaPcm(chs, { blockModeCandidates: cand })).subarray(2048)).equals(bytes(got.units)), 'a Uint8Array of candidates == the array')
  const given = await encodeAeaPcm(chs, { blockModes: got.modes })
  ok(bytes(given).equals(bytes(image)), 'the image == encodeAeaPcm under the chosen blockModes')
  const one = await encodeAeaPcm(chs, { blockModeCandidates: [10] })
  ok(bytes(one.subarray(2048)).equals(bytes(u8('units_const10.u8'))), 'one candidate == that byte on every frame')

  const sched = new Uint8Array(units)
  await rejects(() => encodeAeaPcm(chs, { blockModeCandidates: [0, 58], blockModes: sched }), TypeError,
    ['blockModes', 'blockModeCandidates', 'mutually exclusive'], 'blockModes too')
  await rejects(() => encodeAeaPcm(chs, { blockModeCandidates: [0, 58], allocationBiasCandidates: [1, 2] }), TypeError,
    ['blockModeCandidates', 'allocationBiasCandidates', 'mutually exclusive'], 'allocationBiasCandidates too')
  await rejects(() => encodeAeaPcm(chs, { blockModeCandidates: [] }), RangeError, ['1 to 8'], 'no candidate')
  await rejects(() => encodeAeaPcm(chs, { blockModeCandidates: [0, 2, 8, 10, 48, 50, 56, 58, 0] }), RangeError, ['1 to 8'], 'nine candidates')
  await rejects(() => encodeAeaPcm(chs, { blockModeCandidates: [0, 58, 0] }), Error, ['candidate 2'], 'a candidate given twice')
  await rejects(() => encodeAeaPcm(chs, { blockModeCandidates: [0, 1] }), Error, ['candidate 1', 'low field'], 'a candidate outside the domain')
  await rejects(async () => encodeBestModes(chs, options, [[0, 0]]), TypeError, ['triple'], 'a triple of two')

  if (failures) { console.log(`${failures} FAILURES`); process.exit(1) }
  console.log('ALL OK')
}

main().catch((e) => { console.log('ERROR', e && e.stack ? e.stack : e); process.exit(1) })
