// encodeBestBias(channels, optionSets, modes) and encodeAeaPcm(channels, { allocationBiasCandidates }) (carta1_amd/js/native.js,
// io/processor.js -> c1_encode_best_bias_batch) against what the Python host got for the same PCM, candidates and modes.
// argv[2]: a directory with ch0.f32, ch1.f32 (raw float32), cand.f64 (the candidates), modes.u8, and per case (`m` with the mode
// bytes, `d` under detection) units_X.u8, choice_X.u8, dist_X.f64, energy_X.f64, written by tests/test_js_best_bias.py.
// Prints ALL OK on success.
import fs from 'fs'
import path from 'path'

import { encodeAeaPcm, encodeBestBias, EncoderOptions } from '../carta1_amd/js/index.js'

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
  const cand = f64('cand.f64'), modes = u8('modes.u8')
  const frames = chs[0].length / 512, units = frames * 2, n = cand.length
  const sets = Array.from(cand, (b) => new EncoderOptions({ allocationBias: b }).toNative())
  for (const [tag, m] of [['m', modes], ['d', null]]) {
    const got = encodeBestBias(chs, sets, m)
    ok(got.units instanceof Uint8Array && got.units.length === units * 212, `${tag}: units is a Uint8Array of one unit per frame and channel`)
    ok(got.choice instanceof Uint8Array && got.choice.length === units, `${tag}: choice is one byte per unit`)
    ok(got.distortion instanceof Float64Array && got.distortion.length === units * n, `${tag}: distortion is units * n doubles`)
    ok(got.energy instanceof Float64Array && got.energy.length === units, `${tag}: energy is one double per unit`)
    ok(bytes(got.units).equals(bytes(u8(`units_${tag}.u8`))), `${tag}: units == the Python result`)
    ok(bytes(got.choice).equals(bytes(u8(`choice_${tag}.u8`))), `${tag}: choice == the Python result`)
    ok(bytes(got.distortion).equals(bytes(f64(`dist_${tag}.f64`))), `${tag}: distortion == the Python result, bit for bit`)
    ok(bytes(got.energy).equals(bytes(f64(`energy_${tag}.f64`))), `${tag}: energy == the Python result, bit for bit`)
    ok(new Set(got.choice).size >= 3, `${tag}: at least three candidates win somewhere`)
    const flat = new Float64Array(68 * n)
    sets.forEach((s, k) => flat.set(s, 68 * k))
    ok(bytes(encodeBestBias(chs, flat, m).units).equals(bytes(got.units)), `${tag}: one Float64Array(68 * n) == the array of sets`)

    const image = await encodeAeaPcm(chs, m ? { allocationBiasCandidates: Array.from(cand), blockModes: m } : { allocationBiasCandidates: cand })
    ok(image.length === 2048 + units * 212, `${tag}: the image has a header and one unit per frame and channel`)
    const plain = await encodeAeaPcm(chs, m ? { blockModes: m } : {})
    ok(bytes(image.subarray(0, 2048)).equals(bytes(plain.subarray(0, 2048))), `${tag}: the header is the one encodeAeaPcm writes`)
    ok(bytes(image.subarray(2048)).equals(bytes(got.units)), `${tag}: the body is encodeBestBias's units`)
    ok(!bytes(image.subarray(2048)).equals(bytes(plain.subarray(2048))), `${tag}: the choice is not always the default bias`)
  }
  const one = await encodeAeaPcm(chs, { allocationBiasCandidates: [2] })
  ok(bytes(one).equals(bytes(await encodeAeaPcm(chs, { allocationBias: 2 }))), 'one candidate == allocationBias')

  const sched = new Float64Array(frames).fill(1)
  await rejects(() => encodeAeaPcm(chs, { allocationBiasCandidates: [1, 2], allocationBiases: sched }), TypeError,
    ['allocationBiases', 'allocationBiasCandidates'], 'both options')
  await rejects(() => encodeAeaPcm(chs, { allocationBiasCandidates: [0, 0.5, 1, 1.5, 2, 2.5, 3, 3.5, 4] }), RangeError, ['1 to 8'], 'nine candidates')
  await rejects(() => encodeAeaPcm(chs, { allocationBiasCandidates: [] }), RangeError, ['1 to 8'], 'no candidate')
  await rejects(() => encodeAeaPcm(chs, { allocationBiasCandidates: [1, 2, 1] }), RangeError, ['distinct'], 'a candidate given twice')
  await rejects(() => encodeAeaPcm(chs, { allocationBiasCandidates: [1, 5.5] }), Error, ['allocationBias'], 'a candidate outside allocationBias\'s range')
  await rejects(async () => encodeBestBias(chs, [new Float64Array(67)], null), TypeError, ['toNative'], 'an option set of the wrong size')

  if (failures) { console.log(`${failures} FAILURES`); process.exit(1) }
  console.log('ALL OK')
}

main().catch((e) => { console.log('ERROR', e && e.stack ? e.stack : e); process.exit(1) })
