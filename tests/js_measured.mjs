// encodeMeasured(channels, options, modes) and encodeAeaPcm(channels, { measuredAllocation: true }) (carta1_amd/js/native.js,
// io/processor.js -> c1_encode_measured_batch) against what the Python host got for the same PCM.
// argv[2]: a directory with ch0.f32, ch1.f32 (raw float32), modes.u8 (one mode byte per unit) and, from the Python host,
// units.u8, taken.u8, dist.f64, energy.f64 (under detection) and units_m.u8, taken_m.u8, dist_m.f64, energy_m.f64 (under the
// given modes), written by tests/test_js_measured.py.  Prints ALL OK on success.
import fs from 'fs'
import path from 'path'

import { encodeAeaPcm, encodeMeasured, EncoderOptions } from '../carta1_amd/js/index.js'

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
  const modes = u8('modes.u8')
  const frames = chs[0].length / 512, units = frames * 2
  const options = new EncoderOptions().toNative()
  for (const [given, tag] of [[null, ''], [modes, '_m']]) {
    const got = encodeMeasured(chs, options, given)
    ok(got.units instanceof Uint8Array && got.units.length === units * 212, `units${tag} is a Uint8Array of one unit per frame and channel`)
    ok(got.taken instanceof Uint8Array && got.taken.length === units, `taken${tag} is one byte per unit`)
    ok(got.distortion instanceof Float64Array && got.distortion.length === units * 2, `distortion${tag} is units * 2 doubles`)
    ok(got.energy instanceof Float64Array && got.energy.length === units, `energy${tag} is units doubles`)
    ok(bytes(got.units).equals(bytes(u8(`units${tag}.u8`))), `units${tag} == the Python result`)
    ok(bytes(got.taken).equals(bytes(u8(`taken${tag}.u8`))), `taken${tag} == the Python result`)
    ok(bytes(got.distortion).equals(bytes(f64(`dist${tag}.f64`))), `distortion${tag} == the Python result, bit for bit`)
    ok(bytes(got.energy).equals(bytes(f64(`energy${tag}.f64`))), `energy${tag} == the Python result, bit for bit`)
    ok(got.taken.every((t) => t === 0 || t === 1) && got.taken.some((t) => t === 1), `taken${tag} is 0 or 1, and 1 somewhere`)
    ok(got.taken.every((t, u) => (t ? got.distortion[2 * u + 1] < got.distortion[2 * u] : true)), `taken${tag} only where the error is smaller`)

    const image = await encodeAeaPcm(chs, given ? { measuredAllocation: true, blockModes: given } : { measuredAllocation: true })
    ok(image.length === 2048 + units * 212, 'the image has a header and one unit per frame and channel')
    const plain = await encodeAeaPcm(chs, given ? { blockModes: given } : {})
    ok(bytes(image.subarray(0, 2048)).equals(bytes(plain.subarray(0, 2048))), 'the header is the one encodeAeaPcm writes')
    ok(bytes(image.subarray(2048)).equals(bytes(got.units)), `the body is encodeMeasured's units${tag}`)
    for (let u = 0; u < units; u++) {
      const a = 2048 + u * 212
      const equal = bytes(image.subarray(a, a + 212)).equals(bytes(plain.subarray(a, a + 212)))
      if (equal !== (got.taken[u] === 0)) { ok(false, `unit ${u}${tag}: taken ${got.taken[u]} but the bytes ${equal ? 'equal' : 'differ from'} the plain encode's`); break }
    }
    const off = await encodeAeaPcm(chs, given ? { measuredAllocation: false, blockModes: given } : { measuredAllocation: false })
    ok(bytes(off).equals(bytes(plain)), 'measuredAllocation: false is the plain encode')
  }

  await rejects(() => encodeAeaPcm(chs, { measuredAllocation: true, allocationBiases: new Float64Array(frames).fill(1) }), TypeError,
    ['measuredAllocation', 'allocationBiases', 'mutually exclusive'], 'allocationBiases too')
  await rejects(() => encodeAeaPcm(chs, { measuredAllocation: true, allocationBiasCandidates: [1, 2] }), TypeError,
    ['measuredAllocation', 'allocationBiasCandidates', 'mutually exclusive'], 'allocationBiasCandidates too')
  await rejects(() => encodeAeaPcm(chs, { measuredAllocation: true, blockModeCandidates: [0, 58] }), TypeError,
    ['measuredAllocation', 'blockModeCandidates', 'mutually exclusive'], 'blockModeCandidates too')
  await rejects(() => encodeAeaPcm(chs, { measuredAllocation: 1 }), TypeError, ['measuredAllocation', 'boolean'], 'not a boolean')
  await rejects(() => encodeAeaPcm(chs, { measuredAllocation: true, blockModes: new Uint8Array(3) }), TypeError, ['blockModes'], 'blockModes of the wrong length')
  const bad = Uint8Array.from(modes)
  bad[5] = 1
  await rejects(() => encodeAeaPcm(chs, { measuredAllocation: true, blockModes: bad }), Error, ['frame 2, channel 1', 'low field'], 'a mode byte outside the domain')

  if (failures) { console.log(`${failures} FAILURES`); process.exit(1) }
  console.log('ALL OK')
}

main().catch((e) => { console.log('ERROR', e && e.stack ? e.stack : e); process.exit(1) })
