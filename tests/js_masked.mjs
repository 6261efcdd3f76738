// encodeMeasured(channels, options, modes, scaleFactorOffsets, masking) and encodeAeaPcm(channels, { measuredAllocation: true,
// masking }) (carta1_amd/js/native.js, io/processor.js -> c1_encode_measured_masked_batch) against what the Python host got for
// the same PCM.
// argv[2]: a directory with ch0.f32, ch1.f32 (raw float32), modes.u8 (one mode byte per unit), floor.f64 and spread.f64 (the
// packaged tables as the Python host read them) and, from the Python host, units.u8, taken.u8, shifts.i8, dist.f64, energy.f64,
// weights.f64 (packaged tables, detection), the same with _m (packaged tables, the given modes) and with _s (floor =
// SPECS_PER_BFU without a spread, the given modes, no offsets), written by tests/test_js_masked.py.  Prints ALL OK on success.
import fs from 'fs'
import path from 'path'

import { encodeAeaPcm, encodeMeasured, EncoderOptions, SCALE_FACTOR_OFFSETS, MASKING_DEFAULT, SPECS_PER_BFU, decode, decodeAeaPcm } from '../carta1_amd/js/index.js'

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
  ok(MASKING_DEFAULT.floor instanceof Float64Array && MASKING_DEFAULT.floor.length === 52 && bytes(MASKING_DEFAULT.floor).equals(bytes(f64('floor.f64'))),
    'MASKING_DEFAULT.floor is the JSON, bit for bit as the Python host read it')
  ok(MASKING_DEFAULT.spread instanceof Float64Array && MASKING_DEFAULT.spread.length === 52 * 52 && bytes(MASKING_DEFAULT.spread).equals(bytes(f64('spread.f64'))),
    'MASKING_DEFAULT.spread is the JSON, row-major, bit for bit as the Python host read it')
  const specs = { floor: Array.from(SPECS_PER_BFU), spread: null }
  for (const [given, offsets, masking, tag] of [[null, SCALE_FACTOR_OFFSETS, true, ''], [modes, SCALE_FACTOR_OFFSETS, true, '_m'], [modes, null, specs, '_s']]) {
    const got = encodeMeasured(chs, options, given, offsets, masking)
    ok(got.units instanceof Uint8Array && got.units.length === units * 212, `units${tag} is a Uint8Array of one unit per frame and channel`)
    ok(got.weights instanceof Float64Array && got.weights.length === units * 52, `weights${tag} is 52 doubles per unit`)
    ok(bytes(got.units).equals(bytes(u8(`units${tag}.u8`))), `units${tag} == the Python result`)
    ok(bytes(got.taken).equals(bytes(u8(`taken${tag}.u8`))), `taken${tag} == the Python result`)
    ok(bytes(got.shifts).equals(bytes(u8(`shifts${tag}.i8`))), `shifts${tag} == the Python result`)
    ok(bytes(got.distortion).equals(bytes(f64(`dist${tag}.f64`))), `distortion${tag} == the Python result, bit for bit`)
    ok(bytes(got.energy).equals(bytes(f64(`energy${tag}.f64`))), `energy${tag} == the Python result, bit for bit`)
    ok(bytes(got.weights).equals(bytes(f64(`weights${tag}.f64`))), `weights${tag} == the Python result, bit for bit`)
    ok(got.taken.some((t) => t === 1), `taken${tag} is set somewhere`)

    const extra = { ...(given ? { blockModes: given } : {}), ...(offsets ? { scaleFactorOffsets: offsets } : {}) }
    const image = await encodeAeaPcm(chs, { measuredAllocation: true, masking, ...extra })
    ok(image.length === 2048 + units * 212, 'the image has a header and one unit per frame and channel')
    ok(bytes(image.subarray(2048)).equals(bytes(got.units)), `the body is encodeMeasured's units${tag}`)

    // the project's own decode() of the units is finite: the closure on the left channel's first frames, one unit a call, and
    // (once) decodeAeaPcm on the whole image
    const decoder = decode()
    let finite = true
    for (let f = 0; f < 16 && f < frames && finite; f++) {
      const pcm = decoder(got.units.subarray(2 * f * 212, (2 * f + 1) * 212))
      finite = pcm.length === 512 && pcm.every((v) => Number.isFinite(v))
    }
    if (tag === '') {
      const pcm = await decodeAeaPcm(image)
      finite = finite && pcm.length === 2 && pcm.every((c) => c.length >= frames * 512 && c.every((v) => Number.isFinite(v)))
    }
    ok(finite, `decode() of the units${tag} is finite`)
  }

  // the packaged tables spelled out, and rows instead of a flat matrix, are `true`
  const viaTrue = encodeMeasured(chs, options, modes, SCALE_FACTOR_OFFSETS, true)
  const rowsOf = Array.from({ length: 52 }, (_, b) => Array.from(MASKING_DEFAULT.spread.subarray(52 * b, 52 * b + 52)))
  for (const masking of [MASKING_DEFAULT, { floor: MASKING_DEFAULT.floor, spread: rowsOf }]) {
    const again = encodeMeasured(chs, options, modes, SCALE_FACTOR_OFFSETS, masking)
    ok(bytes(again.units).equals(bytes(viaTrue.units)) && bytes(again.weights).equals(bytes(viaTrue.weights)), 'MASKING_DEFAULT spelled out is masking: true')
  }
  // flat tables are the call without masking
  const flat = encodeMeasured(chs, options, modes, SCALE_FACTOR_OFFSETS, { floor: new Array(52).fill(1), spread: null })
  const plain = encodeMeasured(chs, options, modes, SCALE_FACTOR_OFFSETS)
  ok(bytes(flat.units).equals(bytes(plain.units)) && bytes(flat.taken).equals(bytes(plain.taken)) && bytes(flat.shifts).equals(bytes(plain.shifts)) &&
     bytes(flat.distortion).equals(bytes(plain.distortion)) && bytes(flat.energy).equals(bytes(plain.energy)) &&
     flat.weights.every((w) => w === 1) && plain.weights === undefined, 'flat tables are encodeMeasured without masking')

  const floorWith = (b, v) => { const f = Array.from(MASKING_DEFAULT.floor); f[b] = v; return { floor: f, spread: null } }
  const spreadWith = (i, v) => { const s = Array.from(MASKING_DEFAULT.spread); s[i] = v; return { floor: MASKING_DEFAULT.floor, spread: s } }
  const bad = [[floorWith(3, 0), ['masking.floor[3]']], [floorWith(0, -1), ['masking.floor[0]']], [floorWith(51, NaN), ['masking.floor[51]']],
    [floorWith(7, Infinity), ['masking.floor[7]']], [floorWith(7, 1e-61), ['masking.floor[7]']], [floorWith(7, 1e61), ['masking.floor[7]']],
    [spreadWith(165, -1), ['masking.spread[165]']], [spreadWith(0, NaN), ['masking.spread[0]']], [spreadWith(2703, 1e61), ['masking.spread[2703]']],
    [{ floor: [1, 2, 3], spread: null }, ['masking.floor', '52']], [{ floor: MASKING_DEFAULT.floor, spread: [1, 2] }, ['masking.spread', '52 * 52']],
    ['default', ['masking', 'true or']], [{ spread: null }, ['masking', 'true or']]]
  for (const [masking, needles] of bad) {
    await rejects(() => encodeAeaPcm(chs, { measuredAllocation: true, masking }), TypeError, needles, `masking ${JSON.stringify(needles)}`)
    await rejects(() => encodeMeasured(chs, options, null, null, masking), TypeError, needles, `encodeMeasured with ${JSON.stringify(needles)}`)
  }
  await rejects(() => encodeAeaPcm(chs, { masking: true }), TypeError, ['masking', 'measuredAllocation'], 'masking without measuredAllocation')
  await rejects(() => encodeAeaPcm(chs, { measuredAllocation: false, masking: specs }), TypeError, ['masking', 'measuredAllocation'],
    'masking with measuredAllocation: false')
  await rejects(() => encodeAeaPcm(chs, { measuredAllocation: true, masking: true, scaleFactorOffsets: [0, 9] }), TypeError, ['scaleFactorOffsets[1]'],
    'bad offsets beside masking')

  if (failures) { console.log(`${failures} FAILURES`); process.exit(1) }
  console.log('ALL OK')
}

main().catch((e) => { console.log('ERROR', e && e.stack ? e.stack : e); process.exit(1) })
