// encodeMeasured(channels, options, modes, scaleFactorOffsets) and encodeAeaPcm(channels, { measuredAllocation: true,
// scaleFactorOffsets }) (carta1_amd/js/native.js, io/processor.js -> c1_encode_measured_sf_batch) against what the Python host
// got for the same PCM.
// argv[2]: a directory with ch0.f32, ch1.f32 (raw float32), modes.u8 (one mode byte per unit) and, from the Python host,
// units.u8, taken.u8, shifts.i8, dist.f64, energy.f64 (under detection) and the same with _m (under the given modes), written by
// tests/test_js_scale_factor_choice.py.  Prints ALL OK on success.
import fs from 'fs'
import path from 'path'

import { encodeAeaPcm, encodeMeasured, EncoderOptions, SCALE_FACTOR_OFFSETS, decode, decodeAeaPcm } from '../carta1_amd/js/index.js'

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
  ok(JSON.stringify(SCALE_FACTOR_OFFSETS) === '[0,-1,1,-2,-3]', 'SCALE_FACTOR_OFFSETS is the suggested set')
  for (const [given, tag] of [[null, ''], [modes, '_m']]) {
    const got = encodeMeasured(chs, options, given, SCALE_FACTOR_OFFSETS)
    ok(got.units instanceof Uint8Array && got.units.length === units * 212, `units${tag} is a Uint8Array of one unit per frame and channel`)
    ok(got.taken instanceof Uint8Array && got.taken.length === units, `taken${tag} is one byte per unit`)
    ok(got.shifts instanceof Int8Array && got.shifts.length === units * 52, `shifts${tag} is 52 signed bytes per unit`)
    ok(bytes(got.units).equals(bytes(u8(`units${tag}.u8`))), `units${tag} == the Python result`)
    ok(bytes(got.taken).equals(bytes(u8(`taken${tag}.u8`))), `taken${tag} == the Python result`)
    ok(bytes(got.shifts).equals(bytes(u8(`shifts${tag}.i8`))), `shifts${tag} == the Python result`)
    ok(bytes(got.distortion).equals(bytes(f64(`dist${tag}.f64`))), `distortion${tag} == the Python result, bit for bit`)
    ok(bytes(got.energy).equals(bytes(f64(`energy${tag}.f64`))), `energy${tag} == the Python result, bit for bit`)
    ok(got.taken.some((t) => t === 1) && got.shifts.some((s) => s !== 0), `taken${tag} and shifts${tag} are set somewhere`)

    // one offset of 0 is the call without offsets
    const zero = encodeMeasured(chs, options, given, [0]), plain = encodeMeasured(chs, options, given)
    ok(bytes(zero.units).equals(bytes(plain.units)) && bytes(zero.taken).equals(bytes(plain.taken)) &&
       bytes(zero.distortion).equals(bytes(plain.distortion)) && zero.shifts.every((s) => s === 0) && plain.shifts === undefined,
    `scaleFactorOffsets [0]${tag} is encodeMeasured without offsets`)

    const image = await encodeAeaPcm(chs, { measuredAllocation: true, scaleFactorOffsets: SCALE_FACTOR_OFFSETS, ...(given ? { blockModes: given } : {}) })
    ok(image.length === 2048 + units * 212, 'the image has a header and one unit per frame and channel')
    ok(bytes(image.subarray(2048)).equals(bytes(got.units)), `the body is encodeMeasured's units${tag}`)
    const typed = await encodeAeaPcm(chs, { measuredAllocation: true, scaleFactorOffsets: Int8Array.from(SCALE_FACTOR_OFFSETS), ...(given ? { blockModes: given } : {}) })
    ok(bytes(typed).equals(bytes(image)), 'an Int8Array of offsets is the array')

    // the project's own decode() of the units is finite: the closure on the left channel's first frames, one unit a call, and
    // decodeAeaPcm on the whole image
    const decoder = decode()
    let finite = true
    for (let f = 0; f < 16 && f < frames && finite; f++) {
      const pcm = decoder(got.units.subarray(2 * f * 212, (2 * f + 1) * 212))
      finite = pcm.length === 512 && pcm.every((v) => Number.isFinite(v))
    }
    const pcm = await decodeAeaPcm(image)
    finite = finite && pcm.length === 2 && pcm.every((c) => c.length >= frames * 512 && c.every((v) => Number.isFinite(v)))
    ok(finite, `decode() of the units${tag} is finite`)
  }

  const bad = [[[], ['scaleFactorOffsets', '1 to 8']], [[0, 1, 2, 3, 4, 5, 6, 7, 8], ['scaleFactorOffsets', '1 to 8']],
    [[0, -1, -1], ['scaleFactorOffsets[2]', 'twice']], [[0, 9], ['scaleFactorOffsets[1]', '-8..8']], [[0, 1.5], ['scaleFactorOffsets[1]', 'integer']],
    [[-1, 0], ['scaleFactorOffsets[0]', 'must be 0']], ['0,-1', ['scaleFactorOffsets', 'array']]]
  for (const [list, needles] of bad) {
    await rejects(() => encodeAeaPcm(chs, { measuredAllocation: true, scaleFactorOffsets: list }), TypeError, needles, `scaleFactorOffsets ${JSON.stringify(list)}`)
    await rejects(() => encodeMeasured(chs, options, null, list), TypeError, needles, `encodeMeasured with ${JSON.stringify(list)}`)
  }
  await rejects(() => encodeAeaPcm(chs, { scaleFactorOffsets: [0, -1] }), TypeError, ['scaleFactorOffsets', 'measuredAllocation'], 'offsets without measuredAllocation')
  await rejects(() => encodeAeaPcm(chs, { measuredAllocation: false, scaleFactorOffsets: [0, -1] }), TypeError, ['scaleFactorOffsets', 'measuredAllocation'],
    'offsets with measuredAllocation: false')

  if (failures) { console.log(`${failures} FAILURES`); process.exit(1) }
  console.log('ALL OK')
}

main().catch((e) => { console.log('ERROR', e && e.stack ? e.stack : e); process.exit(1) })
