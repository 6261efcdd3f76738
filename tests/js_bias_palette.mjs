// encodeAeaPcm(channels, { allocationBiases }) (carta1_amd/js/io/processor.js -> native.js encodeBatchBiases ->
// c1_encode_biases_batch) against the reference's own bytes for its bias schedule and against the units the Python host got for
// the same PCM, biases and modes.  argv[2]: a directory with ch0.f32, ch1.f32 (raw float32), sched.f64 (one bias per frame),
// sha.txt (SHA-256 of the reference's units under fixedBlockModes [0,0,0] and that schedule), biases.f64 (one bias per frame
// and channel), modes.u8 and units.u8, written by tests/test_js_bias_palette.py.  Prints ALL OK on success.
import crypto from 'crypto'
import fs from 'fs'
import path from 'path'

import { encodeAeaPcm } from '../carta1_amd/js/index.js'

const dir = process.argv[2]
const raw = (name) => { const b = fs.readFileSync(path.join(dir, name)); return b.buffer.slice(b.byteOffset, b.byteOffset + b.length) }
const f32 = (name) => new Float32Array(raw(name))
const f64 = (name) => new Float64Array(raw(name))
const u8 = (name) => new Uint8Array(fs.readFileSync(path.join(dir, name)))

let failures = 0
function ok(cond, msg) { if (!cond) { failures++; console.log('FAIL', msg) } }
async function rejects(fn, type, msg) {
  let err = null
  try { await fn() } catch (e) { err = e }
  ok(err instanceof type, `${msg}: expected ${type.name}, got ${err}`)
}

async function main() {
  const chs = [f32('ch0.f32'), f32('ch1.f32')]
  const sched = f64('sched.f64'), biases = f64('biases.f64'), modes = u8('modes.u8'), want = Buffer.from(u8('units.u8'))
  const sha = fs.readFileSync(path.join(dir, 'sha.txt'), 'utf8').trim()
  const frames = chs[0].length / 512
  ok(sched.length === frames && biases.length === frames * 2 && modes.length === frames * 2 && want.length === frames * 2 * 212, 'the material has the expected sizes')

  const image = await encodeAeaPcm(chs, { allocationBiases: sched, fixedBlockModes: [0, 0, 0] })
  ok(image.length === 2048 + frames * 2 * 212, 'the image has a header and one unit per frame and channel')
  ok(crypto.createHash('sha256').update(image.subarray(2048)).digest('hex') === sha, 'the bias schedule of the fixture gives the fixture\'s SHA-256')
  const perUnit = Float64Array.from({ length: frames * 2 }, (_, u) => sched[u >> 1])
  const same = await encodeAeaPcm(chs, { allocationBiases: perUnit, fixedBlockModes: [0, 0, 0] })
  ok(Buffer.from(same).equals(Buffer.from(image)), 'one value per frame == the same value for both channels')
  const plain = await encodeAeaPcm(chs, { fixedBlockModes: [0, 0, 0] })
  ok(Buffer.from(image.subarray(0, 2048)).equals(Buffer.from(plain.subarray(0, 2048))), 'the header is the one encodeAeaPcm writes')
  ok(!Buffer.from(plain.subarray(2048)).equals(Buffer.from(image.subarray(2048))), 'the biases are not the default')

  const both = await encodeAeaPcm(chs, { allocationBiases: biases, blockModes: modes })
  ok(Buffer.from(both.subarray(2048)).equals(want), 'allocationBiases with blockModes == the Python result')

  const nine = Float64Array.from({ length: frames }, (_, f) => (f % 9) * 0.5)
  await rejects(() => encodeAeaPcm(chs, { allocationBiases: nine }), RangeError, 'nine distinct values')
  await rejects(() => encodeAeaPcm(chs, { allocationBiases: sched.subarray(1) }), TypeError, 'allocationBiases one value short')
  await rejects(() => encodeAeaPcm(chs, { allocationBiases: Array.from(sched) }), TypeError, 'allocationBiases that is not a Float64Array')
  const out = Float64Array.from(sched); out[7] = 5.5
  await rejects(() => encodeAeaPcm(chs, { allocationBiases: out }), Error, 'a bias outside allocationBias\'s range')

  if (failures) { console.log(`${failures} FAILURES`); process.exit(1) }
  console.log('ALL OK')
}

main().catch((e) => { console.log('ERROR', e && e.stack ? e.stack : e); process.exit(1) })
