// encodeAeaPcm(channels, { blockModes }) (carta1_amd/js/io/processor.js -> native.js encodeBatchModes -> c1_encode_modes_batch)
// against the units the Python host got for the same PCM and modes.  argv[2]: a directory with ch0.f32, ch1.f32 (raw float32),
// modes.u8 and units.u8, written by tests/test_js_block_modes.py.  Prints ALL OK on success.
import fs from 'fs'
import path from 'path'

import { encodeAeaPcm, encodeBatchModes, EncoderOptions } from '../carta1_amd/js/index.js'

const dir = process.argv[2]
const f32 = (name) => { const b = fs.readFileSync(path.join(dir, name)); return new Float32Array(b.buffer.slice(b.byteOffset, b.byteOffset + b.length)) }
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
  const modes = u8('modes.u8'), want = Buffer.from(u8('units.u8'))
  const frames = chs[0].length / 512
  ok(modes.length === frames * 2 && want.length === frames * 2 * 212, 'the material has the expected sizes')

  const image = await encodeAeaPcm(chs, { blockModes: modes })
  ok(image.length === 2048 + want.length && Buffer.from(image.subarray(2048)).equals(want), 'encodeAeaPcm with blockModes == the Python result')
  const plain = await encodeAeaPcm(chs, {})
  ok(Buffer.from(image.subarray(0, 2048)).equals(Buffer.from(plain.subarray(0, 2048))), 'the header is the one encodeAeaPcm writes')
  ok(!Buffer.from(plain.subarray(2048)).equals(want), 'the modes are not the detector\'s')
  ok(Buffer.from(encodeBatchModes(chs, modes, new EncoderOptions({}).toNative())).equals(want), 'encodeBatchModes == the Python result')

  // the last frame is zero padded as without blockModes: 100 samples fewer, the same frame count, the units of the padded PCM
  const cut = chs.map((c) => c.slice(0, c.length - 100))
  const padded = cut.map((c) => { const p = new Float32Array(frames * 512); p.set(c); return p })
  const a = await encodeAeaPcm(cut, { blockModes: modes }), b = await encodeAeaPcm(padded, { blockModes: modes })
  ok(Buffer.from(a).equals(Buffer.from(b)), 'a short last frame is zero padded')

  await rejects(() => encodeAeaPcm(chs, { blockModes: modes.subarray(1) }), TypeError, 'blockModes one byte short')
  await rejects(() => encodeAeaPcm(chs, { blockModes: new Uint8Array(frames) }), TypeError, 'blockModes of frames bytes for two channels')
  await rejects(() => encodeAeaPcm(chs, { blockModes: Array.from(modes) }), TypeError, 'blockModes that is not a Uint8Array')
  const bad = Uint8Array.from(modes); bad[5] = 0x01
  await rejects(() => encodeAeaPcm(chs, { blockModes: bad }), Error, 'a mode byte outside the domain')

  if (failures) { console.log(`${failures} FAILURES`); process.exit(1) }
  console.log('ALL OK')
}

main().catch((e) => { console.log('ERROR', e && e.stack ? e.stack : e); process.exit(1) })
