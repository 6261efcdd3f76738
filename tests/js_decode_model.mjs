// The JavaScript decode option { precision: 'exact' | 'binary32' } (carta1_amd/js/native.js): decodeAeaPcm, decodeAeaPcmMany,
// decodeAeaToWav16, the decode() closure frame by frame and AudioProcessor.decodeStream on 24 mono and 24 stereo frames of a
// KAT file against the Python host's results under decode model 2 (bit for bit) and against the exact decode (RMS <= 1e-5);
// without the option the exact results as before; a pool moved from 'exact' to 'binary32' after 12 frames against the Python
// stream switched at the same frame.  `errors` as the only argument: the option's TypeErrors alone, which need no device.
// Prints ALL OK on success; run by tests/test_js_decode_model.py and tests/test_decode_model_cpu.py.
import fs from 'fs'
import path from 'path'
import { fileURLToPath } from 'url'

import { BufferPool } from '../carta1_amd/js/core/buffers.js'
import { AeaFile } from '../carta1_amd/js/io/serialization.js'
import { AudioProcessor, decodeAeaPcm, decodeAeaPcmMany, decodeAeaToWav16 } from '../carta1_amd/js/io/processor.js'
import { decode } from '../carta1_amd/js/pipeline/decoder.js'

let failures = 0
function ok(cond, what) {
  if (!cond) { failures++; console.log('FAIL', what) }
}
async function throwsTypeError(fn, word, what) {
  try {
    await fn()
    ok(false, `${what}: no error`)
  } catch (e) {
    ok(e instanceof TypeError && e.message.includes(word), `${what}: ${e.constructor.name}: ${e.message}`)
  }
}

async function main() {
  // ---- the option's errors: before any native call ------------------------------------------------------------------------
  const image0 = new Uint8Array(2048 + 212)
  image0.set(AeaFile.createHeader('t', 1, 1), 0)
  for (const bad of ['float', 'Binary32', 32, null, true]) {
    await throwsTypeError(() => decode(new BufferPool(), { precision: bad }), 'precision', `decode ${bad}`)
    await throwsTypeError(() => decodeAeaPcm(image0, { precision: bad }), 'precision', `decodeAeaPcm ${bad}`)
    await throwsTypeError(() => decodeAeaPcmMany([image0], { precision: bad }), 'precision', `decodeAeaPcmMany ${bad}`)
    await throwsTypeError(() => decodeAeaToWav16(image0, { precision: bad }), 'precision', `decodeAeaToWav16 ${bad}`)
    await throwsTypeError(() => AudioProcessor.decodeStream([], { precision: bad }).next(), 'precision', `decodeStream ${bad}`)
  }
  await throwsTypeError(() => decodeAeaPcm(image0, { precision: 'binary32', devices: [0] }), 'devices', 'binary32 with devices')
  if (process.argv[2] === 'errors') return

  // ---- against the Python host ---------------------------------------------------------------------------------------------
  const FRAMES = 24, SWITCH = 12, N = FRAMES * 512
  const G = path.join(path.dirname(fileURLToPath(import.meta.url)), 'golden')
  const kat = fs.readFileSync(path.join(G, 'kat64_pinkT_detect_thr0.3.units.bin'))         // [64 frames, 2 channels, 212]
  const stereoUnits = new Uint8Array(kat.subarray(0, FRAMES * 2 * 212))
  const monoUnits = new Uint8Array(FRAMES * 212)
  for (let f = 0; f < FRAMES; f++) monoUnits.set(stereoUnits.subarray(f * 424, f * 424 + 212), f * 212)
  const raw = fs.readFileSync(process.env.C1_DECODE_MODEL_EXPECTED)
  const all = new Float32Array(raw.buffer.slice(raw.byteOffset, raw.byteOffset + raw.byteLength))
  ok(all.length === 9 * N, 'expected file size')
  const want = {}
  ;['mono32', 'left32', 'right32', 'mono', 'left', 'right', 'switched', 'wav32', 'wav'].forEach((k, i) => { want[k] = all.subarray(i * N, (i + 1) * N) })

  const sameBits = (x, y) => {
    const a = new Uint32Array(x.buffer, x.byteOffset, x.length), b = new Uint32Array(y.buffer, y.byteOffset, y.length)
    if (a.length !== b.length) return false
    for (let i = 0; i < a.length; i++) if (a[i] !== b[i]) return false
    return true
  }
  const rms = (x, y) => {
    let s = 0
    for (let i = 0; i < x.length; i++) s += (x[i] - y[i]) ** 2
    return Math.sqrt(s / x.length)
  }
  const image = (units, nch) => {
    const out = new Uint8Array(2048 + units.length)
    out.set(AeaFile.createHeader('t', units.length / 212, nch), 0)
    out.set(units, 2048)
    return out
  }
  const join = (frames) => {
    const out = new Float32Array(frames.length * 512)
    frames.forEach((f, i) => out.set(f, i * 512))
    return out
  }
  const unit = (units, i) => units.slice(i * 212, (i + 1) * 212)
  const b32 = { precision: 'binary32' }
  const monoImage = image(monoUnits, 1), stereoImage = image(stereoUnits, 2)

  // decodeAeaPcm
  const m32 = await decodeAeaPcm(monoImage, b32), s32 = await decodeAeaPcm(stereoImage, b32)
  ok(sameBits(m32[0], want.mono32), 'decodeAeaPcm binary32 mono')
  ok(sameBits(s32[0], want.left32) && sameBits(s32[1], want.right32), 'decodeAeaPcm binary32 stereo')
  const m = await decodeAeaPcm(monoImage), s = await decodeAeaPcm(stereoImage, { precision: 'exact' })
  ok(sameBits(m[0], want.mono), 'decodeAeaPcm without the option')
  ok(sameBits(s[0], want.left) && sameBits(s[1], want.right), 'decodeAeaPcm exact stereo')
  ok(!sameBits(m32[0], m[0]), 'binary32 is another arithmetic')
  for (const [a, b, what] of [[m32[0], m[0], 'mono'], [s32[0], s[0], 'left'], [s32[1], s[1], 'right']]) {
    const e = rms(a, b)
    ok(e <= 1e-5, `RMS against the exact decode, ${what}: ${e}`)
    console.log(`binary32 against exact, ${what}: RMS ${e.toExponential(3)}`)
  }
  ok(sameBits((await AudioProcessor.decodeAeaPcm(monoImage, b32))[0], want.mono32), 'AudioProcessor.decodeAeaPcm binary32')

  // decodeAeaPcmMany, decodeAeaToWav16
  const many = await decodeAeaPcmMany([monoImage, stereoImage], b32)
  ok(sameBits(many[0][0], want.mono32) && sameBits(many[1][0], want.left32) && sameBits(many[1][1], want.right32), 'decodeAeaPcmMany binary32')
  const manyExact = await decodeAeaPcmMany([monoImage, stereoImage])
  ok(sameBits(manyExact[0][0], want.mono) && sameBits(manyExact[1][1], want.right), 'decodeAeaPcmMany without the option')
  const wav = decodeAeaToWav16(monoImage, b32), wavExact = decodeAeaToWav16(monoImage)     // the 16-bit samples travel as floats
  ok(wav.samples.length === N && wav.samples.every((v, i) => v === want.wav32[i]), 'decodeAeaToWav16 binary32')
  ok(wavExact.samples.length === N && wavExact.samples.every((v, i) => v === want.wav[i]), 'decodeAeaToWav16 without the option')

  // decode() frame by frame
  {
    const d32 = decode(new BufferPool(), b32), d = decode(new BufferPool())
    const a = [], b = []
    for (let f = 0; f < FRAMES; f++) { a.push(d32(unit(monoUnits, f))); b.push(d(unit(monoUnits, f))) }
    ok(sameBits(join(a), want.mono32), 'decode() binary32 frame by frame, mono')
    ok(sameBits(join(b), want.mono), 'decode() without the option')
    const pools = [new BufferPool(), new BufferPool()]
    const ds = pools.map((p) => decode(p, b32))
    const l = [], r = []
    for (let f = 0; f < FRAMES; f++) { l.push(ds[0](unit(stereoUnits, 2 * f))); r.push(ds[1](unit(stereoUnits, 2 * f + 1))) }
    ok(sameBits(join(l), want.left32) && sameBits(join(r), want.right32), 'decode() binary32 frame by frame, stereo')
    // the pool's state in the reference's layout leaves and enters a binary32 pool unchanged
    const fork = new BufferPool()
    fork.setDecoderState(pools[0].getDecoderState())
    const again = decode(fork, b32)(unit(stereoUnits, 2 * (FRAMES - 1)))
    const direct = decode(pools[0], b32)(unit(stereoUnits, 2 * (FRAMES - 1)))
    ok(sameBits(again, direct), 'getDecoderState / setDecoderState on a binary32 pool')
  }

  // AudioProcessor.decodeStream
  {
    const frames = []
    for (let f = 0; f < 2 * FRAMES; f++) frames.push(unit(stereoUnits, f))
    const l = [], r = []
    for await (const [a, b] of AudioProcessor.decodeStream(frames, { channelCount: 2, precision: 'binary32' })) { l.push(a); r.push(b) }
    ok(sameBits(join(l), want.left32) && sameBits(join(r), want.right32), 'decodeStream binary32')
    const e = []
    for await (const a of AudioProcessor.decodeStream(frames.filter((_, i) => i % 2 === 0), {})) e.push(a)
    ok(sameBits(join(e), want.mono), 'decodeStream without the option')
  }

  // one pool, 'exact' for 12 frames, then 'binary32'
  {
    const pool = new BufferPool()
    const first = decode(pool), then = decode(pool, b32)
    const out = []
    for (let f = 0; f < FRAMES; f++) out.push((f < SWITCH ? first : then)(unit(monoUnits, f)))
    const got = join(out)
    ok(sameBits(got, want.switched), 'a pool switched from exact to binary32 after 12 frames')
    ok(sameBits(got.subarray(0, SWITCH * 512), want.mono.subarray(0, SWITCH * 512)), 'the exact half of the switched pool')
  }
}

main().then(() => {
  console.log(failures ? `${failures} FAILURES` : 'ALL OK')
  process.exit(failures ? 1 : 0)
}, (e) => {
  console.log('FAIL', e && e.stack ? e.stack : e)
  process.exit(1)
})
