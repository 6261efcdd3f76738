// Many items in one native call (io/processor.js: encodeAeaPcmMany / decodeAeaPcmMany, the addon's encodeSignals /
// decodeSignals) and the two WAV helpers of AudioProcessor (createWavBlob, assemblePcmFrames).  Without arguments only the host
// side runs: layout helpers, argument shapes and errors, the WAV helpers against values worked out by hand; with --gpu the
// many-item functions are compared byte for byte with the per-item ones, and createWavBlob with decodeAeaToWav16.  Prints ALL OK
// on success; run by tests/test_js_signals.py.
import * as c1 from './index.js'
import { itemsToSignals, interleaveItemUnits, deinterleaveItemUnits } from './io/processor.js'

const GPU = process.argv.includes('--gpu')
let failures = 0
function fail(msg) { failures++; console.log('FAIL', msg) }
function ok(cond, msg) { if (!cond) fail(msg) }
function sameBytes(a, b) { return a.byteLength === b.byteLength && Buffer.from(a.buffer, a.byteOffset, a.byteLength).equals(Buffer.from(b.buffer, b.byteOffset, b.byteLength)) }
async function rejects(fn, type, what) {
  try { await fn() } catch (e) { ok(e instanceof type, `${what}: threw ${e && e.constructor.name}: ${e && e.message}`); return }
  fail(`${what}: did not throw`)
}
function xorshift(seed) {
  let s = seed >>> 0
  return () => { s ^= s << 13; s >>>= 0; s ^= s >>> 17; s ^= s << 5; s >>>= 0; return (s / 4294967296) * 2 - 1 }
}
function white(seed, n) {
  const r = xorshift(seed); const x = new Float32Array(n)
  for (let i = 0; i < n; i++) x[i] = Math.fround(r() * 0.5)
  return x
}

// mono of 700 samples, stereo of 1 sample, stereo with channels of unequal length, mono of 0 samples, stereo of 40 000 samples
const items = [[white(1, 700)], [white(2, 1), white(3, 1)], [white(4, 1300), white(5, 900)], [new Float32Array(0)], [white(6, 40000), white(7, 40000)]]

async function main() {
// ---- host: exports and layout ----
ok(typeof c1.encodeAeaPcmMany === 'function' && typeof c1.decodeAeaPcmMany === 'function', 'the package exports encodeAeaPcmMany and decodeAeaPcmMany')
ok(typeof c1.AudioProcessor.createWavBlob === 'function' && typeof c1.AudioProcessor.createWavBytes === 'function' && typeof c1.AudioProcessor.assemblePcmFrames === 'function', 'AudioProcessor has createWavBlob, createWavBytes and assemblePcmFrames')
{
  const { signals, counts, frameOffsets } = itemsToSignals(items)
  ok(counts.join() === '1,2,2,1,2' && signals.length === 8, 'itemsToSignals: one signal per channel')
  ok(Array.from(frameOffsets).join() === '0,2,3,4,7,10,10,89,168', 'itemsToSignals: frame offsets ' + Array.from(frameOffsets).join())
  ok(signals[4].length === 3 * 512 && signals[4][899] === items[2][1][899] && signals[4].subarray(900).every((v) => v === 0), 'the shorter channel is zero padded to the longer one')
  const units = new Uint8Array(168 * 212)
  for (let s = 0; s < 8; s++) for (let f = frameOffsets[s]; f < frameOffsets[s + 1]; f++) { units[f * 212] = s; units[f * 212 + 1] = f - frameOffsets[s] }
  const body = interleaveItemUnits(units, frameOffsets, 3, 2)
  ok(body.length === 6 * 212 && [0, 1, 2, 3, 4, 5].map((u) => `${body[u * 212]}${body[u * 212 + 1]}`).join() === '30,40,31,41,32,42', 'interleaveItemUnits: L, R order')
  const back = new Uint8Array(6 * 212)
  ok(deinterleaveItemUnits(body, 2, back, 0) === 3 && sameBytes(back, units.subarray(frameOffsets[3] * 212, frameOffsets[5] * 212)), 'deinterleaveItemUnits inverts it')
  ok(interleaveItemUnits(units, frameOffsets, 5, 1).length === 0, 'an empty item has an empty body')
}
// ---- host: argument shapes and errors (nothing reaches the device) ----
await rejects(() => c1.encodeAeaPcmMany('x'), TypeError, 'items not an array')
await rejects(() => c1.encodeAeaPcmMany([[new Float64Array(4)]]), TypeError, 'a channel that is not a Float32Array')
await rejects(() => c1.encodeAeaPcmMany([[]]), TypeError, 'an item without channels')
await rejects(() => c1.encodeAeaPcmMany([[new Float32Array(4)], [new Float32Array(4)]], { title: ['only one'] }), TypeError, 'one title for two items')
await rejects(() => c1.encodeAeaPcmMany([[new Float32Array(4)]], { title: [7] }), TypeError, 'a title that is not a string')
await rejects(() => c1.encodeAeaPcmMany([[new Float32Array(4)]], { allocationBias: 99 }), Error, 'an option out of range')
await rejects(() => c1.decodeAeaPcmMany(new Uint8Array(2048)), TypeError, 'images not an array')
await rejects(() => c1.decodeAeaPcmMany(['text']), TypeError, 'an image that is not bytes')
await rejects(() => c1.decodeAeaPcmMany([new Uint8Array(2048)]), Error, 'an image without the AEA magic')
{
  const empty = await c1.encodeAeaPcmMany([])
  ok(Array.isArray(empty) && empty.length === 0, 'no items: no images, no device call')
  const none = await c1.encodeAeaPcmMany([[new Float32Array(0)], [new Float32Array(0), new Float32Array(0)]], { title: ['a', 'b'] })
  ok(none.length === 2 && none.every((im) => im.length === 2048) && c1.AeaFile.parseHeader(none[1]).channelCount === 2 && c1.AeaFile.parseHeader(none[1]).title === 'b',
    'items without samples: headers only, no device call')
  const pcm = await c1.decodeAeaPcmMany(none)
  ok(pcm.length === 2 && pcm[0].length === 1 && pcm[1].length === 2 && pcm[1][1].length === 0, 'images without units decode to empty channels')
}
// ---- host: the WAV helpers ----
{
  const A = c1.AudioProcessor
  const mono = A.assemblePcmFrames([new Float32Array([1, 2]), new Float32Array([3])], 1)
  ok(mono instanceof Float32Array && Array.from(mono).join() === '1,2,3', 'assemblePcmFrames mono: frames back to back')
  const st = A.assemblePcmFrames([[new Float32Array([1, 2, 3]), new Float32Array([4])], [new Float32Array(0), new Float32Array([5])]], 2)
  ok(Array.from(st).join() === '1,4,2,0,3,0,0,5', 'assemblePcmFrames stereo: interleaved, the shorter side zero filled: ' + Array.from(st).join())
  try { A.assemblePcmFrames([], 3); fail('assemblePcmFrames(…, 3) did not throw') } catch (e) { ok(/Unsupported channel count: 3/.test(e.message), 'assemblePcmFrames channel count message') }
  try { A.createWavBlob([], 3); fail('createWavBlob(…, 3) did not throw') } catch (e) { ok(/Unsupported channel count: 3/.test(e.message), 'createWavBlob channel count message') }
  const frames = [new Float32Array([0, 0.5, -0.5, 1, -1, 2, -2, 1e-6])]
  const b = Buffer.from(A.createWavBytes(frames))
  ok(b.length === 44 + 16, 'createWavBytes: header + 2 bytes per sample')
  if (typeof Blob === 'undefined') {
    try { A.createWavBlob(frames); fail('createWavBlob without Blob did not throw') } catch (e) { ok(/Blob is not available/.test(e.message), 'createWavBlob says that the runtime has no Blob') }
  } else {
    const blob = A.createWavBlob(frames)
    ok(blob instanceof Blob && blob.type === 'audio/wav' && sameBytes(new Uint8Array(await blob.arrayBuffer()), b), 'createWavBlob: an audio/wav Blob of createWavBytes\' bytes')
  }
  ok(b.toString('latin1', 0, 4) === 'RIFF' && b.readUInt32LE(4) === 36 + 16 && b.toString('latin1', 8, 16) === 'WAVEfmt ' && b.readUInt32LE(16) === 16 &&
     b.readUInt16LE(20) === 1 && b.readUInt16LE(22) === 1 && b.readUInt32LE(24) === 44100 && b.readUInt32LE(28) === 88200 && b.readUInt16LE(32) === 2 &&
     b.readUInt16LE(34) === 16 && b.toString('latin1', 36, 40) === 'data' && b.readUInt32LE(40) === 16, 'createWavBytes: the 44-byte PCM header')
  const got = [0, 1, 2, 3, 4, 5, 6, 7].map((i) => b.readInt16LE(44 + 2 * i)).join()
  ok(got === '0,16383,-16384,32767,-32768,32767,-32768,0', 'createWavBytes: clip, scale by 0x7fff / 0x8000, truncate: ' + got)
  const one = Buffer.from(A.createWavBytes(new Float32Array([0.25])))
  ok(one.length === 46 && one.readInt16LE(44) === 8191, 'createWavBytes accepts a lone Float32Array')
  const s = Buffer.from(A.createWavBytes([[new Float32Array([0.5, 0.5]), new Float32Array([-0.5])]], 2, 48000))
  ok(s.readUInt16LE(22) === 2 && s.readUInt32LE(24) === 48000 && s.readUInt32LE(28) === 192000 && s.readUInt16LE(32) === 4 && s.readUInt32LE(40) === 8 &&
     [0, 1, 2, 3].map((i) => s.readInt16LE(44 + 2 * i)).join() === '16383,-16384,16383,0', 'createWavBytes stereo: interleaved pairs, sample rate in the header')
}

if (GPU) {
  for (const options of [{}, { fixedBlockModes: [0, 2, 0], allocationBias: 0.5, title: ['a', 'b', 'c', 'd', 'e'] }, { fixedBlockModes: [0, 0, 0], title: 'one for all' }]) {
    const many = await c1.encodeAeaPcmMany(items, options)
    ok(many.length === items.length, 'one image per item')
    for (let i = 0; i < items.length; i++) {
      const o = { ...options }
      if (Array.isArray(o.title)) o.title = o.title[i]
      const alone = await c1.encodeAeaPcm(items[i], o)
      ok(sameBytes(many[i], alone), `encodeAeaPcmMany item ${i} == encodeAeaPcm alone (${JSON.stringify(options)})`)
    }
  }
  const images = await c1.encodeAeaPcmMany(items)
  images.push(images[4].slice(0, 2048 + 5 * 212))          // a stereo image that ends on a lone left unit
  images.push(images[2].slice(0, images[2].length - 100))  // and one with a trailing partial unit
  images.push(images[0].buffer.slice(0))                   // an ArrayBuffer
  const pcm = await c1.decodeAeaPcmMany(images)
  for (let i = 0; i < images.length; i++) {
    const alone = await c1.decodeAeaPcm(images[i])
    ok(pcm[i].length === alone.length && alone.every((ch, c) => sameBytes(ch, pcm[i][c])), `decodeAeaPcmMany image ${i} == decodeAeaPcm alone`)
  }
  // createWavBlob on the decoded PCM == the device's 16-bit conversion of the same image
  for (const i of [0, 4, 5]) {
    const bytes = images[i]
    const dev = c1.decodeAeaToWav16(bytes)
    const chans = pcm[i]
    const body = c1.AudioProcessor.createWavBytes(chans.length === 1 ? chans : [[chans[0], chans[1]]], chans.length).subarray(44)
    ok(sameBytes(body, dev.samples), `createWavBlob body == decodeAeaToWav16 samples (image ${i})`)
  }
}

}

main().then(() => {
  if (failures) { console.log(`${failures} FAILURE(S)`); process.exit(1) }
  console.log('ALL OK')
}).catch((e) => { console.log('FAIL', e && e.stack ? e.stack : e); process.exit(1) })
