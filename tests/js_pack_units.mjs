// serializeFrames (carta1_amd/js/io/serialization.js) against what the reference's own serializeFrame wrote
// (tests/golden/pack_units.json), pipe() of the four JavaScript encoder stages followed by serializeFrames against the
// committed KAT units, and the RangeErrors of its argument checks.  Prints ALL OK on success; run by
// tests/test_js_pack_units.py.
import fs from 'fs'
import path from 'path'
import { fileURLToPath } from 'url'

import { BufferPool } from '../carta1_amd/js/core/buffers.js'
import { EncoderOptions } from '../carta1_amd/js/core/options.js'
import { SPECS_PER_BFU } from '../carta1_amd/js/core/constants.js'
import { pipe } from '../carta1_amd/js/utils.js'
import { serializeFrames } from '../carta1_amd/js/io/serialization.js'
import { qmfAnalysisStage, blockSelectorStage, mdctStage, quantizationStage } from '../carta1_amd/js/pipeline/encoder.js'

const G = path.join(path.dirname(fileURLToPath(import.meta.url)), 'golden')
const TYPED = { int32: Int32Array, uint8: Uint8Array }
const FIRST = [0]
for (let b = 0; b < 52; b++) FIRST.push(FIRST[b] + SPECS_PER_BFU[b])

function load(c) {
  const raw = fs.readFileSync(path.join(G, c.file))
  const buf = raw.buffer.slice(raw.byteOffset, raw.byteOffset + raw.byteLength)
  const out = {}
  let at = 0
  for (const a of c.arrays) {
    const T = TYPED[a.dtype], per = a.shape.length > 1 ? a.shape[1] : 1, n = a.shape[0] * per
    out[a.name] = { data: new T(buf, at, n), per }
    at += T.BYTES_PER_ELEMENT * n
  }
  return out
}
const row = (a, f) => a.data.subarray(f * a.per, (f + 1) * a.per)
const firstDiff = (x, y) => { if (x.length !== y.length) return -2; for (let i = 0; i < x.length; i++) if (x[i] !== y[i]) return i; return -1 }

// a reference-shaped frameData of fixture row f: all 52 BFUs of every array, as the generator handed them to serializeFrame
function frameData(d, f) {
  const q = row(d.quantized, f)
  return { nBfu: row(d.nbfu, f)[0], blockModes: Array.from(row(d.block_modes, f)), scaleFactorIndices: row(d.sfi, f).slice(),
           wordLengthIndices: row(d.wl, f).slice(), quantizedCoefficients: Array.from(SPECS_PER_BFU, (n, b) => q.slice(FIRST[b], FIRST[b] + n)) }
}

// xorshift32 (SURVEY.md 8c): the KAT signals
function xorshift(seed) {
  let s = seed >>> 0
  return () => { s ^= s << 13; s >>>= 0; s ^= s >>> 17; s ^= s << 5; s >>>= 0; return (s / 4294967296) * 2 - 1 }
}
function white(seed, n) { const r = xorshift(seed); const x = new Float32Array(n); for (let i = 0; i < n; i++) x[i] = Math.fround(r() * 0.5); return x }
function pinkT(seed, n) {
  const r = xorshift(seed); const x = new Float32Array(n); let p = 0
  for (let i = 0; i < n; i++) { const u = r(); p = 0.98 * p + 0.05 * u; let v = p; if ((i >> 9) % 8 === 5 && (i % 512) >= 256) v += 0.8 * r(); x[i] = v }
  return x
}

let failures = 0
const fail = (msg) => { failures++; console.log(msg) }

// ---- the fixture ----
const index = JSON.parse(fs.readFileSync(path.join(G, 'pack_units.json'), 'utf8'))
for (const c of index.cases) {
  const d = load(c)
  const got = serializeFrames(Array.from({ length: c.frames }, (_, f) => frameData(d, f)))
  const at = firstDiff(got, d.units.data)
  if (at !== -1) fail(`${c.name}: first differing byte ${at} (frame ${Math.floor(at / 212)})`)
  console.log(`${c.name}: ${c.frames} frames checked`)
}

// ---- pipe(the four encoder stages) then serializeFrames == the committed units ----
const kat = JSON.parse(fs.readFileSync(path.join(G, 'kat_index.json'), 'utf8'))
for (const name of ['pinkT_detect', 'white_m223_b0.5']) {
  const meta = kat[name]
  const units = fs.readFileSync(path.join(G, `kat64_${name}.units.bin`))
  for (let ch = 0; ch < 2; ch++) {
    const pcm = (meta.signal === 'white' ? white : pinkT)(meta.seeds[ch], meta.frames * 512)
    const staged = pipe({ options: new EncoderOptions(meta.options), bufferPool: new BufferPool() },
      qmfAnalysisStage, blockSelectorStage, mdctStage, quantizationStage)
    const fds = []
    for (let f = 0; f < meta.frames; f++) fds.push(staged(pcm.slice(f * 512, (f + 1) * 512)))
    const got = serializeFrames(fds)
    const want = new Uint8Array(meta.frames * 212)
    for (let f = 0; f < meta.frames; f++) want.set(units.subarray((2 * f + ch) * 212, (2 * f + ch + 1) * 212), f * 212)
    const at = firstDiff(got, want)
    if (at !== -1) fail(`pipe + serializeFrames ${name} channel ${ch}: first differing byte ${at}`)
    console.log(`pipe + serializeFrames: ${name} channel ${ch}, ${meta.frames} frames checked`)
  }
}

// ---- argument checks ----
const expectRange = (fn, what) => {
  try { fn(); fail(`${what}: no error`) } catch (e) { if (!(e instanceof RangeError)) fail(`${what}: ${e.constructor.name} ${e.message}`) }
}
const base = () => frameData(load(index.cases.find((c) => c.name === 'kat_pinkT_detect')), 0)
{
  const fd = base()
  const b = fd.wordLengthIndices.findIndex((w, i) => i < fd.nBfu && w > 0)
  fd.quantizedCoefficients[b] = fd.quantizedCoefficients[b].slice(1)
  expectRange(() => serializeFrames([base(), fd]), 'short BFU array')
  const fe = base()
  fe.quantizedCoefficients[b] = Int32Array.from([...fe.quantizedCoefficients[b], 0])
  expectRange(() => serializeFrames([fe]), 'long BFU array')
  // a BFU without mantissas (word length 0) may hold an array of any length, as may a BFU at or above nBfu
  const fz = base()
  fz.wordLengthIndices[b] = 0
  fz.quantizedCoefficients[b] = new Int32Array(3)
  fz.nBfu = b + 2
  fz.quantizedCoefficients[b + 2] = new Int32Array(1)
  serializeFrames([fz])
}
for (const bad of [53, -1, 20.5, NaN]) expectRange(() => serializeFrames([{ ...base(), nBfu: bad }]), `nBfu ${bad}`)
expectRange(() => serializeFrames([{ ...base(), blockModes: [0, 2 ** 31, 0] }]), 'block mode 2^31')
{
  const fd = base()
  fd.scaleFactorIndices = Array.from(fd.scaleFactorIndices)
  fd.scaleFactorIndices[0] = 1.5
  expectRange(() => serializeFrames([fd]), 'sfi 1.5')
  const fq = base()
  const b = fq.wordLengthIndices.findIndex((w, i) => i < fq.nBfu && w > 0)
  fq.quantizedCoefficients[b] = Array.from(fq.quantizedCoefficients[b])
  fq.quantizedCoefficients[b][0] = -(2 ** 31) - 1
  expectRange(() => serializeFrames([fq]), 'mantissa -2^31 - 1')
}
if (serializeFrames([]).length !== 0) fail('serializeFrames([]) is not empty')

if (failures) { console.log(`${failures} mismatches`); process.exit(1) }
console.log('ALL OK')
