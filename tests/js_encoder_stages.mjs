// The JavaScript encoder stages (carta1_amd/js/pipeline/encoder.js: blockSelectorStage, quantizationStage, with qmfAnalysisStage
// and mdctStage) against what the reference's own stages returned (tests/golden/encoder_stages.json), the four stages composed by
// pipe() against the library's encode() closure, and the reference's messages for a missing bufferPool / options.  Prints ALL OK
// on success; run by tests/test_js_encoder_stages.py.
import fs from 'fs'
import path from 'path'
import { fileURLToPath } from 'url'

import { BufferPool } from '../carta1_amd/js/core/buffers.js'
import { EncoderOptions } from '../carta1_amd/js/core/options.js'
import { SPECS_PER_BFU } from '../carta1_amd/js/core/constants.js'
import { pipe } from '../carta1_amd/js/utils.js'
import { encode, qmfAnalysisStage, blockSelectorStage, mdctStage, quantizationStage } from '../carta1_amd/js/pipeline/encoder.js'

const G = path.join(path.dirname(fileURLToPath(import.meta.url)), 'golden')
const index = JSON.parse(fs.readFileSync(path.join(G, 'encoder_stages.json'), 'utf8'))
const TYPED = { float32: Float32Array, int32: Int32Array, int16: Int16Array, float64: Float64Array }

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
const data = {}
for (const c of index.cases) data[c.name] = load(c)
for (const c of index.cases) {
  if (c.bands_from && !data[c.name].bands) data[c.name].bands = data[c.bands_from].bands
  if (c.coefs_from && !data[c.name].coefficients) data[c.name].coefficients = data[c.coefs_from].coefficients
}
const row = (a, f) => a.data.subarray(f * a.per, (f + 1) * a.per)
const sameBits = (x, y) => {
  const a = new Uint32Array(x.buffer, x.byteOffset, x.length), b = new Uint32Array(y.buffer, y.byteOffset, y.length)
  if (a.length !== b.length) return false
  for (let i = 0; i < a.length; i++) if (a[i] !== b[i]) return false
  return true
}
const sameInts = (x, y) => x.length === y.length && Array.from(x).every((v, i) => v === y[i])

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

// fields of one frame against the fixture
function checkFields(name, d, f, q) {
  const nBfu = row(d.nbfu, f)[0]
  if (q.nBfu !== nBfu) return fail(`${name} frame ${f}: nBfu ${q.nBfu} != ${nBfu}`)
  if (!(q.scaleFactorIndices instanceof Int32Array) || !sameInts(q.scaleFactorIndices, row(d.sfi, f).subarray(0, nBfu))) return fail(`${name} frame ${f}: sfi`)
  if (!(q.wordLengthIndices instanceof Int32Array) || !sameInts(q.wordLengthIndices, row(d.wl, f).subarray(0, nBfu))) return fail(`${name} frame ${f}: wl`)
  if (q.quantizedCoefficients.length !== nBfu) return fail(`${name} frame ${f}: ${q.quantizedCoefficients.length} quantized BFUs`)
  const want = row(d.quantized, f)
  for (let b = 0, at = 0; b < nBfu; at += SPECS_PER_BFU[b], b++) {
    const got = q.quantizedCoefficients[b]
    if (!(got instanceof Int32Array) || !sameInts(got, want.subarray(at, at + SPECS_PER_BFU[b]))) return fail(`${name} frame ${f}: quantized BFU ${b}`)
  }
}

// ---- the chain cases: the four library stages over one pool ----
for (const c of index.cases.filter((x) => x.kind === 'chain')) {
  const d = data[c.name]
  const opts = { allocationBias: c.bias, transientThresholdLow: c.threshold }
  if (c.fixed_block_modes) opts.fixedBlockModes = c.fixed_block_modes
  const options = new EncoderOptions(opts)
  const context = { options, bufferPool: new BufferPool() }
  const qa = qmfAnalysisStage(context), bs = blockSelectorStage(context), md = mdctStage(context), qs = quantizationStage(context)
  const pcm = c.signal === 'white' ? white(c.seed, c.frames * 512) : pinkT(c.seed, c.frames * 512)
  for (let f = 0; f < c.frames; f++) {
    const a = qa(pcm.slice(f * 512, (f + 1) * 512))
    const s = bs(a)
    const bands = new Float32Array(512); bands.set(s.bands[0], 0); bands.set(s.bands[1], 128); bands.set(s.bands[2], 256)
    if (s.bands !== a.bands) fail(`${c.name} frame ${f}: bands are not the input's arrays`)
    if (!sameBits(bands, row(d.bands, f))) fail(`${c.name} frame ${f}: bands`)
    if (!Array.isArray(s.blockModes) || !sameInts(s.blockModes, row(d.block_modes, f))) fail(`${c.name} frame ${f}: block modes`)
    if (c.fixed_block_modes && s.blockModes !== options.fixedBlockModes) fail(`${c.name} frame ${f}: fixed modes are not the options' array`)
    const m = md(s)
    if (!sameBits(m.coefficients, row(d.coefficients, f))) fail(`${c.name} frame ${f}: coefficients`)
    const q = qs(m)
    if (q.blockModes !== m.blockModes) fail(`${c.name} frame ${f}: blockModes not echoed`)
    checkFields(c.name, d, f, q)
  }
  console.log(`${c.name}: ${c.frames} frames checked`)
}

// ---- hand-built bands: one pool, fixedBlockModes switched on and off, thresholds outside EncoderOptions' range ----
{
  const c = index.cases.find((x) => x.name === 'bands'), d = data.bands
  const options = { transientThresholdLow: 1, fixedBlockModes: null }
  const bs = blockSelectorStage({ options, bufferPool: new BufferPool() })
  for (let f = 0; f < c.frames; f++) {
    const x = row(d.bands, f)
    const bands = [x.slice(0, 128), x.slice(128, 256), x.slice(256, 512)]
    options.transientThresholdLow = row(d.threshold, f)[0]
    options.fixedBlockModes = row(d.fixed, f)[0] ? Array.from(row(d.block_modes, f)) : null
    const s = bs({ bands })
    if (s.bands !== bands) fail(`bands frame ${f}: bands are not the input's arrays`)
    if (options.fixedBlockModes && s.blockModes !== options.fixedBlockModes) fail(`bands frame ${f}: fixed modes are not the options' array`)
    if (!sameInts(s.blockModes, row(d.block_modes, f))) fail(`bands frame ${f}: modes ${s.blockModes} != ${Array.from(row(d.block_modes, f))}`)
  }
  console.log(`bands: ${c.frames} frames checked`)
}

// ---- hand-built coefficients ----
for (const c of index.cases.filter((x) => x.kind === 'coefs')) {
  const d = data[c.name]
  const qs = quantizationStage({ options: { allocationBias: c.bias } })
  for (let f = 0; f < c.frames; f++) {
    const blockModes = Array.from(row(d.block_modes, f))
    const q = qs({ coefficients: row(d.coefficients, f).slice(), blockModes })
    if (q.blockModes !== blockModes) fail(`${c.name} frame ${f}: blockModes not echoed`)
    checkFields(c.name, d, f, q)
  }
  console.log(`${c.name}: ${c.frames} frames checked`)
}

// ---- pipe(context, the four stages) == the library's encode() closure ----
for (const [signal, opts] of [['pinkT', {}], ['pinkT', { transientThresholdLow: 0.3 }], ['white', {}],
                              ['white', { fixedBlockModes: [2, 2, 3], allocationBias: 0.5 }], ['white', { fixedBlockModes: [0, 0, 0], allocationBias: 2 }]]) {
  const frames = 24
  const pcm = signal === 'white' ? white(2, frames * 512) : pinkT(4, frames * 512)
  const options = new EncoderOptions(opts)
  const staged = pipe({ options, bufferPool: new BufferPool() }, qmfAnalysisStage, blockSelectorStage, mdctStage, quantizationStage)
  const whole = encode(new EncoderOptions(opts), new BufferPool())
  for (let f = 0; f < frames; f++) {
    const frame = pcm.slice(f * 512, (f + 1) * 512)
    const a = staged(frame), b = whole(frame)
    const same = a.nBfu === b.nBfu && sameInts(a.blockModes, b.blockModes) && sameInts(a.scaleFactorIndices, b.scaleFactorIndices) &&
      sameInts(a.wordLengthIndices, b.wordLengthIndices) &&
      a.quantizedCoefficients.every((q, i) => sameInts(q, b.quantizedCoefficients[i]))
    if (!same) fail(`pipe vs encode() ${signal} ${JSON.stringify(opts)} frame ${f}`)
  }
  console.log(`pipe vs encode(): ${signal} ${JSON.stringify(opts)} ${frames} frames checked`)
}

// ---- the reference's messages ----
const expectThrow = (fn, msg) => {
  try { fn(); fail(`no error, expected "${msg}"`) } catch (e) { if (e.message !== msg) fail(`"${e.message}" != "${msg}"`) }
}
expectThrow(() => blockSelectorStage({ options: new EncoderOptions() }), 'blockSelectorStage: bufferPool is required')
expectThrow(() => blockSelectorStage({ bufferPool: new BufferPool() }), 'blockSelectorStage: options is required')
expectThrow(() => blockSelectorStage(undefined), 'blockSelectorStage: bufferPool is required')
expectThrow(() => quantizationStage({ bufferPool: new BufferPool() }), 'quantizationStage: options is required')
expectThrow(() => quantizationStage(undefined), 'quantizationStage: options is required')

if (failures) { console.log(`${failures} mismatches`); process.exit(1) }
console.log('ALL OK')
