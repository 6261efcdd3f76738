// Golden vectors for the encoder's pipeline stages (codec/pipeline/encoder.js: qmfAnalysisStage :57, blockSelectorStage :111,
// mdctStage :170, quantizationStage :365, composed by encode() :438-450).  Runs the JavaScript reference in place from
// /root/reference through loader.mjs and writes tests/golden/encoder_stages.json plus one encoder_stages_<case>.bin per case --
// inputs and outputs only, never reference source text.
//
//   cd tests/golden/gen && node --experimental-loader ./loader.mjs gen_encoder_stages.mjs
//
// Cases:
//  - the four stage closures over one pool, frame after frame, on the first 24 frames of channel 0 of the KAT signals (pinkT
//    with detection at thresholds 1 and 0.3, white with detection, white with fixed modes [0,0,0] and [2,2,3] at biases 0.5,
//    1 and 2): the unwindowed bands blockSelectorStage saw (stored once per signal), the modes, the coefficients, the fields;
//  - hand-built bands through one blockSelectorStage: impulses, values near the float32 maximum (the FFT overflows), +-Inf,
//    NaN, -0, denormals, thresholds 0, negative, 1e300 and NaN, fixedBlockModes switched on and off between frames;
//  - hand-built coefficients through quantizationStage at biases 0.5, 1 and 2: NaN (quiet and signalling patterns), +-Inf,
//    -0, denormals, magnitudes above 1, every SCALE_FACTORS[i] and its float32 neighbours, all-zero and one-nonzero frames,
//    block modes 1, 3, -1 and 7.
import fs from 'fs'
import path from 'path'
import { fileURLToPath } from 'url'

import { BufferPool } from '/root/reference/codec/core/buffers.js'
import { EncoderOptions } from '/root/reference/codec/core/options.js'
import { SCALE_FACTORS, SPECS_PER_BFU } from '/root/reference/codec/core/constants.js'
import { qmfAnalysisStage, blockSelectorStage, mdctStage, quantizationStage } from '/root/reference/codec/pipeline/encoder.js'

const OUT = path.resolve(path.dirname(fileURLToPath(import.meta.url)), '..')
const FRAMES_KAT = 24

// xorshift32 (SURVEY.md 8c); the KAT signals of gen_golden.mjs
function xorshift(seed) {
  let s = seed >>> 0
  return () => { s ^= s << 13; s >>>= 0; s ^= s >>> 17; s ^= s << 5; s >>>= 0; return s }
}
const unit = (r) => () => (r() / 4294967296) * 2 - 1
function white(seed, n) {
  const r = unit(xorshift(seed)); const x = new Float32Array(n)
  for (let i = 0; i < n; i++) x[i] = Math.fround(r() * 0.5)
  return x
}
function pinkT(seed, n) {
  const r = unit(xorshift(seed)); const x = new Float32Array(n); let p = 0
  for (let i = 0; i < n; i++) {
    const u = r(); p = 0.98 * p + 0.05 * u; let v = p
    if ((i >> 9) % 8 === 5 && (i % 512) >= 256) v += 0.8 * r()
    x[i] = v
  }
  return x
}

// allocationBias's table as bitallocation.js:46-61 builds it (this engine's Math.pow), as hex of the binary64 values
function biasedTable(bias) {
  const t = new Float64Array(64)
  for (let i = 0; i < 64; i++) t[i] = bias === 1 ? SCALE_FACTORS[i] : Math.pow(SCALE_FACTORS[i], bias)
  return Array.from(t, (x) => { const b = Buffer.alloc(8); b.writeDoubleBE(x); return b.toString('hex') })
}

// the library's frame-field layout (include/carta1_hip.h): zeros where the reference leaves entries unset
function toFields(q) {
  const f = { nbfu: new Int32Array([q.nBfu]), sfi: new Int32Array(52), wl: new Int32Array(52), quantized: new Int16Array(512) }
  let at = 0
  for (let b = 0; b < 52; b++) {
    if (b < q.nBfu) {
      f.sfi[b] = q.scaleFactorIndices[b]
      f.wl[b] = q.wordLengthIndices[b]
      f.quantized.set(q.quantizedCoefficients[b], at)            // |mantissa| <= 2^15 - 1 at 16 bits: int16 holds every one
    }
    at += SPECS_PER_BFU[b]
  }
  return f
}
const joinBands = (bands) => { const x = new Float32Array(512); x.set(bands[0], 0); x.set(bands[1], 128); x.set(bands[2], 256); return x }
const split = (x) => [x.slice(0, 128), x.slice(128, 256), x.slice(256, 512)]

const SHAPES = { bands: ['float32', [512]], block_modes: ['int32', [3]], coefficients: ['float32', [512]], nbfu: ['int32', []],
                 sfi: ['int32', [52]], wl: ['int32', [52]], quantized: ['int16', [512]], threshold: ['float64', []], fixed: ['int32', []] }
const TYPED = { float32: Float32Array, int32: Int32Array, int16: Int16Array, float64: Float64Array }

function writeCase(name, rows, keys, extra) {
  const parts = [], arrays = []
  for (const key of keys) {
    const [dtype, shape] = SHAPES[key]
    const per = shape.length ? shape[0] : 1
    const ta = new TYPED[dtype](rows.length * per)
    rows.forEach((r, i) => { if (per === 1) ta[i] = r[key] instanceof Object ? r[key][0] : r[key]; else ta.set(r[key], i * per) })
    parts.push(Buffer.from(ta.buffer))
    arrays.push({ name: key, dtype, shape: [rows.length, ...shape] })
  }
  const file = `encoder_stages_${name}.bin`
  fs.writeFileSync(path.join(OUT, file), Buffer.concat(parts))
  return { name, file, frames: rows.length, arrays, ...extra }
}

const out = { note: 'each case: little-endian arrays concatenated in `arrays` order in `file`; frames are consecutive frames of one ' +
                    'BufferPool from a fresh pool; bands are low128 | mid128 | high256 as qmfAnalysisStage returned them; fields ' +
                    'zero where the reference leaves them unset; bands_from / coefs_from: the case whose file holds the bands / coefficients; biased: allocationBias\'s table (binary64, hex)', cases: [] }

// ---- the four-stage chain ----
const CHAIN = [
  ['pinkT_detect', 'pinkT', {}, null],
  ['pinkT_detect_thr0.3', 'pinkT', { transientThresholdLow: 0.3 }, 'pinkT_detect'],
  ['white_detect', 'white', {}, null],
  ['white_m000_b0.5', 'white', { fixedBlockModes: [0, 0, 0], allocationBias: 0.5 }, 'white_detect'],
  ['white_m000_b1', 'white', { fixedBlockModes: [0, 0, 0], allocationBias: 1 }, 'white_detect'],
  ['white_m000_b2', 'white', { fixedBlockModes: [0, 0, 0], allocationBias: 2 }, 'white_detect'],
  ['white_m223_b0.5', 'white', { fixedBlockModes: [2, 2, 3], allocationBias: 0.5 }, 'white_detect'],
  ['white_m223_b1', 'white', { fixedBlockModes: [2, 2, 3], allocationBias: 1 }, 'white_detect'],
  ['white_m223_b2', 'white', { fixedBlockModes: [2, 2, 3], allocationBias: 2 }, 'white_detect'],
]
for (const [name, signal, opts, bandsFrom] of CHAIN) {
  const pcm = signal === 'white' ? white(1, FRAMES_KAT * 512) : pinkT(3, FRAMES_KAT * 512)
  const options = new EncoderOptions(opts)
  const context = { options, bufferPool: new BufferPool() }
  const qa = qmfAnalysisStage(context), bs = blockSelectorStage(context), md = mdctStage(context), qs = quantizationStage(context)
  const rows = []
  for (let f = 0; f < FRAMES_KAT; f++) {
    const a = qa(pcm.slice(f * 512, (f + 1) * 512))
    const s = bs(a)
    const bands = joinBands(s.bands)                               // before mdctStage windows the arrays in place
    const m = md(s)
    const q = qs(m)
    rows.push({ bands, block_modes: Int32Array.from(s.blockModes), coefficients: Float32Array.from(m.coefficients), ...toFields(q) })
  }
  // the coefficients of a fixed-mode case do not depend on the bias: stored once, with bias 1
  const coefsFrom = opts.fixedBlockModes && opts.allocationBias !== 1 ? name.replace(/_b[0-9.]+$/, '_b1') : name
  const keys = ['block_modes', ...(coefsFrom === name ? ['coefficients'] : []), 'nbfu', 'sfi', 'wl', 'quantized']
  out.cases.push(writeCase(name, rows, bandsFrom ? keys : ['bands', ...keys],
    { kind: 'chain', signal, seed: signal === 'white' ? 1 : 3, channel: 0, bands_from: bandsFrom || name, coefs_from: coefsFrom,
      threshold: options.transientThresholdLow, fixed_block_modes: options.fixedBlockModes, bias: options.allocationBias,
      biased: biasedTable(options.allocationBias) }))
}

// ---- hand-built bands through one blockSelectorStage ----
{
  const rnd = xorshift(4242)
  const rf = () => (rnd() / 4294967296) * 2 - 1
  const F32MAX = 3.4028234663852886e38
  const u32 = (u) => new Float32Array(new Uint32Array([u]).buffer)[0]
  const kinds = ['noise', 'impulse', 'near_max', 'inf', 'nan', 'neg_zero', 'denormal', 'silence', 'noise_loud', 'impulse_train',
                 'mixed', 'noise', 'near_max', 'nan', 'impulse', 'denormal', 'noise', 'silence', 'inf', 'mixed']
  const thresholds = [1, 0, -0.5, 1e300, NaN, 0.3, 1, -1e300, 0, 1, 0.3, NaN, 1, 0, 1e300, -0.5, 1, 0.3, 1, 0]
  const fixedAt = new Set([3, 4, 9, 10, 16])                       // fixedBlockModes on for these frames: history untouched
  const options = { transientThresholdLow: 1, fixedBlockModes: null }
  const context = { options, bufferPool: new BufferPool() }
  const bs = blockSelectorStage(context)
  const rows = []
  for (let f = 0; f < 40; f++) {
    const kind = kinds[f % kinds.length]
    const x = new Float32Array(512)
    for (let i = 0; i < 512; i++) {
      const r = rf()
      switch (kind) {
        case 'noise': x[i] = r * 0.3; break
        case 'noise_loud': x[i] = r * 1e30; break
        case 'impulse': x[i] = i === ((rnd() & 1) ? 17 : 300) ? 1 : 0; break
        case 'impulse_train': x[i] = i % 64 === 5 ? (i & 64 ? -2 : 2) : 0; break
        case 'near_max': x[i] = (i & 1 ? -1 : 1) * F32MAX * (0.5 + 0.5 * Math.abs(r)); break
        case 'inf': x[i] = i % 97 === 3 ? (i & 1 ? -Infinity : Infinity) : r * 0.1; break
        case 'nan': x[i] = i % 53 === 7 ? NaN : r * 0.2; break
        case 'neg_zero': x[i] = -0; break
        case 'denormal': x[i] = u32((rnd() & 0x7fffff) | (i & 1 ? 0x80000000 : 0)); break
        case 'silence': x[i] = 0; break
        case 'mixed': x[i] = i < 128 ? r * 0.5 : (i < 256 ? (i % 31 === 0 ? NaN : -0) : (i % 50 === 1 ? F32MAX : r * 1e-3)); break
      }
    }
    const fixed = fixedAt.has(f % 20)
    options.transientThresholdLow = thresholds[f % thresholds.length]
    options.fixedBlockModes = fixed ? [(f & 1) ? 2 : 0, 0, 3] : null
    const s = bs({ bands: split(x) })
    rows.push({ bands: x, block_modes: Int32Array.from(s.blockModes), threshold: options.transientThresholdLow, fixed: fixed ? 1 : 0 })
  }
  out.cases.push(writeCase('bands', rows, ['bands', 'threshold', 'fixed', 'block_modes'],
    { kind: 'bands', note: 'threshold: transientThresholdLow of the frame; fixed = 1: fixedBlockModes was set (block_modes are ' +
      'those modes, the pool\'s transientDetection was left alone)' }))
}

// ---- hand-built coefficients through quantizationStage ----
{
  const F = 32
  const rnd = xorshift(777)
  const rf = () => (rnd() / 4294967296) * 2 - 1
  const u32 = (u) => new Float32Array(new Uint32Array([u >>> 0]).buffer)[0]
  const bitsOf = (x) => new Uint32Array(new Float32Array([x]).buffer)[0]
  const MODES = [[0, 0, 0], [1, 0, 0], [0, 3, 0], [-1, 0, 7], [2, 2, 3], [7, -1, 1], [0, 0, 1], [3, 1, -1]]
  const frames = []
  for (let f = 0; f < F; f++) {
    const words = new Uint32Array(512)
    const x = new Float32Array(words.buffer)
    const kind = f % 8
    for (let i = 0; i < 512; i++) {
      const r = rnd(), v = rf()
      switch (kind) {
        case 0: x[i] = v * 0.25 * Math.pow(2, -(i >> 5)); break                       // a spectrum
        case 1: {                                                                       // SCALE_FACTORS[i] and neighbours
          const sf = Math.fround(SCALE_FACTORS[(i + f) % 64]), b = bitsOf(sf), d = r % 3
          words[i] = (d === 0 ? b : (d === 1 ? b + 1 : b - 1)) | (r & 8 ? 0x80000000 : 0)
          break
        }
        case 2: {                                                                       // specials among small values
          const c = r % 12
          if (c === 0) words[i] = 0x7fc00000                                             // quiet NaN
          else if (c === 1) words[i] = 0x7f800001 + (r >>> 12 & 0x3fffff)              // signalling NaN patterns
          else if (c === 2) words[i] = 0xff800001 + (r >>> 12 & 0xff)                  // negative signalling NaN
          else if (c === 3) words[i] = 0x7f800000                                       // +Inf
          else if (c === 4) words[i] = 0xff800000                                       // -Inf
          else if (c === 5) words[i] = 0x80000000                                       // -0
          else if (c === 6) words[i] = (r >>> 9) | (r & 1 ? 0x80000000 : 0)            // denormals
          else x[i] = v * 1e-3
          break
        }
        case 3: x[i] = v * (r & 1 ? 1.5 : (r & 2 ? 1e10 : 3e38)); break                // magnitudes above 1
        case 4: break                                                                    // all zero
        case 5: x[i] = i === (f * 37) % 512 ? v * 0.9 : 0; break                        // one nonzero
        case 6: words[i] = r % 5 === 0 ? 0xffc00000 : (r % 5 === 1 ? 0x00000001 : bitsOf(v * 0.1)); break   // NaN + denormal mixes
        case 7: words[i] = r % 3 === 0 ? 0x7f800000 : (r % 3 === 1 ? 0x7fa00000 : bitsOf(v)); break         // +Inf and sNaN
      }
    }
    frames.push({ coefficients: x, block_modes: Int32Array.from(MODES[(f + (f >> 3)) % MODES.length]) })
  }
  for (const bias of [0.5, 1, 2]) {
    const options = { allocationBias: bias }
    const qs = quantizationStage({ options })
    const rows = frames.map((fr) => {
      const input = { coefficients: fr.coefficients.slice(), blockModes: Array.from(fr.block_modes) }
      const q = qs(input)
      return { coefficients: fr.coefficients, block_modes: fr.block_modes, ...toFields(q) }
    })
    out.cases.push(writeCase(`coefs_b${bias}`, rows, [...(bias === 1 ? ['coefficients'] : []), 'block_modes', 'nbfu', 'sfi', 'wl', 'quantized'],
      { kind: 'coefs', coefs_from: 'coefs_b1', bias, biased: biasedTable(bias) }))
  }
}

fs.writeFileSync(path.join(OUT, 'encoder_stages.json'), JSON.stringify(out, null, 1) + '\n')
console.log('wrote encoder_stages.json', out.cases.map((c) => `${c.file} (${c.frames} frames)`).join(', '))
