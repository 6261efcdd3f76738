// Golden vectors over the encoder's option domain: every allocationBias the package carries a table for (0, 0.25, 0.5, 1,
// 1.5, 2, 3.3, 5) plus 0.01, 1.37 and 4.2, crossed with transient detection at thresholds 0.01, 0.3, 1 and 2 and with the
// fixed block modes [0,0,0], [2,2,3], [0,2,0] and [2,0,3].  Runs the JavaScript reference in place from /root/reference
// through loader.mjs (encode() :438, decode(), serializeFrame(), quantizationStage :365) and writes data only:
//   tests/golden/option_domain.json          cases, hashes, the biased tables of 0.01, 1.37 and 4.2, the stage outputs
//   tests/golden/option_domain_digests.bin   per unit of every case, in case order: the first 2 bytes of its SHA-256
//
//   cd tests/golden/gen && node --experimental-loader ./loader.mjs gen_option_domain.mjs
//
// Inputs and coefficient frames are built from xorshift32 of a counter and single Float32 roundings only, so
// tests/option_domain_lib.py rebuilds them bit for bit with numpy.  The SHA-256 of every input is recorded to prove it.
import fs from 'fs'
import path from 'path'
import crypto from 'crypto'
import { fileURLToPath } from 'url'

import { encode, quantizationStage } from '/root/reference/codec/pipeline/encoder.js'
import { decode } from '/root/reference/codec/pipeline/decoder.js'
import { serializeFrame, deserializeFrame } from '/root/reference/codec/io/serialization.js'
import { EncoderOptions } from '/root/reference/codec/core/options.js'
import { SCALE_FACTORS, SPECS_PER_BFU } from '/root/reference/codec/core/constants.js'

const OUT = path.resolve(path.dirname(fileURLToPath(import.meta.url)), '..')
const sha = (buf) => crypto.createHash('sha256').update(buf).digest('hex')
const bytesOf = (ta) => Buffer.from(ta.buffer, ta.byteOffset, ta.byteLength)
const f64hex = (x) => { const b = Buffer.alloc(8); b.writeDoubleBE(x); return b.toString('hex') }

const BIASES = [0, 0.01, 0.25, 0.5, 1, 1.37, 1.5, 2, 3.3, 4.2, 5]
const OPTION_SETS = [
  { transientThresholdLow: 0.01 }, { transientThresholdLow: 0.3 }, { transientThresholdLow: 1 }, { transientThresholdLow: 2 },
  { fixedBlockModes: [0, 0, 0] }, { fixedBlockModes: [2, 2, 3] }, { fixedBlockModes: [0, 2, 0] }, { fixedBlockModes: [2, 0, 3] },
]
const LENGTHS = [1, 2, 3, 5, 17, 40, 63, 65, 100, 129, 200, 257, 300, 90, 31, 150]
const FULL_UNITS_UP_TO = 1                     // cases of at most this many frames store their units whole

// ---- inputs (restated in tests/option_domain_lib.py; keep the two in step) ----
// hash32: two xorshift32 steps around one odd multiply; key(seed, stream, i) = hash32(hash32(seed*K1 + stream*K2) + i)
function hash32(a) {
  let x = a >>> 0
  x ^= x << 13; x >>>= 0; x ^= x >>> 17; x ^= x << 5; x >>>= 0
  x = Math.imul(x, 0x2C1B3C6D) >>> 0
  x ^= x << 13; x >>>= 0; x ^= x >>> 17; x ^= x << 5; x >>>= 0
  return x
}
const base = (seed, stream) => hash32((Math.imul(seed, 0x9E3779B1) + Math.imul(stream, 0x85EBCA77)) >>> 0)
const key = (b, i) => hash32((b + i) >>> 0)
const uni = (v) => ((v >>> 8) - 8388608) * 1.1920928955078125e-7           // exact in [-1, 1), 24 bits
const f = Math.fround

// one period of a piecewise parabola, +-4t(1-t) over each half (t = k / 2048 exact): the partials' oscillator
const WAVE = new Float32Array(4096)
for (let k = 0; k < 4096; k++) { const t = (k & 2047) / 2048; WAVE[k] = (k < 2048 ? 1 : -1) * f(4 * t * (1 - t)) }

// one material over the global sample indices [i0, i0 + n)
function material(spec, seed, i0, n) {
  const x = new Float32Array(n)
  const g = Math.pow(2, spec.exp || 0)                                           // an exact power of two
  switch (spec.kind) {
    case 'white': {
      const b = base(seed, 1)
      for (let j = 0; j < n; j++) x[j] = f(uni(key(b, i0 + j)) * g)
      break
    }
    case 'pink': {                                                                // Voss: eight octave-held white rows, bursts
      const bs = []
      for (let k = 0; k < 8; k++) bs.push(base(seed, 2 + k))
      const bb = base(seed, 10)
      for (let j = 0; j < n; j++) {
        const i = i0 + j
        let acc = 0
        for (let k = 0; k < 8; k++) acc = f(acc + f(uni(key(bs[k], i >>> k)) * 0.125))
        if ((i >>> 9) % 8 === 5 && (i & 511) >= 256) acc = f(acc + f(uni(key(bb, i)) * 0.75))
        x[j] = f(acc * g)
      }
      break
    }
    case 'partials': {                                                            // six stationary partials from WAVE
      const inc = [], ph = []
      for (let k = 0; k < 6; k++) {
        inc.push((key(base(seed, 20), k) % 858993459) + 100000)                  // up to about 8.8 kHz
        ph.push(key(base(seed, 21), k))
      }
      for (let j = 0; j < n; j++) {
        const i = i0 + j
        let acc = 0
        for (let k = 0; k < 6; k++) {
          const idx = ((ph[k] + Math.imul(i, inc[k])) >>> 0) >>> 20
          acc = f(acc + f(WAVE[idx] * Math.pow(2, -1 - k)))
        }
        x[j] = f(acc * g)
      }
      break
    }
    case 'square': {
      const inc = (key(base(seed, 30), 0) % 107374182) + 1073742              // 0.01 .. 1.1 kHz
      const ph = key(base(seed, 31), 0)
      for (let j = 0; j < n; j++) x[j] = ((ph + Math.imul(i0 + j, inc)) >>> 0) >= 0x80000000 ? -g : g
      break
    }
    case 'impulses': {
      const b = base(seed, 40), ba = base(seed, 41)
      for (let j = 0; j < n; j++) x[j] = (key(b, i0 + j) & 1023) < 3 ? f(uni(key(ba, i0 + j)) * g) : 0
      break
    }
    case 'silence':
      break
    case 'zeros': {                                                               // +0 and -0
      const b = base(seed, 50)
      for (let j = 0; j < n; j++) x[j] = (key(b, i0 + j) & 1) ? -0 : 0
      break
    }
    case 'patch': {                                                               // segments of 1..24 frames of the others
      const bl = base(seed, 60), bm = base(seed, 61), bs = base(seed, 62)
      let at = 0
      for (let k = 0; at < i0 + n; k++) {
        const len = (1 + key(bl, k) % 24) * 512
        const lo = Math.max(at, i0), hi = Math.min(at + len, i0 + n)
        if (hi > lo) x.set(material(PATCH[key(bm, k) % PATCH.length], key(bs, k), lo, hi - lo), lo - i0)
        at += len
      }
      break
    }
    default: throw new Error(spec.kind)
  }
  return x
}
const PATCH = [
  { kind: 'white', exp: -140 }, { kind: 'white', exp: -100 }, { kind: 'white', exp: -20 }, { kind: 'white', exp: -1 },
  { kind: 'white', exp: 3 }, { kind: 'pink', exp: 0 }, { kind: 'partials', exp: 0 }, { kind: 'partials', exp: -30 },
  { kind: 'square', exp: -2 }, { kind: 'impulses', exp: 0 }, { kind: 'silence' }, { kind: 'zeros' },
]
const MATERIALS = [
  { kind: 'white', exp: -140 }, { kind: 'white', exp: -126 }, { kind: 'white', exp: -60 }, { kind: 'white', exp: -6 },
  { kind: 'white', exp: -1 }, { kind: 'white', exp: 0 }, { kind: 'white', exp: 3 }, { kind: 'pink', exp: 0 },
  { kind: 'pink', exp: -12 }, { kind: 'partials', exp: 0 }, { kind: 'partials', exp: -1 }, { kind: 'partials', exp: -16 },
  { kind: 'partials', exp: -40 },
  { kind: 'square', exp: -1 }, { kind: 'square', exp: 0 }, { kind: 'impulses', exp: 0 }, { kind: 'impulses', exp: 3 },
  { kind: 'silence' }, { kind: 'zeros' }, { kind: 'patch' }, { kind: 'patch' }, { kind: 'patch' },
]

// ---- the reference ----
function biasedTable(bias) {                                                     // bitallocation.js:46-61
  const t = new Float64Array(64)
  for (let i = 0; i < 64; i++) t[i] = bias === 1 ? SCALE_FACTORS[i] : Math.pow(SCALE_FACTORS[i], bias)
  return Array.from(t, f64hex)
}

function encodeStream(chs, frames, opts) {
  const encs = chs.map(() => encode(new EncoderOptions(opts)))
  const units = []
  for (let fr = 0; fr < frames; fr++)
    for (let c = 0; c < chs.length; c++) units.push(Buffer.from(serializeFrame(encs[c](chs[c].slice(fr * 512, (fr + 1) * 512)))))
  return units
}
function decodeStream(units, nch, frames) {
  const ds = []
  for (let c = 0; c < nch; c++) ds.push(decode())
  const out = new Float32Array(frames * nch * 512)                            // per frame: L then R
  for (let fr = 0; fr < frames; fr++)
    for (let c = 0; c < nch; c++) out.set(ds[c](deserializeFrame(new Uint8Array(units[fr * nch + c]))), (fr * nch + c) * 512)
  return out
}

const out = {
  note: 'generated by tests/golden/gen/gen_option_domain.mjs from the reference encoder; inputs: tests/option_domain_lib.py ' +
        'restates the generator (xorshift32 of a counter, single Float32 roundings). ' +
        'units: frames x channels 212-byte units, per frame L then R (hex, short cases only); pcm_sha256: the decoded Float32 PCM, per frame L then R; halo: encode frames cut.. from the input ' +
        'starting at frame cut - halo; biased: allocationBias\'s table as the reference built it (binary64, hex) for the ' +
        'biases tests/golden/tables.json does not hold',
  biases: BIASES.map(String),
  biased: {},
  cases: [],
  stage: null,
}
for (const b of [0.01, 1.37, 4.2]) out.biased[String(b)] = biasedTable(b)

const digests = []
let ci = 0
for (const bias of BIASES) {
  for (let oi = 0; oi < OPTION_SETS.length; oi++, ci++) {
    {
      const opts = { ...OPTION_SETS[oi], allocationBias: bias }
      const h = key(base(ci, 90), 0)
      const spec = MATERIALS[(ci * 7) % MATERIALS.length]
      const frames = LENGTHS[(ci * 3 + (h & 7)) % LENGTHS.length]
      const nch = 1 + ((h >>> 4) & 1)
      const seed = 1000 + ci
      const chs = []
      for (let c = 0; c < nch; c++) chs.push(material(spec, seed + 7919 * c, 0, frames * 512))
      const units = encodeStream(chs, frames, opts)
      const pcm = decodeStream(units, nch, frames)
      const cut = frames > 1 ? 1 + (h >>> 8) % (frames - 1) : 0
      const all = Buffer.concat(units)
      const c = {
        id: ci, bias: String(bias), options: opts, material: spec, seed, frames, channels: nch,
        input_sha256: chs.map((x) => sha(bytesOf(x))),
        cut, halo: Math.min(2, cut),
        units_sha256: sha(all), pcm_sha256: sha(bytesOf(pcm)),
      }
      for (const u of units) digests.push(crypto.createHash('sha256').update(u).digest().subarray(0, 2))
      if (frames <= FULL_UNITS_UP_TO) c.units = all.toString('hex')
      out.cases.push(c)
    }
  }
}

// ---- quantizationStage on coefficient frames at every bias ----
{
  const F = 48
  const MODES = [[0, 0, 0], [2, 2, 3], [0, 2, 0], [2, 0, 3]]
  const coefs = new Float32Array(F * 512)
  const modes = []
  for (let fr = 0; fr < F; fr++) {
    const x = coefs.subarray(fr * 512, (fr + 1) * 512)
    const b = base(fr, 70), kind = [0, 1, 2, 5, 6, 7][fr % 6]
    const sf = (s) => f(SCALE_FACTORS[s])
    switch (kind) {
      case 0:                                                                     // one scale factor in every BFU
        for (let i = 0; i < 512; i++) x[i] = f(uni(key(b, i)) * sf(10 + fr % 50))
        break
      case 1: {                                                                   // three shared scale factors
        const s = [5 + fr % 20, 30 + fr % 20, 55 + fr % 8]
        for (let i = 0; i < 512; i++) x[i] = f(uni(key(b, i)) * sf(s[(i >>> 6) % 3]))
        break
      }
      case 2:                                                                     // a falling spectrum
        for (let i = 0; i < 512; i++) x[i] = f(uni(key(b, i)) * Math.pow(2, -(i >>> 5)))
        break
      case 5:                                                                     // every coefficient one scale factor exactly
        for (let i = 0; i < 512; i++) x[i] = (key(b, i) & 1 ? -1 : 1) * sf(20 + fr % 40)
        break
      case 6:                                                                     // a few BFUs of the low band: budgets saturate
        for (let i = 0; i < 128; i++) x[i] = (key(b, i >>> 3) & 3) === 0 ? f(uni(key(b, i)) * 0.5) : 0
        break
      case 7:                                                                     // two or three coefficients anywhere
        for (let i = 0; i < 512; i++) x[i] = (key(b, i) & 255) === 0 ? f(uni(key(b, i + 512)) * 0.25) : 0
        break
    }
    modes.push(MODES[(fr + (fr >> 2)) % MODES.length])
  }
  const stage = { note: 'quantizationStage on the coefficient frames (frames x 512 Float32) with block_modes; per bias and ' +
                        'frame: nbfu, and the first 4 bytes of SHA-256 of the int32 fields nbfu | sfi[52] | wl[52] | quantized[512] ' +
                        '(zero past nbfu), hex',
                  frames: F, block_modes: modes, coefs_sha256: sha(bytesOf(coefs)), by_bias: {} }
  for (const bias of BIASES) {
    const qs = quantizationStage({ options: { allocationBias: bias } })
    const rows = { nbfu: [], fields: [] }
    for (let fr = 0; fr < F; fr++) {
      const r = qs({ coefficients: coefs.slice(fr * 512, (fr + 1) * 512), blockModes: modes[fr].slice() })
      const v = new Int32Array(1 + 52 + 52 + 512)
      v[0] = r.nBfu
      let at = 105
      for (let bf = 0; bf < 52; bf++) {
        if (bf < r.nBfu) {
          v[1 + bf] = r.scaleFactorIndices[bf]
          v[53 + bf] = r.wordLengthIndices[bf]
          v.set(r.quantizedCoefficients[bf], at)
        }
        at += SPECS_PER_BFU[bf]
      }
      rows.nbfu.push(r.nBfu)
      rows.fields.push(sha(bytesOf(v)).slice(0, 8))
    }
    stage.by_bias[String(bias)] = rows
  }
  out.stage = stage
}

// one line per case, per table and per bias of the stage outputs
const lines = (o, ind) => '{\n' + Object.entries(o).map(([k, v]) => ind + JSON.stringify(k) + ': ' +
  (Array.isArray(v) && typeof v[0] === 'object' ? '[\n' + v.map((x) => ind + ' ' + JSON.stringify(x)).join(',\n') + ']'
    : (v && typeof v === 'object' && !Array.isArray(v) && k !== 'options' ? lines(v, ind + ' ') : JSON.stringify(v)))).join(',\n') + '}'
fs.writeFileSync(path.join(OUT, 'option_domain_digests.bin'), Buffer.concat(digests))
fs.writeFileSync(path.join(OUT, 'option_domain.json'), lines(out, ' ') + '\n')
const units = out.cases.reduce((a, c) => a + c.frames * c.channels, 0)
console.log('wrote option_domain.json:', out.cases.length, 'cases,', units, 'units; stage frames', out.stage.frames)
