// Golden vectors for the single-stage exports (quantize, dequantize, FFT.fft, qmfAnalysisStage -> mdctStage) over the whole
// domain their C entry points accept: every word length the reference gives a meaning (the shift count of
// (1 << (bitsPerSample - 1)) - 1 is taken mod 32, so 1 and 33 give range 0 and 32 gives -2147483649), special values,
// half-way points of the rounding, the ToInt32 wrap of `| 0`, every FFT size up to 2^22 with V8's own twiddles, and the
// analysis stages over 64 frames in all 8 block-mode combinations.  Runs the JavaScript reference in place from
// /root/reference through loader.mjs and writes inputs and outputs only, never reference source text:
//   tests/golden/export_domain.json   the index: cases, their offsets into the .bin, hashes of large outputs
//   tests/golden/export_domain.bin    little-endian float32 / int32 records the index points at
//
//   cd tests/golden/gen && node --experimental-loader ./loader.mjs gen_export_domain.mjs
import crypto from 'crypto'
import fs from 'fs'
import path from 'path'
import { fileURLToPath } from 'url'

import { FFT } from '/root/reference/codec/transforms/fft.js'
import { BufferPool } from '/root/reference/codec/core/buffers.js'
import { quantize, dequantize } from '/root/reference/codec/coding/quantization.js'
import { qmfAnalysisStage, mdctStage } from '/root/reference/codec/pipeline/encoder.js'
import { SCALE_FACTORS } from '/root/reference/codec/core/constants.js'

const OUT = path.resolve(path.dirname(fileURLToPath(import.meta.url)), '..')
const bytes = (ta) => Buffer.from(ta.buffer, ta.byteOffset, ta.byteLength)
const sha = (...tas) => { const h = crypto.createHash('sha256'); for (const t of tas) h.update(bytes(t)); return h.digest('hex') }
const f64hex = (x) => { const b = Buffer.alloc(8); b.writeDoubleLE(x); return b.toString('hex') }

// inputs: a counter hash (vectorises in numpy; tests/test_gpu_export_domain.py restates it) and xorshift32 for the
// quantizer's noise.  hashNoise(seed, n, amp)[i] = fround(((h / 2^32) * 2 - 1) * amp), h a murmur3-style mix of i ^ seed.
function hashNoise(seed, n, amp) {
  const x = new Float32Array(n)
  for (let i = 0; i < n; i++) {
    let h = Math.imul((i ^ seed) >>> 0, 0x9e3779b1) >>> 0
    h = (h ^ (h >>> 15)) >>> 0
    h = Math.imul(h, 0x85ebca77) >>> 0
    h = (h ^ (h >>> 13)) >>> 0
    x[i] = Math.fround(((h / 4294967296) * 2 - 1) * amp)
  }
  return x
}
function xorshiftInts(seed, n) {
  let s = seed >>> 0
  const out = new Int32Array(n)
  for (let i = 0; i < n; i++) { s ^= s << 13; s >>>= 0; s ^= s >>> 17; s ^= s << 5; s >>>= 0; out[i] = s | 0 }
  return out
}

// the .bin: records appended in order, each 4-byte aligned; the index holds element offsets (in 4-byte words)
const chunks = []
let words = 0
function put(ta) { const off = words; chunks.push(Buffer.from(bytes(ta))); words += ta.length; return off }

// float32 one ulp either way (finite, nonzero-magnitude steps; crosses zero through the subnormals)
const f32b = new Float32Array(1), u32b = new Uint32Array(f32b.buffer)
function ulpStep(x, dir) {
  f32b[0] = x
  if (x === 0) { u32b[0] = 1; return dir > 0 ? f32b[0] : -f32b[0] }
  if ((x > 0) === (dir > 0)) u32b[0] += 1; else u32b[0] -= 1
  return f32b[0]
}

const out = {
  note: 'index into export_domain.bin (little-endian 4-byte words; offsets and lengths in words).  Inputs that are not ' +
        'stored are hashNoise(seed, n, amp) as gen_export_domain.mjs defines it.  sha256 fields hash the little-endian bytes ' +
        'of the outputs named, concatenated in the order named.',
}

// ---- quantize / dequantize -------------------------------------------------------------------------------------------
const FLT_MAX = 3.4028234663852886e38, DENORM_MIN = 1.401298464324817e-45
const SFI_FEW = [0, 1, 2, 3, 31, 62, 63]
const BITS_OUTSIDE = [-2147483648, -1, 33, 48, 2147483647]
const grid = []
const seen = new Set()
const add = (sfi, bits) => { const k = sfi + ',' + bits; if (!seen.has(k)) { seen.add(k); grid.push([sfi, bits]) } }
for (let bits = 0; bits <= 32; bits++) for (const sfi of SFI_FEW) add(sfi, bits)
for (const bits of [2, 16, 17, 24, 31, 32]) for (let sfi = 0; sfi < 64; sfi++) add(sfi, bits)
for (const bits of BITS_OUTSIDE) for (const sfi of SFI_FEW) add(sfi, bits)

// normFactor as quantize forms it, only to place the half-way and wrap points among the inputs
const norm = (sfi, bits) => ((1 << (bits - 1)) - 1) / SCALE_FACTORS[sfi]

const specials = [0, -0, DENORM_MIN, -DENORM_MIN, FLT_MAX, -FLT_MAX, Infinity, -Infinity, NaN]
const mantissaNoise = xorshiftInts(0x5eed, 64)
out.dequantize_noise = { seed: 0x5eed, n: 64, note: 'xorshift32 state after each step, as int32', words: put(mantissaNoise) }
out.quantize = []
let seed = 1000
for (const [sfi, bits] of grid) {
  const xs = []
  for (const amp of [1e-6, 0.05, 1.5, 1e6]) xs.push(...hashNoise(seed++, 8, amp))
  xs.push(...specials)
  const nf = norm(sfi, bits)
  if (Number.isFinite(nf) && nf !== 0) {
    const r = Math.abs((1 << (bits - 1)) - 1)
    const ks = [0, 1, 2, 3, r - 1, r, r + 1, 1e5].filter((k) => k >= 0)
    for (const k of ks) {
      for (const sgn of [1, -1]) {
        const x0 = Math.fround((sgn * (k + 0.5)) / nf)
        if (!Number.isFinite(x0)) continue
        xs.push(x0, ulpStep(x0, 1), ulpStep(x0, -1))
      }
    }
    for (const t of [2147483647.5, 2147483648.5, 2147484648, 4294967295.5, 4294967296.5, 6442450944, 8589934599]) {
      for (const sgn of [1, -1]) {
        const x0 = Math.fround((sgn * t) / nf)
        if (Number.isFinite(x0)) xs.push(x0)
      }
    }
  }
  const x = Float32Array.from(xs)
  const q = quantize(x, sfi, bits)
  // dequantize: 0, +-1, +-range, +-(range+1), INT32_MIN, INT32_MAX, then the 64 noise mantissas (not stored again)
  const r = (1 << (bits - 1)) - 1
  const m = Int32Array.from([0, 1, -1, r | 0, -r | 0, (r + 1) | 0, -(r + 1) | 0, -2147483648, 2147483647, ...mantissaNoise])
  const d = dequantize(m, sfi, bits)
  out.quantize.push({ sfi, bits, n: x.length, x: put(x), q: put(q), nm: m.length, m: put(m.subarray(0, 9)), d: put(d) })
}

// ---- FFT.fft -----------------------------------------------------------------------------------------------------------
// V8's (cos, sin)(-2 pi / stride) for every stride the reference can reach with a 2^22-point transform
out.fft_twiddles = []
for (let stride = 2; stride <= 1 << 22; stride <<= 1) {
  const angle = (-2 * Math.PI) / stride
  out.fft_twiddles.push([stride, f64hex(Math.cos(angle)), f64hex(Math.sin(angle))])
}
out.fft = []
for (let lg = 0; lg <= 12; lg++) {
  const n = 1 << lg
  const re = hashNoise(2000 + lg, n, 1.0), im = hashNoise(3000 + lg, n, 1.0)
  FFT.fft(re, im)
  out.fft.push({ n, seed_real: 2000 + lg, seed_imag: 3000 + lg, amp: 1.0, real: put(re), imag: put(im) })
}
for (const lg of [14, 16, 18, 20, 22]) {
  const n = 1 << lg
  const re = hashNoise(2000 + lg, n, 1.0), im = hashNoise(3000 + lg, n, 1.0)
  FFT.fft(re, im)
  out.fft.push({ n, seed_real: 2000 + lg, seed_imag: 3000 + lg, amp: 1.0, sha256: sha(re, im) })
}
{
  const n = 64
  const re = new Float32Array(n).fill(-0), im = new Float32Array(n).fill(-0)
  FFT.fft(re, im)
  out.fft_special = [{ n, input: 'all -0', real: put(re), imag: put(im) }]
  const re2 = hashNoise(4000, 32, 1.0), im2 = hashNoise(4001, 32, 1.0)
  re2[5] = Infinity; im2[17] = NaN
  const xin = [put(re2), put(im2)]
  FFT.fft(re2, im2)
  out.fft_special.push({ n: 32, input: 'stored', in_real: xin[0], in_imag: xin[1], real: put(re2), imag: put(im2) })
}

// ---- qmfAnalysisStage -> mdctStage ---------------------------------------------------------------------------------------
// per frame: the bands as qmfAnalysisStage returns them, the bands after mdctStage's in-place windowing, the coefficients;
// sha256 truncated to 16 hex digits
const h16 = (ta) => sha(ta).slice(0, 16)
const FRAMES = 64
const streams = [
  { name: 'white', seed: 5001, amp: 0.5, zero_frames: 0 },
  { name: 'neg_zero_then_white', seed: 5002, amp: 0.5, zero_frames: 4 },
  { name: 'overload', seed: 5003, amp: 4.0, zero_frames: 0 },
  { name: 'subnormal', seed: 5004, amp: 1e-40, zero_frames: 0 },
]
const streamPcm = (s) => { const x = hashNoise(s.seed, FRAMES * 512, s.amp); x.fill(-0, 0, s.zero_frames * 512); return x }
out.stages = []
for (const s of streams) {
  const pcm = streamPcm(s)
  const runs = []
  let bandsRaw = null
  for (let combo = 0; combo < 8; combo++) {
    const modes = [combo & 1 ? 2 : 0, combo & 2 ? 2 : 0, combo & 4 ? 3 : 0]
    const ctx = { bufferPool: new BufferPool() }
    const qmf = qmfAnalysisStage(ctx), mdct = mdctStage(ctx)
    const raw = [], after = [], coefs = []
    for (let f = 0; f < FRAMES; f++) {
      const a = qmf(pcm.subarray(f * 512, (f + 1) * 512))
      raw.push(h16(Float32Array.from([...a.bands[0], ...a.bands[1], ...a.bands[2]])))
      const r = mdct({ bands: a.bands, blockModes: modes, originalFrame: null })
      after.push(h16(Float32Array.from([...r.bands[0], ...r.bands[1], ...r.bands[2]])))
      coefs.push(h16(r.coefficients))
    }
    if (bandsRaw === null) bandsRaw = raw
    else if (raw.join() !== bandsRaw.join()) throw new Error('qmfAnalysisStage depends on the block modes?')
    runs.push({ modes, bands_after: after, coefficients: coefs })
  }
  out.stages.push({ ...s, frames: FRAMES, bands_raw: bandsRaw, runs })
}

const bin = Buffer.concat(chunks)
out.bin_words = words
out.bin_sha256 = crypto.createHash('sha256').update(bin).digest('hex')
fs.writeFileSync(path.join(OUT, 'export_domain.bin'), bin)
fs.writeFileSync(path.join(OUT, 'export_domain.json'), JSON.stringify(out) + '\n')
console.log(`wrote export_domain.json, export_domain.bin (${bin.length} bytes)`)
