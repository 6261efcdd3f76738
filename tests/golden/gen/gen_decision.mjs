// Golden vectors for the reference's decision functions: performFFT and detectTransient (codec/analysis/transient.js:17-55),
// findScaleFactor and allocateBits (codec/coding/bitallocation.js:74-142, :290-299), and Math.log2 (findScaleFactor's
// :297).  Runs the JavaScript reference in place from /root/reference through loader.mjs and writes
// tests/golden/decision.json (the index) and tests/golden/decision.bin (little-endian float64 words) -- inputs and outputs only,
// never reference source text.
//
//   cd tests/golden/gen && node --experimental-loader ./loader.mjs gen_decision.mjs
//
// Cases:
//  - the reference tests' inputs: silence, step and sine spectra (tests/transient.test.js), 52 BFUs of size 10
//    (tests/bitallocation.test.js);
//  - performFFT: fftSize 1 .. 4096, inputs shorter and longer than fftSize, zeros, values under 1e-10, NaN, +-Inf, +-0;
//  - detectTransient: random and adversarial spectra of equal, unequal and odd lengths, empty arrays, a falsy prevCoeffs,
//    thresholds including NaN and +-Inf.  detectTransient returns only `score > threshold`; the score itself is recovered
//    exactly by bisecting the threshold over the ordered binary64 patterns (the score is NaN, +Inf or >= +0);
//  - findScaleFactor: all 64 boundaries 2^(i/3 - 21) +- 4 ulp as Float32 and as double, random, NaN / Inf / +-0 / denormal
//    values, length beyond the array and <= 0;
//  - allocateBits: sizes 0, negative and above 20, BFU arrays shorter than their size, maxBfuCount 0 .. 52, biases 0 .. 5.
import fs from 'fs'
import path from 'path'
import { fileURLToPath } from 'url'

import { performFFT, detectTransient } from '/root/reference/codec/analysis/transient.js'
import { allocateBits, findScaleFactor } from '/root/reference/codec/coding/bitallocation.js'
import { SCALE_FACTORS, SPECS_PER_BFU } from '/root/reference/codec/core/constants.js'

const OUT = path.resolve(path.dirname(fileURLToPath(import.meta.url)), '..')
const words = []
function put(arr) {
  const off = words.length
  for (const v of arr) words.push(v)
  return [off, arr.length]
}

let s = 0x2545f491 >>> 0
function rnd() { s ^= s << 13; s >>>= 0; s ^= s >>> 17; s ^= s << 5; s >>>= 0; return s / 4294967296 }
const pick = (a) => a[Math.floor(rnd() * a.length)]
const f64buf = new DataView(new ArrayBuffer(8))
function fromBits(b) { f64buf.setBigUint64(0, b); return f64buf.getFloat64(0) }
function toBits(x) { f64buf.setFloat64(0, x); return f64buf.getBigUint64(0) }
function ulps(x, k) { return fromBits(toBits(x) + BigInt(k)) }           // x > 0
function ulps32(x, k) { const b = new Float32Array([x]); const u = new Uint32Array(b.buffer); u[0] += k; return b[0] }
const EDGE = [0, -0, 1e-12, -1e-12, 5e-324, 1e-300, NaN, Infinity, -Infinity, 3.4028234663852886e38, 1e300]

// ---- Math.log2
const log2 = []
{
  const xs = [0, -0, 1, 2, 0.5, 3, 5e-324, 2.2250738585072014e-308, 1e-300, 1e300, Infinity, NaN, -1, 0.7071067811865476,
    1.4142135623730951, 1 + 2 ** -52, 1 - 2 ** -53]
  for (let i = 0; i < 64; i++) for (let k = -4; k <= 4; k++) xs.push(ulps(SCALE_FACTORS[i], k), ulps32(Math.fround(SCALE_FACTORS[i]), k))
  for (let i = 0; i < 6000; i++) {
    const r = rnd(), t = rnd()
    if (i % 3 === 0) xs.push(Math.pow(2, -70 + 140 * r))
    else if (i % 3 === 1) xs.push(1 + (r - 0.5) * Math.pow(2, -Math.floor(t * 40)))
    else xs.push(fromBits((BigInt(Math.floor(r * 0x7ff00000)) << 32n) | BigInt(Math.floor(t * 4294967296))))
  }
  for (const x of xs) log2.push(x, Math.log2(x))
}

// ---- performFFT
const sine = (freq, n) => { const a = new Float32Array(n); for (let i = 0; i < n; i++) a[i] = Math.sin((2 * Math.PI * freq * i) / 44100); return a }
const step = (pos, n) => { const a = new Float32Array(n); for (let i = pos; i < n; i++) a[i] = 1; return a }
function randomSignal(n, kind) {
  const a = new Float64Array(n)
  for (let i = 0; i < n; i++) {
    const r = rnd()
    a[i] = kind === 0 ? 2 * r - 1 : kind === 1 ? (r - 0.5) * 1e-11 : kind === 2 ? (rnd() < 0.1 ? pick(EDGE) : 2 * r - 1) : (r - 0.5) * 1e30
  }
  return a
}
const fft = []
function fftCase(name, x, n) {
  const w = []
  for (let stride = 2; stride <= n; stride <<= 1) w.push(Math.cos((-2 * Math.PI) / stride), Math.sin((-2 * Math.PI) / stride))
  const y = performFFT(x, n)
  fft.push({ name, n, x: put(Array.from(x)), y: put(Array.from(y)), w: put(w) })
  return y
}
for (let n = 1; n <= 4096; n <<= 1) {
  fftCase('random', randomSignal(n, 0), n)
  fftCase('long', randomSignal(n + 3, 0), n)
  if (n > 512) continue
  fftCase('silence', new Float32Array(n), n)
  fftCase('sine1000', sine(1000, n), n)
  fftCase('short', randomSignal(Math.max(0, (n >> 1) - 1), 0), n)
  fftCase('tiny', randomSignal(n, 1), n)
  fftCase('edge', randomSignal(n, 2), n)
  fftCase('huge', randomSignal(n, 3), n)
}
fftCase('neg_zero', new Float64Array(64).fill(-0), 64)

// ---- detectTransient: exact score by bisection over [+0, +Inf]
function scoreOf(c, p) {
  if (!p || detectTransient(c, p, -Infinity) === false) return NaN
  let lo = 0n, hi = 0x7ff0000000000000n                     // smallest t with !(score > t) is the score itself
  if (detectTransient(c, p, Infinity)) throw new Error('score above +Inf')
  while (lo < hi) {
    const mid = (lo + hi) >> 1n
    if (detectTransient(c, p, fromBits(mid))) lo = mid + 1n
    else hi = mid
  }
  return fromBits(lo)
}
const detect = []
function detectCase(name, c, p, thresholds) {
  const score = put([scoreOf(c, p)])[0], cw = put(Array.from(c)), pw = p ? put(Array.from(p)) : null
  for (const t of thresholds) detect.push({ name, c: cw, p: pw, t: put([t])[0], r: detectTransient(c, p, t), s: score })
}
{
  const size = 256
  const silent = performFFT(new Float32Array(size), size), stepC = performFFT(step(0, size), size)
  const sineC = performFFT(sine(440, size), size), sine2 = performFFT(sine(880, size), size)
  detectCase('step_after_silence', stepC, silent, [0.1, 0.01])
  detectCase('sine_after_sine', sineC, sineC, [0.01])
  detectCase('sine_change', sine2, sineC, [0.1])
  detectCase('step_after_silence_thresholds', stepC, silent, [0.05, 0.5, 1, 10])
  detectCase('null_prev', sineC, null, [10, -Infinity])
  detectCase('empty_both', new Float32Array(0), new Float32Array(0), [10, 0, -1])
  detectCase('empty_prev', sineC, new Float32Array(0), [0.1])
  detectCase('zero_prev', sineC, new Float32Array(size / 2), [99999, 0.5])
  const mags = (n, kind) => Float32Array.from(randomSignal(n, kind), Math.abs)
  for (let i = 0; i < 40; i++) {
    const n = pick([1, 2, 3, 7, 64, 65, 128, 255, 256])
    const m = pick([n, n, n, 0, 1, n - 1, n + 1, n + 5, Math.max(0, n >> 1), 2 * n])
    const kc = pick([0, 0, 1, 2, 3]), kp = pick([0, 0, 1, 2, 3])
    const c = rnd() < 0.5 ? mags(n, kc) : randomSignal(n, kc)
    const p = rnd() < 0.5 ? mags(m, kp) : randomSignal(Math.max(0, m), kp)
    detectCase('random', c, p, [pick([0.1, 0.3, 0.5, 1, 2]), NaN, rnd()])
  }
  detectCase('nan_energy', Float64Array.of(NaN, 1, 2, 3), Float64Array.of(1, 2, 3, 4), [0.1, -1])
  detectCase('inf_bins', Float64Array.of(Infinity, 1, 2, 3), Float64Array.of(1, 2, 3, 4), [0.1])
  detectCase('prev_inf', Float64Array.of(1, 2, 3, 4), Float64Array.of(Infinity, 1, 2, 3), [0.1])
  detectCase('signed_zeros', Float64Array.of(-0, 0, -0, 0), Float64Array.of(0, -0, 0, -0), [0, -1])
  detectCase('tiny_bins', Float64Array.of(1e-11, -1e-11, 5e-324, 1e-10), Float64Array.of(1e-12, 0, 0, 1e-10), [0.01])
  detectCase('negative_values', Float64Array.of(-1, -2, 3, -4, 5), Float64Array.of(1, -2, -3, 4, -5), [0.1])
  detectCase('prev_shorter', Float64Array.of(1, 2, 3, 4, 5), Float64Array.of(1, 2), [0.1, 1e300])
  detectCase('prev_longer', Float64Array.of(1, 2), Float64Array.of(1, 2, 3, 4, 5, 6, 7), [0.1])
}

// ---- findScaleFactor
const sf = []
function sfCase(name, x, len) {
  sf.push({ name, x: put(Array.from(x)), len, r: findScaleFactor(x, len) })
}
for (let i = 0; i < 64; i++) {
  for (let k = -4; k <= 4; k++) {
    sfCase('boundary_f64', Float64Array.of(0.5 * SCALE_FACTORS[0], ulps(SCALE_FACTORS[i], k)), 2)
    sfCase('boundary_f32', Float32Array.of(ulps32(Math.fround(SCALE_FACTORS[i]), k)), 1)
  }
}
for (let i = 0; i < 200; i++) {
  const n = pick([0, 1, 4, 8, 20])
  const x = rnd() < 0.5 ? Float32Array.from(randomSignal(n, pick([0, 1, 2, 3]))) : randomSignal(n, pick([0, 1, 2, 3]))
  sfCase('random', x, pick([n, n, n + 3, n - 1, 0, -2]))
}
sfCase('reference_test', Float32Array.of(0.01, 0.05, 0.1, 0.2), 4)
sfCase('inf', Float64Array.of(1, Infinity), 2)
sfCase('neg_inf', Float64Array.of(-Infinity), 1)
sfCase('nan_only', Float64Array.of(NaN, NaN), 2)
sfCase('nan_then_value', Float64Array.of(NaN, 0.25), 2)
sfCase('zeros', Float64Array.of(-0, 0), 2)
sfCase('denormal', Float64Array.of(5e-324), 1)
sfCase('f32_denormal', Float32Array.of(1e-45), 1)
sfCase('beyond', Float64Array.of(0.5, 0.25), 10)
sfCase('negative_length', Float64Array.of(0.5), -1)
sfCase('huge', Float64Array.of(1e300), 1)

// ---- allocateBits
const alloc = []
const tables = {}
function table(bias) {
  if (!tables[bias]) tables[bias] = put(Array.from(SCALE_FACTORS, (x) => (bias === 1 ? x : Math.pow(x, bias))))[0]
  return tables[bias]
}
function allocCase(name, bfuData, sizes, mb, bias) {
  const res = allocateBits(bfuData, sizes, mb, bias)
  const data = []
  for (let i = 0; i < Math.min(mb, bfuData.length); i++) data.push(put(Array.from(bfuData[i])))
  alloc.push({ name, bias, table: table(bias), mb, sizes: Array.from({ length: mb }, (_, i) => sizes[i] | 0), data,
    count: res.bfuCount, wl: Array.from(res.allocation), sfi: Array.from(res.scaleFactorIndices) })
}
{
  const sizes10 = new Array(52).fill(10)
  allocCase('reference_ones', sizes10.map((n) => new Float32Array(n).fill(1)), sizes10, 52, 1.0)
  allocCase('reference_zeros', sizes10.map((n) => new Float32Array(n).fill(0)), sizes10, 52, 1.0)
  allocCase('reference_energy', sizes10.map((n, i) => new Float32Array(n).fill(i < 5 ? 2.0 : i < 10 ? 1.0 : 0.1)), sizes10, 52, 1.0)
  const specs = Array.from(SPECS_PER_BFU)
  for (const bias of [0, 1, 2, 3, 4, 5]) {
    for (let k = 0; k < 5; k++) {
      const mb = k === 0 ? 52 : pick([0, 5, 19, 20, 21, 28, 33, 40, 47, 52])
      const sizes = specs.map((n) => (rnd() < 0.15 ? pick([0, -3, 21, 25, 1, 40]) : n))
      const bfus = sizes.map((n) => {
        const len = rnd() < 0.15 ? Math.max(0, n - 2) : Math.max(0, n)
        return rnd() < 0.5 ? Float32Array.from(randomSignal(len, pick([0, 0, 1, 2])), (v) => v * Math.pow(2, -20 * rnd())) : randomSignal(len, pick([0, 2]))
      })
      allocCase('random', bfus, sizes, mb, bias)
    }
  }
  allocCase('all_zero_sizes', specs.map((n) => new Float32Array(n).fill(1)), new Array(52).fill(0), 52, 1)
  allocCase('negative_sizes', specs.map((n) => new Float32Array(n).fill(0.5)), specs.map((n, i) => (i % 2 ? -n : n)), 52, 1)
  allocCase('large_sizes', specs.map(() => new Float32Array(20).fill(0.25)), new Array(52).fill(200), 52, 1)
  allocCase('huge_values', specs.map((n) => new Float64Array(n).fill(1e300)), specs, 52, 5)
  allocCase('inf_values', specs.map((n) => Float64Array.of(Infinity, ...new Array(n - 1).fill(1))), specs, 52, 2)
  allocCase('nan_values', specs.map((n) => new Float64Array(n).fill(NaN)), specs, 52, 1)
  allocCase('short_arrays', specs.map(() => Float64Array.of(0.5)), specs, 52, 1)
  allocCase('mb_below_20', specs.map((n) => new Float32Array(n).fill(1)), specs, 19, 1)
  allocCase('mb_zero', [], [], 0, 1)
  allocCase('bias_0.5', specs.map((n) => Float32Array.from(randomSignal(n, 0))), specs, 52, 0.5)
}

const log2Pairs = put(log2)
const bin = Buffer.alloc(8 * words.length)
words.forEach((v, i) => bin.writeDoubleLE(v, 8 * i))
fs.writeFileSync(path.join(OUT, 'decision.bin'), bin)
fs.writeFileSync(path.join(OUT, 'decision.json'), JSON.stringify({ log2: log2Pairs, fft, detect, sf, alloc, tables }) + '\n')
console.log('words', words.length, 'fft', fft.length, 'detect', detect.length, 'sf', sf.length, 'alloc', alloc.length, 'log2', log2.length / 2)
