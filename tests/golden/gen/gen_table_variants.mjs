// Golden vectors of the reference under tables another engine could build.  c1_set_tables() installs the sine, cosine and pow
// tables of the host's own engine (carta1_amd/js/native.js); these fixtures pin what the reference computes when its Math.sin,
// Math.cos and Math.pow return other values.  Runs the JavaScript reference in place from /root/reference through loader.mjs,
// one node process per variant: the child replaces Math.sin / cos / pow by deterministic wrappers BEFORE it loads the
// reference with import() (constants.js and mdct.js build their tables at load; fft.js:38-39 calls Math.cos / sin on every
// transform, so the wrappers stay installed).  Math.log2, sqrt and log1p are left alone.  Writes data only:
//   tests/golden/table_variants.json        per variant: the tables the reference built (c1_tables order, binary64 hex),
//                                           the gates it is meant to hit, case metadata, how many outputs differ from the
//                                           default tables' and the offsets into the .bin
//   tests/golden/table_variants_<v>.bin     per variant: the four KAT streams' units; the first 8 bytes of the SHA-256 of
//                                           every decoded frame per channel; quantizationStage on crafted coefficient
//                                           frames (inputs and fields); quantize() at crafted points (inputs and outputs)
//
//   cd tests/golden/gen && node --experimental-loader ./loader.mjs gen_table_variants.mjs
//
// Inputs come from xorshift32 and exact arithmetic only (they never call the patched functions).
import fs from 'fs'
import path from 'path'
import crypto from 'crypto'
import { execFileSync } from 'child_process'
import { fileURLToPath } from 'url'

import { install, floorF32, ceilF32 } from './table_variant_math.mjs'

const HERE = path.dirname(fileURLToPath(import.meta.url))
const OUT = path.resolve(HERE, '..')
const sha = (buf) => crypto.createHash('sha256').update(buf).digest('hex')
const bytesOf = (ta) => Buffer.from(ta.buffer, ta.byteOffset, ta.byteLength)
const f64hex = (x) => { const b = Buffer.alloc(8); b.writeDoubleBE(x); return b.toString('hex') }

// name -> what the wrappers change, and the gates of the library (c1_table_fast_paths: scale_factor_bits; the speculative
// paths) each variant is built to hit
const VARIANTS = {
  ulp: { note: '+-1 ulp on about 2/3 of the sin, cos and non-integer-exponent pow results (another libm)', gates: { sf_fast: 1, spec_ok: 1 } },
  inside: { note: 'MDCT / window sin and cos up to 1e-10 relative, FFT (cos, sin)(-2 pi / stride) up to 2 ulps, the scale factors ' +
                  'i % 3 != 0 moved inside their binary32 cell', gates: { sf_fast: 1, spec_ok: 1 } },
  sfshift: { note: 'every i % 3 == 1 scale factor times (1 + 2^-20): out of its binary32 cell, the same in every octave', gates: { sf_fast: 1, spec_ok: 1 } },
  sfpow2: { note: 'pow(2, e) one ulp low for the integers e = -21 .. -17: SCALE_FACTORS[0, 3, .., 12] (INV_POWER_OF_TWO, e = 0 .. -16, ' +
                  'is compiled into the library and left alone)', gates: { sf_fast: 0, spec_ok: 0 } },
  twiddle: { note: 'FFT (cos, sin)(-2 pi / stride) about 1e-9 relative off', gates: { sf_fast: 1, spec_ok: 0 } },
}

// ---- inputs: gen_golden.mjs's xorshift32 signals ----
function xorshift(seed) {
  let s = seed >>> 0
  return () => { s ^= s << 13; s >>>= 0; s ^= s >>> 17; s ^= s << 5; s >>>= 0; return s }
}
const unit = (r) => (r / 4294967296) * 2 - 1
function white(seed, n) {
  const r = xorshift(seed); const x = new Float32Array(n)
  for (let i = 0; i < n; i++) x[i] = Math.fround(unit(r()) * 0.5)
  return x
}
function pinkT(seed, n) {
  const r = xorshift(seed); const x = new Float32Array(n); let p = 0
  for (let i = 0; i < n; i++) {
    const u = unit(r()); p = 0.98 * p + 0.05 * u; let v = p
    if ((i >> 9) % 8 === 5 && (i % 512) >= 256) v += 0.8 * unit(r())
    x[i] = v
  }
  return x
}
const FRAMES = 64
const KAT = [
  ['white_m000', 'white', { fixedBlockModes: [0, 0, 0] }],
  ['white_m223', 'white', { fixedBlockModes: [2, 2, 3] }],
  ['pinkT_detect', 'pinkT', {}],
  ['pinkT_detect_thr0.3', 'pinkT', { transientThresholdLow: 0.3 }],
]
const FFT_CASES = [[8, 42], [64, 43], [256, 44]]           // (n, seed): real part white(seed, n), imaginary white(seed + 100, n)
const MDCT_MODES = [[0, 0, 0], [2, 2, 3]]
const FIELDS_FRAMES = 12                                      // the hand-built frames of decoder_stages_fields.bin
const kat64Name = { white_m000: 'white_m000_b1', white_m223: 'white_m223_b1', pinkT_detect: 'pinkT_detect', 'pinkT_detect_thr0.3': 'pinkT_detect_thr0.3' }

// ---- the child: one variant ----
async function child(variant) {
  if (variant !== 'default') install(variant)
  const K = await import('/root/reference/codec/core/constants.js')
  const M = await import('/root/reference/codec/transforms/mdct.js')
  const { encode, quantizationStage } = await import('/root/reference/codec/pipeline/encoder.js')
  const { decode } = await import('/root/reference/codec/pipeline/decoder.js')
  const { serializeFrame, deserializeFrame } = await import('/root/reference/codec/io/serialization.js')
  const { EncoderOptions } = await import('/root/reference/codec/core/options.js')
  const { quantize } = await import('/root/reference/codec/coding/quantization.js')
  const { qmfAnalysisStage, mdctStage } = await import('/root/reference/codec/pipeline/encoder.js')
  const { dequantizationStage, imdctStage, qmfSynthesisStage } = await import('/root/reference/codec/pipeline/decoder.js')
  const { BufferPool } = await import('/root/reference/codec/core/buffers.js')
  const { FFT } = await import('/root/reference/codec/transforms/fft.js')
  const { performFFT } = await import('/root/reference/codec/analysis/transient.js')
  const d8 = (ta) => crypto.createHash('sha256').update(bytesOf(ta)).digest().subarray(0, 8)

  // the tables in c1_tables order, as the reference built them
  const w = []
  for (let stride = 2; stride <= 256; stride <<= 1) { const a = (-2 * Math.PI) / stride; w.push(Math.cos(a), Math.sin(a)) }
  const tables = [...K.SCALE_FACTORS, ...K.WINDOW_SHORT, ...M.mdct64.sinCosTable, ...M.mdct256.sinCosTable, ...M.mdct512.sinCosTable,
                  ...M.imdct64.sinCosTable, ...M.imdct256.sinCosTable, ...M.imdct512.sinCosTable, ...w, Math.log1p(10)]
  const SF = K.SCALE_FACTORS
  const parts = []
  const out = { tables_f64: tables.map(f64hex), biased_b1_f64: Array.from(SF).map(f64hex), kat: {}, offsets: {} }
  const put = (key, ta) => { out.offsets[key] = [parts.reduce((n, p) => n + p.length, 0), ta.byteLength]; parts.push(Buffer.from(bytesOf(ta))) }

  // 1. the KAT streams: two independent encoders, units interleaved L, R; decoded per frame and channel
  for (const [name, sig, opts] of KAT) {
    const n = FRAMES * 512
    const chs = sig === 'white' ? [white(1, n), white(2, n)] : [pinkT(3, n), pinkT(4, n)]
    const encs = chs.map(() => encode(new EncoderOptions(opts)))
    const decs = chs.map(() => decode())
    const units = new Uint8Array(FRAMES * 2 * 212), dig = new Uint8Array(FRAMES * 2 * 8)
    const pcmAll = [new Float32Array(n), new Float32Array(n)]
    for (let f = 0; f < FRAMES; f++)
      for (let c = 0; c < 2; c++) {
        const u = serializeFrame(encs[c](chs[c].slice(f * 512, (f + 1) * 512)))
        units.set(u, (f * 2 + c) * 212)
        const pcm = decs[c](deserializeFrame(u))
        pcmAll[c].set(pcm, f * 512)
        dig.set(crypto.createHash('sha256').update(bytesOf(pcm)).digest().subarray(0, 8), (f * 2 + c) * 8)
      }
    out.kat[name] = { signal: sig, options: opts, frames: FRAMES, input_sha256: chs.map((c) => sha(bytesOf(c))),
                      units_sha256: sha(units), decoded_sha256: pcmAll.map((c) => sha(bytesOf(c))), kat64: kat64Name[name] }
    put(`kat_${name}_units`, units)
    put(`kat_${name}_pcm8`, dig)
  }

  // 2. quantizationStage (bias 1: SCALE_FACTORS itself) on frames whose BFU maxima sit on the scale-factor boundaries:
  // 2^k, this table's SCALE_FACTORS[i], its binary32 floor and ceiling, and one binary32 ulp either side of those
  const targets = []
  for (let k = -22; k <= 0; k++) targets.push(2 ** k)
  const F32 = new Float32Array(1)
  const f32ulp = (x, k) => { F32[0] = x; const u = new Uint32Array(F32.buffer); u[0] += k; return F32[0] }
  for (let i = 0; i < 64; i++) {
    const lo = floorF32(SF[i]), hi = ceilF32(SF[i])
    targets.push(Math.fround(SF[i]), lo, hi, f32ulp(lo, -1), f32ulp(hi, 1), f32ulp(lo, 1), f32ulp(hi, -1))
  }
  const MODES = [[0, 0, 0], [2, 2, 3]]
  const qframes = []
  const rnd = xorshift(4242)
  const F = Math.ceil(targets.length / 52) * MODES.length
  for (let f = 0; f < F; f++) {
    const x = new Float32Array(512)
    for (let b = 0; b < 52; b++) {
      const t = targets[((f % Math.ceil(targets.length / 52)) * 52 + b) % targets.length]
      const mode = MODES[Math.floor(f / Math.ceil(targets.length / 52))][b >= 36 ? 2 : (b >= 20 ? 1 : 0)]
      const at = (mode === 0 ? K.BFU_START_LONG : K.BFU_START_SHORT)[b], len = K.SPECS_PER_BFU[b]       // groupIntoBFUs' layout
      const peak = (rnd() % len)
      for (let j = 0; j < len; j++) {
        const s = (rnd() & 1) ? -1 : 1
        x[at + j] = j === peak ? s * t : Math.fround(s * t * ((rnd() >>> 8) / 16777216) * 0.999)
      }
    }
    qframes.push({ x, modes: MODES[Math.floor(f / Math.ceil(targets.length / 52))] })
  }
  const qs = quantizationStage({ options: new EncoderOptions({}) })
  const qin = new Float32Array(F * 512), qmodes = new Int32Array(F * 3), qfields = new Int32Array(F * (1 + 52 + 52 + 512))
  qframes.forEach((fr, f) => {
    qin.set(fr.x, f * 512); qmodes.set(fr.modes, f * 3)
    const q = qs({ coefficients: fr.x.slice(), blockModes: Array.from(fr.modes) })
    const o = f * 617
    qfields[o] = q.nBfu
    let at = 0
    for (let b = 0; b < 52; b++) {
      if (b < q.nBfu) {
        qfields[o + 1 + b] = q.scaleFactorIndices[b]
        qfields[o + 53 + b] = q.wordLengthIndices[b]
        for (let j = 0; j < K.SPECS_PER_BFU[b]; j++) qfields[o + 105 + at + j] = q.quantizedCoefficients[b][j]
      }
      at += K.SPECS_PER_BFU[b]
    }
  })
  out.quant_frames = F
  put('quant_coefs', qin); put('quant_modes', qmodes); put('quant_fields', qfields)

  // 3. quantize() at the rounding midpoints of this table's normFactor = range / SCALE_FACTORS[sfi], and a binary32 ulp either side
  const pts = [], psfi = [], pbits = []
  for (let s = 1; s < 64; s++)
    for (const bits of [2, 3, 4, 6, 9, 12, 16]) {
      const range = (1 << (bits - 1)) - 1
      for (let r = 0; r < 2; r++) {
        const k = rnd() % range, sgn = (rnd() & 1) ? -1 : 1
        const mid = Math.fround(sgn * (k + 0.5) * SF[s] / range)
        for (const d of [-1, 0, 1]) { pts.push(f32ulp(mid, d)); psfi.push(s); pbits.push(bits) }
      }
    }
  const qx = Float32Array.from(pts), qsfi = Int32Array.from(psfi), qbits = Int32Array.from(pbits), qy = new Int32Array(pts.length)
  for (let i = 0; i < pts.length; i++) qy[i] = quantize(qx.subarray(i, i + 1), qsfi[i], qbits[i])[0]
  out.quantize_points = pts.length
  put('quantize_x', qx); put('quantize_sfi', qsfi); put('quantize_bits', qbits); put('quantize_q', qy)

  // 4. the stage functions under this table: performFFT's magnitudes (the transient detector's FFT) over 8 frames of
  // pinkT(3); FFT.fft on white(seed) pairs (its w from this engine's Math.cos / sin at run time, fft.js:37-39);
  // qmfAnalysisStage -> mdctStage over 4 frames of white(51) in two block-mode sets; and the decoder's stages
  // (dequantizationStage -> imdctStage -> qmfSynthesisStage, decoder.js) over the hand-built frame fields of
  // decoder_stages_fields.bin, kept as the first 8 bytes of the SHA-256 of each frame's coefficients, bands and PCM
  {
    const p = pinkT(3, 8 * 512)
    const qa = qmfAnalysisStage({ bufferPool: new BufferPool(), options: new EncoderOptions({}) })
    const mags = new Float32Array(8 * 256)
    for (let f = 0; f < 8; f++) {
      const a = qa(p.slice(f * 512, (f + 1) * 512))
      mags.set(performFFT(a.bands[0], 128), f * 256)
      mags.set(performFFT(a.bands[1], 128), f * 256 + 64)
      mags.set(performFFT(a.bands[2], 256), f * 256 + 128)
    }
    put('stage_mags', mags)
  }
  {
    const fft = []
    for (const [n, seed] of FFT_CASES) {
      const re = white(seed, n), im = white(seed + 100, n)
      FFT.fft(re, im)
      fft.push(...re, ...im)
    }
    put('stage_fft', Float32Array.from(fft))
  }
  {
    const coefs = new Float32Array(MDCT_MODES.length * 4 * 512)
    MDCT_MODES.forEach((modes, m) => {
      const context = { bufferPool: new BufferPool() }
      const qa = qmfAnalysisStage(context), md = mdctStage(context)
      const pcm = white(51, 4 * 512)
      for (let f = 0; f < 4; f++) {
        const a = qa(pcm.subarray(f * 512, (f + 1) * 512))
        coefs.set(md({ bands: a.bands, blockModes: modes, originalFrame: null }).coefficients, (m * 4 + f) * 512)
      }
    })
    put('stage_mdct', coefs)
  }
  {
    const raw = fs.readFileSync(path.join(OUT, 'decoder_stages_fields.bin'))
    const n = FIELDS_FRAMES
    if (raw.length !== n * (1 + 3 + 52 + 52 + 512 * 4) * 4) throw new Error('decoder_stages_fields.bin: unexpected size')
    const i32 = new Int32Array(raw.buffer.slice(raw.byteOffset, raw.byteOffset + raw.length))
    const context = { bufferPool: new BufferPool() }
    const dq = dequantizationStage(), im = imdctStage(context), qsyn = qmfSynthesisStage(context)
    const dig = new Uint8Array(n * 3 * 8)
    for (let f = 0; f < n; f++) {
      const q = i32.subarray(108 * n + f * 512, 108 * n + (f + 1) * 512), quantizedCoefficients = []
      for (let b = 0, at = 0; b < 52; b++) { quantizedCoefficients.push(Int32Array.from(q.subarray(at, at + K.SPECS_PER_BFU[b]))); at += K.SPECS_PER_BFU[b] }
      const fd = { nBfu: i32[f], blockModes: Array.from(i32.subarray(n + 3 * f, n + 3 * f + 3)),
                   scaleFactorIndices: Int32Array.from(i32.subarray(4 * n + 52 * f, 4 * n + 52 * (f + 1))),
                   wordLengthIndices: Int32Array.from(i32.subarray(56 * n + 52 * f, 56 * n + 52 * (f + 1))), quantizedCoefficients }
      const d = dq(fd)
      const coefficients = Float32Array.from(d.coefficients)
      const b = im(d)
      const bands = new Float32Array(512)
      bands.set(b[0], 0); bands.set(b[1], 128); bands.set(b[2], 256)
      const pcm = Float32Array.from(qsyn(b))
      dig.set(d8(coefficients), (f * 3) * 8); dig.set(d8(bands), (f * 3 + 1) * 8); dig.set(d8(pcm), (f * 3 + 2) * 8)
    }
    put('stage_decoder_d8', dig)
  }

  const bin = Buffer.concat(parts)
  fs.writeFileSync(path.join(OUT, `table_variants_${variant}.bin`), bin)
  process.stdout.write(JSON.stringify(out))
}

// ---- the parent: every variant in a process of its own, then what each changes against the default tables ----
function parent() {
  const run = (v) => JSON.parse(execFileSync(process.execPath, ['--no-warnings', '--experimental-loader', './loader.mjs', 'gen_table_variants.mjs', v],
                                             { cwd: HERE, maxBuffer: 1 << 26 }).toString())
  const def = run('default')
  const defBin = fs.readFileSync(path.join(OUT, 'table_variants_default.bin'))
  fs.unlinkSync(path.join(OUT, 'table_variants_default.bin'))
  const slice = (bin, o) => bin.subarray(o[0], o[0] + o[1])
  const result = { note: 'tests/golden/gen/gen_table_variants.mjs', frames: FRAMES, fft_cases: FFT_CASES, mdct_modes: MDCT_MODES,
                   fields_frames: FIELDS_FRAMES, variants: {} }
  for (const [v, meta] of Object.entries(VARIANTS)) {
    const r = run(v)
    const bin = fs.readFileSync(path.join(OUT, `table_variants_${v}.bin`))
    const differs = { tables: r.tables_f64.filter((h, i) => h !== def.tables_f64[i]).length }
    for (const [key, o] of Object.entries(r.offsets)) {
      const a = slice(bin, o), b = slice(defBin, def.offsets[key])
      const step = key.endsWith('_units') ? 212 : (key.endsWith('_pcm8') || key.endsWith('_d8') ? 8 : (key === 'quant_fields' ? 617 * 4 : 4))
      let n = 0
      for (let i = 0; i < a.length; i += step) if (a.subarray(i, i + step).compare(b.subarray(i, i + step)) !== 0) n++
      differs[key] = n
    }
    result.variants[v] = { ...meta, ...r, differs_from_default: differs }
  }
  fs.writeFileSync(path.join(OUT, 'table_variants.json'), JSON.stringify(result, null, 1) + '\n')
  for (const [v, r] of Object.entries(result.variants)) console.log(v, JSON.stringify(r.differs_from_default))
}

if (process.argv[2]) child(process.argv[2]).catch((e) => { console.error(e); process.exit(1) })
else parent()
