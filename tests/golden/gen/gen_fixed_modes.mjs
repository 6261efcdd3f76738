// Golden vectors over the whole fixedBlockModes domain the encoder accepts: low and mid band 0..2, high band 0..3, all 36
// triples (encoder.js:131 takes the option as is; quantization.js:117 and the MDCT test blockMode === 0;
// serialization.js:48-50 writes 2 - m, 2 - m, 3 - m).  Runs the JavaScript reference in place from /root/reference through
// loader.mjs and writes data only:
//   tests/golden/fixed_modes.json          cases and hashes
//   tests/golden/fixed_modes_digests.bin   per unit of every case, in case order: the first 2 bytes of its SHA-256
//
//   cd tests/golden/gen && node --experimental-loader ./loader.mjs gen_fixed_modes.mjs
//
// Per triple one stereo case of 40 frames of the `patch` material (80 units: just above the 64 from which the library
// speculates) with its own seed, at allocationBias 1, with a halo cut inside; and for four triples outside the canonical
// six a mono case of 3 frames.  The input generator is gen_option_domain.mjs's (hash32 / material), so
// tests/option_domain_lib.py rebuilds every input bit for bit; the SHA-256 of every input is recorded to prove it.
import fs from 'fs'
import path from 'path'
import crypto from 'crypto'
import { fileURLToPath } from 'url'

import { encode } from '/root/reference/codec/pipeline/encoder.js'
import { decode } from '/root/reference/codec/pipeline/decoder.js'
import { serializeFrame, deserializeFrame } from '/root/reference/codec/io/serialization.js'
import { EncoderOptions } from '/root/reference/codec/core/options.js'

const OUT = path.resolve(path.dirname(fileURLToPath(import.meta.url)), '..')
const sha = (buf) => crypto.createHash('sha256').update(buf).digest('hex')
const bytesOf = (ta) => Buffer.from(ta.buffer, ta.byteOffset, ta.byteLength)

const FRAMES = 40, SHORT_FRAMES = 3
const SHORT_TRIPLES = [[1, 1, 1], [1, 0, 2], [2, 2, 1], [0, 1, 0]]
const PATCH_SPEC = { kind: 'patch' }

// ---- inputs (gen_option_domain.mjs's, restated in tests/option_domain_lib.py; keep the three in step) ----
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

// ---- the reference ----
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
  note: 'generated by tests/golden/gen/gen_fixed_modes.mjs from the reference encoder; inputs: the patch material of ' +
        'tests/option_domain_lib.py, channel c from seed + 7919 c. pcm_sha256: the decoded Float32 PCM, per frame L then R; ' +
        'halo: encode frames cut.. from the input starting at frame cut - halo; header: the first two bytes of the first unit (hex)',
  cases: [],
}
const digests = []
function addCase(modes, frames, nch) {
  const ci = out.cases.length
  const opts = { fixedBlockModes: modes, allocationBias: 1 }
  const h = key(base(ci, 91), 0)
  const seed = 5000 + ci
  const chs = []
  for (let c = 0; c < nch; c++) chs.push(material(PATCH_SPEC, seed + 7919 * c, 0, frames * 512))
  const units = encodeStream(chs, frames, opts)
  const pcm = decodeStream(units, nch, frames)
  const cut = 1 + h % (frames - 1)
  const all = Buffer.concat(units)
  out.cases.push({
    id: ci, bias: '1', options: opts, material: PATCH_SPEC, seed, frames, channels: nch,
    input_sha256: chs.map((x) => sha(bytesOf(x))),
    cut, halo: Math.min(2, cut), header: units[0].subarray(0, 2).toString('hex'),
    units_sha256: sha(all), pcm_sha256: sha(bytesOf(pcm)),
  })
  for (const u of units) digests.push(crypto.createHash('sha256').update(u).digest().subarray(0, 2))
}
for (let m0 = 0; m0 < 3; m0++) for (let m1 = 0; m1 < 3; m1++) for (let m2 = 0; m2 < 4; m2++) addCase([m0, m1, m2], FRAMES, 2)
for (const m of SHORT_TRIPLES) addCase(m, SHORT_FRAMES, 1)

fs.writeFileSync(path.join(OUT, 'fixed_modes_digests.bin'), Buffer.concat(digests))
fs.writeFileSync(path.join(OUT, 'fixed_modes.json'), '{\n "note": ' + JSON.stringify(out.note) + ',\n "cases": [\n' +
  out.cases.map((c) => '  ' + JSON.stringify(c)).join(',\n') + ']}\n')
console.log('wrote fixed_modes.json:', out.cases.length, 'cases,', digests.length, 'units')
