// Golden vectors for serializeFrame (codec/io/serialization.js:41-98), the inverse of deserializeFrame.  Runs the JavaScript
// reference in place from /root/reference through loader.mjs and writes tests/golden/pack_units.json plus one
// pack_units_<case>.bin per case -- inputs and outputs only, never reference source text.
//
//   cd tests/golden/gen && node --experimental-loader ./loader.mjs gen_pack_units.mjs
//
// Cases:
//  - canonical fields: deserializeFrame of the first frames of channel 0 of two KAT unit files (one with transient detection
//    and short blocks, one all long), and quantizationStage's output on the reference's own qmf / block selection / MDCT
//    chain at allocation biases 0.5, 1 and 2;
//  - hand-built fields: nBfu 0, 1, 19, 21 and 52; block modes 1, -1, 5, 7, INT32_MIN and INT32_MAX; word lengths 16, 31, -1
//    and INT32_MIN among others; scale factors 64, -1 and 2^31-1; mantissas beyond their word length and at the int32 ends;
//    streams that end exactly at bit 1672, inside the zeroed last three bytes, and far past bit 1696 (nBfu 52, every wl 15);
//  - random fields: every value a random int32 or an edge value, nBfu 0..52.
// Entries the reference does not read (BFUs at or above nBfu) are random too in the hand-built and random cases.
import fs from 'fs'
import path from 'path'
import { fileURLToPath } from 'url'

import { BufferPool } from '/root/reference/codec/core/buffers.js'
import { EncoderOptions } from '/root/reference/codec/core/options.js'
import { SPECS_PER_BFU } from '/root/reference/codec/core/constants.js'
import { serializeFrame, deserializeFrame } from '/root/reference/codec/io/serialization.js'
import { qmfAnalysisStage, blockSelectorStage, mdctStage, quantizationStage } from '/root/reference/codec/pipeline/encoder.js'

const OUT = path.resolve(path.dirname(fileURLToPath(import.meta.url)), '..')
const FRAMES_KAT = 16
const FRAMES_QUANT = 16
const FRAMES_RANDOM = 64
const I32_MIN = -2147483648, I32_MAX = 2147483647
const FIRST = [0]
for (let b = 0; b < 52; b++) FIRST.push(FIRST[b] + SPECS_PER_BFU[b])

// xorshift32 (SURVEY.md 8c); the pinkT KAT signal of gen_golden.mjs
function xorshift(seed) {
  let s = seed >>> 0
  return () => { s ^= s << 13; s >>>= 0; s ^= s >>> 17; s ^= s << 5; s >>>= 0; return s }
}
const unit = (r) => () => (r() / 4294967296) * 2 - 1
function pinkT(seed, n) {
  const r = unit(xorshift(seed)); const x = new Float32Array(n); let p = 0
  for (let i = 0; i < n; i++) {
    const u = r(); p = 0.98 * p + 0.05 * u; let v = p
    if ((i >> 9) % 8 === 5 && (i % 512) >= 256) v += 0.8 * r()
    x[i] = v
  }
  return x
}

// the library's frame-field layout (include/carta1_hip.h) of a reference-shaped frameData: zeros where it has no entries
function toFields(fd) {
  const f = { nbfu: new Int32Array([fd.nBfu]), block_modes: Int32Array.from(fd.blockModes), sfi: new Int32Array(52),
              wl: new Int32Array(52), quantized: new Int32Array(512) }
  for (let b = 0; b < 52; b++) {
    if (b < fd.scaleFactorIndices.length) f.sfi[b] = fd.scaleFactorIndices[b]
    if (b < fd.wordLengthIndices.length) f.wl[b] = fd.wordLengthIndices[b]
    if (b < fd.quantizedCoefficients.length) f.quantized.set(fd.quantizedCoefficients[b], FIRST[b])
  }
  return f
}
// and back: all 52 BFUs of every array, as the reference would be handed them
function toFrameData(f) {
  return { nBfu: f.nbfu[0], blockModes: Array.from(f.block_modes), scaleFactorIndices: f.sfi.slice(), wordLengthIndices: f.wl.slice(),
           quantizedCoefficients: Array.from(SPECS_PER_BFU, (n, b) => f.quantized.slice(FIRST[b], FIRST[b] + n)) }
}

const ARRAYS = [['nbfu', 'int32', []], ['block_modes', 'int32', [3]], ['sfi', 'int32', [52]], ['wl', 'int32', [52]],
                ['quantized', 'int32', [512]], ['units', 'uint8', [212]]]

function writeCase(name, rows, extra) {
  const parts = [], arrays = []
  for (const [key, dtype, shape] of ARRAYS) {
    const per = shape.length ? shape[0] : 1
    const ta = dtype === 'int32' ? new Int32Array(rows.length * per) : new Uint8Array(rows.length * per)
    rows.forEach((r, i) => ta.set(r[key], i * per))
    parts.push(Buffer.from(ta.buffer))
    arrays.push({ name: key, dtype, shape: [rows.length, ...shape] })
  }
  const file = `pack_units_${name}.bin`
  fs.writeFileSync(path.join(OUT, file), Buffer.concat(parts))
  return { name, file, frames: rows.length, arrays, ...extra }
}

// one row: the fields and what the reference's serializeFrame makes of them
function row(fd) {
  const fields = toFields(fd)
  return { ...fields, units: serializeFrame(fd) }
}
function rowOfFields(f) {
  return { ...f, units: serializeFrame(toFrameData(f)) }
}

const out = { note: 'each case: little-endian arrays concatenated in `arrays` order in `file`; units = serializeFrame of the ' +
                    'fields; fields zero where a canonical frameData has no entries', cases: [] }

// ---- canonical fields ----
for (const kat of ['pinkT_detect', 'white_m000_b1']) {
  const units = fs.readFileSync(path.join(OUT, `kat64_${kat}.units.bin`))
  const rows = []
  for (let f = 0; f < FRAMES_KAT; f++) {
    const at = (2 * f) * 212                                   // channel 0 of the interleaved stereo units
    rows.push(row(deserializeFrame(new Uint8Array(units.buffer, units.byteOffset + at, 212).slice())))
  }
  out.cases.push(writeCase(`kat_${kat}`, rows, { kind: 'canonical', source: `kat64_${kat}.units.bin`, channel: 0, channels: 2, first_frame: 0 }))
}
for (const bias of [0.5, 1, 2]) {
  const pcm = pinkT(3, FRAMES_QUANT * 512)
  const context = { options: new EncoderOptions({ allocationBias: bias }), bufferPool: new BufferPool() }
  const qa = qmfAnalysisStage(context), bs = blockSelectorStage(context), md = mdctStage(context), qs = quantizationStage(context)
  const rows = []
  for (let f = 0; f < FRAMES_QUANT; f++) rows.push(row(qs(md(bs(qa(pcm.slice(f * 512, (f + 1) * 512)))))))
  out.cases.push(writeCase(`quant_b${bias}`, rows, { kind: 'canonical', source: 'quantizationStage, pinkT seed 3, transient detection', bias }))
}

// ---- hand-built fields ----
const rnd = xorshift(4242)
const EDGE = [0, 1, -1, 15, 16, 31, 63, 64, I32_MIN, I32_MAX, I32_MIN + 1, I32_MAX - 1, 65535, 65536, -65536, 32767, -32768]
const anyInt = () => { const r = rnd(); return r % 4 === 0 ? EDGE[(r >>> 2) % EDGE.length] : rnd() | 0 }

// a frame with random entries everywhere (also at and above nBfu), then the caller's edits
function baseFields(nbfu, modes) {
  const f = { nbfu: new Int32Array([nbfu]), block_modes: Int32Array.from(modes), sfi: new Int32Array(52), wl: new Int32Array(52),
              quantized: new Int32Array(512) }
  for (let b = 0; b < 52; b++) { f.sfi[b] = rnd() % 64; f.wl[b] = rnd() % 16 }
  for (let b = 0; b < 52; b++) {
    const bits = f.wl[b] ? f.wl[b] + 1 : 0, range = bits ? (1 << (bits - 1)) - 1 : 0
    for (let j = FIRST[b]; j < FIRST[b + 1]; j++) f.quantized[j] = (rnd() % (2 * range + 1)) - range
  }
  for (let b = nbfu; b < 52; b++) { f.sfi[b] = anyInt(); f.wl[b] = anyInt() }
  return f
}
// word lengths of BFUs 0..nbfu-1 (each 0..15) whose mantissas take exactly `bits` bits: a reachability table over the BFUs
function wlsFor(nbfu, bits) {
  const reach = [new Map([[0, null]])]
  for (let b = 0; b < nbfu; b++) {
    const next = new Map()
    for (const s of reach[b].keys()) {
      for (let wl = 15; wl >= 0; wl--) {
        const t = s + (wl ? wl + 1 : 0) * SPECS_PER_BFU[b]
        if (t <= bits && !next.has(t)) next.set(t, [s, wl])
      }
    }
    reach.push(next)
  }
  if (!reach[nbfu].has(bits)) throw new Error(`no word lengths for ${nbfu} BFUs and ${bits} bits`)
  const wls = new Int32Array(nbfu)
  for (let b = nbfu, s = bits; b > 0; b--) { const [p, wl] = reach[b].get(s); wls[b - 1] = wl; s = p }
  return wls
}
function withStreamBits(f, total) {
  const n = f.nbfu[0]
  f.wl.set(wlsFor(n, total - 16 - 10 * n))
  for (let b = 0; b < n; b++) {
    const bits = f.wl[b] ? f.wl[b] + 1 : 0
    for (let j = FIRST[b]; j < FIRST[b + 1]; j++) f.quantized[j] = bits ? rnd() | 0 : f.quantized[j]
  }
  return f
}

{
  const rows = []
  const add = (f, what) => rows.push({ ...rowOfFields(f), what })
  add(baseFields(0, [0, 0, 0]), 'nbfu 0')
  add(baseFields(1, [1, -1, 5]), 'nbfu 1, modes 1 -1 5')
  add(baseFields(19, [0, 0, 0]), 'nbfu 19 (header ffe0)')
  add(baseFields(20, [1, -2, 7]), 'nbfu 20, modes 1 -2 7 (header f000)')
  add(baseFields(21, [I32_MIN, I32_MAX, 7]), 'nbfu 21, modes INT32_MIN INT32_MAX 7')
  {
    const f = baseFields(52, [2, 2, 3])
    f.wl.fill(15)
    for (let j = 0; j < 512; j++) f.quantized[j] = anyInt()
    add(f, 'nbfu 52, every wl 15: far past bit 1696')
  }
  {
    const f = baseFields(52, [I32_MAX, I32_MIN, I32_MIN])
    f.wl[3] = 16; f.wl[9] = 31; f.wl[20] = -1; f.wl[33] = I32_MIN; f.wl[40] = I32_MAX; f.wl[47] = -16
    add(f, 'wl 16 31 -1 INT32_MIN INT32_MAX -16 in the middle')
  }
  {
    const f = baseFields(36, [5, 7, -1])
    f.sfi[0] = 64; f.sfi[7] = -1; f.sfi[17] = I32_MAX; f.sfi[35] = I32_MIN; f.sfi[22] = 127
    add(f, 'sfi 64 -1 INT32_MAX INT32_MIN 127')
  }
  {
    const f = baseFields(44, [0, 1, 0])
    for (let b = 0; b < 44; b++) {
      if (!f.wl[b]) f.wl[b] = 1 + (b % 15)
      const bits = f.wl[b] + 1, range = (1 << (bits - 1)) - 1
      for (let j = FIRST[b]; j < FIRST[b + 1]; j++) {
        const k = j % 6
        f.quantized[j] = k === 0 ? range + 1 : (k === 1 ? -range - 2 : (k === 2 ? I32_MIN : (k === 3 ? I32_MAX : (k === 4 ? 1 << bits : rnd() | 0))))
      }
    }
    add(f, 'mantissas beyond their word length and at the int32 ends')
  }
  add(withStreamBits(baseFields(52, [0, 0, 0]), 1672), 'stream ends at bit 1672')
  add(withStreamBits(baseFields(40, [2, 2, 3]), 1672), 'stream ends at bit 1672, nbfu 40')
  add(withStreamBits(baseFields(48, [0, 2, 0]), 1680), 'stream ends at bit 1680 (zeroed bytes)')
  add(withStreamBits(baseFields(52, [2, 0, 3]), 1694), 'stream ends at bit 1694 (zeroed bytes)')
  add(withStreamBits(baseFields(52, [0, 0, 3]), 1696), 'stream ends at bit 1696')
  add(withStreamBits(baseFields(32, [0, 0, 0]), 1700), 'stream ends at bit 1700')
  add(withStreamBits(baseFields(52, [2, 2, 0]), 1710), 'stream ends at bit 1710')
  add(withStreamBits(baseFields(28, [0, 2, 3]), 1200), 'stream ends at bit 1200')
  const what = rows.map((r) => r.what)
  out.cases.push(writeCase('hand', rows, { kind: 'hand', what }))
}

// ---- random fields ----
{
  const rows = []
  for (let f = 0; f < FRAMES_RANDOM; f++) {
    const n = f < 53 ? f : rnd() % 53
    const fl = baseFields(n, [anyInt(), anyInt(), anyInt()])
    for (let b = 0; b < 52; b++) {
      const r = rnd() % 4
      fl.wl[b] = r === 0 ? anyInt() : rnd() % 16
      fl.sfi[b] = r === 1 ? anyInt() : rnd() % 64
    }
    for (let j = 0; j < 512; j++) fl.quantized[j] = anyInt()
    rows.push(rowOfFields(fl))
  }
  out.cases.push(writeCase('random', rows, { kind: 'random', source: 'xorshift32 seed 4242' }))
}

fs.writeFileSync(path.join(OUT, 'pack_units.json'), JSON.stringify(out, null, 1) + '\n')
console.log('wrote pack_units.json', out.cases.map((c) => `${c.file} (${c.frames} frames)`).join(', '))
