// Golden vectors for the decoder's pipeline stages the reference exports next to decode() (codec/pipeline/decoder.js:52, :116,
// :349) and for deserializeFrame (codec/io/serialization.js:111-176).  Runs the JavaScript reference in place from
// /root/reference through loader.mjs and writes tests/golden/decoder_stages.json plus one decoder_stages_<case>.bin per case --
// inputs and outputs only, never reference source text.
//
//   cd tests/golden/gen && node --experimental-loader ./loader.mjs gen_decoder_stages.mjs
//
// Cases: the stage chain deserializeFrame -> dequantizationStage -> imdctStage -> qmfSynthesisStage over the first frames of
// channel 0 of two KAT unit files (one with transient detection, short blocks in every band in some frames; one all long), and
// hand-built frame fields no encoder writes (nBfu outside BFU_AMOUNTS, mantissas beyond their word length, word length 0
// between others, band modes of 1, sfi 0 and 63) fed to the same three stage closures over consecutive frames of one pool.
import fs from 'fs'
import path from 'path'
import { fileURLToPath } from 'url'

import { BufferPool } from '/root/reference/codec/core/buffers.js'
import { SPECS_PER_BFU } from '/root/reference/codec/core/constants.js'
import { deserializeFrame } from '/root/reference/codec/io/serialization.js'
import { dequantizationStage, imdctStage, qmfSynthesisStage } from '/root/reference/codec/pipeline/decoder.js'

const OUT = path.resolve(path.dirname(fileURLToPath(import.meta.url)), '..')
const FRAMES_KAT = 24
const FRAMES_FIELDS = 12

// the layout of the library's frame fields (include/carta1_hip.h): zeros where the reference leaves entries unset
function toFields(fd) {
  const f = { nbfu: new Int32Array([fd.nBfu]), block_modes: Int32Array.from(fd.blockModes), sfi: new Int32Array(52),
              wl: new Int32Array(52), quantized: new Int32Array(512) }
  let at = 0
  for (let b = 0; b < 52; b++) {
    if (b < fd.nBfu) {
      f.sfi[b] = fd.scaleFactorIndices[b]
      f.wl[b] = fd.wordLengthIndices[b]
      f.quantized.set(fd.quantizedCoefficients[b], at)
    }
    at += SPECS_PER_BFU[b]
  }
  return f
}

const ARRAYS = [['nbfu', 'int32', []], ['block_modes', 'int32', [3]], ['sfi', 'int32', [52]], ['wl', 'int32', [52]],
                ['quantized', 'int32', [512]], ['coefficients', 'float32', [512]], ['bands', 'float32', [512]], ['pcm', 'float32', [512]]]

// one pool, the three stage closures, frame after frame (what decode() composes, decoder.js:408-411)
function runChain(frameDatas) {
  const context = { bufferPool: new BufferPool() }
  const dq = dequantizationStage(), im = imdctStage(context), qs = qmfSynthesisStage(context)
  const rows = []
  for (const fd of frameDatas) {
    const fields = toFields(fd)
    const d = dq(fd)
    const coefficients = Float32Array.from(d.coefficients)
    const b = im(d)
    const bands = new Float32Array(512)
    bands.set(b[0], 0); bands.set(b[1], 128); bands.set(b[2], 256)
    const pcm = Float32Array.from(qs(b))
    rows.push({ ...fields, coefficients, bands, pcm })
  }
  return rows
}

function writeCase(name, rows, extra) {
  const parts = [], arrays = []
  for (const [key, dtype, shape] of ARRAYS) {
    const per = shape.length ? shape[0] : 1
    const ta = dtype === 'int32' ? new Int32Array(rows.length * per) : new Float32Array(rows.length * per)
    rows.forEach((r, i) => ta.set(r[key], i * per))
    parts.push(Buffer.from(ta.buffer))
    arrays.push({ name: key, dtype, shape: [rows.length, ...shape] })
  }
  const file = `decoder_stages_${name}.bin`
  fs.writeFileSync(path.join(OUT, file), Buffer.concat(parts))
  return { name, file, frames: rows.length, arrays, ...extra }
}

// xorshift32 (SURVEY.md 8c)
function xorshift(seed) {
  let s = seed >>> 0
  return () => { s ^= s << 13; s >>>= 0; s ^= s >>> 17; s ^= s << 5; s >>>= 0; return s }
}

const out = { note: 'each case: little-endian arrays concatenated in `arrays` order in `file`; frames are consecutive frames of one ' +
                    'BufferPool from a fresh pool; bands are low128 | mid128 | high256; fields zero where the reference leaves them unset',
              cases: [] }

for (const kat of ['pinkT_detect', 'white_m000_b1']) {
  const units = fs.readFileSync(path.join(OUT, `kat64_${kat}.units.bin`))
  const fds = []
  for (let f = 0; f < FRAMES_KAT; f++) {
    const at = (2 * f) * 212                                   // channel 0 of the interleaved stereo units
    fds.push(deserializeFrame(new Uint8Array(units.buffer, units.byteOffset + at, 212)))
  }
  out.cases.push(writeCase(kat, runChain(fds), { source: `kat64_${kat}.units.bin`, channel: 0, channels: 2, first_frame: 0 }))
}

// hand-built fields
{
  const rnd = xorshift(2024)
  const nbfus = [0, 1, 52, 7, 21, 45, 2, 33, 52, 13, 51, 29]
  const modes = [[1, 0, 0], [0, 1, 0], [1, 1, 3], [0, 0, 0], [2, 2, 3], [1, 1, 1], [0, 1, 2], [1, 0, 3], [0, 0, 0], [1, 2, 0], [2, 1, 1], [1, 1, 0]]
  const fds = []
  for (let f = 0; f < FRAMES_FIELDS; f++) {
    const nBfu = nbfus[f]
    const scaleFactorIndices = new Int32Array(52), wordLengthIndices = new Int32Array(52), quantizedCoefficients = []
    for (let b = 0; b < 52; b++) {
      const r = rnd()
      const wl = (r & 3) === 0 ? 0 : (r >>> 2) % 16                     // word length 0 between non-zero ones
      const sfi = b % 11 === 0 ? 63 : (b % 13 === 5 ? 0 : (r >>> 8) % 64)
      scaleFactorIndices[b] = sfi
      wordLengthIndices[b] = wl
      const q = new Int32Array(SPECS_PER_BFU[b])
      const bits = wl === 0 ? 0 : wl + 1, range = bits ? (1 << (bits - 1)) - 1 : 0
      for (let j = 0; j < q.length; j++) {
        const v = rnd(), kind = v % 8
        if (kind < 3) q[j] = (v >>> 3) % (2 * range + 1) - range                    // in range
        else if (kind === 3) q[j] = range + 1 + ((v >>> 3) % 1000)                  // just past the range
        else if (kind === 4) q[j] = -(range + 1 + ((v >>> 3) % 100000))             // negative, past the range
        else if (kind === 5) q[j] = (v | 0x80000000) | 0                            // large negative int32
        else if (kind === 6) q[j] = j === 0 ? -2147483648 : 2147483647              // the int32 ends
        else q[j] = v | 0                                                           // any int32
      }
      quantizedCoefficients.push(q)
    }
    fds.push({ nBfu, scaleFactorIndices, wordLengthIndices, quantizedCoefficients, blockModes: modes[f] })
  }
  out.cases.push(writeCase('fields', runChain(fds), { source: 'hand-built frame fields (xorshift32 seed 2024)' }))
}

fs.writeFileSync(path.join(OUT, 'decoder_stages.json'), JSON.stringify(out, null, 1) + '\n')
console.log('wrote decoder_stages.json', out.cases.map((c) => `${c.file} (${c.frames} frames)`).join(', '))
