// Golden-vector generator: the reference's BufferPool as resumable stream state (aynik/carta1 v1.1.10, read in place from
// /root/reference through loader.mjs).  encode(options, pool) and decode(pool) continue from whatever the pool holds
// (codec/pipeline/encoder.js:438-441, codec/core/buffers.js:30-72); this dumps pools mid-stream, pools filled with values no
// PCM could have produced, and what the reference's closures compute from them.  Writes stream_state.json (the index and
// the recipes) and stream_state.bin (every blob, back to back; float arrays as little-endian binary32 bit patterns).
//
//   cd tests/golden/gen && node --experimental-loader ./loader.mjs gen_stream_state.mjs
import fs from 'fs'
import path from 'path'
import crypto from 'crypto'
import { fileURLToPath } from 'url'

import { encode } from '/root/reference/codec/pipeline/encoder.js'
import { decode } from '/root/reference/codec/pipeline/decoder.js'
import { serializeFrame, deserializeFrame } from '/root/reference/codec/io/serialization.js'
import { EncoderOptions } from '/root/reference/codec/core/options.js'
import { BufferPool } from '/root/reference/codec/core/buffers.js'

const OUT = path.resolve(path.dirname(fileURLToPath(import.meta.url)), '..')

// the KAT generators (gen_golden.mjs): xorshift32, u in [-1, 1)
function xorshift(seed) {
  let s = seed >>> 0
  return () => { s ^= s << 13; s >>>= 0; s ^= s >>> 17; s ^= s << 5; s >>>= 0; return (s / 4294967296) * 2 - 1 }
}
function white(seed, n) {
  const r = xorshift(seed); const x = new Float32Array(n)
  for (let i = 0; i < n; i++) x[i] = Math.fround(r() * 0.5)
  return x
}
function pinkT(seed, n) {
  const r = xorshift(seed); const x = new Float32Array(n); let p = 0
  for (let i = 0; i < n; i++) {
    const u = r(); p = 0.98 * p + 0.05 * u; let v = p
    if ((i >> 9) % 8 === 5 && (i % 512) >= 256) v += 0.8 * r()
    x[i] = v
  }
  return x
}
const GEN = { white, pinkT }
const SIGNALS = { white12: [['white', 1], ['white', 2]], pinkT34: [['pinkT', 3], ['pinkT', 4]] }
const OPTION_SETS = {
  detect_t1: { transientThresholdLow: 1.0 },
  detect_t03: { transientThresholdLow: 0.3 },
  fixed000: { fixedBlockModes: [0, 0, 0] },
  fixed223: { fixedBlockModes: [2, 2, 3] },
  fixed020: { fixedBlockModes: [0, 2, 0] },
}
const DUMP_AT = 5, MORE = 4

// ---- the blob file ----
const blobs = []
let at = 0
function put(bytes) {
  const b = Buffer.from(bytes.buffer, bytes.byteOffset, bytes.byteLength)
  blobs.push(Buffer.from(b))
  const ref = [at, b.length]
  at += b.length
  return ref
}
function f32bytes(arrays) {
  const n = arrays.reduce((a, x) => a + x.length, 0)
  const out = new Float32Array(n)
  let o = 0
  for (const x of arrays) { out.set(x, o); o += x.length }
  return new Uint8Array(out.buffer)
}
// c1_enc_state: qmfDelays low 46 | mid 46 | high 39 | mdctOverlap 3 x 32 | transientDetection 64 | 64 | 128
function encState(pool) {
  return f32bytes([pool.qmfDelays.lowBand, pool.qmfDelays.midBand, pool.qmfDelays.highBand, ...pool.mdctOverlap, ...pool.transientDetection])
}
// c1_dec_state: qmfDelays low 46 | mid 46 | high 39 | the last 16 entries of each imdctOverlap
function decState(pool) {
  return f32bytes([pool.qmfDelays.lowBand, pool.qmfDelays.midBand, pool.qmfDelays.highBand,
                   ...pool.imdctOverlap.map((x) => x.slice(x.length - 16))])
}
function concatBytes(list) { return new Uint8Array(Buffer.concat(list.map((x) => Buffer.from(x.buffer, x.byteOffset, x.byteLength)))) }
function sha(list) {
  const h = crypto.createHash('sha256')
  for (const x of list) h.update(Buffer.from(x.buffer, x.byteOffset, x.byteLength))
  return h.digest('hex')
}

const out = {
  note: 'pools of the reference mid-stream and what its closures compute from them.  Blobs are [offset, length] into ' +
        'stream_state.bin.  enc_states / dec_states: one c1_enc_state / c1_dec_state per channel (include/carta1_hip.h), binary32 ' +
        'little-endian.  units: 212-byte sound units interleaved by frame (L, R); units_more / units_from_dump: those of the ' +
        'frames from the dump on.  pcm_sha256: SHA-256 over the decoded ' +
        'frames in order, per frame channel 0 then channel 1, 512 little-endian binary32 each.',
  dump_at: DUMP_AT,
  more: MORE,
  signals: SIGNALS,
  option_sets: OPTION_SETS,
  cases: {},
  foreign: {},
  switch: {},
}

// ---- pools dumped after DUMP_AT frames, and the MORE frames behind them ----
for (const [sig, spec] of Object.entries(SIGNALS)) {
  for (const [oname, oset] of Object.entries(OPTION_SETS)) {
    const frames = DUMP_AT + MORE
    const chs = spec.map(([g, seed]) => GEN[g](seed, frames * 512))
    const options = new EncoderOptions(Object.assign({ allocationBias: 1 }, oset))
    const pools = chs.map(() => new BufferPool())
    const encs = pools.map((p) => encode(options, p))
    const units = []
    let dump = null
    for (let f = 0; f < frames; f++) {
      if (f === DUMP_AT) dump = concatBytes(pools.map(encState))
      for (let c = 0; c < chs.length; c++) units.push(serializeFrame(encs[c](chs[c].slice(f * 512, (f + 1) * 512))))
    }
    const entry = {
      enc_states: put(dump),
      units_more: put(concatBytes(units.slice(DUMP_AT * chs.length))),
    }
    // decoder: the same units through decode()
    const dpools = chs.map(() => new BufferPool())
    const decs = dpools.map((p) => decode(p))
    const pcm = []
    for (let f = 0; f < frames; f++) {
      if (f === DUMP_AT) entry.dec_states = put(concatBytes(dpools.map(decState)))
      for (let c = 0; c < chs.length; c++) {
        const y = decs[c](deserializeFrame(units[f * chs.length + c]))
        if (f >= DUMP_AT) pcm.push(Float32Array.from(y))
      }
    }
    entry.pcm_sha256 = sha(pcm)
    out.cases[sig + '/' + oname] = entry
  }
}

// ---- foreign pools: every state array filled with xorshift32 values in [-1, 1) ----
function fillForeign(arrays, seed) {
  const r = xorshift(seed)
  for (const a of arrays) for (let i = 0; i < a.length; i++) a[i] = Math.fround(r())
}
const FOREIGN_ENC_SEED = 0xF00D1, FOREIGN_DEC_SEED = 0xF00D2, FOREIGN_FRAMES = 3
out.foreign.recipe = 'x[i] = Math.fround(u), u the next xorshift32 value (s ^= s << 13; s ^= s >>> 17; s ^= s << 5; u = s / 2^32 * 2 - 1), ' +
  'filling in order qmfDelays.lowBand, midBand, highBand, then mdctOverlap[0..2] and transientDetection[0..2] (encoder, seed ' +
  FOREIGN_ENC_SEED + ') or every entry of imdctOverlap[0..2] (decoder, seed ' + FOREIGN_DEC_SEED + '); mono; PCM = white seed 5'
out.foreign.enc_seed = FOREIGN_ENC_SEED
out.foreign.dec_seed = FOREIGN_DEC_SEED
out.foreign.frames = FOREIGN_FRAMES
out.foreign.pcm = [['white', 5]]
{
  const x = white(5, FOREIGN_FRAMES * 512)
  out.foreign.enc = {}
  for (const [oname, oset] of Object.entries({ detect_t1: {}, fixed203: { fixedBlockModes: [2, 0, 3] } })) {
    const pool = new BufferPool()
    fillForeign([pool.qmfDelays.lowBand, pool.qmfDelays.midBand, pool.qmfDelays.highBand, ...pool.mdctOverlap, ...pool.transientDetection], FOREIGN_ENC_SEED)
    const start = encState(pool)
    const enc = encode(new EncoderOptions(Object.assign({ allocationBias: 1 }, oset)), pool)
    const units = []
    for (let f = 0; f < FOREIGN_FRAMES; f++) units.push(serializeFrame(enc(x.slice(f * 512, (f + 1) * 512))))
    out.foreign.enc[oname] = { options: oset, enc_state: put(start), units: put(concatBytes(units)), enc_state_end: put(encState(pool)) }
  }
  // decoder: three valid units (the same PCM through a fresh default encoder) decoded from a foreign pool
  const enc = encode(new EncoderOptions(), new BufferPool())
  const units = []
  for (let f = 0; f < FOREIGN_FRAMES; f++) units.push(serializeFrame(enc(x.slice(f * 512, (f + 1) * 512))))
  const pool = new BufferPool()
  fillForeign([pool.qmfDelays.lowBand, pool.qmfDelays.midBand, pool.qmfDelays.highBand, ...pool.imdctOverlap], FOREIGN_DEC_SEED)
  const start = decState(pool)
  const dec = decode(pool)
  const pcm = units.map((u) => Float32Array.from(dec(deserializeFrame(u))))
  out.foreign.dec = { dec_state: put(start), units: put(concatBytes(units)), pcm: put(f32bytes(pcm)), dec_state_end: put(decState(pool)) }
}

// ---- one schedule with a switch: detection, fixed modes, detection again; the pool dumped under fixed modes ----
const SWITCH = { fixed_from: 3, fixed_modes: [2, 2, 3], dump_at: 6, detect_from: 8, frames: 12 }
out.switch.schedule = SWITCH
out.switch.results = {}
for (const [sig, spec] of Object.entries(SIGNALS)) {
  const chs = spec.map(([g, seed]) => GEN[g](seed, SWITCH.frames * 512))
  const options = new EncoderOptions({ allocationBias: 1 })
  const pools = chs.map(() => new BufferPool())
  const encs = pools.map((p) => encode(options, p))
  const units = []
  let dump = null
  for (let f = 0; f < SWITCH.frames; f++) {
    if (f === SWITCH.fixed_from) options.setValue('fixedBlockModes', SWITCH.fixed_modes)
    if (f === SWITCH.detect_from) options.setValue('fixedBlockModes', null)
    if (f === SWITCH.dump_at) dump = concatBytes(pools.map(encState))
    for (let c = 0; c < chs.length; c++) units.push(serializeFrame(encs[c](chs[c].slice(f * 512, (f + 1) * 512))))
  }
  out.switch.results[sig] = { enc_states: put(dump), units_from_dump: put(concatBytes(units.slice(SWITCH.dump_at * chs.length))) }
}

fs.writeFileSync(path.join(OUT, 'stream_state.bin'), Buffer.concat(blobs))
fs.writeFileSync(path.join(OUT, 'stream_state.json'), JSON.stringify(out, null, 1) + '\n')
console.log('stream_state.json', fs.statSync(path.join(OUT, 'stream_state.json')).size, 'bytes; stream_state.bin', at, 'bytes')
