// Golden-vector generator: the reference's own encode() closures (aynik/carta1 v1.1.10, read in place from /root/reference
// through loader.mjs) with their EncoderOptions changed by setValue between frames of one stream, as an application may do
// (the closure reads the options on every call, codec/pipeline/encoder.js:131-140, :393).  Writes option_changes.json:
// per schedule and signal the SHA-256 of all units, the block modes of every unit, and the units at and right after every
// switch.
//
//   cd tests/golden/gen && node --experimental-loader ./loader.mjs gen_option_changes.mjs
import fs from 'fs'
import path from 'path'
import crypto from 'crypto'
import { fileURLToPath } from 'url'

import { encode } from '/root/reference/codec/pipeline/encoder.js'
import { serializeFrame } from '/root/reference/codec/io/serialization.js'
import { EncoderOptions } from '/root/reference/codec/core/options.js'
import { BufferPool } from '/root/reference/codec/core/buffers.js'

const OUT = path.resolve(path.dirname(fileURLToPath(import.meta.url)), '..')
const FRAMES = 96

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

const SIGNALS = {
  white1: [['white', 1]],
  pinkT3: [['pinkT', 3]],
  white12: [['white', 1], ['white', 2]],
  pinkT34: [['pinkT', 3], ['pinkT', 4]],
}
const GEN = { white, pinkT }

// biases with committed tables only (tables.json)
const BIASES = [0, 0.25, 0.5, 1, 1.5, 2, 3.3, 5]
const THRESHOLDS = [0.3, 0.5, 1, 1.5, 2]
const MODES = [null, null, [0, 0, 0], [2, 2, 3], [2, 0, 3], [0, 2, 0], [0, 0, 3]]

// a schedule: the options of frame 0 and [frame, { key: value }] changes applied by setValue before that frame
function everyFrame() {
  const r = xorshift(0x5eed)
  const pick = (list) => list[Math.min(list.length - 1, Math.floor((r() + 1) / 2 * list.length))]
  const changes = []
  for (let f = 1; f < FRAMES; f++) {
    changes.push([f, { allocationBias: pick(BIASES), transientThresholdLow: pick(THRESHOLDS), fixedBlockModes: pick(MODES) }])
  }
  return { initial: { fixedBlockModes: [2, 2, 3], allocationBias: 0.5 }, changes }
}
const SCHEDULES = {
  bias_fixed000: { initial: { fixedBlockModes: [0, 0, 0], allocationBias: 1 },
                   changes: [[32, { allocationBias: 0.5 }], [64, { allocationBias: 2 }]] },
  threshold: { initial: {}, changes: [[32, { transientThresholdLow: 0.5 }], [64, { transientThresholdLow: 1.5 }]] },
  fixed000_then_detect: { initial: { fixedBlockModes: [0, 0, 0] }, changes: [[16, { fixedBlockModes: null }]] },
  detect_223_detect: { initial: {}, changes: [[16, { fixedBlockModes: [2, 2, 3] }], [40, { fixedBlockModes: null }]] },
  detect_000_223_detect: { initial: {},
                           changes: [[16, { fixedBlockModes: [0, 0, 0] }], [32, { fixedBlockModes: [2, 2, 3] }],
                                     [48, { fixedBlockModes: null }]] },
  every_frame: everyFrame(),
}

const out = {
  note: 'the reference encode() closures, one per channel on one shared EncoderOptions, setValue(key, value) of every change ' +
        'before the frame it names; units interleaved by frame (L, R); modes: 3 digits per unit; switch_units: frame -> ' +
        'hex of the units of that frame and the next (every_frame: the first 8 switches only)',
  frames: FRAMES,
  signals: SIGNALS,
  schedules: {},
}
for (const [name, sched] of Object.entries(SCHEDULES)) {
  const entry = { initial: sched.initial, changes: sched.changes, results: {} }
  for (const [sig, spec] of Object.entries(SIGNALS)) {
    const chs = spec.map(([g, seed]) => GEN[g](seed, FRAMES * 512))
    const options = new EncoderOptions(sched.initial)
    const encs = chs.map(() => encode(options, new BufferPool()))
    const units = []
    let modes = ''
    for (let f = 0; f < FRAMES; f++) {
      for (const [at, change] of sched.changes) {
        if (at !== f) continue
        for (const [k, v] of Object.entries(change)) options.setValue(k, v)
      }
      for (let c = 0; c < chs.length; c++) {
        const res = encs[c](chs[c].slice(f * 512, (f + 1) * 512))
        units.push(Buffer.from(serializeFrame(res)))
        modes += res.blockModes.join('')
      }
    }
    const all = Buffer.concat(units)
    const switches = {}
    const at = sched.changes.map(([f]) => f).slice(0, name === 'every_frame' ? 8 : undefined)
    for (const f of at) {
      const n = chs.length
      switches[f] = Buffer.concat(units.slice(f * n, Math.min(FRAMES, f + 2) * n)).toString('hex')
    }
    entry.results[sig] = { sha256: crypto.createHash('sha256').update(all).digest('hex'), modes, switch_units: switches }
  }
  out.schedules[name] = entry
}
fs.writeFileSync(path.join(OUT, 'option_changes.json'), JSON.stringify(out, null, 1) + '\n')
console.log('option_changes.json', fs.statSync(path.join(OUT, 'option_changes.json')).size, 'bytes')
