// The JavaScript encode() closure (carta1_amd/js/pipeline/encoder.js) and AudioProcessor.encodeStream with batchFrames 1
// and 16, under the option schedules of tests/golden/option_changes.json: the EncoderOptions are changed with setValue
// between frames of one stream, as the reference's generator (gen_option_changes.mjs) changed its own, and the units must
// be the reference's bit for bit.  Under fixed modes the closure's blockModes is options.fixedBlockModes itself.  Prints
// ALL OK on success; run by tests/test_js_option_changes.py.
import fs from 'fs'
import path from 'path'
import crypto from 'crypto'
import { fileURLToPath } from 'url'

import { EncoderOptions } from '../carta1_amd/js/core/options.js'
import { BufferPool } from '../carta1_amd/js/core/buffers.js'
import { serializeFrame } from '../carta1_amd/js/io/serialization.js'
import { AudioProcessor } from '../carta1_amd/js/io/processor.js'
import { encode } from '../carta1_amd/js/pipeline/encoder.js'

const G = path.join(path.dirname(fileURLToPath(import.meta.url)), 'golden')
const fixture = JSON.parse(fs.readFileSync(path.join(G, 'option_changes.json'), 'utf8'))
const FRAMES = fixture.frames

// the KAT generators (tests/golden/gen/gen_golden.mjs)
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

let failures = 0
function fail(msg) { failures++; console.log('FAIL', msg) }

function applyChanges(options, changes, f) {
  for (const [at, change] of changes) {
    if (at !== f) continue
    for (const [k, v] of Object.entries(change)) options.setValue(k, v)
  }
}

function check(what, result, units, modes, nch) {
  const all = Buffer.concat(units.map((u) => Buffer.from(u)))
  if (modes !== result.modes) return fail(`${what}: block modes differ`)
  for (const [f, hex] of Object.entries(result.switch_units)) {
    const got = all.subarray(Number(f) * nch * 212, Math.min(FRAMES, Number(f) + 2) * nch * 212).toString('hex')
    if (got !== hex) return fail(`${what}: units at the switch before frame ${f} differ`)
  }
  if (crypto.createHash('sha256').update(all).digest('hex') !== result.sha256) return fail(`${what}: SHA-256 differs`)
}

async function main() {
  let cases = 0
  for (const [name, sched] of Object.entries(fixture.schedules)) {
    for (const [sig, result] of Object.entries(sched.results)) {
      const chs = fixture.signals[sig].map(([g, seed]) => GEN[g](seed, FRAMES * 512))
      const nch = chs.length

      // the encode() closure, one per channel on one EncoderOptions
      {
        const options = new EncoderOptions(sched.initial)
        const encs = chs.map(() => encode(options, new BufferPool()))
        const units = []
        let modes = ''
        let sameArray = true
        for (let f = 0; f < FRAMES; f++) {
          applyChanges(options, sched.changes, f)
          for (let c = 0; c < nch; c++) {
            const fields = encs[c](chs[c].slice(f * 512, (f + 1) * 512))
            if (options.fixedBlockModes && fields.blockModes !== options.fixedBlockModes) sameArray = false
            units.push(serializeFrame(fields))
            modes += fields.blockModes.join('')
          }
        }
        if (!sameArray) fail(`${name}/${sig} encode(): blockModes is not options.fixedBlockModes under fixed modes`)
        check(`${name}/${sig} encode()`, result, units, modes, nch)
      }

      // encodeStream: the options are changed as each frame is handed over
      for (const batchFrames of [1, 16]) {
        const options = new EncoderOptions(sched.initial)
        async function* frames() {
          for (let f = 0; f < FRAMES; f++) {
            applyChanges(options, sched.changes, f)
            const parts = chs.map((c) => c.slice(f * 512, (f + 1) * 512))
            yield nch === 1 ? parts[0] : parts
          }
        }
        const units = []
        let modes = ''
        for await (const fields of AudioProcessor.encodeStream(frames(), { channelCount: nch, encoderOptions: options, batchFrames })) {
          units.push(serializeFrame(fields))
          modes += fields.blockModes.join('')
        }
        check(`${name}/${sig} encodeStream batchFrames ${batchFrames}`, result, units, modes, nch)
      }
      cases++
    }
  }
  if (cases !== 24) fail(`expected 24 cases, ran ${cases}`)

  // batchFrames 16: a frame's blockModes is the fixedBlockModes array of the options it was collected under
  {
    const options = new EncoderOptions({ fixedBlockModes: [2, 2, 3] })
    const arrays = []
    async function* frames() {
      for (let f = 0; f < 20; f++) {
        if (f === 5) options.setValue('fixedBlockModes', [2, 2, 3])   // same values, another array: no switch, new identity
        arrays.push(options.fixedBlockModes)
        yield white(1, 512)
      }
    }
    let f = 0
    for await (const fields of AudioProcessor.encodeStream(frames(), { encoderOptions: options, batchFrames: 16 })) {
      if (fields.blockModes !== arrays[f]) fail(`encodeStream frame ${f}: blockModes is not the array of its options`)
      f++
    }
    if (f !== 20) fail(`encodeStream gave ${f} frames, expected 20`)
  }
  if (failures) { console.log(`${failures} FAILURES`); process.exit(1) }
  console.log('ALL OK')
}

main().catch((e) => { console.log('ERROR', e && e.stack ? e.stack : e); process.exit(1) })
