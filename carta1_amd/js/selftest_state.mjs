// BufferPool state in the reference's layout (core/buffers.js: getEncoderState / setEncoderState / getDecoderState /
// setDecoderState) against tests/golden/stream_state.json, the reference's own dumped pools and what its encode() / decode()
// computed from them (tests/golden/gen/gen_stream_state.mjs).  Without arguments only the host side runs (shapes, a set kept
// until the stream exists, bad shapes); with --gpu the closures continue from the fixture's pools.  Prints ALL OK on success;
// run by tests/test_js_stream_state.py.
import fs from 'fs'
import path from 'path'
import crypto from 'crypto'
import { fileURLToPath } from 'url'

import { BufferPool } from './core/buffers.js'
import { EncoderOptions } from './core/options.js'
import { serializeFrame } from './io/serialization.js'
import { encode } from './pipeline/encoder.js'
import { decode } from './pipeline/decoder.js'

const GPU = process.argv.includes('--gpu')
const G = path.join(path.dirname(fileURLToPath(import.meta.url)), '..', '..', 'tests', 'golden')
const fixture = JSON.parse(fs.readFileSync(path.join(G, 'stream_state.json'), 'utf8'))
const blobs = fs.readFileSync(path.join(G, 'stream_state.bin'))

let failures = 0
function fail(msg) { failures++; console.log('FAIL', msg) }
function ok(cond, msg) { if (!cond) fail(msg) }

function f32(ref) { return new Float32Array(blobs.buffer.slice(blobs.byteOffset + ref[0], blobs.byteOffset + ref[0] + ref[1])) }
function u8(ref) { return new Uint8Array(blobs.buffer.slice(blobs.byteOffset + ref[0], blobs.byteOffset + ref[0] + ref[1])) }
function sameBits(a, b) {
  if (a.length !== b.length) return false
  const x = new Uint32Array(a.buffer, a.byteOffset, a.length), y = new Uint32Array(b.buffer, b.byteOffset, b.length)
  for (let i = 0; i < x.length; i++) if (x[i] !== y[i]) return false
  return true
}
function sameBytes(a, b) { return Buffer.from(a.buffer, a.byteOffset, a.byteLength).equals(Buffer.from(b.buffer, b.byteOffset, b.byteLength)) }

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

// A pool shaped like the reference's own (codec/core/buffers.js:7-81) from channel c of a dumped c1_enc_state / c1_dec_state:
// work buffers it also carries, whole imdctOverlap arrays with the live 16 samples at their end
class ReferenceShapedPool {
  constructor(enc, dec) {
    this.transformBuffers = { 64: new Float32Array(64), 128: new Float32Array(128), 256: new Float32Array(256), 512: new Float32Array(512) }
    this.qmfDelays = { lowBand: new Float32Array(46), midBand: new Float32Array(46), highBand: new Float32Array(39) }
    this.transientDetection = [new Float32Array(64), new Float32Array(64), new Float32Array(128)]
    this.mdctOverlap = [new Float32Array(32), new Float32Array(32), new Float32Array(32)]
    this.imdctOverlap = [new Float32Array(256), new Float32Array(256), new Float32Array(512)]
    const src = enc || dec
    this.qmfDelays.lowBand.set(src.subarray(0, 46))
    this.qmfDelays.midBand.set(src.subarray(46, 92))
    this.qmfDelays.highBand.set(src.subarray(92, 131))
    if (enc) {
      for (let b = 0; b < 3; b++) this.mdctOverlap[b].set(enc.subarray(131 + 32 * b, 163 + 32 * b))
      this.transientDetection[0].set(enc.subarray(227, 291))
      this.transientDetection[1].set(enc.subarray(291, 355))
      this.transientDetection[2].set(enc.subarray(355, 483))
    } else {
      for (let b = 0; b < 3; b++) {
        this.imdctOverlap[b].fill(0.25) // stale entries the reference leaves there: ignored on import
        this.imdctOverlap[b].set(dec.subarray(131 + 16 * b, 147 + 16 * b), this.imdctOverlap[b].length - 16)
      }
    }
  }
}
function flatEnc(s) {
  const out = new Float32Array(483)
  let at = 0
  for (const a of [s.qmfDelays.lowBand, s.qmfDelays.midBand, s.qmfDelays.highBand, ...s.mdctOverlap, ...s.transientDetection]) { out.set(a, at); at += a.length }
  return out
}
function flatDec(s) {
  const out = new Float32Array(179)
  let at = 0
  for (const a of [s.qmfDelays.lowBand, s.qmfDelays.midBand, s.qmfDelays.highBand]) { out.set(a, at); at += a.length }
  for (const a of s.imdctOverlap) { out.set(a.subarray(a.length - 16), at); at += 16 }
  return out
}
function throwsTypeError(fn, needle, what) {
  try { fn() } catch (e) {
    ok(e instanceof TypeError && String(e.message).includes(needle), `${what}: expected a TypeError naming ${needle}, got ${e}`)
    return
  }
  fail(`${what}: did not throw`)
}

// ---- host side: shapes, pending states, bad shapes (no stream exists, so no device is touched) ----
{
  const pool = new BufferPool()
  const e = pool.getEncoderState()
  ok(e.qmfDelays.lowBand.length === 46 && e.qmfDelays.midBand.length === 46 && e.qmfDelays.highBand.length === 39, 'encoder qmfDelays shapes')
  ok(e.mdctOverlap.length === 3 && e.mdctOverlap.every((a) => a instanceof Float32Array && a.length === 32), 'mdctOverlap shapes')
  ok(e.transientDetection.map((a) => a.length).join() === '64,64,128', 'transientDetection shapes')
  ok(flatEnc(e).every((v) => v === 0), 'a fresh pool exports zeros')
  const d = pool.getDecoderState()
  ok(d.imdctOverlap.map((a) => a.length).join() === '256,256,512' && d.qmfDelays.highBand.length === 39, 'decoder shapes')
  const first = Object.values(fixture.cases)[0]
  const enc0 = f32(first.enc_states).subarray(0, 483), dec0 = f32(first.dec_states).subarray(0, 179)
  pool.setEncoderState(new ReferenceShapedPool(enc0, null))
  ok(sameBits(flatEnc(pool.getEncoderState()), enc0), 'a set before the stream exists is kept')
  pool.setDecoderState(new ReferenceShapedPool(null, dec0))
  const back = pool.getDecoderState()
  ok(sameBits(flatDec(back), dec0), 'decoder: a set before the stream exists is kept')
  ok(back.imdctOverlap[2].subarray(0, 496).every((v) => v === 0), 'decoder: entries before the live 16 are zeros on export')
  const good = pool.getEncoderState()
  throwsTypeError(() => pool.setEncoderState(Object.assign({}, good, { mdctOverlap: [good.mdctOverlap[0], new Float32Array(31), good.mdctOverlap[2]] })), 'mdctOverlap[1]', 'short overlap')
  throwsTypeError(() => pool.setEncoderState(Object.assign({}, good, { qmfDelays: { lowBand: good.qmfDelays.lowBand, midBand: 'x', highBand: good.qmfDelays.highBand } })), 'qmfDelays.midBand', 'string delay line')
  throwsTypeError(() => pool.setEncoderState({ qmfDelays: good.qmfDelays, mdctOverlap: good.mdctOverlap }), 'transientDetection', 'missing field')
  throwsTypeError(() => pool.setDecoderState({ qmfDelays: good.qmfDelays, imdctOverlap: [new Float32Array(256), new Float32Array(256), new Float32Array(16)] }), 'imdctOverlap[2]', 'tail-only overlap')
  throwsTypeError(() => pool.setEncoderState(null), 'qmfDelays', 'null state')
  ok(sameBits(flatEnc(pool.getEncoderState()), enc0), 'a rejected set changes nothing')
}

// ---- device: the closures continue from the fixture's pools ----
if (GPU) {
  const DUMP = fixture.dump_at, MORE = fixture.more
  for (const [name, e] of Object.entries(fixture.cases)) {
    const [sig, oname] = name.split('/')
    const spec = fixture.signals[sig]
    const chs = spec.map(([g, seed]) => GEN[g](seed, (DUMP + MORE) * 512))
    const options = new EncoderOptions(Object.assign({ allocationBias: 1 }, fixture.option_sets[oname]))
    const encStates = f32(e.enc_states), decStates = f32(e.dec_states)
    const want = u8(e.units_more)
    // a fixture pool set on a fresh BufferPool (one with no stream yet, one whose stream already ran), then encode()
    const pools = chs.map((_, c) => {
      const p = new BufferPool()
      if (c === 1) encode(options, p)(chs[c].subarray(0, 512).slice())   // the stream exists and holds other history
      p.setEncoderState(new ReferenceShapedPool(encStates.subarray(483 * c, 483 * (c + 1)), null))
      return p
    })
    const encs = pools.map((p) => encode(options, p))
    // a get on one pool followed by a set on another continues identically
    const forks = pools.map((p) => { const q = new BufferPool(); q.setEncoderState(p.getEncoderState()); return q })
    const fencs = forks.map((p) => encode(options, p))
    const got = [], fgot = []
    for (let f = DUMP; f < DUMP + MORE; f++) {
      for (let c = 0; c < chs.length; c++) {
        got.push(serializeFrame(encs[c](chs[c].slice(f * 512, (f + 1) * 512))))
        fgot.push(serializeFrame(fencs[c](chs[c].slice(f * 512, (f + 1) * 512))))
      }
    }
    ok(sameBytes(new Uint8Array(Buffer.concat(got.map((u) => Buffer.from(u)))), want), `${name}: encode() from the reference's pool`)
    ok(sameBytes(new Uint8Array(Buffer.concat(fgot.map((u) => Buffer.from(u)))), want), `${name}: encode() from a forked pool`)
    for (let c = 0; c < chs.length; c++) ok(sameBits(flatEnc(pools[c].getEncoderState()), flatEnc(forks[c].getEncoderState())), `${name}: pools agree after the run`)
    // decode()
    const dpools = chs.map((_, c) => { const p = new BufferPool(); p.setDecoderState(new ReferenceShapedPool(null, decStates.subarray(179 * c, 179 * (c + 1)))); return p })
    const decs = dpools.map((p) => decode(p))
    const dforks = dpools.map((p) => { const q = new BufferPool(); q.setDecoderState(p.getDecoderState()); return q })
    const fdecs = dforks.map((p) => decode(p))
    const h = crypto.createHash('sha256'), fh = crypto.createHash('sha256')
    for (let f = 0; f < MORE; f++) {
      for (let c = 0; c < chs.length; c++) {
        const unit = want.slice((f * chs.length + c) * 212, (f * chs.length + c + 1) * 212)
        const y = decs[c](unit), fy = fdecs[c](unit)
        h.update(Buffer.from(y.buffer, y.byteOffset, y.byteLength))
        fh.update(Buffer.from(fy.buffer, fy.byteOffset, fy.byteLength))
      }
    }
    ok(h.digest('hex') === e.pcm_sha256, `${name}: decode() from the reference's pool`)
    ok(fh.digest('hex') === e.pcm_sha256, `${name}: decode() from a forked pool`)
  }
  // foreign pools: state no PCM could have produced
  const F = fixture.foreign
  const x = white(F.pcm[0][1], F.frames * 512)
  for (const [oname, e] of Object.entries(F.enc)) {
    const pool = new BufferPool()
    pool.setEncoderState(new ReferenceShapedPool(f32(e.enc_state), null))
    const enc = encode(new EncoderOptions(Object.assign({ allocationBias: 1 }, e.options)), pool)
    const got = []
    for (let f = 0; f < F.frames; f++) got.push(serializeFrame(enc(x.slice(f * 512, (f + 1) * 512))))
    ok(sameBytes(new Uint8Array(Buffer.concat(got.map((u) => Buffer.from(u)))), u8(e.units)), `foreign ${oname}: units`)
    ok(sameBits(flatEnc(pool.getEncoderState()), f32(e.enc_state_end)), `foreign ${oname}: the pool afterwards`)
  }
  {
    const d = F.dec
    const pool = new BufferPool()
    pool.setDecoderState(new ReferenceShapedPool(null, f32(d.dec_state)))
    const dec = decode(pool)
    const units = u8(d.units), want = f32(d.pcm)
    for (let f = 0; f < F.frames; f++) ok(sameBits(dec(units.slice(f * 212, (f + 1) * 212)), want.subarray(f * 512, (f + 1) * 512)), `foreign decode: frame ${f}`)
    ok(sameBits(flatDec(pool.getDecoderState()), f32(d.dec_state_end)), 'foreign decode: the pool afterwards')
  }
}

if (failures) { console.log(`${failures} FAILED`); process.exit(1) }
console.log('ALL OK')
