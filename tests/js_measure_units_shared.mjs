// measureUnits(channels, units, { masking, haloFrames, thresholdFrom }) (carta1_amd/js/native.js -> c1_measure_units_batch or,
// under thresholdFrom 'long', c1_measure_units_shared_batch) against what the Python host got for the same PCM and units.
// argv[2]: a directory with, per tag (_1: 24 mono frames, _2: 24 stereo frames), ch0<tag>.f32 and ch1_2.f32 (raw float32),
// units<tag>.u8 and, from the Python host under the packaged tables, noise, signal, totals and weights <tag>_own.f64 and
// <tag>_long.f64, written by tests/test_js_measure_units_shared.py.  Prints ALL OK on success.
import fs from 'fs'
import path from 'path'

import * as api from '../carta1_amd/js/index.js'

const { measureUnits, MASKING_DEFAULT } = api
const dir = process.argv[2]
const raw = (name) => { const b = fs.readFileSync(path.join(dir, name)); return b.buffer.slice(b.byteOffset, b.byteOffset + b.length) }
const f32 = (name) => new Float32Array(raw(name))
const f64 = (name) => new Float64Array(raw(name))
const u8 = (name) => new Uint8Array(fs.readFileSync(path.join(dir, name)))
const bytes = (a) => Buffer.from(a.buffer, a.byteOffset, a.byteLength)

// codec/index.js:26-47 of the reference
const REFERENCE_EXPORTS = ['encode', 'decode', 'qmfAnalysisStage', 'mdctStage', 'serializeFrame', 'deserializeFrame', 'AeaFile', 'AudioProcessor',
  'quantize', 'dequantize', 'FFT', 'BufferPool', 'EncoderOptions', 'pipe', 'WORD_LENGTH_BITS', 'SPECS_PER_BFU', 'SCALE_FACTORS', 'BFU_START_LONG',
  'encodeAeaPcm', 'decodeAeaPcm']
const OUTPUTS = [['noise', 52], ['signal', 52], ['totals', 2], ['weights', 52]]

let failures = 0
function ok(cond, msg) { if (!cond) { failures++; console.log('FAIL', msg) } }
function rejects(fn, needles, msg) {
  let err = null
  try { fn() } catch (e) { err = e }
  ok(err instanceof TypeError && needles.every((n) => String(err.message).includes(n)), `${msg}: expected a TypeError naming ${needles}, got ${err}`)
}

function main() {
  ok(REFERENCE_EXPORTS.length === 20 && REFERENCE_EXPORTS.every((n) => api[n] !== undefined), 'the twenty reference names are still exported')
  ok(typeof api.measureUnits === 'function' && api.measureUnitsShared === undefined, 'measureUnits is the one exported name')
  for (const [tag, nch] of [['_1', 1], ['_2', 2]]) {
    const chs = nch === 1 ? [f32('ch0_1.f32')] : [f32('ch0_2.f32'), f32('ch1_2.f32')]
    const units = u8(`units${tag}.u8`)
    const count = (chs[0].length / 512) * nch
    for (const [options, suffix, what] of [[{ masking: true, thresholdFrom: 'long' }, '_long', 'long'], [{ masking: true, thresholdFrom: 'own' }, '_own', 'own'],
      [{ masking: true }, '_own', 'absent']]) {
      const got = measureUnits(chs, units, options)
      for (const [name, width] of OUTPUTS) {
        ok(got[name] instanceof Float64Array && got[name].length === count * width, `${name}${tag} (${what}) is a Float64Array of ${width} per unit`)
        ok(bytes(got[name]).equals(bytes(f64(`${name}${tag}${suffix}.f64`))), `${name}${tag} (${what}) == the Python result, bit for bit`)
      }
    }
    const long = measureUnits(chs, units, { masking: true, thresholdFrom: 'long' })
    const own = measureUnits(chs, units, { masking: true })
    ok(bytes(long.noise).equals(bytes(own.noise)) && bytes(long.signal).equals(bytes(own.signal)), `noise and signal do not depend on thresholdFrom (${tag})`)
    ok(!bytes(long.weights).equals(bytes(own.weights)) && !bytes(long.totals).equals(bytes(own.totals)), `weights and totals do (${tag})`)
    // the packaged tables spelled out are `true`; the last frames from a halo are the rows of the whole call
    const again = measureUnits(chs, units, { masking: { floor: MASKING_DEFAULT.floor, spread: MASKING_DEFAULT.spread }, thresholdFrom: 'long' })
    ok(bytes(again.totals).equals(bytes(long.totals)) && bytes(again.weights).equals(bytes(long.weights)), `MASKING_DEFAULT spelled out is masking: true (${tag})`)
    const tail = measureUnits(chs, units.subarray(2 * nch * 212), { masking: true, haloFrames: 2, thresholdFrom: 'long' })
    ok(bytes(tail.weights).equals(bytes(long.weights.subarray(2 * nch * 52))) && bytes(tail.totals).equals(bytes(long.totals.subarray(2 * nch * 2))),
      `two frames of halo give the rows of the whole call (${tag})`)
    // without tables 'own' is still the table-less call
    const plain = measureUnits(chs, units, { thresholdFrom: 'own' })
    ok(plain.weights === undefined && bytes(plain.noise).equals(bytes(own.noise)), `thresholdFrom 'own' without masking (${tag})`)
  }

  const chs = [f32('ch0_2.f32'), f32('ch1_2.f32')]
  const units = u8('units_2.u8')
  const withFirst = (u, v) => { const b = Uint8Array.from(units); b[212 * u] = v; return b }
  for (const bad of ['short', 'Long', null, 0, true, ['long']]) {
    rejects(() => measureUnits(chs, units, { masking: true, thresholdFrom: bad }), ['thresholdFrom', "'own' or 'long'"], `thresholdFrom ${String(bad)}`)
  }
  rejects(() => measureUnits(chs, units, { thresholdFrom: 'long' }), ['thresholdFrom', 'needs masking'], "'long' without masking")
  rejects(() => measureUnits(chs, units, { thresholdFrom: 'long', masking: null }), ['thresholdFrom', 'needs masking'], "'long' with masking null")
  rejects(() => measureUnits(chs, withFirst(5, 0x40), { masking: true, thresholdFrom: 'long' }), ['units', 'frame 2, channel 1', 'low block mode', 'is 1, not 0 or 2'],
    'a low field the encoder never writes')
  rejects(() => measureUnits(chs, units.subarray(212), { masking: true, thresholdFrom: 'long' }), ['units', '212 bytes'], 'a unit short')
  rejects(() => measureUnits(chs, units, { masking: true, thresholdFrom: 'long', haloFrames: 3 }), ['haloFrames'], 'three frames of halo')
  rejects(() => measureUnits(chs, units, { masking: 'default', thresholdFrom: 'long' }), ['masking', 'true or'], 'masking as a string')
  rejects(() => measureUnits(chs, units, { thresholdFrom: 'long', masking: { floor: Array.from(MASKING_DEFAULT.floor, (v, b) => (b === 3 ? 0 : v)), spread: null } }),
    ['masking.floor[3]'], 'a floor of zero')

  if (failures) { console.log(`${failures} FAILURES`); process.exit(1) }
  console.log('ALL OK')
}

try { main() } catch (e) { console.log('ERROR', e && e.stack ? e.stack : e); process.exit(1) }
