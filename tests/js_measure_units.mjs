// measureUnits(channels, units, { masking, haloFrames }) (carta1_amd/js/native.js -> c1_measure_units_batch) against what the
// Python host got for the same PCM and units.
// argv[2]: a directory with, per tag (_1: 24 mono frames, _2: 24 stereo frames), ch0<tag>.f32 and ch1_2.f32 (raw float32),
// units<tag>.u8 and, from the Python host, noise, signal and totals <tag>.f64 (no masking) and noise, signal, totals and weights
// <tag>_p.f64 (the packaged tables), written by tests/test_js_measure_units.py.  Prints ALL OK on success.
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

let failures = 0
function ok(cond, msg) { if (!cond) { failures++; console.log('FAIL', msg) } }
function rejects(fn, needles, msg) {
  let err = null
  try { fn() } catch (e) { err = e }
  ok(err instanceof TypeError && needles.every((n) => String(err.message).includes(n)), `${msg}: expected a TypeError naming ${needles}, got ${err}`)
}

function main() {
  ok(REFERENCE_EXPORTS.length === 20 && REFERENCE_EXPORTS.every((n) => api[n] !== undefined), 'the twenty reference names are still exported')
  ok(typeof api.measureUnits === 'function' && typeof api.encodeMeasured === 'function', 'measureUnits is exported next to encodeMeasured')
  for (const [tag, nch] of [['_1', 1], ['_2', 2]]) {
    const chs = nch === 1 ? [f32('ch0_1.f32')] : [f32('ch0_2.f32'), f32('ch1_2.f32')]
    const units = u8(`units${tag}.u8`)
    const count = (chs[0].length / 512) * nch
    for (const [masking, suffix] of [[null, ''], [true, '_p']]) {
      const got = measureUnits(chs, units, masking === null ? {} : { masking })
      for (const [name, width] of [['noise', 52], ['signal', 52], ['totals', 2]]) {
        ok(got[name] instanceof Float64Array && got[name].length === count * width, `${name}${tag}${suffix} is a Float64Array of ${width} per unit`)
        ok(bytes(got[name]).equals(bytes(f64(`${name}${tag}${suffix}.f64`))), `${name}${tag}${suffix} == the Python result, bit for bit`)
      }
      if (masking === null) ok(got.weights === undefined, `no weights without masking (${tag})`)
      else ok(got.weights instanceof Float64Array && bytes(got.weights).equals(bytes(f64(`weights${tag}_p.f64`))), `weights${tag}_p == the Python result, bit for bit`)
      ok(got.totals.some((v) => v > 0), `totals${tag}${suffix} are not all zero`)
    }
    // the packaged tables spelled out are `true`; the last frames from a halo are the rows of the whole call
    const whole = measureUnits(chs, units, { masking: true })
    const again = measureUnits(chs, units, { masking: { floor: MASKING_DEFAULT.floor, spread: MASKING_DEFAULT.spread } })
    ok(bytes(again.totals).equals(bytes(whole.totals)) && bytes(again.weights).equals(bytes(whole.weights)), `MASKING_DEFAULT spelled out is masking: true (${tag})`)
    const tail = measureUnits(chs, units.subarray(2 * nch * 212), { masking: true, haloFrames: 2 })
    ok(bytes(tail.noise).equals(bytes(whole.noise.subarray(2 * nch * 52))) && bytes(tail.totals).equals(bytes(whole.totals.subarray(2 * nch * 2))),
      `two frames of halo give the rows of the whole call (${tag})`)
  }

  const chs = [f32('ch0_2.f32'), f32('ch1_2.f32')]
  const units = u8('units_2.u8')
  const withFirst = (u, v) => { const b = Uint8Array.from(units); b[212 * u] = v; return b }
  rejects(() => measureUnits(chs, withFirst(5, 0x40)), ['units', 'frame 2, channel 1', 'low block mode', 'is 1, not 0 or 2'], 'a low field the encoder never writes')
  rejects(() => measureUnits(chs, withFirst(4, 0x9c)), ['frame 2, channel 0', 'mid block mode'], 'a mid field the encoder never writes')
  rejects(() => measureUnits(chs, withFirst(0, 0xa4)), ['frame 0, channel 0', 'high block mode', 'is 2, not 0 or 3'], 'a high field the encoder never writes')
  rejects(() => measureUnits([chs[0]], withFirst(3, 0xc8).subarray(0, units.length / 2)), ['units: frame 3:', 'low block mode', 'is -1'], 'mono names the frame alone')
  rejects(() => measureUnits(chs, units.subarray(212)), ['units', '212 bytes'], 'a unit short')
  rejects(() => measureUnits(chs, Array.from(units)), ['units', 'Uint8Array'], 'units as a plain array')
  rejects(() => measureUnits([chs[0], chs[1].subarray(512)], units), ['channels', 'equal length'], 'channels of unequal length')
  rejects(() => measureUnits([Array.from(chs[0])], units), ['channels', 'Float32Array'], 'a channel as a plain array')
  rejects(() => measureUnits(chs, units, { haloFrames: 3 }), ['haloFrames'], 'three frames of halo')
  rejects(() => measureUnits(chs, units, null), ['options'], 'options null')
  rejects(() => measureUnits(chs, units, { masking: 'default' }), ['masking', 'true or'], 'masking as a string')
  rejects(() => measureUnits(chs, units, { masking: { floor: Array.from(MASKING_DEFAULT.floor, (v, b) => (b === 3 ? 0 : v)), spread: null } }),
    ['masking.floor[3]'], 'a floor of zero')
  rejects(() => measureUnits(chs, units, { masking: { floor: MASKING_DEFAULT.floor, spread: Array.from(MASKING_DEFAULT.spread, (v, i) => (i === 165 ? -1 : v)) } }),
    ['masking.spread[165]'], 'a negative spread entry')

  if (failures) { console.log(`${failures} FAILURES`); process.exit(1) }
  console.log('ALL OK')
}

try { main() } catch (e) { console.log('ERROR', e && e.stack ? e.stack : e); process.exit(1) }
