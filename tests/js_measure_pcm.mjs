// measurePcm(channels, units, { haloFrames, haloUnits }) (carta1_amd/js/native.js -> c1_measure_pcm_batch) against what the
// Python host got for the same PCM and units.
// argv[2]: a directory with, per tag (_1: 24 mono frames, _2: 24 stereo frames), ch0<tag>.f32 and ch1_2.f32 (raw float32),
// units<tag>.u8 and, from the Python host, noise, signal and totals <tag>.f64, written by tests/test_js_measure_pcm.py.
// Prints ALL OK on success.
import fs from 'fs'
import path from 'path'

import * as api from '../carta1_amd/js/index.js'

const { measurePcm } = api
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
  ok(typeof api.measurePcm === 'function' && typeof api.measureUnits === 'function', 'measurePcm is exported next to measureUnits')
  ok(api.PCM_DELAY === 266, 'PCM_DELAY is 266')
  for (const [tag, nch] of [['_1', 1], ['_2', 2]]) {
    const chs = nch === 1 ? [f32('ch0_1.f32')] : [f32('ch0_2.f32'), f32('ch1_2.f32')]
    const units = u8(`units${tag}.u8`)
    const count = (chs[0].length / 512) * nch
    const whole = measurePcm(chs, units)
    for (const [name, width] of [['noise', 16], ['signal', 16], ['totals', 2]]) {
      ok(whole[name] instanceof Float64Array && whole[name].length === count * width, `${name}${tag} is a Float64Array of ${width} per unit`)
      ok(bytes(whole[name]).equals(bytes(f64(`${name}${tag}.f64`))), `${name}${tag} == the Python result, bit for bit`)
    }
    ok(whole.totals.some((v) => v > 0) && Object.keys(whole).length === 3, `totals${tag} are not all zero`)
    // the last frames from both halos are the rows of the whole call, with one and with two frames of PCM
    for (const haloFrames of [1, 2]) {
      const start = 4
      const tail = measurePcm(chs.map((c) => c.subarray((start - haloFrames) * 512)), units.subarray((start - 1) * nch * 212), { haloFrames, haloUnits: 1 })
      ok(bytes(tail.noise).equals(bytes(whole.noise.subarray(start * nch * 16))) && bytes(tail.signal).equals(bytes(whole.signal.subarray(start * nch * 16))) &&
        bytes(tail.totals).equals(bytes(whole.totals.subarray(start * nch * 2))), `the halos give the rows of the whole call (${tag}, haloFrames ${haloFrames})`)
    }
    // without the halos the first rows differ and the later ones do not
    const bare = measurePcm(chs.map((c) => c.subarray(4 * 512)), units.subarray(4 * nch * 212))
    ok(!bytes(bare.noise.subarray(0, 16)).equals(bytes(whole.noise.subarray(4 * nch * 16, 4 * nch * 16 + 16))) &&
      bytes(bare.noise.subarray(2 * nch * 16)).equals(bytes(whole.noise.subarray(6 * nch * 16))), `a fresh start differs for two frames at most (${tag})`)
  }

  const chs = [f32('ch0_2.f32'), f32('ch1_2.f32')]
  const units = u8('units_2.u8')
  rejects(() => measurePcm(chs, units.subarray(212)), ['units', '212 bytes'], 'a unit short')
  rejects(() => measurePcm(chs, units, { haloUnits: 1 }), ['units', '50 sound units'], 'no room for the halo unit')
  rejects(() => measurePcm(chs, Array.from(units)), ['units', 'Uint8Array'], 'units as a plain array')
  rejects(() => measurePcm([chs[0], chs[1].subarray(512)], units), ['channels', 'equal length'], 'channels of unequal length')
  rejects(() => measurePcm([Array.from(chs[0])], units), ['channels', 'Float32Array'], 'a channel as a plain array')
  rejects(() => measurePcm([chs[0], chs[1], chs[0]], units), ['channels', 'one or two'], 'three channels')
  rejects(() => measurePcm(chs, units, { haloFrames: 3 }), ['haloFrames'], 'three frames of halo')
  rejects(() => measurePcm(chs, units, { haloFrames: 0.5 }), ['haloFrames'], 'half a frame of halo')
  rejects(() => measurePcm(chs, units, { haloUnits: 2 }), ['haloUnits'], 'two halo units')
  rejects(() => measurePcm(chs, units, null), ['options'], 'options null')

  if (failures) { console.log(`${failures} FAILURES`); process.exit(1) }
  console.log('ALL OK')
}

try { main() } catch (e) { console.log('ERROR', e && e.stack ? e.stack : e); process.exit(1) }
