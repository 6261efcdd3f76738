// The encode(options, bufferPool, measured) frame closure with measuredModeCandidates (carta1_amd/js/pipeline/encoder.js ->
// c1_enc_stream_push_measured_modes) against what the Python host's EncoderStream.push_measured_modes got for the same PCM, frame
// by frame.
// argv[2]: a directory with ch0.f32 (raw float32, mono) and, from the Python host, one unit per frame in units_sf.u8 (the eight
// candidates and the suggested offsets), units_plain.u8 (the candidates alone) and units_mixed.u8 (even frames EncoderStream.push,
// odd frames the candidates with the offsets, on one stream), and the chosen mode byte per frame in modes_sf.u8 and modes_plain.u8,
// written by tests/test_js_stream_measured_modes.py.  Prints ALL OK on success.
import fs from 'fs'
import path from 'path'

import * as api from '../carta1_amd/js/index.js'

const { encode, serializeFrame, EncoderOptions, BufferPool, SCALE_FACTOR_OFFSETS } = api
const dir = process.argv[2]
const raw = (name) => { const b = fs.readFileSync(path.join(dir, name)); return b.buffer.slice(b.byteOffset, b.byteOffset + b.length) }
const u8 = (name) => new Uint8Array(fs.readFileSync(path.join(dir, name)))
const bytes = (a) => Buffer.from(a.buffer, a.byteOffset, a.byteLength)
const CANDIDATES = [0, 48, 8, 56, 2, 50, 10, 58]

let failures = 0
function ok(cond, msg) { if (!cond) { failures++; console.log('FAIL', msg) } }
function throwsA(kind, fn, needles, msg) {
  let err = null
  try { fn() } catch (e) { err = e }
  ok(err instanceof kind && needles.every((n) => String(err.message).includes(n)), `${msg}: expected ${kind.name} naming ${needles}, got ${err}`)
}

function main() {
  const REFERENCE_EXPORTS = ['encode', 'decode', 'qmfAnalysisStage', 'mdctStage', 'serializeFrame', 'deserializeFrame', 'AeaFile', 'AudioProcessor',
    'quantize', 'dequantize', 'FFT', 'BufferPool', 'EncoderOptions', 'pipe', 'WORD_LENGTH_BITS', 'SPECS_PER_BFU', 'SCALE_FACTORS', 'BFU_START_LONG',
    'encodeAeaPcm', 'decodeAeaPcm']
  ok(REFERENCE_EXPORTS.length === 20 && REFERENCE_EXPORTS.every((n) => api[n] !== undefined), 'the twenty reference names are still exported')
  ok(api.modeCandidateBytes === undefined && api.encStreamPushMeasuredModes === undefined, 'index.js gains no name')
  const pcm = new Float32Array(raw('ch0.f32'))
  const frames = pcm.length / 512
  const frame = (f) => pcm.slice(f * 512, (f + 1) * 512)
  const run = (closureOf, modes) => {
    const enc = closureOf()
    const units = []
    for (let f = 0; f < frames; f++) {
      const fields = enc(frame(f), f)
      ok(fields.blockModes.length === 3 && Number.isInteger(fields.nBfu), `frame ${f}: a fields object`)
      if (modes) {
        const byte = fields.blockModes[0] | (fields.blockModes[1] << 2) | (fields.blockModes[2] << 4)
        ok(byte === modes[f], `frame ${f}: blockModes ${fields.blockModes} are the unit's, byte ${modes[f]}`)
      }
      units.push(Buffer.from(serializeFrame(fields)))
    }
    return Buffer.concat(units)
  }
  const sf = { measuredAllocation: true, measuredModeCandidates: CANDIDATES, scaleFactorOffsets: SCALE_FACTOR_OFFSETS }
  const triples = CANDIDATES.map((b) => [b & 3, (b >> 2) & 3, (b >> 4) & 3])
  const cases = [
    ['sf', () => encode(new EncoderOptions(), new BufferPool(), sf)],
    ['sf', () => encode(new EncoderOptions(), new BufferPool(), { ...sf, measuredModeCandidates: Uint8Array.from(CANDIDATES) })],
    ['sf', () => encode(new EncoderOptions(), new BufferPool(), { ...sf, measuredModeCandidates: triples })],
    ['plain', () => encode(new EncoderOptions(), new BufferPool(), { measuredAllocation: true, measuredModeCandidates: CANDIDATES })],
    // whatever the options' block modes are: the candidates choose, and the fields carry the unit's modes
    ['sf', () => encode(new EncoderOptions({ fixedBlockModes: [2, 2, 0] }), new BufferPool(), sf)],
  ]
  for (const [tag, closureOf] of cases) {
    ok(run(closureOf, u8(`modes_${tag}.u8`)).equals(bytes(u8(`units_${tag}.u8`))), `the closure's serialised fields == the Python stream's units_${tag}`)
  }
  ok(!bytes(u8('units_sf.u8')).equals(bytes(u8('units_plain.u8'))), 'the offsets change some unit')
  // the object is read per call: one closure, even frames plain, odd frames searched
  const how = {}
  ok(run(() => {
    const enc = encode(new EncoderOptions(), new BufferPool(), how)
    return (x, f) => {
      how.measuredAllocation = f % 2 === 1
      how.measuredModeCandidates = f % 2 === 1 ? CANDIDATES : undefined
      how.scaleFactorOffsets = f % 2 === 1 ? SCALE_FACTOR_OFFSETS : undefined
      return enc(x)
    }
  }).equals(bytes(u8('units_mixed.u8'))), 'the third argument is read per call')

  // the TypeErrors of encodeAeaPcm, naming the options; the pool goes on as if the call had not been made
  const pool = new BufferPool()
  const wrong = { ...sf }
  const enc = encode(new EncoderOptions(), pool, wrong)
  const first = Buffer.from(serializeFrame(enc(frame(0))))
  const bad = [[TypeError, { measuredModeCandidates: CANDIDATES }, ['measuredModeCandidates', 'measuredAllocation']],
    [TypeError, { measuredAllocation: false, measuredModeCandidates: CANDIDATES }, ['measuredModeCandidates', 'measuredAllocation']],
    [TypeError, { ...sf, masking: true }, ['measuredModeCandidates', 'masking']],
    [RangeError, { measuredAllocation: true, measuredModeCandidates: [] }, ['measuredModeCandidates', '1 to 8']],
    [RangeError, { measuredAllocation: true, measuredModeCandidates: [0, 2, 8, 10, 48, 50, 56, 58, 0] }, ['measuredModeCandidates', '1 to 8']],
    [TypeError, { measuredAllocation: true, measuredModeCandidates: [[2, 2]] }, ['triple']],
    [TypeError, { measuredAllocation: true, measuredModeCandidates: [0.5] }, ['mode bytes']],
    [TypeError, { ...sf, scaleFactorOffsets: [0, 9] }, ['scaleFactorOffsets[1]']],
    [Error, { measuredAllocation: true, measuredModeCandidates: [0, 1] }, ['candidate 1', 'low field']],
    [Error, { measuredAllocation: true, measuredModeCandidates: [10, 10] }, ['candidate 1', "candidate 0's"]]]
  for (const [kind, values, needles] of bad) {
    for (const k of Object.keys(wrong)) delete wrong[k]
    Object.assign(wrong, values)
    throwsA(kind, () => enc(frame(1)), needles, JSON.stringify(values))
  }
  for (const k of Object.keys(wrong)) delete wrong[k]
  Object.assign(wrong, sf)
  const second = Buffer.from(serializeFrame(enc(frame(1))))
  ok(Buffer.concat([first, second]).equals(bytes(u8('units_sf.u8')).subarray(0, 2 * 212)), 'after the errors the stream goes on as before')

  if (failures) { console.log(`${failures} FAILURES`); process.exit(1) }
  console.log('ALL OK')
}

try { main() } catch (e) { console.log('ERROR', e && e.stack ? e.stack : e); process.exit(1) }
