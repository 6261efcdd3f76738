// The encode(options, bufferPool, measured) frame closure (carta1_amd/js/pipeline/encoder.js -> c1_enc_stream_push_measured)
// against what the Python host's EncoderStream.push_measured got for the same PCM, frame by frame.
// argv[2]: a directory with ch0.f32 (raw float32, mono) and, from the Python host, one unit per frame in units_masked.u8
// (packaged tables and the suggested offsets), units_sf.u8 (the offsets alone), units_measured.u8 (neither), units_plain.u8
// (EncoderStream.push) and units_mixed.u8 (even frames plain, odd frames masked, on one stream), written by
// tests/test_js_stream_measured.py.  Prints ALL OK on success.
import fs from 'fs'
import path from 'path'

import { encode, serializeFrame, EncoderOptions, BufferPool, SCALE_FACTOR_OFFSETS, MASKING_DEFAULT } from '../carta1_amd/js/index.js'

const dir = process.argv[2]
const raw = (name) => { const b = fs.readFileSync(path.join(dir, name)); return b.buffer.slice(b.byteOffset, b.byteOffset + b.length) }
const u8 = (name) => new Uint8Array(fs.readFileSync(path.join(dir, name)))
const bytes = (a) => Buffer.from(a.buffer, a.byteOffset, a.byteLength)

let failures = 0
function ok(cond, msg) { if (!cond) { failures++; console.log('FAIL', msg) } }
function throwsTypeError(fn, needles, msg) {
  let err = null
  try { fn() } catch (e) { err = e }
  ok(err instanceof TypeError && needles.every((n) => String(err.message).includes(n)), `${msg}: expected TypeError naming ${needles}, got ${err}`)
}

function main() {
  const pcm = new Float32Array(raw('ch0.f32'))
  const frames = pcm.length / 512
  const frame = (f) => pcm.slice(f * 512, (f + 1) * 512)
  const run = (closureOf) => {
    const enc = closureOf()
    const units = []
    for (let f = 0; f < frames; f++) {
      const fields = enc(frame(f), f)
      ok(fields.blockModes.length === 3 && Number.isInteger(fields.nBfu), `frame ${f}: a fields object`)
      units.push(Buffer.from(serializeFrame(fields)))
    }
    return Buffer.concat(units)
  }
  const masked = { measuredAllocation: true, scaleFactorOffsets: SCALE_FACTOR_OFFSETS, masking: true }
  const cases = [
    ['masked', () => encode(new EncoderOptions(), new BufferPool(), masked)],
    ['masked', () => encode(new EncoderOptions(), new BufferPool(), { ...masked, masking: MASKING_DEFAULT })],
    ['sf', () => encode(new EncoderOptions(), new BufferPool(), { measuredAllocation: true, scaleFactorOffsets: SCALE_FACTOR_OFFSETS })],
    ['measured', () => encode(new EncoderOptions(), new BufferPool(), { measuredAllocation: true })],
    // without the third argument, or with measuredAllocation falsy, the closure is the reference's
    ['plain', () => encode(new EncoderOptions(), new BufferPool())],
    ['plain', () => encode(new EncoderOptions(), new BufferPool(), {})],
    ['plain', () => encode(new EncoderOptions(), new BufferPool(), { measuredAllocation: false })],
    ['plain', () => encode(new EncoderOptions(), new BufferPool(), null)],
  ]
  for (const [tag, closureOf] of cases) {
    ok(run(closureOf).equals(bytes(u8(`units_${tag}.u8`))), `the closure's serialised fields == the Python stream's units_${tag}`)
  }
  ok(!bytes(u8('units_masked.u8')).equals(bytes(u8('units_plain.u8'))), 'the measured allocation changes some unit')
  // the object is read per call: one closure, even frames plain, odd frames masked
  const how = {}
  ok(run(() => {
    const enc = encode(new EncoderOptions(), new BufferPool(), how)
    return (x, f) => {
      how.measuredAllocation = f % 2 === 1
      how.scaleFactorOffsets = f % 2 === 1 ? SCALE_FACTOR_OFFSETS : undefined
      how.masking = f % 2 === 1 ? true : undefined
      return enc(x)
    }
  }).equals(bytes(u8('units_mixed.u8'))), 'the third argument is read per call')

  // the TypeErrors of encodeAeaPcm, naming the option; the pool goes on as if the call had not been made
  const pool = new BufferPool()
  const wrong = {}
  const enc = encode(new EncoderOptions(), pool, wrong)
  const first = Buffer.from(serializeFrame(enc(frame(0))))
  const bad = [[{ scaleFactorOffsets: [0, -1] }, ['scaleFactorOffsets', 'measuredAllocation']],
    [{ masking: true }, ['masking', 'measuredAllocation']],
    [{ measuredAllocation: false, masking: true }, ['masking', 'measuredAllocation']],
    [{ measuredAllocation: false, scaleFactorOffsets: [0] }, ['scaleFactorOffsets', 'measuredAllocation']],
    [{ measuredAllocation: 1 }, ['measuredAllocation', 'boolean']],
    [{ measuredAllocation: true, scaleFactorOffsets: [0, 9] }, ['scaleFactorOffsets[1]']],
    [{ measuredAllocation: true, scaleFactorOffsets: [1, 0] }, ['scaleFactorOffsets[0]']],
    [{ measuredAllocation: true, masking: { floor: [1, 2, 3], spread: null } }, ['masking.floor', '52']],
    [{ measuredAllocation: true, masking: 'default' }, ['masking', 'true or']]]
  for (const [values, needles] of bad) {
    for (const k of Object.keys(wrong)) delete wrong[k]
    Object.assign(wrong, values)
    throwsTypeError(() => enc(frame(1)), needles, JSON.stringify(values))
  }
  for (const k of Object.keys(wrong)) delete wrong[k]
  const second = Buffer.from(serializeFrame(enc(frame(1))))
  ok(Buffer.concat([first, second]).equals(bytes(u8('units_plain.u8')).subarray(0, 2 * 212)), 'after the TypeErrors the stream goes on as before')

  if (failures) { console.log(`${failures} FAILURES`); process.exit(1) }
  console.log('ALL OK')
}

try { main() } catch (e) { console.log('ERROR', e && e.stack ? e.stack : e); process.exit(1) }
