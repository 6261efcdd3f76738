// The JavaScript decode() closure (carta1_amd/js/pipeline/decoder.js) over the frameData objects of every case of
// tests/golden/decoder_stages.json, one BufferPool per case, compared bit for bit with the reference's own decode() PCM;
// the hand-built case holds fields serializeFrame does not carry, where decoding through a serialized unit gives other PCM.
// Sound units and frameData objects mixed in one closure decode as objects alone, and an index the device cannot name
// throws what dequantizationStage throws for it.  Prints ALL OK on success; run by tests/test_js_decode_fields.py.
import fs from 'fs'
import path from 'path'
import { fileURLToPath } from 'url'

import { BufferPool } from '../carta1_amd/js/core/buffers.js'
import { SPECS_PER_BFU } from '../carta1_amd/js/core/constants.js'
import { serializeFrame } from '../carta1_amd/js/io/serialization.js'
import { decode, dequantizationStage } from '../carta1_amd/js/pipeline/decoder.js'

const G = path.join(path.dirname(fileURLToPath(import.meta.url)), 'golden')
const index = JSON.parse(fs.readFileSync(path.join(G, 'decoder_stages.json'), 'utf8'))

function load(c) {
  const raw = fs.readFileSync(path.join(G, c.file))
  const buf = raw.buffer.slice(raw.byteOffset, raw.byteOffset + raw.byteLength)
  const out = {}
  let at = 0
  for (const a of c.arrays) {
    const per = a.shape.length > 1 ? a.shape[1] : 1
    const n = a.shape[0] * per
    out[a.name] = { data: a.dtype === 'int32' ? new Int32Array(buf, at, n) : new Float32Array(buf, at, n), per }
    at += 4 * n
  }
  return out
}
const row = (a, f) => a.data.subarray(f * a.per, (f + 1) * a.per)
const sameBits = (x, y) => {
  const a = new Uint32Array(x.buffer, x.byteOffset, x.length), b = new Uint32Array(y.buffer, y.byteOffset, y.length)
  if (a.length !== b.length) return false
  for (let i = 0; i < a.length; i++) if (a[i] !== b[i]) return false
  return true
}
function frameDataOf(d, f) {
  const nBfu = row(d.nbfu, f)[0]
  const q = row(d.quantized, f), quantizedCoefficients = []
  for (let b = 0, at = 0; b < nBfu; at += SPECS_PER_BFU[b], b++) quantizedCoefficients.push(q.slice(at, at + SPECS_PER_BFU[b]))
  return { nBfu, scaleFactorIndices: row(d.sfi, f).slice(0, nBfu), wordLengthIndices: row(d.wl, f).slice(0, nBfu),
           quantizedCoefficients, blockModes: Array.from(row(d.block_modes, f)) }
}
function unitsOf(c) {   // the case's own sound units, where it was unpacked from a KAT file
  if (!c.source || !c.source.endsWith('.units.bin')) return null
  const all = fs.readFileSync(path.join(G, c.source))
  const out = []
  for (let f = 0; f < c.frames; f++) {
    const at = ((c.first_frame + f) * c.channels + c.channel) * 212
    out.push(new Uint8Array(all.subarray(at, at + 212)))
  }
  return out
}

let failures = 0
const fail = (msg) => { failures++; console.log(msg) }
for (const c of index.cases) {
  const d = load(c)
  const frames = []
  for (let f = 0; f < c.frames; f++) frames.push(frameDataOf(d, f))
  const dec = decode(new BufferPool())
  const pcm = frames.map((fd) => dec(fd))
  pcm.forEach((p, f) => { if (!(p instanceof Float32Array) || !sameBits(p, row(d.pcm, f))) fail(`${c.name} frame ${f}: pcm differs`) })
  // the former route: serializeFrame, then the unit
  let serialized = true
  try {
    const old = decode(new BufferPool())
    for (let f = 0; f < c.frames; f++) if (!sameBits(old(serializeFrame(frames[f])), row(d.pcm, f))) serialized = false
  } catch (e) { serialized = false }
  if (c.name === 'fields' && serialized) fail('fields: the serialized route decodes as the reference; the case shows nothing')
  // units and objects mixed in one closure
  const units = unitsOf(c)
  if (units) {
    const mixed = decode(new BufferPool())
    for (let f = 0; f < c.frames; f++) {
      const p = mixed((f % 3 === 1) ? frames[f] : units[f])
      if (!sameBits(p, pcm[f])) fail(`${c.name} frame ${f}: mixed units and objects differ from objects alone`)
    }
  }
  console.log(`${c.name}: ${c.frames} frames checked`)
}

// an index the device cannot name: the closure throws what dequantizationStage throws (same code, same message after the
// entry point's name)
{
  const d = load(index.cases.find((c) => c.name === 'fields'))
  const base = frameDataOf(d, 3)                                // nBfu 7
  const edits = [['nBfu', 53], ['nBfu', -1], ['wl', 16], ['sfi', 64], ['wl', -1]]
  for (const [what, value] of edits) {
    const fd = { ...base, scaleFactorIndices: Int32Array.from(base.scaleFactorIndices), wordLengthIndices: Int32Array.from(base.wordLengthIndices) }
    if (what === 'nBfu') fd.nBfu = value
    else if (what === 'wl') fd.wordLengthIndices[base.nBfu - 1] = value
    else fd.scaleFactorIndices[base.nBfu - 1] = value
    const caught = (fn) => { try { fn(); return null } catch (e) { return e } }
    const a = caught(() => decode(new BufferPool())(fd)), b = caught(() => dequantizationStage()(fd))
    const tail = (e) => e && e.message.replace(/^carta1_hip: [a-z ]+: /, '')
    if (!a || !b || a.code !== 'C1_ERR_ARG' || a.code !== b.code || tail(a) !== tail(b)) {
      fail(`${what} ${value}: decode() threw ${a && a.code} '${a && a.message}', dequantizationStage ${b && b.code} '${b && b.message}'`)
    }
  }
  // junk at and above nBfu is not read
  const junk = { ...base, scaleFactorIndices: Int32Array.from([...base.scaleFactorIndices, 99, -3]),
                 wordLengthIndices: Int32Array.from([...base.wordLengthIndices, 77, 16]) }
  if (!sameBits(decode(new BufferPool())(junk), decode(new BufferPool())(base))) fail('junk above nBfu changed the output')
}
if (failures) { console.log(`${failures} mismatches`); process.exit(1) }
console.log('ALL OK')
