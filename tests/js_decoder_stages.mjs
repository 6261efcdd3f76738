// The JavaScript decoder stages (carta1_amd/js/pipeline/decoder.js: dequantizationStage, imdctStage, qmfSynthesisStage) over the
// frames of every case of tests/golden/decoder_stages.json, one BufferPool per case as the reference's generator ran them,
// compared bit for bit with what the reference's own stages returned.  Prints ALL OK on success; run by
// tests/test_js_decoder_stages.py.
import fs from 'fs'
import path from 'path'
import { fileURLToPath } from 'url'

import { BufferPool } from '../carta1_amd/js/core/buffers.js'
import { SPECS_PER_BFU } from '../carta1_amd/js/core/constants.js'
import { dequantizationStage, imdctStage, qmfSynthesisStage } from '../carta1_amd/js/pipeline/decoder.js'

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

let failures = 0
for (const c of index.cases) {
  const d = load(c)
  const context = { bufferPool: new BufferPool() }
  const dq = dequantizationStage(), im = imdctStage(context), qs = qmfSynthesisStage(context)
  for (let f = 0; f < c.frames; f++) {
    const nBfu = row(d.nbfu, f)[0]
    const q = row(d.quantized, f), quantizedCoefficients = []
    for (let b = 0, at = 0; b < nBfu; at += SPECS_PER_BFU[b], b++) quantizedCoefficients.push(q.slice(at, at + SPECS_PER_BFU[b]))
    const frameData = { nBfu, scaleFactorIndices: row(d.sfi, f).slice(0, nBfu), wordLengthIndices: row(d.wl, f).slice(0, nBfu),
                        quantizedCoefficients, blockModes: Array.from(row(d.block_modes, f)) }
    const r = dq(frameData)
    if (r.blockModes !== frameData.blockModes || !sameBits(r.coefficients, row(d.coefficients, f))) { failures++; console.log(`${c.name} frame ${f}: coefficients differ`) }
    const bands = im(r)
    const want = row(d.bands, f)
    if (bands.length !== 3 || !sameBits(bands[0], want.subarray(0, 128)) || !sameBits(bands[1], want.subarray(128, 256)) ||
        !sameBits(bands[2], want.subarray(256, 512))) { failures++; console.log(`${c.name} frame ${f}: bands differ`) }
    const pcm = qs(bands)
    if (!(pcm instanceof Float32Array) || !sameBits(pcm, row(d.pcm, f))) { failures++; console.log(`${c.name} frame ${f}: pcm differs`) }
  }
  console.log(`${c.name}: ${c.frames} frames checked`)
}
if (failures) { console.log(`${failures} mismatches`); process.exit(1) }
console.log('ALL OK')
