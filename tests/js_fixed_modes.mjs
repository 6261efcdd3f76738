// The JavaScript encode() frame closures and encodeAeaPcm under fixedBlockModes triples outside the canonical header values
// ([1,1,1], [1,0,2], [2,2,1], [0,1,0]: tests/golden/fixed_modes.json, written by the reference under all 36 triples), and the
// way back through decode() closures and decodeAeaPcm: units and PCM must be the reference's bit for bit.  The inputs are
// the fixture's, written as raw Float32 files case<id>_c<channel>.f32 into the directory given as the only argument by
// tests/test_js_fixed_modes.py (tests/option_domain_lib.py rebuilds them; their SHA-256 is checked here).  Prints ALL OK
// on success.
import fs from 'fs'
import path from 'path'
import crypto from 'crypto'
import { fileURLToPath } from 'url'

import { EncoderOptions } from '../carta1_amd/js/core/options.js'
import { BufferPool } from '../carta1_amd/js/core/buffers.js'
import { serializeFrame, deserializeFrame } from '../carta1_amd/js/io/serialization.js'
import { encodeAeaPcm, decodeAeaPcm } from '../carta1_amd/js/io/processor.js'
import { encode } from '../carta1_amd/js/pipeline/encoder.js'
import { decode } from '../carta1_amd/js/pipeline/decoder.js'

const G = path.join(path.dirname(fileURLToPath(import.meta.url)), 'golden')
const fixture = JSON.parse(fs.readFileSync(path.join(G, 'fixed_modes.json'), 'utf8'))
const DIR = process.argv[2]
const TRIPLES = ['1,1,1', '1,0,2', '2,2,1', '0,1,0']
const sha = (buf) => crypto.createHash('sha256').update(buf).digest('hex')
const bytesOf = (ta) => Buffer.from(ta.buffer, ta.byteOffset, ta.byteLength)

let failures = 0
function fail(msg) { failures++; console.log('FAIL', msg) }

// planar channels -> the fixture's order: per frame L then R
function interleaveFrames(chs, frames) {
  const out = new Float32Array(frames * chs.length * 512)
  for (let f = 0; f < frames; f++)
    for (let c = 0; c < chs.length; c++) out.set(chs[c].subarray(f * 512, (f + 1) * 512), (f * chs.length + c) * 512)
  return out
}

async function main() {
  let cases = 0
  for (const c of fixture.cases) {
    const modes = c.options.fixedBlockModes
    if (!TRIPLES.includes(modes.join(','))) continue
    const what = `[${modes}] ${c.frames} frames x ${c.channels}`
    const nch = c.channels, frames = c.frames
    const chs = []
    for (let ch = 0; ch < nch; ch++) {
      const raw = fs.readFileSync(path.join(DIR, `case${c.id}_c${ch}.f32`))
      const x = new Float32Array(raw.buffer.slice(raw.byteOffset, raw.byteOffset + raw.byteLength))
      if (x.length !== frames * 512 || sha(bytesOf(x)) !== c.input_sha256[ch]) fail(`${what}: input of channel ${ch} is not the fixture's`)
      chs.push(x)
    }

    // encode() closures, one per channel, and decode() closures back
    {
      const options = new EncoderOptions({ fixedBlockModes: modes.slice(), allocationBias: 1 })
      const encs = chs.map(() => encode(options, new BufferPool()))
      const decs = chs.map(() => decode(new BufferPool()))
      const units = []
      const pcm = new Float32Array(frames * nch * 512)
      for (let f = 0; f < frames; f++) {
        for (let ch = 0; ch < nch; ch++) {
          const fields = encs[ch](chs[ch].slice(f * 512, (f + 1) * 512))
          if (fields.blockModes.join(',') !== modes.join(',')) fail(`${what} encode(): frame ${f} has block modes ${fields.blockModes}`)
          const unit = serializeFrame(fields)
          units.push(Buffer.from(unit))
          pcm.set(decs[ch](deserializeFrame(unit)), (f * nch + ch) * 512)
        }
      }
      const all = Buffer.concat(units)
      if (all.subarray(0, 2).toString('hex') !== c.header) fail(`${what} encode(): header ${all.subarray(0, 2).toString('hex')}, expected ${c.header}`)
      if (sha(all) !== c.units_sha256) fail(`${what} encode(): units differ from the reference's`)
      if (sha(bytesOf(pcm)) !== c.pcm_sha256) fail(`${what} decode(): PCM differs from the reference's`)
    }

    // encodeAeaPcm and decodeAeaPcm
    {
      const image = await encodeAeaPcm(chs, { fixedBlockModes: modes.slice(), allocationBias: 1 })
      const body = Buffer.from(image.buffer, image.byteOffset + 2048, image.byteLength - 2048)
      if (body.length !== frames * nch * 212) fail(`${what} encodeAeaPcm: ${body.length} bytes of units`)
      if (sha(body) !== c.units_sha256) fail(`${what} encodeAeaPcm: units differ from the reference's`)
      const back = await decodeAeaPcm(image)
      if (back.length !== nch || sha(bytesOf(interleaveFrames(back, frames))) !== c.pcm_sha256) fail(`${what} decodeAeaPcm: PCM differs from the reference's`)
    }
    cases++
  }
  if (cases !== 8) fail(`expected 8 cases (four triples, stereo and mono), ran ${cases}`)
  if (failures) { console.log(`${failures} FAILURES`); process.exit(1) }
  console.log('ALL OK')
}

main().catch((e) => { console.log('ERROR', e && e.stack ? e.stack : e); process.exit(1) })
