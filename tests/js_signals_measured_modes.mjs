// encodeSignalsMeasuredModes(pcm, frameOffsets, nativeOptions, candidates, scaleFactorOffsets) (carta1_amd/js/native.js -> the
// addon's encodeSignalsMeasuredModes -> c1_encode_signals_measured_modes): every channel of every item one signal of ONE call,
// against encodeAeaPcm(item, { measuredAllocation: true, measuredModeCandidates, ... }) for every item alone, byte for byte, and
// against the images the Python host made of the same items.
// argv[2]: a directory with item<k>_<c>.f32 (raw float32, channel c of item k), counts.json (the channel count of every item) and,
// from the Python host, image_<tag>_<k>.aea for tag in sf, plain, written by tests/test_js_signals_measured_modes.py.
// Prints ALL OK on success.
import fs from 'fs'
import path from 'path'

import { encodeAeaPcm, encodeAeaPcmMany, encodeSignalsMeasured, encodeSignalsMeasuredModes, EncoderOptions, SCALE_FACTOR_OFFSETS } from '../carta1_amd/js/index.js'

const dir = process.argv[2]
const f32 = (name) => { const b = fs.readFileSync(path.join(dir, name)); return new Float32Array(b.buffer.slice(b.byteOffset, b.byteOffset + b.length)) }
const bytes = (a) => Buffer.from(a.buffer, a.byteOffset, a.byteLength)
const CANDIDATES = [0, 10, 58]
const HEADER = 2048, UNIT = 212

let failures = 0
function ok(cond, msg) { if (!cond) { failures++; console.log('FAIL', msg) } }
async function rejects(fn, type, needles, msg) {
  let err = null
  try { await fn() } catch (e) { err = e }
  ok(err instanceof type && needles.every((n) => String(err.message).includes(n)), `${msg}: expected ${type.name} naming ${needles}, got ${err}`)
}

// items -> the concatenated whole frames of every channel (both channels of an item padded to the longer one), the frame
// offsets of the signals and the frame count of every item
function layout(items) {
  const frames = items.map((chs) => Math.ceil(Math.max(...chs.map((c) => c.length)) / 512))
  const count = items.reduce((n, chs) => n + chs.length, 0)
  const frameOffsets = new Float64Array(count + 1)
  let s = 0
  items.forEach((chs, k) => chs.forEach(() => { frameOffsets[s + 1] = frameOffsets[s] + frames[k]; s++ }))
  const pcm = new Float32Array(frameOffsets[count] * 512)
  s = 0
  items.forEach((chs) => chs.forEach((c) => { pcm.set(c, frameOffsets[s] * 512); s++ }))
  return { pcm, frameOffsets, frames }
}

// the units of the signals -> per item its body, channels interleaved frame by frame
function bodies(units, items, frameOffsets, frames) {
  let s = 0
  return items.map((chs, k) => {
    const body = new Uint8Array(frames[k] * chs.length * UNIT)
    chs.forEach((_, c) => {
      for (let f = 0; f < frames[k]; f++) {
        body.set(units.subarray((frameOffsets[s] + f) * UNIT, (frameOffsets[s] + f + 1) * UNIT), (f * chs.length + c) * UNIT)
      }
      s++
    })
    return body
  })
}

async function main() {
  const counts = JSON.parse(fs.readFileSync(path.join(dir, 'counts.json'), 'utf8'))
  const items = counts.map((nch, k) => Array.from({ length: nch }, (_, c) => f32(`item${k}_${c}.f32`)))
  ok(Array.from(SCALE_FACTOR_OFFSETS).join() === '0,-1,1,-2,-3', 'the five offsets')
  const { pcm, frameOffsets, frames } = layout(items)
  const opts = (values = {}) => new EncoderOptions(values).toNative()
  const on = { measuredAllocation: true, measuredModeCandidates: CANDIDATES }
  const kinds = [['sf', { ...on, scaleFactorOffsets: SCALE_FACTOR_OFFSETS }, SCALE_FACTOR_OFFSETS], ['plain', on, null]]
  for (const [tag, options, offsets] of kinds) {
    const units = encodeSignalsMeasuredModes(pcm, frameOffsets, opts(), CANDIDATES, offsets)
    ok(units instanceof Uint8Array && units.length === frameOffsets[frameOffsets.length - 1] * UNIT, `${tag}: one unit per frame of the concatenation`)
    const many = bodies(units, items, frameOffsets, frames)
    const measured = bodies(encodeSignalsMeasured(pcm, frameOffsets, opts(), offsets, null), items, frameOffsets, frames)
    let differs = false
    for (let k = 0; k < items.length; k++) {
      const one = await encodeAeaPcm(items[k], options)
      ok(one.length === HEADER + many[k].length && bytes(many[k]).equals(bytes(one.subarray(HEADER))), `${tag}: item ${k} == encodeAeaPcm(item, sameOptions)`)
      const image = fs.readFileSync(path.join(dir, `image_${tag}_${k}.aea`))
      ok(bytes(one).equals(image), `${tag}: item ${k}: encodeAeaPcm's image == the Python host's image`)
      ok(bytes(many[k]).equals(image.subarray(HEADER)), `${tag}: item ${k} == the Python host's units`)
      if (!bytes(many[k]).equals(bytes(measured[k]))) differs = true
    }
    ok(differs, `${tag}: the search chose some unit's modes`)
  }
  // a Uint8Array and triples are the same candidates; the encoder's options pass through
  const first = encodeSignalsMeasuredModes(pcm, frameOffsets, opts(), CANDIDATES, SCALE_FACTOR_OFFSETS)
  ok(bytes(encodeSignalsMeasuredModes(pcm, frameOffsets, opts(), Uint8Array.from(CANDIDATES), SCALE_FACTOR_OFFSETS)).equals(bytes(first)), 'a Uint8Array of candidates')
  ok(bytes(encodeSignalsMeasuredModes(pcm, frameOffsets, opts(), [[0, 0, 0], [2, 2, 0], [2, 2, 3]], SCALE_FACTOR_OFFSETS)).equals(bytes(first)), 'triples')
  const biased = bodies(encodeSignalsMeasuredModes(pcm, frameOffsets, opts({ allocationBias: 2 }), CANDIDATES, null), items, frameOffsets, frames)
  for (let k = 0; k < items.length; k++) {
    ok(bytes(biased[k]).equals(bytes((await encodeAeaPcm(items[k], { ...on, allocationBias: 2 })).subarray(HEADER))), `allocationBias 2: item ${k}`)
  }
  // neither the threshold nor the fixed modes are read
  ok(bytes(encodeSignalsMeasuredModes(pcm, frameOffsets, opts({ fixedBlockModes: [2, 2, 3] }), CANDIDATES, SCALE_FACTOR_OFFSETS)).equals(bytes(first)),
    'block-mode options do not matter')

  // the errors: the candidates and offsets as encodeMeasuredModes judges them, the layout as encodeSignalsMeasured does
  const call = (cand, offsets = null, p = pcm, off = frameOffsets) => async () => encodeSignalsMeasuredModes(p, off, opts(), cand, offsets)
  await rejects(call([]), RangeError, ['1 to 8'], 'no candidate')
  await rejects(call([0, 2, 8, 10, 48, 50, 56, 58, 0]), RangeError, ['1 to 8'], 'nine candidates')
  await rejects(call([0, 58, 0]), Error, ['candidate 2'], 'a candidate given twice')
  await rejects(call([0, 1]), Error, ['candidate 1', 'low field'], 'a candidate outside the domain')
  await rejects(call([[2, 2]]), TypeError, ['triple'], 'a short triple')
  await rejects(call([0.5]), TypeError, ['mode bytes'], 'a fraction')
  await rejects(call(CANDIDATES, [1, 0]), TypeError, ['scaleFactorOffsets[0] must be 0'], 'offsets not starting at 0')
  await rejects(call(CANDIDATES, [0, 9]), TypeError, ['scaleFactorOffsets[1]'], 'an offset out of range')
  await rejects(call(CANDIDATES, null, pcm.subarray(512)), TypeError, ['frameOffsets[n] frames'], 'pcm shorter than the offsets say')
  // encodeAeaPcm's TypeErrors for the option, and encodeAeaPcmMany as it was: the option stays unsupported there
  const sched = new Uint8Array(4)
  await rejects(() => encodeAeaPcm(items[0], { measuredModeCandidates: CANDIDATES }), TypeError, ['measuredModeCandidates', 'measuredAllocation: true'], 'without measuredAllocation')
  await rejects(() => encodeAeaPcm(items[0], { ...on, masking: true }), TypeError, ['measuredModeCandidates', 'masking', 'mutually exclusive'], 'masking too')
  await rejects(() => encodeAeaPcm(items[0], { ...on, blockModes: sched }), TypeError, ['measuredModeCandidates', 'blockModes', 'mutually exclusive'], 'blockModes too')
  await rejects(() => encodeAeaPcm(items[0], { ...on, blockModeCandidates: [0, 58] }), TypeError, ['measuredModeCandidates', 'blockModeCandidates', 'mutually exclusive'], 'blockModeCandidates too')
  // without the call the bytes are today's
  const today = await encodeAeaPcmMany(items)
  for (let k = 0; k < items.length; k++) ok(bytes(today[k]).equals(bytes(await encodeAeaPcm(items[k]))), `plain: item ${k} == encodeAeaPcm(item)`)

  console.log(failures === 0 ? 'ALL OK' : `${failures} FAILURES`)
  process.exit(failures === 0 ? 0 : 1)
}

main().catch((e) => { console.log('ERROR', e); process.exit(1) })
