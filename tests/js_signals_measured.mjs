// encodeAeaPcmMany(items, { measuredAllocation: true, scaleFactorOffsets, masking }) (carta1_amd/js/io/processor.js -> the addon's
// encodeSignalsMeasured -> c1_encode_signals_measured) against encodeAeaPcm(item, sameOptions) for every item alone, byte for
// byte, and against the images the Python host made of the same items.
// argv[2]: a directory with item<k>_<c>.f32 (raw float32, channel c of item k), counts.json (the channel count of every item) and,
// from the Python host, image_<tag>_<k>.aea for tag in measured, sf, masked, written by tests/test_js_signals_measured.py.
// Prints ALL OK on success.
import fs from 'fs'
import path from 'path'

import { encodeAeaPcm, encodeAeaPcmMany, SCALE_FACTOR_OFFSETS } from '../carta1_amd/js/index.js'

const dir = process.argv[2]
const f32 = (name) => { const b = fs.readFileSync(path.join(dir, name)); return new Float32Array(b.buffer.slice(b.byteOffset, b.byteOffset + b.length)) }
const bytes = (a) => Buffer.from(a.buffer, a.byteOffset, a.byteLength)

let failures = 0
function ok(cond, msg) { if (!cond) { failures++; console.log('FAIL', msg) } }
async function rejects(fn, type, needles, msg) {
  let err = null
  try { await fn() } catch (e) { err = e }
  ok(err instanceof type && needles.every((n) => String(err.message).includes(n)), `${msg}: expected ${type.name} naming ${needles}, got ${err}`)
}

async function main() {
  const counts = JSON.parse(fs.readFileSync(path.join(dir, 'counts.json'), 'utf8'))
  const items = counts.map((nch, k) => Array.from({ length: nch }, (_, c) => f32(`item${k}_${c}.f32`)))
  const kinds = [['measured', { measuredAllocation: true }],
    ['sf', { measuredAllocation: true, scaleFactorOffsets: SCALE_FACTOR_OFFSETS }],
    ['masked', { measuredAllocation: true, scaleFactorOffsets: SCALE_FACTOR_OFFSETS, masking: true }]]
  const plain = await encodeAeaPcmMany(items)
  for (const [tag, options] of kinds) {
    const many = await encodeAeaPcmMany(items, options)
    ok(Array.isArray(many) && many.length === items.length, `${tag}: one image per item`)
    let differs = false
    for (let k = 0; k < items.length; k++) {
      const one = await encodeAeaPcm(items[k], options)
      ok(bytes(many[k]).equals(bytes(one)), `${tag}: item ${k} == encodeAeaPcm(item, sameOptions)`)
      ok(bytes(many[k]).equals(fs.readFileSync(path.join(dir, `image_${tag}_${k}.aea`))), `${tag}: item ${k} == the Python host's image`)
      if (!bytes(many[k]).equals(bytes(plain[k]))) differs = true
    }
    ok(differs, `${tag}: the measured allocation took some unit`)
  }
  // masking without offsets: the single offset 0
  const alone = await encodeAeaPcmMany(items, { measuredAllocation: true, masking: true })
  for (let k = 0; k < items.length; k++) {
    ok(bytes(alone[k]).equals(bytes(await encodeAeaPcm(items[k], { measuredAllocation: true, masking: true }))), `masking alone: item ${k}`)
  }
  // without the option the bytes are today's, item by item and with the option false
  const off = await encodeAeaPcmMany(items, { measuredAllocation: false })
  for (let k = 0; k < items.length; k++) {
    ok(bytes(plain[k]).equals(bytes(await encodeAeaPcm(items[k]))), `plain: item ${k} == encodeAeaPcm(item)`)
    ok(bytes(off[k]).equals(bytes(plain[k])), `measuredAllocation: false is the plain call, item ${k}`)
  }
  // titles and encoder options still pass through
  const titled = await encodeAeaPcmMany(items, { measuredAllocation: true, title: items.map((_, k) => `item ${k}`), allocationBias: 2 })
  for (let k = 0; k < items.length; k++) {
    ok(bytes(titled[k]).equals(bytes(await encodeAeaPcm(items[k], { measuredAllocation: true, title: `item ${k}`, allocationBias: 2 }))), `titles and bias: item ${k}`)
  }

  await rejects(() => encodeAeaPcmMany(items, { measuredAllocation: 1 }), TypeError, ['measuredAllocation must be a boolean'], 'a number for the flag')
  await rejects(() => encodeAeaPcmMany(items, { scaleFactorOffsets: [0, 1] }), TypeError, ['scaleFactorOffsets needs measuredAllocation'], 'offsets alone')
  await rejects(() => encodeAeaPcmMany(items, { masking: true }), TypeError, ['masking needs measuredAllocation'], 'masking alone')
  await rejects(() => encodeAeaPcmMany(items, { measuredAllocation: true, scaleFactorOffsets: [1, 0] }), TypeError, ['scaleFactorOffsets[0] must be 0'], 'offsets not starting at 0')
  await rejects(() => encodeAeaPcmMany(items, { measuredAllocation: true, scaleFactorOffsets: [0, 9] }), TypeError, ['scaleFactorOffsets[1]'], 'an offset out of range')
  await rejects(() => encodeAeaPcmMany(items, { measuredAllocation: true, masking: { floor: [1, 2] } }), TypeError, ['masking.floor must hold 52 numbers'], 'a short floor')
  await rejects(() => encodeAeaPcmMany(items, { measuredAllocation: true, blockModes: new Uint8Array(4) }), TypeError, ['blockModes', 'not supported'], 'blockModes')
  await rejects(() => encodeAeaPcmMany(items, { measuredAllocation: true, measuredModeCandidates: [0, 0x3a] }), TypeError, ['measuredModeCandidates', 'not supported'], 'measuredModeCandidates')
  await rejects(() => encodeAeaPcmMany(items, { blockModeCandidates: [0, 0x3a] }), TypeError, ['blockModeCandidates', 'not supported'], 'blockModeCandidates')
  await rejects(() => encodeAeaPcmMany(items, { allocationBiasCandidates: [1, 2] }), TypeError, ['allocationBiasCandidates', 'not supported'], 'allocationBiasCandidates')

  console.log(failures === 0 ? 'ALL OK' : `${failures} FAILURES`)
  process.exit(failures === 0 ? 0 : 1)
}

main().catch((e) => { console.log('ERROR', e); process.exit(1) })
