// The JavaScript quantize / dequantize wrappers (carta1_amd/js/coding/quantization.js) over every (sfi, bitsPerSample) record of
// tests/golden/export_domain.json + .bin, compared bit for bit (NaN for NaN) with what the reference's own functions returned,
// and the arguments they refuse.  Prints ALL OK on success; run by tests/test_js_export_domain.py.
import fs from 'fs'
import path from 'path'
import { fileURLToPath } from 'url'

import { quantize, dequantize } from '../carta1_amd/js/coding/quantization.js'

const G = path.join(path.dirname(fileURLToPath(import.meta.url)), 'golden')
const index = JSON.parse(fs.readFileSync(path.join(G, 'export_domain.json'), 'utf8'))
const raw = fs.readFileSync(path.join(G, 'export_domain.bin'))
const words = (T, off, n) => new T(raw.buffer.slice(raw.byteOffset + 4 * off, raw.byteOffset + 4 * (off + n)))

let failures = 0
const noise = words(Int32Array, index.dequantize_noise.words, index.dequantize_noise.n)
for (const v of index.quantize) {
  const m = Int32Array.from([...words(Int32Array, v.m, v.nm - noise.length), ...noise])
  const q = quantize(words(Float32Array, v.x, v.n), v.sfi, v.bits)
  const d = dequantize(m, v.sfi, v.bits)
  const wq = words(Int32Array, v.q, v.n), wd = words(Float32Array, v.d, v.nm)
  if (!(q instanceof Int32Array) || q.length !== wq.length || !wq.every((y, i) => y === q[i])) {
    failures++
    console.log(`quantize sfi ${v.sfi} bits ${v.bits}: differs from the reference`)
  }
  if (!(d instanceof Float32Array) || d.length !== wd.length || !wd.every((y, i) => Object.is(y, d[i]) || (Number.isNaN(y) && Number.isNaN(d[i])))) {
    failures++
    console.log(`dequantize sfi ${v.sfi} bits ${v.bits}: differs from the reference`)
  }
}
console.log(`${index.quantize.length} (sfi, bits) records, bits -2^31 .. 2^31 - 1`)

const rangeError = (f) => { try { f(); return false } catch (e) { return e instanceof RangeError } }
for (const [what, f] of [
  ['quantize sfi 64', () => quantize([1], 64, 8)],
  ['dequantize sfi -1', () => dequantize([1], -1, 8)],
  ['quantize sfi 2.5', () => quantize([1], 2.5, 8)],
  ['quantize bits 1.5', () => quantize([1], 5, 1.5)],
  ['dequantize bits 2^31', () => dequantize([1], 5, 2 ** 31)],
  ['dequantize bits NaN', () => dequantize([1], 5, NaN)],
]) {
  if (!rangeError(f)) { failures++; console.log(`${what}: not refused with a RangeError`) }
}
if (quantize([0.5], 40, -2147483648)[0] !== 2147483647 || quantize([0.5], 40, 32)[0] !== 2147483647) {
  failures++
  console.log('bits 32 / -2^31: every output should be ToInt32(-2147483649) = 2147483647')
}

console.log(failures ? `${failures} FAILED` : 'ALL OK')
process.exit(failures ? 1 : 0)
