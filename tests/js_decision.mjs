// performFFT / detectTransient (carta1_amd/js/analysis/transient.js) and findScaleFactor / allocateBits
// (carta1_amd/js/coding/bitallocation.js) against what the reference's own functions returned (tests/golden/decision.json,
// decision.bin): the same values, return types and lengths, from typed arrays and from plain Arrays, and the RangeErrors of
// the documented deviations.  Prints ALL OK on success; run by tests/test_js_decision.py.
import fs from 'fs'
import path from 'path'
import { fileURLToPath } from 'url'

import { performFFT, detectTransient } from '../carta1_amd/js/analysis/transient.js'
import { allocateBits, findScaleFactor } from '../carta1_amd/js/coding/bitallocation.js'

const G = path.join(path.dirname(fileURLToPath(import.meta.url)), 'golden')
const index = JSON.parse(fs.readFileSync(path.join(G, 'decision.json'), 'utf8'))
const raw = fs.readFileSync(path.join(G, 'decision.bin'))
const words = new Float64Array(raw.buffer.slice(raw.byteOffset, raw.byteOffset + raw.byteLength))
const span = (r) => words.slice(r[0], r[0] + r[1])
const same = (a, b) => a.length === b.length && Array.from(a).every((v, i) => Object.is(v, b[i]))
let failures = 0
function check(ok, what) {
  if (!ok) {
    failures++
    if (failures < 20) console.log('FAIL', what)
  }
}

for (const [k, r] of index.fft.entries()) {
  const x = span(r.x)
  const y = performFFT(k % 2 ? Array.from(x) : x, r.n)
  check(y instanceof Float32Array && same(y, span(r.y)), `performFFT ${r.name} ${r.n}`)
}
for (const [k, r] of index.detect.entries()) {
  const c = span(r.c), p = r.p === null ? null : span(r.p)
  const got = detectTransient(k % 3 === 1 ? Array.from(c) : c, p && k % 3 === 2 ? Array.from(p) : p, words[r.t])
  check(got === r.r, `detectTransient ${r.name} #${k}`)
}
check(detectTransient(new Float32Array(4), undefined, -1) === false, 'detectTransient(undefined prev)')
check(detectTransient(new Float32Array(4), 0, -1) === false, 'detectTransient(0 prev)')
for (const [k, r] of index.sf.entries()) {
  const x = span(r.x)
  const got = findScaleFactor(k % 2 ? Array.from(x) : x, r.len)
  check(typeof got === 'number' && got === r.r, `findScaleFactor ${r.name} #${k}`)
}
for (const [k, r] of index.alloc.entries()) {
  const bfus = r.data.map((d) => span(d))
  const sizes = k % 2 ? Int32Array.from(r.sizes) : r.sizes.slice()
  const got = allocateBits(k % 3 ? bfus : bfus.map((b) => Array.from(b)), sizes, r.mb, r.bias)
  check(got.bfuCount === r.count && got.allocation instanceof Int32Array && same(got.allocation, r.wl) &&
    got.scaleFactorIndices instanceof Int32Array && same(got.scaleFactorIndices, r.sfi), `allocateBits ${r.name} #${k}`)
}

function throwsRange(f, what) {
  try {
    f()
    check(false, what + ' did not throw')
  } catch (e) {
    check(e instanceof RangeError, what + ' threw ' + e)
  }
}
throwsRange(() => performFFT(new Float32Array(8), 6), 'performFFT(6)')
throwsRange(() => performFFT(new Float32Array(8), 0), 'performFFT(0)')
throwsRange(() => performFFT(new Float32Array(8), 1 << 23), 'performFFT(2^23)')
throwsRange(() => allocateBits([], [], 53, 1), 'allocateBits(maxBfuCount 53)')
throwsRange(() => allocateBits([], [], 2.5, 1), 'allocateBits(maxBfuCount 2.5)')
check(performFFT(new Float32Array(3), 1).length === 0, 'performFFT(x, 1) is empty')

console.log(failures ? `FAILED ${failures}` : 'ALL OK')
