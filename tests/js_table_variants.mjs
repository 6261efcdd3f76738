// The library's JavaScript host under another engine's Math (tests/golden/table_variants.json): with Math.sin / cos / pow
// wrapped as gen_table_variants.mjs wraps them, installed BEFORE carta1_amd/js loads,
//   node tests/js_table_variants.mjs <variant>       buildNativeTables() equals the tables the reference built (no device)
//   node tests/js_table_variants.mjs <variant> gpu   encode() / decode() reproduce the reference's units and decoded frames
// Prints ALL OK on success; run by tests/test_js_table_variants.py.
import fs from 'fs'
import path from 'path'
import crypto from 'crypto'
import { fileURLToPath } from 'url'

import { install } from './golden/gen/table_variant_math.mjs'

const G = path.join(path.dirname(fileURLToPath(import.meta.url)), 'golden')
const [variant, where] = process.argv.slice(2)
install(variant)
const v = JSON.parse(fs.readFileSync(path.join(G, 'table_variants.json'), 'utf8')).variants[variant]
const raw = fs.readFileSync(path.join(G, `table_variants_${variant}.bin`))
const part = (key) => raw.subarray(v.offsets[key][0], v.offsets[key][0] + v.offsets[key][1])
const f64hex = (x) => { const b = Buffer.alloc(8); b.writeDoubleBE(x); return b.toString('hex') }
let failures = 0
const fail = (msg) => { failures++; console.log('FAIL ' + msg) }

function xorshift(seed) {
  let s = seed >>> 0
  return () => { s ^= s << 13; s >>>= 0; s ^= s >>> 17; s ^= s << 5; s >>>= 0; return (s / 4294967296) * 2 - 1 }
}
function white(seed, n) {
  const r = xorshift(seed); const x = new Float32Array(n)
  for (let i = 0; i < n; i++) x[i] = Math.fround(r() * 0.5)
  return x
}
function pinkT(seed, n) {
  const r = xorshift(seed); const x = new Float32Array(n); let p = 0
  for (let i = 0; i < n; i++) {
    const u = r(); p = 0.98 * p + 0.05 * u; let s = p
    if ((i >> 9) % 8 === 5 && (i % 512) >= 256) s += 0.8 * r()
    x[i] = s
  }
  return x
}

async function main() {
  const { buildNativeTables } = await import('../carta1_amd/js/core/constants.js')
  const got = Array.from(buildNativeTables()).map(f64hex)
  const bad = got.map((h, i) => (h === v.tables_f64[i] ? -1 : i)).filter((i) => i >= 0)
  if (got.length !== v.tables_f64.length || bad.length) fail(`${variant}: buildNativeTables differs at ${bad.length} entries, first ${bad[0]}`)
  else console.log(`${variant}: buildNativeTables == the reference's tables (${got.length} doubles)`)
  if (where === 'gpu') {
    const c1 = await import('../carta1_amd/js/index.js')
    for (const [name, k] of Object.entries(v.kat)) {
      const n = k.frames * 512
      const chs = k.signal === 'white' ? [white(1, n), white(2, n)] : [pinkT(3, n), pinkT(4, n)]
      const encs = chs.map(() => c1.encode(new c1.EncoderOptions(k.options)))
      const decs = chs.map(() => c1.decode())
      const units = part(`kat_${name}_units`), dig = part(`kat_${name}_pcm8`)
      let badU = 0, badP = 0
      for (let f = 0; f < k.frames; f++)
        for (let c = 0; c < 2; c++) {
          const at = f * 2 + c
          const u = c1.serializeFrame(encs[c](chs[c].slice(f * 512, (f + 1) * 512)))
          if (Buffer.compare(Buffer.from(u), units.subarray(at * 212, (at + 1) * 212)) !== 0) badU++
          const pcm = decs[c](c1.deserializeFrame(units.subarray(at * 212, (at + 1) * 212)))
          const h = crypto.createHash('sha256').update(Buffer.from(pcm.buffer, pcm.byteOffset, pcm.byteLength)).digest().subarray(0, 8)
          if (Buffer.compare(h, dig.subarray(at * 8, (at + 1) * 8)) !== 0) badP++
        }
      if (badU || badP) fail(`${variant} ${name}: ${badU} units and ${badP} decoded frames differ`)
      else console.log(`${variant} ${name}: ${k.frames * 2} units and decoded frames equal the reference's`)
    }
  }
  console.log(failures ? `${failures} FAILURES` : 'ALL OK')
  process.exit(failures ? 1 : 0)
}
main().catch((e) => { console.error(e); process.exit(1) })
