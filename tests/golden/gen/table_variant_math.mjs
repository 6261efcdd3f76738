// Math.sin / cos / pow wrappers of the table variants (gen_table_variants.mjs; tests/js_table_variants.mjs installs the same
// ones before the library's JavaScript host loads).  install(variant) replaces the three functions for good.
const F64 = new Float64Array(1), U32 = new Uint32Array(F64.buffer), I64 = new BigInt64Array(F64.buffer)
function hash32(a) {
  let x = a >>> 0
  x ^= x << 13; x >>>= 0; x ^= x >>> 17; x ^= x << 5; x >>>= 0
  x = Math.imul(x, 0x2C1B3C6D) >>> 0
  x ^= x << 13; x >>>= 0; x ^= x >>> 17; x ^= x << 5; x >>>= 0
  return x
}
function hashArg(x, salt) { F64[0] = x; return hash32(U32[0] ^ hash32((U32[1] ^ salt) >>> 0)) }
function ulps(x, k) { if (k === 0 || x === 0 || !Number.isFinite(x)) return x; F64[0] = x; I64[0] += BigInt(k); return F64[0] }
const F32 = new Float32Array(1)
export function floorF32(x) { F32[0] = x; let f = F32[0]; if (f > x) { F32[0] = f; const u = new Uint32Array(F32.buffer); u[0] -= 1; f = F32[0] } return f }
export function ceilF32(x) { F32[0] = x; let f = F32[0]; if (f < x) { F32[0] = f; const u = new Uint32Array(F32.buffer); u[0] += 1; f = F32[0] } return f }

export function install(variant) {
  const sin = Math.sin, cos = Math.cos, pow = Math.pow
  const trig = (fn, salt) => (x) => {
    const r = fn(x), h = hashArg(x, salt)
    if (variant === 'ulp') return ulps(r, (h % 3) - 1)
    if (variant === 'inside') return x < 0 ? ulps(r, (h % 5) - 2) : r * (1 + (((h % 2001) - 1000) / 1000) * 1e-10)
    if (variant === 'twiddle') return x < 0 ? r * (1 + ((h & 1) ? 1e-9 : -1e-9)) : r
    return r
  }
  Math.sin = trig(sin, 0x51)
  Math.cos = trig(cos, 0xC0)
  Math.pow = (b, e) => {
    const r = pow(b, e)
    const integer = Number.isInteger(e)
    if (variant === 'ulp') return integer ? r : ulps(r, (hashArg(e, 0x90 ^ hashArg(b, 7)) % 3) - 1)
    if (b !== 2 || integer) {
      if (variant === 'sfpow2' && b === 2 && e >= -21 && e <= -17) return ulps(r, -1)
      return r
    }
    const i = Math.round((e + 21) * 3)
    if (variant === 'inside') {                                 // strictly between the binary32 neighbours of r
      const lo = floorF32(r), hi = ceilF32(r)
      if (lo === hi) return r
      const t = 0.05 + 0.9 * (hashArg(e, 0x17) / 4294967296)
      const v = lo + (hi - lo) * t
      return v > lo && v < hi ? v : r
    }
    if (variant === 'sfshift' && i % 3 === 1) return r * (1 + 9.5367431640625e-7)          // 2^-20: 8 binary32 ulps up
    return r
  }
}

