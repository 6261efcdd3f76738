// allocateBits / findScaleFactor: the exports of the reference's codec/coding/bitallocation.js (:74-142, :290-299), same
// signatures and return types, computed on the device in the reference's arithmetic (c1_allocate_bits, c1_find_scale_factors).
// The encoder allocates inside its own kernels and never comes through here; these exist for code that imports the module,
// e.g. a custom quantization stage.  Inputs are typed arrays or plain Arrays, read as doubles; sizes are bfuSizes[i] | 0.
// Deviations (INTEGRATION.md section 2): maxBfuCount outside the integers 0 .. 52 is a RangeError, and a plain-Array size that
// is not an integer is read as size | 0 everywhere (the reference's distortion total reads it unrounded).
import { native, context } from '../native.js'
import { SCALE_FACTORS } from '../core/constants.js'

const FALLBACK_BFU_COUNT = 20 // BFU_AMOUNTS[0]
const NUM_BFUS = 52

// buildBiasedScaleFactorTable (:46-61) with this engine's Math.pow, as EncoderOptions.toNative builds it
const biasedTables = new Map()
export function biasedTable(bias) {
  if (!biasedTables.has(bias)) {
    biasedTables.set(bias, Float64Array.from(SCALE_FACTORS, (sf) => (bias === 1 ? sf : Math.pow(sf, bias))))
  }
  return biasedTables.get(bias)
}

// the first n values of an array-like as doubles: reads past its end are undefined (NaN), which findScaleFactor skips
function head(x, n) {
  const m = Math.min(n, x.length)
  return Float64Array.from(typeof x.subarray === 'function' ? x.subarray(0, m) : Array.prototype.slice.call(x, 0, m))
}

export function findScaleFactor(coefficients, length) {
  const n = Math.ceil(Number(length)) // the loop reads i = 0, 1, .. while i < length
  if (!(n > 0)) return 0
  const x = head(coefficients, n)
  return native().findScaleFactor(context(), x, x.length)
}

export function allocateBits(bfuData, bfuSizes, maxBfuCount, allocationBias) {
  if (!Number.isInteger(maxBfuCount) || maxBfuCount < 0 || maxBfuCount > NUM_BFUS) {
    throw new RangeError(`allocateBits: maxBfuCount ${maxBfuCount} outside 0 .. ${NUM_BFUS}`)
  }
  const sizes = new Int32Array(NUM_BFUS)
  const offsets = new Int32Array(NUM_BFUS)
  const lengths = new Int32Array(NUM_BFUS)
  const parts = []
  let total = 0
  for (let i = 0; i < maxBfuCount; i++) {
    const sz = bfuSizes[i] | 0
    sizes[i] = sz
    if (sz <= 0) continue // a size of 0 is skipped (:80), a negative one reads nothing
    const x = head(bfuData[i], sz) // TypeError for a missing BFU, as findScaleFactor(undefined, sz) throws
    offsets[i] = total
    lengths[i] = x.length
    parts.push(x)
    total += x.length
  }
  const data = new Float64Array(total)
  for (let i = 0, k = 0; i < maxBfuCount; i++) if (sizes[i] > 0) data.set(parts[k++], offsets[i])
  const [bfuCount, allocation, scaleFactorIndices, fallback] = native().allocateBits(
    context(), data, offsets, lengths, sizes, maxBfuCount, biasedTable(allocationBias))
  if (fallback) {
    return { bfuCount: FALLBACK_BFU_COUNT, allocation: new Int32Array(FALLBACK_BFU_COUNT), scaleFactorIndices: new Int32Array(NUM_BFUS) }
  }
  return { bfuCount, allocation: allocation.slice(0, bfuCount), scaleFactorIndices: scaleFactorIndices.slice(0, maxBfuCount) }
}
