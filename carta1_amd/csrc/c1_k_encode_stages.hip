// c1_k_encode_stages.hip -- the encoder's middle and last pipeline stages on their own (codec/pipeline/encoder.js exports them
// next to encode()): blockSelectorStage's detection branch (encoder.js:111-152) from stored bands, quantizationStage
// (:365-418) from stored coefficients, and serializeFrame (io/serialization.js:41-98) from frame fields, batched over
// consecutive frames of one channel in the reference's number model.  The transient FFT, the feature sums and the decision
// are the exact detector's own device code (c1_detect_core.h); the bit allocation is the encoder's k_alloc_* chain
// (c1_k_allocate.hip, launched by the host); quantize is k_quantize_one's (quantize_into, c1_device.h).  The hot path never
// calls these kernels: c1_encode_* runs its own fused analysis and packs in k_pack.
#include "c1_detect_core.h"

namespace {

// ---- blockSelectorStage -----------------------------------------------------------------------------------------------
// The history the reference keeps (bufferPool.transientDetection, encoder.js:142) is performFFT's magnitudes of the last
// frame detection ran on: a function of that frame's bands.  So every row -- the halo included -- gets its magnitudes
// first, and then every frame decides against the row before it, independently.

// performFFT (transient.js:17-35) of every row of bands: one wave per row, mags = 256 floats per row (64 | 64 | 128)
struct alignas(16) StageMagsLds {
  alignas(16) float band[512];
  alignas(16) float2 z[576];               // transient FFT points, 1 pad slot per 8 (tslot)
};
__global__ __launch_bounds__(C1_WAVE) void k_stage_mags(const C1DevTables *tables, const float *__restrict__ bands, int64_t rows,
                                                       float *__restrict__ mags) {
  __shared__ StageMagsLds S;
  const int lane = threadIdx.x;
  const int64_t r = blockIdx.x;
  if (r >= rows) return;
  const TGeom G = tfft_geometry(lane);
  const TablesRsrc RT = tables_rsrc(tables);
  TablesPtr T = C1_TABLES(tables);
  const float4 *src = reinterpret_cast<const float4 *>(bands + r * 512);
  reinterpret_cast<float4 *>(S.band)[lane] = src[lane];
  reinterpret_cast<float4 *>(S.band)[64 + lane] = src[64 + lane];
  wave_fence();
  float mg[4];
  tfft_exact(S.band, S.z, G, T, RT, mg);
#pragma unroll
  for (int i = 0; i < 4; i++) mags[r * 256 + G.mag + i * G.S] = mg[i];
}

// detectTransient (transient.js:63-226) of the three bands of every frame against the previous row's magnitudes (or a fresh
// pool's zeros when the frame has none), the LOW threshold for all three (encoder.js:137-141); one wave per frame.  mags
// points at row -halo.  modes: 3 int32 per frame, 0 or max(band + 1, 2) (:143).
struct alignas(16) StageDecideLds {
  alignas(16) double term[4][256];
  alignas(16) double feat_c[kFeatureWsDoubles];
  alignas(16) double feat_p[kFeatureWsDoubles];
};
__global__ __launch_bounds__(C1_WAVE) void k_stage_decide(const C1DevTables *tables, const float *__restrict__ mags, int64_t frames,
                                                         int halo, double threshold, int32_t *__restrict__ modes) {
  __shared__ StageDecideLds S;
  const int lane = threadIdx.x;
  const int64_t f = blockIdx.x;
  if (f >= frames) return;
  const TGeom G = tfft_geometry(lane);
  const bool have_prev = f - 1 >= -(int64_t)halo;
  const float *cur = mags + (f + halo) * 256;
  float mg[4], pmag[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  if (have_prev) {
    const float *prev = cur - 256;
#pragma unroll
    for (int i = 0; i < 4; i++) pmag[i] = prev[G.mag + i * G.S];
    const float zero[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    exact_sums(S.term, G, lane, pmag, zero, S.feat_p);        // its flux sum is not used
    wave_fence();
  }
#pragma unroll
  for (int i = 0; i < 4; i++) mg[i] = cur[G.mag + i * G.S];
  exact_sums(S.term, G, lane, mg, pmag, S.feat_c);
  wave_fence();
  if (lane < 3) modes[3 * f + lane] = detect_band_mode<true>(S.feat_c, have_prev ? S.feat_p : nullptr, lane, C1_TABLES(tables)->log1p10, threshold, nullptr);
}

// ---- quantizationStage ------------------------------------------------------------------------------------------------
// groupIntoBFUs (quantization.js:106-149; a band is long only when its mode is exactly 0) + findScaleFactor
// (bitallocation.js:290-299) per BFU -> the 64-byte side records the k_alloc_* chain reads (sfi[52], then zeros).  The
// maximum is the reference's `a > maxAmplitude` scan on the magnitudes' bit patterns, which order like the values for
// everything but NaN: NaN (any payload, signalling or quiet) is skipped, +Inf gives 63, -0 and denormals give 0.  One wave
// per frame, lane b < 52 scans BFU b.
__global__ __launch_bounds__(C1_WAVE) void k_stage_scale_factors(const C1DevTables *tables, const float *__restrict__ coefs,
                                                                const int32_t *__restrict__ modes, int64_t frames, uint8_t *__restrict__ side) {
  const int lane = threadIdx.x;
  const int64_t f = blockIdx.x;
  if (f >= frames) return;
  TablesPtr T = C1_TABLES(tables);
  int sfi = 0;
  if (lane < 52) {
    const bool lng = modes[3 * f + band_of_bfu(lane)] == 0;
    const uint32_t *x = reinterpret_cast<const uint32_t *>(coefs + f * 512 + (lng ? kStartLong[lane] : kStartShort[lane]));
    const int n = kSpecs[lane];
    uint32_t mx = 0u;
    for (int j = 0; j < n; j++) {
      const uint32_t a = x[j] & 0x7fffffffu;                  // Math.abs
      if (a <= 0x7f800000u && a > mx) mx = a;                 // not NaN, and a > maxAmplitude
    }
    const float m = __uint_as_float(mx);
    sfi = scale_factor_index_fast(m, T->sf_m1, T->sf_m2);
  }
  side[f * kSideBytes + lane] = (uint8_t)sfi;                 // lanes 52..63: the rest of the record, zeros
}

// The frame fields (include/carta1_hip.h, as c1_unpack_units writes them) from the allocation record and the side record:
// nBfu (BFU_AMOUNTS[amount index], 20 for the fallback of bitallocation.js:132-139), wl and sfi below nBfu (sfi as
// findScaleFactor gave it, zeros for the fallback), and quantize (quantization.js:34-56) of every coefficient of those BFUs;
// zeros elsewhere.  One wave per frame, eight consecutive slots per lane.
__global__ __launch_bounds__(C1_WAVE) void k_stage_fields(const C1DevTables *tables, const float *__restrict__ coefs,
                                                         const int32_t *__restrict__ modes, const uint8_t *__restrict__ side,
                                                         const uint8_t *__restrict__ alloc, int64_t frames, int32_t *__restrict__ nbfu,
                                                         int32_t *__restrict__ sfi_out, int32_t *__restrict__ wl_out,
                                                         int32_t *__restrict__ q_out) {
  __shared__ int32_t wl_s[52], sf_s[52];
  const int lane = threadIdx.x;
  const int64_t f = blockIdx.x;
  if (f >= frames) return;
  const uint32_t *al = reinterpret_cast<const uint32_t *>(alloc + f * kAllocBytes);
  const uint32_t a7 = al[7];
  const bool fallback = (a7 >> 27) & 1;
  const int n = bfu_amount((int)(a7 >> 28) & 7);
  if (lane < 52) {
    const int wl = lane < n ? (int)((al[lane >> 3] >> ((lane & 7) * 4)) & 15) : 0;
    const int sf = lane < n && !fallback ? (int)side[f * kSideBytes + lane] : 0;
    wl_s[lane] = wl;
    sf_s[lane] = sf;
    wl_out[f * 52 + lane] = wl;
    sfi_out[f * 52 + lane] = sf;
  }
  if (lane == 0) nbfu[f] = n;
  wave_fence();
  const int m0 = modes[3 * f], m1 = modes[3 * f + 1], m2 = modes[3 * f + 2];
#pragma unroll
  for (int m = 0; m < 8; m++) {
    const int slot = 8 * lane + m, b = bfu_of_slot(slot), j = slot - (int)kBfuFirst[b];
    const int band = band_of_bfu(b), mode = band == 0 ? m0 : (band == 1 ? m1 : m2);
    const int at = (mode == 0 ? (int)kStartLong[b] : (int)kStartShort[b]) + j;
    quantize_into(tables, coefs + f * 512 + at, sf_s[b], wl_bits(wl_s[b]), q_out + f * 512 + slot);
  }
}

// ---- block modes -> the MDCT's inputs ----------------------------------------------------------------------------------
// k_mdct_bands reads a mode byte per unit (2 bits per band: 2, 2, 3 for a short band, as c1_mdct_batch packs them) and two
// frame lists, long units (every band mode 0) and the others, with their counts in lists[0] and lists[1].  The stream's
// option-switch frame has its modes on the device only (k_stage_decide): one lane walks its few frames in order.
__global__ void k_stage_mode_lists(const int32_t *__restrict__ modes, int64_t frames, uint8_t *__restrict__ mode_bytes,
                                   uint32_t *__restrict__ lists) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  uint32_t n_long = 0u, n_short = 0u;
  for (int64_t f = 0; f < frames; f++) {
    const int m0 = modes[3 * f] ? 2 : 0, m1 = modes[3 * f + 1] ? 2 : 0, m2 = modes[3 * f + 2] ? 3 : 0;
    const uint8_t b = (uint8_t)(m0 | (m1 << 2) | (m2 << 4));
    mode_bytes[f] = b;
    if (b == 0) lists[4 + n_long++] = (uint32_t)f;
    else lists[4 + frames + n_short++] = (uint32_t)f;
  }
  lists[0] = n_long;
  lists[1] = n_short;
  lists[2] = lists[3] = 0u;
}

// ---- serializeFrame ---------------------------------------------------------------------------------------------------
// serializeFrame (serialization.js:41-98): the mirror of k_unpack_units, one wave per unit.  The unit is 53 big-endian
// words in LDS; every field lands on bits no other field uses, so OR-ing a field into the (at most two) words it touches
// is its insert, and the bits of a field past the 1 696th are dropped as packBits drops them (bitstream.js:15-38).
// Fields are taken as any int32: the header in wrapping uint32 arithmetic, wl & 15, sfi & 63, q & mask, and no mantissas
// for a BFU whose wl is outside 1..15 (WORD_LENGTH_BITS[wl] is 0 or undefined there).  nbfu is 0..52 (checked by the host).
__device__ __forceinline__ void or_bits_be(uint32_t *words, int pos, int nbits, uint32_t v) {
  const int w = pos >> 5, o = pos & 31;
  if (w >= 53) return;
  const uint64_t two = (uint64_t)v << (64 - o - nbits);      // o + nbits <= 47: the field sits in the top 47 bits
  __hip_atomic_fetch_or(&words[w], (uint32_t)(two >> 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
  const uint32_t lo = (uint32_t)two;
  if (lo != 0u && w + 1 < 53) __hip_atomic_fetch_or(&words[w + 1], lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
}

__global__ __launch_bounds__(C1_WAVE) void k_pack_units(const int32_t *__restrict__ nbfu, const int32_t *__restrict__ modes,
                                                       const int32_t *__restrict__ sfi, const int32_t *__restrict__ wl,
                                                       const int32_t *__restrict__ q, int64_t frames, uint8_t *__restrict__ units) {
  __shared__ uint32_t words[53];
  __shared__ uint32_t desc[52];           // per BFU: bits(5) | mantissa bit offset << 5
  const int lane = threadIdx.x;
  const int64_t f = blockIdx.x;
  if (f >= frames) return;
  if (lane < 53) words[lane] = 0u;
  const int n = nbfu[f];
  wave_fence();
  if (lane == 0) {
    // BFU_AMOUNTS.indexOf(nBfu): -1 sets bits 5..15; 2 - mode wraps, and the shifted fields overlap when a mode is out of range
    const int idx = n == 20 ? 0 : ((n >= 28 && (n & 3) == 0) ? (n - 24) >> 2 : -1);
    const uint32_t header = ((2u - (uint32_t)modes[3 * f]) << 14) | ((2u - (uint32_t)modes[3 * f + 1]) << 12) |
                            ((3u - (uint32_t)modes[3 * f + 2]) << 10) | ((uint32_t)idx << 5);
    words[0] = header << 16;
  }
  int w = 0, s = 0;
  if (lane < n) {
    w = wl[f * 52 + lane];
    s = sfi[f * 52 + lane];
  }
  const int bits = lane < n && w >= 1 && w <= 15 ? w + 1 : 0;
  const int mybits = lane < 52 ? bits * (int)kSpecs[lane] : 0;
  const int scan = wave_inclusive_scan(mybits);
  if (lane < 52) desc[lane] = (uint32_t)bits | ((uint32_t)(16 + 10 * n + scan - mybits) << 5);
  wave_fence();
  if (lane < n) {
    or_bits_be(words, 16 + 4 * lane, 4, (uint32_t)w & 15u);
    or_bits_be(words, 16 + 4 * n + 6 * lane, 6, (uint32_t)s & 63u);
  }
#pragma unroll
  for (int m = 0; m < 8; m++) {
    const int slot = 8 * lane + m, b = bfu_of_slot(slot);
    const uint32_t d = desc[b];
    const int fb = (int)(d & 31u);
    if (fb != 0) or_bits_be(words, (int)(d >> 5) + (slot - (int)kBfuFirst[b]) * fb, fb, (uint32_t)q[f * 512 + slot] & ((1u << fb) - 1u));
  }
  wave_fence();
  if (lane < 53) {
    const uint32_t v = lane == 52 ? words[52] & 0xff000000u : words[lane];   // bytes 209..211 are zeroed (:92-94)
    reinterpret_cast<uint32_t *>(units + f * C1_UNIT_BYTES)[lane] = __builtin_bswap32(v);
  }
}

}  // namespace

void c1k_launch_pack_units(const int32_t *nbfu, const int32_t *modes, const int32_t *sfi, const int32_t *wl, const int32_t *q,
                           int64_t frames, uint8_t *units, hipStream_t stream) {
  hipLaunchKernelGGL(k_pack_units, dim3((unsigned)frames), dim3(C1_WAVE), 0, stream, nbfu, modes, sfi, wl, q, frames, units);
}
void c1k_launch_block_modes_from_bands(const C1DevTables *tables, const float *bands, int64_t frames, int halo, double threshold,
                                       float *mags, int32_t *modes, hipStream_t stream) {
  hipLaunchKernelGGL(k_stage_mags, dim3((unsigned)(frames + halo)), dim3(C1_WAVE), 0, stream, tables, bands, frames + halo, mags);
  hipLaunchKernelGGL(k_stage_decide, dim3((unsigned)frames), dim3(C1_WAVE), 0, stream, tables, (const float *)mags, frames, halo,
                     threshold, modes);
}
void c1k_launch_stage_scale_factors(const C1DevTables *tables, const float *coefs, const int32_t *modes, int64_t frames, uint8_t *side,
                                    hipStream_t stream) {
  hipLaunchKernelGGL(k_stage_scale_factors, dim3((unsigned)frames), dim3(C1_WAVE), 0, stream, tables, coefs, modes, frames, side);
}
void c1k_launch_stage_fields(const C1DevTables *tables, const float *coefs, const int32_t *modes, const uint8_t *side,
                             const uint8_t *alloc, int64_t frames, int32_t *nbfu, int32_t *sfi, int32_t *wl, int32_t *q,
                             hipStream_t stream) {
  hipLaunchKernelGGL(k_stage_fields, dim3((unsigned)frames), dim3(C1_WAVE), 0, stream, tables, coefs, modes, side, alloc, frames,
                     nbfu, sfi, wl, q);
}
void c1k_launch_stage_mode_lists(const int32_t *modes, int64_t frames, uint8_t *mode_bytes, uint32_t *lists, hipStream_t stream) {
  hipLaunchKernelGGL(k_stage_mode_lists, dim3(1), dim3(C1_WAVE), 0, stream, modes, frames, mode_bytes, lists);
}
