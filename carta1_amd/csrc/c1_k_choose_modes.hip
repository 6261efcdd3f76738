// c1_k_choose_modes.hip -- the block modes of every sound unit chosen from candidates by least coding error
// (c1_encode_best_modes_device): constant-mode work lists for the second analysis, the side record of a candidate composed
// from the all-long and the all-short analysis, the weighted quantization error of every (unit, candidate) from the trial
// allocations, and the winner's coefficients, side record and allocation handed to the packing kernels
#include "c1_device.h"

namespace {

// the domain of a mode byte is what blockSelectorStage writes (encoder.js:143): 0 or 2 in the low and mid fields, 0 or 3 in
// the high one.  Every candidate byte is brought into it before anything selects or indexes with its fields
__device__ __forceinline__ int mode_in_domain(int b) { return (b & 0x02) | (b & 0x08) | ((b & 0x30) == 0x30 ? 0x30 : 0); }

// =====================================================================================================
// k_const_mode_lists : mode bytes and k_mdct_bands' work lists when every unit has the same modes
// =====================================================================================================
// One lane per unit: the byte into modes[unit], the unit into the all-long (byte 0) or the mixed list at its own index -- the
// lists k_modes_lists would write for a constant byte, in unit order and without a counter.
__global__ __launch_bounds__(256) void k_const_mode_lists(int byte, int64_t units, uint8_t *__restrict__ modes, uint32_t *__restrict__ lists) {
  const int64_t unit = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int b = mode_in_domain(byte);
  if (unit == 0) {
    lists[0] = b == 0 ? (uint32_t)units : 0u;
    lists[1] = b == 0 ? 0u : (uint32_t)units;
    lists[2] = 0u;
    lists[3] = 0u;
  }
  if (unit >= units) return;
  modes[unit] = (uint8_t)b;
  lists[4 + (b == 0 ? 0 : units) + unit] = (uint32_t)unit;
}

// word w of a side record (sfi[52], mode byte, padding): which band's mode decides it (BFUs 0-19 low, 20-35 mid, 36-51 high)
__device__ __forceinline__ int band_of_side_word(int w) { return w < 5 ? 0 : (w < 9 ? 1 : 2); }

__device__ __forceinline__ uint32_t composed_side_word(const uint8_t *side_long, const uint8_t *side_short, int64_t unit, int w, int byte) {
  if (w == 13) return (uint32_t)byte;                          // the mode byte where k_mdct_bands keeps it, then padding
  if (w > 13) return 0u;
  const bool is_short = ((byte >> (2 * band_of_side_word(w))) & 3) != 0;
  return reinterpret_cast<const uint32_t *>((is_short ? side_short : side_long) + unit * kSideBytes)[w];
}

// =====================================================================================================
// k_compose_side : the side record of every unit under one candidate, a per-band selection of the two analyses' records
// =====================================================================================================
// One lane per 32-bit word.  The allocation chain reads the scale-factor indices of a side record and nothing else
// (load_sfi, c1_k_allocate.hip), so a candidate's coefficients are never composed: only the winner's are (k_choose_modes).
__global__ __launch_bounds__(256) void k_compose_side(const uint8_t *__restrict__ side_long, const uint8_t *__restrict__ side_short, int64_t units,
                                                       int byte, uint8_t *__restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= units * 16) return;
  const int64_t unit = i >> 4;
  const int w = (int)(i & 15);
  reinterpret_cast<uint32_t *>(out + unit * kSideBytes)[w] = composed_side_word(side_long, side_short, unit, w, mode_in_domain(byte));
}

// =====================================================================================================
// k_choose_modes : quantize and dequantize every candidate as k_choose_bias does every palette entry, weight the squared
// errors by the transform's scaling, pick the candidate with the least sum
// =====================================================================================================
// One wave per sound unit, kChooseModesWaves independent waves per workgroup, a bounded grid whose waves stride over the units.
// A lane owns the 8 consecutive BFU-major slots 8 lane .. 8 lane + 7, as in k_pack and k_choose_bias.  The low band is slots
// 0..127, the mid band 128..255, the high band 256..511: a lane's band is lane < 16 ? low : lane < 32 ? mid : high, so the
// block mode of a slot, and with it the weight, is one value per lane and candidate.  A lane holds its slots' coefficient
// from the all-long analysis (slot order == coefficient order: two float4 loads) and from the all-short one (gathered through
// BFU_START_SHORT), and lanes 0..51 their BFU's scale-factor index from both; a plane no candidate needs is not read.
//   quantizer, dequantizer   exactly k_choose_bias's (c1_k_choose.hip): k_pack's quantizer, the decode core's dequantizer forms
//   terms        t = c - d and c in binary64; a lane adds t * t (and c * c) over its 8 slots in slot order, multiplies the
//                sum by W -- 1 for a long band, 1/4 for the low or mid band short, 1/2 for the high band short: a power of
//                two, so W * (a + b) == W * a + W * b bit for bit and the sum is that of the weighted terms -- then one
//                butterfly over the lanes (xor 1, 2, .. 32).  No fused operation.
//   choice       the smallest candidate whose sum no other's is below; a NaN never wins, all NaN selects candidate 0
//   winner       lanes 0..7 copy its trial record to L.alloc, lanes 0..15 write its side record to L.side, and a lane whose
//                band (in coefficient order: coefficients 8 lane .. 8 lane + 7, the same three ranges) the winner codes short
//                copies its 8 coefficients of the all-short plane over the all-long plane's, which packing then reads.  A
//                lane overwrites only the 8 long coefficients it loaded itself.
constexpr int kChooseModesWaves = 4;
constexpr int kChooseModesBlocks = 2048;   // as k_choose_bias: past 8 192 units the waves stride

struct C1ModeCandidates {
  uint8_t byte[C1_MAX_MODE_CANDIDATES];
};

struct alignas(16) ChooseModesLds {
  double norm[52];            // quantRange / SCALE_FACTORS[sfi]; 0 when the BFU codes nothing
  double sf[52];              // dq_step: SCALE_FACTORS[sfi] * RN(1 / range); else SCALE_FACTORS[sfi]
  double inv[52];             // RN(1 / range) (the reciprocal form)
  int32_t range[52];          // 2^(bits - 1) - 1; 0 when the BFU codes nothing
};

__device__ __forceinline__ double wave_sum_fixed(double v) {
#pragma unroll
  for (int d = 1; d < C1_WAVE; d <<= 1) v += __shfl_xor(v, d, C1_WAVE);
  return v;
}

__global__ __launch_bounds__(C1_WAVE * kChooseModesWaves) void k_choose_modes(C1EncodeLaunch L, const float *__restrict__ coefs_short,
                                                                               const uint8_t *__restrict__ side_short,
                                                                               const uint8_t *__restrict__ trial, int64_t trial_stride,
                                                                               C1ModeCandidates cand, int n_cand, int has_long, int has_short,
                                                                               int finalize, uint8_t *__restrict__ choice,
                                                                               uint8_t *__restrict__ modes_out, double *__restrict__ distortion,
                                                                               double *__restrict__ energy) {
  __shared__ ChooseModesLds lds[kChooseModesWaves];
  TablesPtr T = C1_TABLES(L.tables);
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  ChooseModesLds &S = lds[wave];
  int slot_b[8], at_short[8];
#pragma unroll
  for (int m = 0; m < 8; m++) {
    const int p = 8 * lane + m;
    slot_b[m] = bfu_of_slot(p);
    at_short[m] = kStartShort[slot_b[m]] + (p - kBfuFirst[slot_b[m]]);
  }
  const int band_shift = lane < 16 ? 0 : (lane < 32 ? 2 : 4);                 // the lane's slots (and its 8 coefficients)
  const double w_short = lane < 32 ? 0.25 : 0.5;
  const int bfu_shift = lane < 20 ? 0 : (lane < 36 ? 2 : 4);                  // BFU `lane`
  const int dq_step = T->dq_step, dq_fast = T->dq_fast;
  const int64_t units_total = L.frames * L.channels;
  const int64_t stride = (int64_t)gridDim.x * kChooseModesWaves;
  for (int64_t unit = (int64_t)blockIdx.x * kChooseModesWaves + wave; unit < units_total; unit += stride) {
    int sfi_long = 0, sfi_short = 0;
    float xl[8], xs[8];
#pragma unroll
    for (int m = 0; m < 8; m++) xl[m] = xs[m] = 0.0f;
    if (has_long) {
      const uint32_t *side = reinterpret_cast<const uint32_t *>(L.side + unit * kSideBytes);
      if (lane < 52) sfi_long = (int)((side[lane >> 2] >> ((lane & 3) * 8)) & 63);
      const float4 *c4 = reinterpret_cast<const float4 *>(L.coefs + (unit << 9));
      const float4 a = c4[2 * lane], c = c4[2 * lane + 1];
      xl[0] = a.x; xl[1] = a.y; xl[2] = a.z; xl[3] = a.w; xl[4] = c.x; xl[5] = c.y; xl[6] = c.z; xl[7] = c.w;
    }
    if (has_short) {
      const uint32_t *side = reinterpret_cast<const uint32_t *>(side_short + unit * kSideBytes);
      if (lane < 52) sfi_short = (int)((side[lane >> 2] >> ((lane & 3) * 8)) & 63);
      const float *cs = coefs_short + (unit << 9);
#pragma unroll
      for (int m = 0; m < 8; m++) xs[m] = cs[at_short[m]];
    }
    double e_long = 0.0, e_short = 0.0;
#pragma unroll
    for (int m = 0; m < 8; m++) {
      e_long += (double)xl[m] * (double)xl[m];
      e_short += (double)xs[m] * (double)xs[m];
    }
    double best = 0.0;
    int best_k = 0;
    bool have = false;
    for (int k = 0; k < n_cand; k++) {                         // wave-uniform (a kernel argument), at most C1_MAX_MODE_CANDIDATES
      const int byte = mode_in_domain(cand.byte[k]);
      const bool lane_short = ((byte >> band_shift) & 3) != 0;
      const bool bfu_short = ((byte >> bfu_shift) & 3) != 0;
      const double w = lane_short ? w_short : 1.0;
      const uint32_t *al = reinterpret_cast<const uint32_t *>(trial + (int64_t)k * trial_stride + unit * kAllocBytes);
      const uint32_t a7 = al[7];                               // amount index, fallback flag
      const bool fallback = (a7 >> 27) & 1;
      const int nb = bfu_amount((int)(a7 >> 28) & 7);
      if (lane < 52) {
        const int wl = lane < nb ? (int)((al[lane >> 3] >> ((lane & 7) * 4)) & 15) : 0;
        const int sf = fallback ? 0 : (bfu_short ? sfi_short : sfi_long);
        const int bits = wl_bits(wl);
        const bool coded = sf != 0 && bits != 0;
        const double y = T->inv_range[wl];
        S.norm[lane] = coded ? T->norm[sf * 16 + wl] : 0.0;
        S.range[lane] = coded ? (1 << (bits - 1)) - 1 : 0;
        S.sf[lane] = coded ? (dq_step ? T->scale_factors[sf] * y : T->scale_factors[sf]) : 0.0;
        S.inv[lane] = y;
      }
      wave_fence();
      double acc = 0.0;
#pragma unroll
      for (int m = 0; m < 8; m++) {
        const int b = slot_b[m];
        const float x = lane_short ? xs[m] : xl[m];
        const int32_t range = S.range[b];
        const double xn = (double)x * S.norm[b];
        const double v = xn + (xn >= 0 ? 0.5 : -0.5);          // round half away from zero ...
        int32_t q = (int32_t)v;                                // ... then `| 0`: truncation; exact wrap below
        if (__builtin_expect(!(fabs(v) < 2147483648.0), 0)) q = to_int32(v);
        q = q > range ? range : (q < -range ? -range : q);     // range 0 (nothing coded): 0
        const double sfv = S.sf[b];
        float d;
        if (dq_step) d = f32((double)q * sfv);                 // == Float32((q * SF) / range) for every input (checked on the host)
        else if (range == 0) d = 0.0f;
        else {
          const double a = (double)q * sfv;
          if (dq_fast) {
            const double yy = S.inv[b], q0 = a * yy;
            d = f32(__builtin_fma(__builtin_fma(-q0, (double)range, a), yy, q0));   // == a / range (checked on the host)
          } else d = f32(a / (double)range);
        }
        const double t = (double)x - (double)d;
        acc += t * t;
      }
      wave_fence();                                            // the next candidate rewrites the block
      acc = wave_sum_fixed(w * acc);
      const double e = wave_sum_fixed(w * (lane_short ? e_short : e_long));
      if (lane == 0) {
        if (distortion) distortion[unit * n_cand + k] = acc;
        if (energy) energy[unit * n_cand + k] = e;
      }
      if (acc == acc && (!have || acc < best)) { best = acc; best_k = k; have = true; }
    }
    const int win = mode_in_domain(cand.byte[best_k]);
    if (finalize) {
      if (lane < 8)
        reinterpret_cast<uint32_t *>(L.alloc + unit * kAllocBytes)[lane] =
            reinterpret_cast<const uint32_t *>(trial + (int64_t)best_k * trial_stride + unit * kAllocBytes)[lane];
      if (lane < 16) {
        const uint32_t word = composed_side_word(L.side, side_short, unit, lane, win);
        reinterpret_cast<uint32_t *>(L.side + unit * kSideBytes)[lane] = word;
      }
      if ((win >> band_shift) & 3) {
        const float4 *src = reinterpret_cast<const float4 *>(coefs_short + (unit << 9));
        float4 *dst = reinterpret_cast<float4 *>(L.coefs + (unit << 9));
        const float4 a = src[2 * lane], c = src[2 * lane + 1];
        dst[2 * lane] = a;
        dst[2 * lane + 1] = c;
      }
    }
    if (lane == 0) {
      if (choice) choice[unit] = (uint8_t)best_k;
      if (modes_out) modes_out[unit] = (uint8_t)win;
    }
  }
}

}  // namespace

void c1k_launch_const_mode_lists(int byte, int64_t units, uint8_t *modes_ws, uint32_t *lists_ws, hipStream_t stream) {
  if (units <= 0) return;
  hipLaunchKernelGGL(k_const_mode_lists, dim3((unsigned)((units + 255) / 256)), dim3(256), 0, stream, byte, units, modes_ws, lists_ws);
}

void c1k_launch_compose_side(const uint8_t *side_long, const uint8_t *side_short, int64_t units, int byte, uint8_t *out, hipStream_t stream) {
  if (units <= 0) return;
  hipLaunchKernelGGL(k_compose_side, dim3((unsigned)((units * 16 + 255) / 256)), dim3(256), 0, stream, side_long, side_short, units, byte, out);
}

void c1k_launch_choose_modes(const C1EncodeLaunch &L, const float *coefs_short, const uint8_t *side_short, const uint8_t *trial,
                             int64_t trial_stride, const uint8_t *cand, int n_cand, bool finalize, uint8_t *choice, uint8_t *modes_out,
                             double *distortion, double *energy, hipStream_t stream) {
  const int64_t units = L.frames * L.channels;
  if (units <= 0 || n_cand <= 0 || n_cand > C1_MAX_MODE_CANDIDATES) return;
  C1ModeCandidates c;
  int has_long = 0, has_short = 0;
  for (int k = 0; k < C1_MAX_MODE_CANDIDATES; k++) {
    c.byte[k] = k < n_cand ? cand[k] : 0;
    if (k >= n_cand) continue;
    if ((cand[k] & 0x3f) != 0x3a) has_long = 1;               // some band long (bytes are in the domain here)
    if ((cand[k] & 0x3f) != 0) has_short = 1;
  }
  const dim3 grid((unsigned)std::min<int64_t>(kChooseModesBlocks, (units + kChooseModesWaves - 1) / kChooseModesWaves)), block(C1_WAVE * kChooseModesWaves);
  hipLaunchKernelGGL(k_choose_modes, grid, block, 0, stream, L, coefs_short, side_short, trial, trial_stride, c, n_cand, has_long, has_short,
                     finalize ? 1 : 0, choice, modes_out, distortion, energy);
}
