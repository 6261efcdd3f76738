// c1_k_choose.hip -- the allocation bias of every sound unit chosen from a palette by least coding error
// (c1_encode_best_bias_device): the real quantization error of every (unit, palette entry) from the trial allocations, and
// the allocation of the entry with the least error handed to the packing kernels
#include "c1_device.h"

namespace {

// =====================================================================================================
// k_choose_bias : quantize (quantization.js:34-56) under every trial allocation, dequantize as the decoder does
// (quantization.js:65-78, decoder.js:52-98), sum (c - d)^2 in binary64, pick the entry with the least sum
// =====================================================================================================
// One wave per sound unit, kChooseWaves independent waves per workgroup, a bounded grid whose waves stride over the units.
// A lane owns the 8 consecutive coefficient slots 8 lane .. 8 lane + 7 in BFU-major order, as in k_pack: for an all-long
// unit that is coefficient order and the 512 coefficients arrive as two float4 loads per lane; a band coded with short
// blocks has its BFUs interleaved over the blocks (BFU_START_SHORT, constants.js:46-52) and its slots are gathered.  The
// coefficients and the scale-factor indices are read ONCE per unit; per palette entry the wave reads the entry's 32 trial
// bytes, lanes 0..51 put what their BFU needs (quantizer norm, range, the dequantizer's scale factor and reciprocal) into
// the wave's LDS block, and every lane walks its 8 slots.
//   quantizer    k_pack's exact one: x * (quantRange / SCALE_FACTORS[sfi]) from the host's table, half away from zero,
//                ToInt32, the clamp -- so the mantissas are the ones the packing kernels write
//   dequantizer  Float32((q * SCALE_FACTORS[sfi]) / range) in the decode core's forms: one product with SF * RN(1 / range)
//                (dq_step), the reciprocal with its correction (dq_fast), or the division -- as the host verified for the
//                installed tables (c1_table_fast_paths)
//   sums         a lane adds its 8 squared differences in slot order, then a butterfly over the lanes (xor 1, 2, .. 32):
//                one fixed tree, and as a + b == b + a every lane ends with the same bits.  No fused operation.
//   choice       the smallest entry whose sum no other entry's is below; a NaN never wins, all NaN selects entry 0
// A unit codes nothing where a BFU is at or above the amount, has word length 0 or scale factor 0 (every BFU of a unit that
// took the allocation's fallback): q = 0 and d = 0 there, the term is c^2.
constexpr int kChooseWaves = 4;
constexpr int kChooseBlocks = 2048;      // two rounds of the 4 workgroups (115 VGPRs: 4 waves per SIMD) each of 256 compute units holds; past 8 192 units the waves stride

struct alignas(16) ChooseLds {
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

__global__ __launch_bounds__(C1_WAVE * kChooseWaves) void k_choose_bias(C1EncodeLaunch L, const uint8_t *__restrict__ trial, int64_t trial_stride,
                                                                         int n_palette, int all_long, uint8_t *__restrict__ choice,
                                                                         double *__restrict__ distortion, double *__restrict__ energy) {
  __shared__ ChooseLds lds[kChooseWaves];
  TablesPtr T = C1_TABLES(L.tables);
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  ChooseLds &S = lds[wave];
  int slot_b[8], at_long[8], at_short[8];
#pragma unroll
  for (int m = 0; m < 8; m++) {
    const int p = 8 * lane + m;
    slot_b[m] = bfu_of_slot(p);
    const int j = p - kBfuFirst[slot_b[m]];
    at_long[m] = kStartLong[slot_b[m]] + j;
    at_short[m] = kStartShort[slot_b[m]] + j;
  }
  const int dq_step = T->dq_step, dq_fast = T->dq_fast;
  const int64_t units_total = L.frames * L.channels;
  const int64_t stride = (int64_t)gridDim.x * kChooseWaves;
  for (int64_t unit = (int64_t)blockIdx.x * kChooseWaves + wave; unit < units_total; unit += stride) {
    const uint32_t *side = reinterpret_cast<const uint32_t *>(L.side + unit * kSideBytes);
    const int sfi = lane < 52 ? (int)((side[lane >> 2] >> ((lane & 3) * 8)) & 63) : 0;
    const int modes = all_long ? 0 : (int)(side[13] & 0xff);
    const int m0 = modes & 3, m1 = (modes >> 2) & 3, m2 = (modes >> 4) & 3;
    const float *coefs = L.coefs + (unit << 9);
    float x[8];
    if (modes == 0) {                                          // all long: coefficient order == slot order
      const float4 a = reinterpret_cast<const float4 *>(coefs)[2 * lane], c = reinterpret_cast<const float4 *>(coefs)[2 * lane + 1];
      x[0] = a.x; x[1] = a.y; x[2] = a.z; x[3] = a.w; x[4] = c.x; x[5] = c.y; x[6] = c.z; x[7] = c.w;
    } else {
#pragma unroll
      for (int m = 0; m < 8; m++) {
        const int mode = slot_b[m] >= 36 ? m2 : (slot_b[m] >= 20 ? m1 : m0);
        x[m] = coefs[mode == 0 ? at_long[m] : at_short[m]];
      }
    }
    double e = 0.0;
#pragma unroll
    for (int m = 0; m < 8; m++) e += (double)x[m] * (double)x[m];
    e = wave_sum_fixed(e);
    double best = 0.0;
    int best_k = 0;
    bool have = false;
    for (int k = 0; k < n_palette; k++) {                      // wave-uniform (a kernel argument), at most C1_MAX_BIAS_PALETTE
      const uint32_t *al = reinterpret_cast<const uint32_t *>(trial + (int64_t)k * trial_stride + unit * kAllocBytes);
      const uint32_t a7 = al[7];                               // amount index, fallback flag
      const bool fallback = (a7 >> 27) & 1;
      const int nb = bfu_amount((int)(a7 >> 28) & 7);
      if (lane < 52) {
        const int wl = lane < nb ? (int)((al[lane >> 3] >> ((lane & 7) * 4)) & 15) : 0;
        const int sf = fallback ? 0 : sfi;
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
        const int32_t range = S.range[b];
        const double xs = (double)x[m] * S.norm[b];
        const double v = xs + (xs >= 0 ? 0.5 : -0.5);          // round half away from zero ...
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
        const double t = (double)x[m] - (double)d;
        acc += t * t;
      }
      wave_fence();                                            // the next entry rewrites the block
      acc = wave_sum_fixed(acc);
      if (distortion && lane == 0) distortion[unit * n_palette + k] = acc;
      if (acc == acc && (!have || acc < best)) { best = acc; best_k = k; have = true; }
    }
    if (lane < 8)
      reinterpret_cast<uint32_t *>(L.alloc + unit * kAllocBytes)[lane] =
          reinterpret_cast<const uint32_t *>(trial + (int64_t)best_k * trial_stride + unit * kAllocBytes)[lane];
    if (lane == 0) {
      if (choice) choice[unit] = (uint8_t)best_k;
      if (energy) energy[unit] = e;
    }
  }
}

}  // namespace

void c1k_launch_choose_bias(const C1EncodeLaunch &L, const uint8_t *trial, int64_t trial_stride, int n_palette, bool all_long,
                            uint8_t *choice, double *distortion, double *energy, hipStream_t stream) {
  const int64_t units = L.frames * L.channels;
  if (units <= 0 || n_palette <= 0) return;
  const dim3 grid((unsigned)std::min<int64_t>(kChooseBlocks, (units + kChooseWaves - 1) / kChooseWaves)), block(C1_WAVE * kChooseWaves);
  hipLaunchKernelGGL(k_choose_bias, grid, block, 0, stream, L, trial, trial_stride, n_palette, all_long ? 1 : 0, choice, distortion, energy);
}
