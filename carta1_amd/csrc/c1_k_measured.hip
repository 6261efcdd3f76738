// c1_k_measured.hip -- the word lengths of every sound unit allocated by the measured coding error (c1_encode_measured_device):
// the weighted quantization error of every (BFU, word length) of a unit, a greedy allocation over that table for each of the
// eight BFU amounts, and the least of them handed to the packing kernels where it beats the reference's own record
#include "c1_device.h"

namespace {

// the domain of a mode byte is what blockSelectorStage writes (encoder.js:143): 0 or 2 in the low and mid fields, 0 or 3 in
// the high one.  Every mode byte is brought into it before anything selects with its fields.  The byte read here is the
// analysis' own, and under fixedBlockModes such as [1,1,1] or [2,2,1] its fields are the option's: a field that is not zero
// means short blocks (quantization.js:117 and the MDCT test blockMode === 0), as the packing kernels read it
__device__ __forceinline__ int mode_in_domain(int b) { return ((b & 0x03) ? 0x02 : 0) | ((b & 0x0c) ? 0x08 : 0) | ((b & 0x30) ? 0x30 : 0); }

// =====================================================================================================
// k_measured_alloc : e(b, w) for every BFU b and word length w, the greedy allocation for every amount, the fallback
// =====================================================================================================
// One wave per sound unit, kMeasuredWaves independent waves per workgroup, a bounded grid whose waves stride over the units.
// The definition (include/carta1_hip.h) in the kernel's terms:
//   table     A lane owns the 8 consecutive BFU-major slots 8 lane .. 8 lane + 7 (as k_pack and k_choose_bias) and reads its
//             coefficients once.  Per coded word length w = 1 .. 15 lanes 0..51 put what their BFU needs at that length into
//             the wave's LDS block, every lane quantizes and dequantizes its 8 slots (k_pack's exact quantizer, the decode
//             core's dequantizer forms, as k_choose_bias) and leaves the 8 squared differences in LDS; lane b then adds BFU
//             b's terms in ascending slot order and stores e(b, w) = W_b * sum.  W_b is a power of two (1 long, 1/4 low or mid
//             short, 1/2 high short), so W * (a + b) == W * a + W * b bit for bit.  e(b, 0) is the sum of the squares; a BFU
//             whose scale-factor index is 0 codes nothing, so e(b, w) == e(b, 0) comes out of the same arithmetic.  No fused
//             operation.
//   gains     The gain of raising BFU b from word length w, (e(b,w) - e(b,w+1)) / cost, does not depend on the amount or on
//             the step: lane b divides once per (b, w) and keeps the quotient's bit pattern as a 64-bit key in LDS, 0 where the
//             gain is not positive (or a NaN) or the BFU codes nothing.  A positive binary64 orders as its bit pattern does.
//   greedy    Lane b holds BFU b's word length, the key of its next level and that level's cost in bits.  A step is a
//             wave-wide maximum of the keys' high words over the eligible lanes, then -- only when more than one lane holds
//             it -- of the low words among those, the lowest lane that holds both, and that lane's update: one LDS read.  At
//             most 52 * 15 steps.  The eight amounts run one after the other over the same keys.
//   totals    The lanes leave their BFU's current error in LDS and every lane adds the 52 values in BFU order: T is the same
//             bits in every lane.  The first amount of least T wins; a NaN never wins.
//   fallback  T_ref is the same sum over the record the allocation chain left in L.alloc (every BFU at word length 0 when its
//             fallback flag is set).  taken = T(n*) < T_ref; only then, and only when the call packs, the record is replaced.
// Any bytes in the side and allocation records are memory-safe here: indices are masked (sfi & 63, wl & 15, amount & 7).
constexpr int kMeasuredWaves = 4;
constexpr int kMeasuredBlocks = 2048;    // as the choose kernels: past 8 192 units the waves stride
constexpr int kTableStride = 52;         // doubles between the rows (word lengths) of the tables
constexpr int kMaxSteps = 52 * 15;

struct alignas(16) MeasuredLds {
  double table[16 * kTableStride];   // e(b, w) at [w * kTableStride + b]
  union {
    struct {                         // while the table is built
      double terms[512];             // one word length's squared differences, BFU-major slot order
      double norm[52];               // quantRange / SCALE_FACTORS[sfi]; 0 when the BFU codes nothing
      double sf[52];                 // dq_step: SCALE_FACTORS[sfi] * RN(1 / range); else SCALE_FACTORS[sfi]
      int32_t range[52];             // 2^(bits - 1) - 1; 0 when the BFU codes nothing
    };
    struct {                         // after it
      unsigned long long key[15 * kTableStride];   // the gain of raising BFU b from w at [w * kTableStride + b], as an ordered key
      double cur[52];                // the BFUs' errors under one allocation, for the total
      uint32_t wl[56];               // the winner's word lengths, for the record's nibbles
    };
  };
};

// the maximum of an unsigned value over the 64 lanes, the same in every lane: shifts within the rows of 16 lanes, then the rows'
// last lanes broadcast to the rows behind them (data-parallel primitives: no LDS traffic); 0 is the identity.  All 64 lanes
// must be active
__device__ __forceinline__ uint32_t wave_umax32(uint32_t v) {
  auto umax = [](uint32_t a, uint32_t b) { return a > b ? a : b; };
  v = umax(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false));   // row_shr:1
  v = umax(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false));   // row_shr:2
  v = umax(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, false));   // row_shr:4
  v = umax(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, false));   // row_shr:8: lane 15 of a row holds the row's
  v = umax(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false));   // row_bcast:15 into rows 1 and 3
  v = umax(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false));   // row_bcast:31 into rows 2 and 3
  return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}

// the 52 errors in S.cur added in BFU order; every lane reads the same addresses and ends with the same bits
__device__ __forceinline__ double total_in_bfu_order(const MeasuredLds &S) {
  double t = 0.0;
#pragma unroll 4
  for (int b = 0; b < 52; b++) t += S.cur[b];
  return t;
}

__global__ __launch_bounds__(C1_WAVE * kMeasuredWaves) void k_measured_alloc(C1EncodeLaunch L, int all_long, int finalize,
                                                                             uint8_t *__restrict__ taken, double *__restrict__ distortion,
                                                                             double *__restrict__ energy) {
  __shared__ MeasuredLds lds[kMeasuredWaves];
  TablesPtr T = C1_TABLES(L.tables);
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  MeasuredLds &S = lds[wave];
  int slot_b[8], at_long[8], at_short[8];
#pragma unroll
  for (int m = 0; m < 8; m++) {
    const int p = 8 * lane + m;
    slot_b[m] = bfu_of_slot(p);
    const int j = p - kBfuFirst[slot_b[m]];
    at_long[m] = kStartLong[slot_b[m]] + j;
    at_short[m] = kStartShort[slot_b[m]] + j;
  }
  const int bl = lane < 52 ? lane : 51;                        // lanes 52..63 shadow BFU 51 and never take part
  const int my_first = kBfuFirst[bl], my_size = kSpecs[bl];
  const int bfu_shift = bl < 20 ? 0 : (bl < 36 ? 2 : 4);
  const double w_short = bl < 36 ? 0.25 : 0.5;
  const int dq_step = T->dq_step, dq_fast = T->dq_fast;
  const int64_t units_total = L.frames * L.channels;
  const int64_t stride = (int64_t)gridDim.x * kMeasuredWaves;
  for (int64_t unit = (int64_t)blockIdx.x * kMeasuredWaves + wave; unit < units_total; unit += stride) {
    const uint32_t *side = reinterpret_cast<const uint32_t *>(L.side + unit * kSideBytes);
    const int sfi = lane < 52 ? (int)((side[lane >> 2] >> ((lane & 3) * 8)) & 63) : 0;
    const int modes = all_long ? 0 : mode_in_domain((int)(side[13] & 0xff));
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
    const double W = ((modes >> bfu_shift) & 3) != 0 ? w_short : 1.0;   // BFU `lane`'s weight

    // ---- the table ----
    for (int w = 0; w < 16; w++) {                             // wave-uniform
      if (lane < 52) {
        const int bits = wl_bits(w);
        const bool coded = sfi != 0 && bits != 0;
        const double y = T->inv_range[w];
        S.norm[lane] = coded ? T->norm[sfi * 16 + w] : 0.0;
        S.range[lane] = coded ? (1 << (bits - 1)) - 1 : 0;
        S.sf[lane] = coded ? (dq_step ? T->scale_factors[sfi] * y : T->scale_factors[sfi]) : 0.0;
      }
      wave_fence();
      const double yy = T->inv_range[w];
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
        if (range == 0) d = 0.0f;
        else if (dq_step) d = f32((double)q * sfv);            // == Float32((q * SF) / range) for every input (checked on the host)
        else {
          const double a = (double)q * sfv;
          if (dq_fast) {
            const double q0 = a * yy;
            d = f32(__builtin_fma(__builtin_fma(-q0, (double)range, a), yy, q0));   // == a / range (checked on the host)
          } else d = f32(a / (double)range);
        }
        const double t = (double)x[m] - (double)d;
        S.terms[8 * lane + m] = t * t;
      }
      wave_fence();
      if (lane < 52) {
        double acc = 0.0;
        for (int j = 0; j < my_size; j++) acc += S.terms[my_first + j];
        S.table[w * kTableStride + lane] = W * acc;
      }
      wave_fence();                                            // the next word length rewrites the block
    }

    // ---- the gains ----
    if (lane < 52) {
      double e0 = S.table[lane];
      for (int w = 0; w < 15; w++) {
        const double e1 = S.table[(w + 1) * kTableStride + lane];
        const double gain = (e0 - e1) / (double)((w == 0 ? 2 : 1) * my_size);   // cost = (bits(w + 1) - bits(w)) * size
        S.key[w * kTableStride + lane] = (sfi != 0 && gain > 0.0) ? (unsigned long long)__double_as_longlong(gain) : 0ull;
        e0 = e1;
      }
    }
    wave_fence();

    // ---- the reference's record: T_ref ----
    const uint32_t *al = reinterpret_cast<const uint32_t *>(L.alloc + unit * kAllocBytes);
    const uint32_t a7 = al[7];                                 // amount index, fallback flag
    const bool ref_fallback = (a7 >> 27) & 1;
    const int ref_n = bfu_amount((int)(a7 >> 28) & 7);
    if (lane < 52) {
      const int wl = (lane < ref_n && !ref_fallback) ? (int)((al[lane >> 3] >> ((lane & 7) * 4)) & 15) : 0;
      S.cur[lane] = S.table[wl * kTableStride + lane];
    }
    wave_fence();
    const double t_ref = total_in_bfu_order(S);
    wave_fence();
    if (lane < 52) S.cur[lane] = S.table[lane];
    wave_fence();
    const double e_unit = total_in_bfu_order(S);
    wave_fence();

    // ---- the greedy allocation for every amount ----
    double best_t = 0.0;
    int best_wl = 0, best_a = 0;
    bool have = false;
    for (int a = 0; a < 8; a++) {                              // wave-uniform
      const int n = bfu_amount(a);
      int rem = 1696 - 40 - 10 * n;
      const bool mine = lane < n;                               // n <= 52
      int wl = 0;
      unsigned long long key = S.key[bl];
      int cost = 2 * my_size;                                  // (bits(1) - bits(0)) * size
      for (int step = 0; step < kMaxSteps; step++) {
        const bool eligible = mine && cost <= rem && key != 0ull;          // word length 15: the key is 0
        const uint32_t hi = eligible ? (uint32_t)(key >> 32) : 0u, top_hi = wave_umax32(hi);
        unsigned long long holders = __ballot(eligible && hi == top_hi);
        if (holders == 0ull) break;                            // wave-uniform
        if (holders & (holders - 1)) {                         // wave-uniform and rare: the high words tie, the low words decide
          const bool tied = eligible && hi == top_hi;
          const uint32_t lo = tied ? (uint32_t)key : 0u, top_lo = wave_umax32(lo);
          holders = __ballot(tied && lo == top_lo);
        }
        const int winner = __builtin_ctzll(holders);           // the smallest BFU on a tie
        rem -= __builtin_amdgcn_readlane(cost, winner);
        if (lane == winner) {
          wl++;
          cost = my_size;                                      // (bits(w + 1) - bits(w)) * size, w >= 1
          key = wl < 15 ? S.key[wl * kTableStride + bl] : 0ull;
        }
      }
      const double e_cur = S.table[wl * kTableStride + bl];
      if (lane < 52) S.cur[lane] = lane < n ? e_cur : S.table[lane];
      wave_fence();
      const double t = total_in_bfu_order(S);
      wave_fence();
      if (a == 0) best_t = t;                                  // all NaN: the first amount's total is reported, and nothing is taken
      if (t == t && (!have || t < best_t)) { best_t = t; best_wl = wl; best_a = a; have = true; }
    }
    const bool take = have && best_t < t_ref;

    if (finalize && take) {                                    // wave-uniform: every lane holds the same totals
      const int nb = bfu_amount(best_a);
      if (lane < 56) S.wl[lane] = lane < nb ? (uint32_t)best_wl : 0u;
      wave_fence();
      if (lane < 8) {
        uint32_t word = (uint32_t)best_a << 28;
        if (lane < 7) {
          word = 0u;
#pragma unroll
          for (int k = 0; k < 8; k++) word |= (S.wl[8 * lane + k] & 15u) << (4 * k);
        }
        reinterpret_cast<uint32_t *>(L.alloc + unit * kAllocBytes)[lane] = word;
      }
      wave_fence();
    }
    if (lane == 0) {
      if (taken) taken[unit] = take ? 1 : 0;
      if (distortion) { distortion[2 * unit] = t_ref; distortion[2 * unit + 1] = best_t; }
      if (energy) energy[unit] = e_unit;
    }
  }
}

}  // namespace

void c1k_launch_measured_alloc(const C1EncodeLaunch &L, bool all_long, bool finalize, uint8_t *taken, double *distortion, double *energy,
                               hipStream_t stream) {
  const int64_t units = L.frames * L.channels;
  if (units <= 0) return;
  const dim3 grid((unsigned)std::min<int64_t>(kMeasuredBlocks, (units + kMeasuredWaves - 1) / kMeasuredWaves)), block(C1_WAVE * kMeasuredWaves);
  hipLaunchKernelGGL(k_measured_alloc, grid, block, 0, stream, L, all_long ? 1 : 0, finalize ? 1 : 0, taken, distortion, energy);
}
