// c1_k_measured_wide.hip -- the measured allocation of c1_k_measured.hip, c1_k_measured_sf.hip and c1_k_measured_masked.hip for a
// launch of few units (a streaming push, a frame closure): a workgroup of eight waves per unit instead of one wave, so that the
// sixteen rows of the error table and the eight greedy chains, which do not depend on each other, run beside each other.  Every
// output is bit for bit what those kernels give: no floating-point operation is reordered, only handed to another wave
#include "c1_device.h"

namespace {

// the domain of a mode byte is what blockSelectorStage writes (encoder.js:143): 0 or 2 in the low and mid fields, 0 or 3 in
// the high one.  Every mode byte is brought into it before anything selects with its fields.  The byte read here is the
// analysis' own, and under fixedBlockModes such as [1,1,1] or [2,2,1] its fields are the option's: a field that is not zero
// means short blocks (quantization.js:117 and the MDCT test blockMode === 0), as the packing kernels read it
__device__ __forceinline__ int mode_in_domain(int b) { return ((b & 0x03) ? 0x02 : 0) | ((b & 0x0c) ? 0x08 : 0) | ((b & 0x30) ? 0x30 : 0); }

// =====================================================================================================
// k_measured_wide : k_measured_masked's unit function, a workgroup per unit
// =====================================================================================================
// The helpers of c1_k_measured_masked.hip are repeated here so that its code stays as it is.  The definition is
// include/carta1_hip.h's; mask == null is P_b = 1 without the weight phase (k_measured_sf), one offset
// besides is k_measured_alloc.  In the kernel's terms, where it differs from k_measured_masked:
//   table     Every wave has a norm / range / sf / terms block of its own.  Every wave runs level 0 (one pass) and forms P_b from
//             it, so that no wave waits for another before its first compare; wave 0 alone writes the row.  The coded levels 1 ..
//             15 are dealt over the waves (wave v: v + 1 and v + 9); all candidates of one (b, w) stay in that wave, in candidate
//             order, and the strict-less compare runs on P_b (W acc) as there.  pick(b, w) goes to LDS, a byte per entry, and
//             e'_0(b, wl_ref[b]) is left by the wave that owns level wl_ref[b].  Barrier.
//   gains     Row w of the keys by wave w & 7: every key is a function of two table entries alone.  Waves 1 and 2 add T_ref and the
//             unit's energy in BFU order meanwhile.  Barrier.
//   greedy    Wave a runs amount a with k_measured_masked's step and leaves T(a) and its 52 word lengths in LDS.  Barrier.
//   the rest  Wave 0: the first amount of least non-NaN T in amount order, then that kernel's finalisation and stores.
// Every barrier is outside any loop and outside any branch: all eight waves reach each of the three.  Any bytes in the side and
// allocation records are memory-safe here: indices are masked (sfi & 63, wl & 15, amount & 7), and s0 + offset is range-checked
// before it indexes a table.  The grid is the unit count: no wave strides
constexpr int kWideWaves = 8;
constexpr int kTableStride = 52;         // doubles between the rows (word lengths) of the tables
constexpr int kMaxSteps = 52 * 15;

struct alignas(16) WideWaveLds {       // a wave's own block
  double terms[512];                   // one pass' squared differences, BFU-major slot order
  double norm[52];                     // quantRange / SCALE_FACTORS[sfi]; 0 when the BFU codes nothing.  After level 0: E_c
  double sf[52];                       // dq_step: SCALE_FACTORS[sfi] * RN(1 / range); else SCALE_FACTORS[sfi]
  double cur[52];                      // the BFUs' errors under one allocation, for the total
  int32_t range[52];                   // 2^(bits - 1) - 1; 0 when the BFU codes nothing
  uint32_t wl[56];                     // the wave's greedy word lengths; wave 0 at the end: the winner's, with the written indices
};

struct alignas(16) WideLds {
  double table[16 * kTableStride];               // e'(b, w) at [w * kTableStride + b]
  unsigned long long key[15 * kTableStride];     // the gain of raising BFU b from w at [w * kTableStride + b], as an ordered key
  double e_ref[52];                              // e'_0(b, wl_ref[b])
  double t[kWideWaves];                          // T(a)
  double t_ref, e_unit;
  uint8_t pick[16 * kTableStride];               // the candidate of e'(b, w)
  WideWaveLds w[kWideWaves];
};

// the maximum of an unsigned value over the 64 lanes, the same in every lane (as c1_k_measured.hip's): shifts within the rows of
// 16 lanes, then the rows' last lanes broadcast to the rows behind them; 0 is the identity.  All 64 lanes must be active
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

// 52 errors added in BFU order; every lane reads the same addresses and ends with the same bits
__device__ __forceinline__ double total_in_bfu_order(const double *cur) {
  double t = 0.0;
#pragma unroll 4
  for (int b = 0; b < 52; b++) t += cur[b];
  return t;
}

// candidate k's offset: the eight signed bytes travel in one 64-bit kernel argument, byte k = sf_offsets[k]
__device__ __forceinline__ int offset_of(unsigned long long packed, int k) { return (int)(int8_t)(packed >> (8 * (k & 7))); }

__global__ __launch_bounds__(C1_WAVE * kWideWaves) void k_measured_wide(C1EncodeLaunch L, int all_long, int finalize, unsigned long long offsets,
                                                                        int n_offsets, const double *__restrict__ mask, int has_spread,
                                                                        uint8_t *__restrict__ taken, int8_t *__restrict__ shifts,
                                                                        double *__restrict__ distortion, double *__restrict__ energy,
                                                                        double *__restrict__ weights) {
  __shared__ WideLds S;
  TablesPtr T = C1_TABLES(L.tables);
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) & (kWideWaves - 1);
  WideWaveLds &V = S.w[wave];
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
  const int n_cand = n_offsets < 1 ? 1 : (n_offsets > 8 ? 8 : n_offsets);
  const bool masked = mask != nullptr;                         // workgroup-uniform
  const int64_t units_total = L.frames * L.channels;
  // the grid is the unit count; a workgroup past it (none is launched) would still reach every barrier, on the last unit, and
  // store nothing
  const bool in_range = (int64_t)blockIdx.x < units_total;
  const int64_t unit = in_range ? (int64_t)blockIdx.x : units_total - 1;

  const uint32_t *side = reinterpret_cast<const uint32_t *>(L.side + unit * kSideBytes);
  const int sfi = lane < 52 ? (int)((side[lane >> 2] >> ((lane & 3) * 8)) & 63) : 0;
  const int modes = all_long ? 0 : mode_in_domain((int)(side[13] & 0xff));
  const int m0 = modes & 3, m1 = (modes >> 2) & 3, m2 = (modes >> 4) & 3;
  const float *coefs = L.coefs + (unit << 9);
  float x[8];
  if (modes == 0) {                                            // all long: coefficient order == slot order
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

  // ---- the reference's record: the word length whose e_0 the wave of that level has to keep ----
  const uint32_t *al = reinterpret_cast<const uint32_t *>(L.alloc + unit * kAllocBytes);
  const uint32_t a7 = al[7];                                   // amount index, fallback flag
  const bool ref_fallback = (a7 >> 27) & 1;
  const int ref_n = bfu_amount((int)(a7 >> 28) & 7);
  const int wl_ref = (lane < 52 && lane < ref_n && !ref_fallback) ? (int)((al[lane >> 3] >> ((lane & 7) * 4)) & 15) : 0;

  // ---- the table: level 0 in every wave, then the wave's own levels ----
  double P = 1.0;                                              // P_b; level 0 goes by unweighted
  for (int i = 0; i < 3; i++) {                                // wave-uniform: i = 0 is level 0
    const int w = i == 0 ? 0 : wave + 1 + 8 * (i - 1);
    if (w > 15) break;                                         // wave 7 has one coded level; no barrier inside this loop
    const int passes = w == 0 ? 1 : n_cand;                    // e(b, 0) has no index in it
    const double yy = T->inv_range[w];
    double best = 0.0;                                         // e'(b, w) so far, and its candidate
    int best_k = 0;
    for (int k = 0; k < passes; k++) {                         // wave-uniform
      const int sk = sfi + offset_of(offsets, k);
      const bool valid = sfi != 0 && sk >= 1 && sk <= 63;      // k = 0: offset 0, valid wherever the BFU codes anything
      const int at = valid ? sk : 0;                           // range-checked before it indexes a table
      if (lane < 52) {
        const int bits = wl_bits(w);
        const bool coded = valid && bits != 0;
        V.norm[lane] = coded ? T->norm[at * 16 + w] : 0.0;
        V.range[lane] = coded ? (1 << (bits - 1)) - 1 : 0;
        V.sf[lane] = coded ? (dq_step ? T->scale_factors[at] * yy : T->scale_factors[at]) : 0.0;
      }
      wave_fence();
#pragma unroll
      for (int m = 0; m < 8; m++) {
        const int b = slot_b[m];
        const int32_t range = V.range[b];
        const double xs = (double)x[m] * V.norm[b];
        const double v = xs + (xs >= 0 ? 0.5 : -0.5);          // round half away from zero ...
        int32_t q = (int32_t)v;                                // ... then `| 0`: truncation; exact wrap below
        if (__builtin_expect(!(fabs(v) < 2147483648.0), 0)) q = to_int32(v);
        q = q > range ? range : (q < -range ? -range : q);     // range 0 (nothing coded): 0
        const double sfv = V.sf[b];
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
        V.terms[8 * lane + m] = t * t;
      }
      wave_fence();
      if (lane < 52) {
        // four terms in flight per wait, added in ascending order all the same; a slot past the BFU's last adds +0.0, which
        // leaves a sum of squares as it is, bit for bit (my_first + 19 <= 511: the reads stay inside the block)
        double acc = 0.0;
        for (int j = 0; j < my_size; j += 4) {
          const double t0 = V.terms[my_first + j], t1 = V.terms[my_first + j + 1], t2 = V.terms[my_first + j + 2],
                       t3 = V.terms[my_first + j + 3];
          acc += t0;
          acc += j + 1 < my_size ? t1 : 0.0;
          acc += j + 2 < my_size ? t2 : 0.0;
          acc += j + 3 < my_size ? t3 : 0.0;
        }
        const double e = masked ? P * (W * acc) : W * acc;      // the finished e_k(b, w), then the weight
        if (k == 0) {
          best = e;
          if (w != 0 && w == wl_ref) S.e_ref[lane] = e;        // one wave owns the level: one writer per BFU
        } else if (valid && e < best) {                        // strictly smaller: the first candidate of least error stays
          best = e;
          best_k = k;
        }
      }
      wave_fence();                                            // the next pass rewrites the block
    }
    if (w == 0) {                                              // wave-uniform: `best` is E_b
      if (masked) {
        if (lane < 52) V.norm[lane] = best;
        wave_fence();
        double M = 0.0;
        if (has_spread) {
          const double *my_spread = mask + 52 + bl;            // the matrix transposed: consecutive doubles over the lanes for each c
#pragma unroll 4
          for (int c = 0; c < 52; c++) {
            const double prod = my_spread[52 * c] * V.norm[c];
            M += prod;
          }
        }
        const double my_floor = mask[bl];
        const double thr = M > my_floor ? M : my_floor;        // a NaN M_b falls to the floor
        P = 1.0 / thr;
        wave_fence();                                          // every lane has read the row
        best = P * best;
      }
      if (wave == 0 && lane < 52) {
        S.table[lane] = best;
        if (wl_ref == 0) S.e_ref[lane] = best;
      }
    } else if (lane < 52) {
      S.table[w * kTableStride + lane] = best;
      S.pick[w * kTableStride + lane] = (uint8_t)best_k;
    }
  }
  __syncthreads();

  // ---- the gains (row w by wave w & 7); T_ref over the reference's own indices and the unit's energy meanwhile ----
  for (int w = wave; w < 15; w += kWideWaves) {
    if (lane < 52) {
      const double e0 = S.table[w * kTableStride + lane], e1 = S.table[(w + 1) * kTableStride + lane];
      const double gain = (e0 - e1) / (double)((w == 0 ? 2 : 1) * my_size);   // cost = (bits(w + 1) - bits(w)) * size
      S.key[w * kTableStride + lane] = (sfi != 0 && gain > 0.0) ? (unsigned long long)__double_as_longlong(gain) : 0ull;
    }
  }
  if (wave == 1) {
    const double t_ref = total_in_bfu_order(S.e_ref);
    if (lane == 0) S.t_ref = t_ref;
  } else if (wave == 2) {
    const double e_unit = total_in_bfu_order(S.table);
    if (lane == 0) S.e_unit = e_unit;
  }
  __syncthreads();

  // ---- the greedy allocation: amount `wave` ----
  {
    const int n = bfu_amount(wave);
    int rem = 1696 - 40 - 10 * n;
    const bool mine = lane < n;                                // n <= 52
    int wl = 0;
    unsigned long long key = S.key[bl];
    int cost = 2 * my_size;                                    // (bits(1) - bits(0)) * size
    for (int step = 0; step < kMaxSteps; step++) {
      const bool eligible = mine && cost <= rem && key != 0ull;            // word length 15: the key is 0
      const uint32_t hi = eligible ? (uint32_t)(key >> 32) : 0u, top_hi = wave_umax32(hi);
      unsigned long long holders = __ballot(eligible && hi == top_hi);
      if (holders == 0ull) break;                              // wave-uniform
      if (holders & (holders - 1)) {                           // wave-uniform and rare: the high words tie, the low words decide
        const bool tied = eligible && hi == top_hi;
        const uint32_t lo = tied ? (uint32_t)key : 0u, top_lo = wave_umax32(lo);
        holders = __ballot(tied && lo == top_lo);
      }
      const int winner = __builtin_ctzll(holders);             // the smallest BFU on a tie
      rem -= __builtin_amdgcn_readlane(cost, winner);
      if (lane == winner) {
        wl++;
        cost = my_size;                                        // (bits(w + 1) - bits(w)) * size, w >= 1
        key = wl < 15 ? S.key[wl * kTableStride + bl] : 0ull;
      }
    }
    const double e_cur = S.table[(wl & 15) * kTableStride + bl];
    if (lane < 52) V.cur[lane] = lane < n ? e_cur : S.table[lane];
    wave_fence();
    const double t = total_in_bfu_order(V.cur);
    if (lane < 56) V.wl[lane] = (uint32_t)wl;
    if (lane == 0) S.t[wave] = t;
  }
  __syncthreads();
  if (wave != 0) return;                                       // no barrier follows

  // ---- wave 0: the first amount of least total, in amount order; all NaN: the first amount's total is reported, nothing taken ----
  double best_t = S.t[0];
  int best_a = 0;
  bool have = false;
  for (int a = 0; a < kWideWaves; a++) {
    const double t = S.t[a];
    if (t == t && (!have || t < best_t)) { best_t = t; best_a = a; have = true; }
  }
  const int best_wl = have ? (int)(S.w[best_a].wl[bl] & 15u) : 0;
  const double t_ref = S.t_ref, e_unit = S.e_unit;
  const bool take = have && best_t < t_ref;

  // the offset written for BFU `lane`: the pick of its final level where it is coded in a taken unit, else 0
  const int nb = bfu_amount(best_a);
  const bool shifted = take && lane < nb && best_wl > 0;       // nb <= 52
  const int my_offset = shifted ? offset_of(offsets, (int)(S.pick[best_wl * kTableStride + bl] & 7)) : 0;
  wave_fence();                                                // V.wl is rewritten below (best_a may be 0)

  if (!in_range) return;
  if (finalize && take) {                                      // wave-uniform: every lane holds the same totals
    // my_offset belongs to a candidate that was valid for this BFU: the index stays within 1 .. 63 (masked all the same)
    if (lane < 56) V.wl[lane] = lane < nb ? ((uint32_t)best_wl & 15u) | ((uint32_t)((sfi + my_offset) & 63) << 8)
                                          : (lane < 52 ? (uint32_t)sfi << 8 : 0u);
    wave_fence();
    if (lane < 8) {
      uint32_t word = (uint32_t)best_a << 28;
      if (lane < 7) {
        word = 0u;
#pragma unroll
        for (int k = 0; k < 8; k++) word |= (V.wl[8 * lane + k] & 15u) << (4 * k);
      }
      reinterpret_cast<uint32_t *>(L.alloc + unit * kAllocBytes)[lane] = word;
    }
    if (lane < 13) {                                           // the 52 scale-factor bytes; dword 13 (the mode byte) stays
      uint32_t word = 0u;
#pragma unroll
      for (int k = 0; k < 4; k++) word |= ((V.wl[4 * lane + k] >> 8) & 63u) << (8 * k);
      reinterpret_cast<uint32_t *>(L.side + unit * kSideBytes)[lane] = word;
    }
  }
  if (shifts && lane < 52) shifts[unit * 52 + lane] = (int8_t)my_offset;
  if (weights && lane < 52) weights[unit * 52 + lane] = P;
  if (lane == 0) {
    if (taken) taken[unit] = take ? 1 : 0;
    if (distortion) { distortion[2 * unit] = t_ref; distortion[2 * unit + 1] = best_t; }
    if (energy) energy[unit] = e_unit;
  }
}

}  // namespace

void c1k_launch_measured_wide(const C1EncodeLaunch &L, bool all_long, bool finalize, const int8_t *sf_offsets, int n_offsets,
                              const double *mask, bool has_spread, uint8_t *taken, int8_t *shifts, double *distortion, double *energy,
                              double *weights, hipStream_t stream) {
  const int64_t units = L.frames * L.channels;
  if (units <= 0) return;
  unsigned long long packed = 0ull;
  for (int k = 0; k < n_offsets && k < 8; k++) packed |= (unsigned long long)(uint8_t)sf_offsets[k] << (8 * k);
  const dim3 grid((unsigned)units), block(C1_WAVE * kWideWaves);   // a chunk holds fewer than 2^29 units
  hipLaunchKernelGGL(k_measured_wide, grid, block, 0, stream, L, all_long ? 1 : 0, finalize ? 1 : 0, packed, n_offsets, mask,
                     has_spread && mask ? 1 : 0, taken, shifts, distortion, energy, weights);
}
