// c1_k_measured_sf.hip -- the measured allocation with the scale-factor index of every BFU chosen by the same error
// (c1_encode_measured_sf_device): k_measured_alloc's table, greedy and fallback, over the least error of up to eight candidate
// indices findScaleFactor + offset per (BFU, word length), and the chosen indices written into the unit's side record
#include "c1_device.h"

namespace {

// the domain of a mode byte is what blockSelectorStage writes (encoder.js:143): 0 or 2 in the low and mid fields, 0 or 3 in
// the high one.  Every mode byte is brought into it before anything selects with its fields.  The byte read here is the
// analysis' own, and under fixedBlockModes such as [1,1,1] or [2,2,1] its fields are the option's: a field that is not zero
// means short blocks (quantization.js:117 and the MDCT test blockMode === 0), as the packing kernels read it
__device__ __forceinline__ int mode_in_domain(int b) { return ((b & 0x03) ? 0x02 : 0) | ((b & 0x0c) ? 0x08 : 0) | ((b & 0x30) ? 0x30 : 0); }

// =====================================================================================================
// k_measured_sf : e(b, w) = min_k e_k(b, w) and pick(b, w), the greedy allocation for every amount, the fallback
// =====================================================================================================
// k_measured_alloc's shape (c1_k_measured.hip): one wave per sound unit, kSfWaves independent waves per workgroup, a bounded grid
// whose waves stride over the units, the same LDS block.  The definition (include/carta1_hip.h) in the kernel's
// terms, where it differs from that kernel's:
//   table     Per coded word length w = 1 .. 15 and per candidate k (both wave-uniform) lanes 0..51 put what their BFU needs at
//             index s0 + offset[k] into the wave's LDS block, every lane quantizes and dequantizes its 8 slots and lane b adds
//             BFU b's terms in ascending slot order.  Candidate 0 (offset 0) stores e_0(b, w); a later candidate replaces the
//             entry only when its index lies in 1 .. 63 and its error is strictly smaller.  A candidate whose index is out of
//             range is not branched around: its lanes' BFU quantizes with a range of 0 like a BFU that codes nothing, and lane b
//             leaves the entry alone.  pick(b, w), 3 bits per level, lives in a 64-bit register of lane b, not in LDS.  Lane b
//             reads its terms four per wait and adds them in ascending order (2.5 ms a pass on 2^21 units with one read per
//             wait, 2.2 ms so).
//   T_ref     The minimum table no longer holds e_0(b, wl_ref[b]): lane b keeps it as candidate 0 goes by that level.
//   gains, greedy, totals: k_measured_alloc's, unchanged.
//   records   When the call packs and the unit is taken, the allocation record is replaced as there, and the 52 scale-factor
//             bytes of the side record are rewritten with s0 + offset[pick(b, wl[b])] where b < nBfu and wl[b] > 0, s0
//             elsewhere; the mode byte behind them is not touched.  The packing kernels read both.
// Any bytes in the side and allocation records are memory-safe here: indices are masked (sfi & 63, wl & 15, amount & 7), and
// s0 + offset is range-checked before it indexes a table.
constexpr int kSfWaves = 4;
constexpr int kSfBlocks = 2048;          // as the choose kernels: past 8 192 units the waves stride
constexpr int kTableStride = 52;         // doubles between the rows (word lengths) of the tables
constexpr int kMaxSteps = 52 * 15;

struct alignas(16) MeasuredSfLds {
  double table[16 * kTableStride];   // e(b, w) at [w * kTableStride + b]
  union {
    struct {                         // while the table is built
      double terms[512];             // one pass' squared differences, BFU-major slot order
      double norm[52];               // quantRange / SCALE_FACTORS[sfi]; 0 when the BFU codes nothing
      double sf[52];                 // dq_step: SCALE_FACTORS[sfi] * RN(1 / range); else SCALE_FACTORS[sfi]
      int32_t range[52];             // 2^(bits - 1) - 1; 0 when the BFU codes nothing
    };
    struct {                         // after it
      unsigned long long key[15 * kTableStride];   // the gain of raising BFU b from w at [w * kTableStride + b], as an ordered key
      double cur[52];                // the BFUs' errors under one allocation, for the total
      uint32_t wl[56];               // the winner's word lengths (bits 0-3) and written scale-factor indices (bits 8-13)
    };
  };
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

// the 52 errors in S.cur added in BFU order; every lane reads the same addresses and ends with the same bits
__device__ __forceinline__ double total_in_bfu_order(const MeasuredSfLds &S) {
  double t = 0.0;
#pragma unroll 4
  for (int b = 0; b < 52; b++) t += S.cur[b];
  return t;
}

// candidate k's offset: the eight signed bytes travel in one 64-bit kernel argument, byte k = sf_offsets[k]
__device__ __forceinline__ int offset_of(unsigned long long packed, int k) { return (int)(int8_t)(packed >> (8 * (k & 7))); }

__global__ __launch_bounds__(C1_WAVE * kSfWaves) void k_measured_sf(C1EncodeLaunch L, int all_long, int finalize, unsigned long long offsets,
                                                                    int n_offsets, uint8_t *__restrict__ taken, int8_t *__restrict__ shifts,
                                                                    double *__restrict__ distortion, double *__restrict__ energy) {
  __shared__ MeasuredSfLds lds[kSfWaves];
  TablesPtr T = C1_TABLES(L.tables);
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  MeasuredSfLds &S = lds[wave];
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
  const int64_t units_total = L.frames * L.channels;
  const int64_t stride = (int64_t)gridDim.x * kSfWaves;
  for (int64_t unit = (int64_t)blockIdx.x * kSfWaves + wave; unit < units_total; unit += stride) {
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

    // ---- the reference's record: the word length whose e_0 lane b has to keep ----
    const uint32_t *al = reinterpret_cast<const uint32_t *>(L.alloc + unit * kAllocBytes);
    const uint32_t a7 = al[7];                                 // amount index, fallback flag
    const bool ref_fallback = (a7 >> 27) & 1;
    const int ref_n = bfu_amount((int)(a7 >> 28) & 7);
    const int wl_ref = (lane < 52 && lane < ref_n && !ref_fallback) ? (int)((al[lane >> 3] >> ((lane & 7) * 4)) & 15) : 0;

    // ---- the table ----
    unsigned long long pick = 0ull;                            // 3 bits per coded level: candidate of e(b, w) at bits 3 (w - 1) ..
    double e_ref = 0.0;                                        // e_0(b, wl_ref)
    for (int w = 0; w < 16; w++) {                             // wave-uniform
      const int passes = w == 0 ? 1 : n_cand;                  // e(b, 0) has no index in it
      const double yy = T->inv_range[w];
      for (int k = 0; k < passes; k++) {                       // wave-uniform
        const int sk = sfi + offset_of(offsets, k);
        const bool valid = sfi != 0 && sk >= 1 && sk <= 63;    // k = 0: offset 0, valid wherever the BFU codes anything
        const int at = valid ? sk : 0;                         // range-checked before it indexes a table
        if (lane < 52) {
          const int bits = wl_bits(w);
          const bool coded = valid && bits != 0;
          S.norm[lane] = coded ? T->norm[at * 16 + w] : 0.0;
          S.range[lane] = coded ? (1 << (bits - 1)) - 1 : 0;
          S.sf[lane] = coded ? (dq_step ? T->scale_factors[at] * yy : T->scale_factors[at]) : 0.0;
        }
        wave_fence();
#pragma unroll
        for (int m = 0; m < 8; m++) {
          const int b = slot_b[m];
          const int32_t range = S.range[b];
          const double xs = (double)x[m] * S.norm[b];
          const double v = xs + (xs >= 0 ? 0.5 : -0.5);        // round half away from zero ...
          int32_t q = (int32_t)v;                              // ... then `| 0`: truncation; exact wrap below
          if (__builtin_expect(!(fabs(v) < 2147483648.0), 0)) q = to_int32(v);
          q = q > range ? range : (q < -range ? -range : q);   // range 0 (nothing coded): 0
          const double sfv = S.sf[b];
          float d;
          if (range == 0) d = 0.0f;
          else if (dq_step) d = f32((double)q * sfv);          // == Float32((q * SF) / range) for every input (checked on the host)
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
          // four terms in flight per wait, added in ascending order all the same; a slot past the BFU's last adds +0.0, which
          // leaves a sum of squares as it is, bit for bit (my_first + 19 <= 511: the reads stay inside the block)
          double acc = 0.0;
          for (int j = 0; j < my_size; j += 4) {
            const double t0 = S.terms[my_first + j], t1 = S.terms[my_first + j + 1], t2 = S.terms[my_first + j + 2],
                         t3 = S.terms[my_first + j + 3];
            acc += t0;
            acc += j + 1 < my_size ? t1 : 0.0;
            acc += j + 2 < my_size ? t2 : 0.0;
            acc += j + 3 < my_size ? t3 : 0.0;
          }
          const double e = W * acc;
          if (k == 0) {
            S.table[w * kTableStride + lane] = e;
            if (w == wl_ref) e_ref = e;
          } else if (valid && e < S.table[w * kTableStride + lane]) {   // strictly smaller: the first candidate of least error stays
            S.table[w * kTableStride + lane] = e;
            const int sh = 3 * (w - 1);
            pick = (pick & ~(7ull << sh)) | ((unsigned long long)k << sh);
          }
        }
        wave_fence();                                          // the next pass rewrites the block
      }
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

    // ---- T_ref over the reference's own indices, the unit's energy ----
    if (lane < 52) S.cur[lane] = e_ref;
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

    // the offset written for BFU `lane`: the pick of its final level where it is coded in a taken unit, else 0
    const int nb = bfu_amount(best_a);
    const bool shifted = take && lane < nb && best_wl > 0;     // nb <= 52
    const int my_offset = shifted ? offset_of(offsets, (int)((pick >> (3 * ((best_wl > 0 ? best_wl : 1) - 1))) & 7)) : 0;

    if (finalize && take) {                                    // wave-uniform: every lane holds the same totals
      // my_offset belongs to a candidate that was valid for this BFU: the index stays within 1 .. 63 (masked all the same)
      if (lane < 56) S.wl[lane] = lane < nb ? ((uint32_t)best_wl & 15u) | ((uint32_t)((sfi + my_offset) & 63) << 8)
                                            : (lane < 52 ? (uint32_t)sfi << 8 : 0u);
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
      if (lane < 13) {                                         // the 52 scale-factor bytes; dword 13 (the mode byte) stays
        uint32_t word = 0u;
#pragma unroll
        for (int k = 0; k < 4; k++) word |= ((S.wl[4 * lane + k] >> 8) & 63u) << (8 * k);
        reinterpret_cast<uint32_t *>(L.side + unit * kSideBytes)[lane] = word;
      }
      wave_fence();
    }
    if (shifts && lane < 52) shifts[unit * 52 + lane] = (int8_t)my_offset;
    if (lane == 0) {
      if (taken) taken[unit] = take ? 1 : 0;
      if (distortion) { distortion[2 * unit] = t_ref; distortion[2 * unit + 1] = best_t; }
      if (energy) energy[unit] = e_unit;
    }
  }
}

}  // namespace

void c1k_launch_measured_sf(const C1EncodeLaunch &L, bool all_long, bool finalize, const int8_t *sf_offsets, int n_offsets, uint8_t *taken,
                            int8_t *shifts, double *distortion, double *energy, hipStream_t stream) {
  const int64_t units = L.frames * L.channels;
  if (units <= 0) return;
  unsigned long long packed = 0ull;
  for (int k = 0; k < n_offsets && k < 8; k++) packed |= (unsigned long long)(uint8_t)sf_offsets[k] << (8 * k);
  const dim3 grid((unsigned)std::min<int64_t>(kSfBlocks, (units + kSfWaves - 1) / kSfWaves)), block(C1_WAVE * kSfWaves);
  hipLaunchKernelGGL(k_measured_sf, grid, block, 0, stream, L, all_long ? 1 : 0, finalize ? 1 : 0, packed, n_offsets, taken, shifts,
                     distortion, energy);
}
