// c1_k_measured_modes_masked.hip -- the mode search of c1_k_measured_modes.hip with every candidate's errors weighed by one masking
// threshold per unit and BFU (c1_encode_measured_modes_masked_device): P_b = 1 / max(floor[b], the unit's all-long energies spread by
// the caller's matrix), formed once per unit in front of the candidate loop, multiplies every finished table entry of every
// candidate.  The helpers and the unit function of c1_k_measured_modes.hip are repeated here so that its code stays as it is
#include "c1_device.h"

namespace {

// the domain of a mode byte is what blockSelectorStage writes (encoder.js:143): 0 or 2 in the low and mid fields, 0 or 3 in
// the high one.  Every candidate byte is brought into it before anything selects with its fields
__device__ __forceinline__ int mode_in_domain(int b) { return (b & 0x02) | (b & 0x08) | ((b & 0x30) == 0x30 ? 0x30 : 0); }

// =====================================================================================================
// k_measured_modes_masked : P_b once per unit; per candidate the composed unit's e'(b, w) = P_b e(b, w) and pick(b, w), T_ref over
// the candidate's trial record, the greedy allocation for every amount; T_final = taken ? T(n*) : T_ref decides between the candidates
// =====================================================================================================
// It stands where k_choose_modes stands and runs on that call's workspace: L.coefs / L.side hold the all-long analysis,
// coefs_short / side_short the all-short one, trial record k the reference's allocation under candidate k's composed side record.
// One wave per sound unit, kMmWaves independent waves per workgroup, a bounded grid whose waves stride over the units.  A lane
// owns the 8 BFU-major slots 8 lane .. 8 lane + 7 and holds their coefficient from both planes, read once as in k_choose_modes
// (the all-short plane is not read when no candidate needs it; the all-long one always is: the weights come from it); lanes 0..51
// hold their BFU's scale-factor index from both side records.  A slot's band is one value per lane (lane < 16 low, < 32 mid, else
// high), BFU `lane`'s another (lane < 20, < 36).
//   weights         (include/carta1_hip.h; k_measured_masked's under constant modes 0, bit for bit)  Every lane
//                   squares its 8 all-long coefficients in binary64 into the terms block, lane b adds BFU b's in ascending slot
//                   order into E_b, and E goes into the table's first row, which no candidate has written yet.  Lane b then adds
//                   spread[b][c] * E_c for c = 0 .. 51 in that order, each product rounded before it is added (the unit is built
//                   without contraction): E_c is a broadcast read of LDS, the matrix lies transposed in global memory
//                   (mask[52 + 52 c + b]), so the lanes read consecutive doubles for each c; a matrix the caller did not give
//                   skips the loop.  P_b = 1 / max(M_b, floor[b]) (a NaN M_b: the floor) stays in a register of lane b.  It
//                   depends neither on the candidates nor on the offsets.  Lanes 52..63 shadow BFU 51: every table read stays
//                   inside the 52 + 52 * 52 doubles.
//   per candidate   x[m] and s0 are selected by the candidate's mode of the band; from there on the arithmetic is k_measured_sf's
//                   statement by statement -- the table pass per (word length, offset), lane b's sum in ascending slot order
//                   times W_b, then times P_b, the strictly-smaller rule for pick, e_0 at the trial record's word length for T_ref, the gains
//                   and their keys, the totals in BFU order, the eight greedy amounts -- so with P_b = 1 T_ref, T(n*), taken, the energy
//                   and the record are bit for bit what c1_encode_measured_sf_* gives under that constant byte.  The table is
//                   rebuilt per candidate in the one LDS block of k_measured_sf (13.5 KB a wave): a long and a short table side
//                   by side would save six of eight table phases, about 7 % of a candidate's time, and cost the latency-bound
//                   greedy two of its three waves per SIMD.
//   choice          the smallest candidate whose T_final no other's is below; a NaN never wins, all NaN selects candidate 0.
//                   A lane keeps the best candidate's word length, offset and index (its BFU's), the amount and `taken`.
//   winner          as k_choose_modes hands it on, with k_measured_sf's records: lanes 0..7 write the allocation record (the
//                   greedy's when taken, else trial record `choice`), lanes 0..15 the side record (the composed indices, moved
//                   by the chosen offsets when taken; the mode byte; padding), and a lane whose band the winner codes short
//                   copies its 8 coefficients of the all-short plane over the all-long plane's.  The lane id is re-derived
//                   through lane_for_this_frame (c1_device.h) for this block: its addresses are then formed per unit, not kept
//                   across the whole unit loop, which with P_b live left one register too few for 3 waves per SIMD (170 VGPRs
//                   or 8 bytes of scratch without, 158 with; k_measured_modes: 159).
// Any bytes in the side and trial records and any candidate bytes are memory-safe here: indices are masked (sfi & 63, wl & 15,
// amount & 7), s0 + offset is range-checked before it indexes a table, a candidate byte passes mode_in_domain first, and the only
// loop bounds that are not constants are n_cand (1 .. C1_MAX_MODE_CANDIDATES, clamped) and n_offsets (1 .. 8, clamped).
constexpr int kMmWaves = 4;
constexpr int kMmBlocks = 2048;          // as the choose kernels: past 8 192 units the waves stride
constexpr int kTableStride = 52;         // doubles between the rows (word lengths) of the tables
constexpr int kMaxSteps = 52 * 15;

struct C1ModeCandidates {
  uint8_t byte[C1_MAX_MODE_CANDIDATES];
};

struct alignas(16) MeasuredModesLds {   // k_measured_sf's block
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
__device__ __forceinline__ double total_in_bfu_order(const MeasuredModesLds &S) {
  double t = 0.0;
#pragma unroll 4
  for (int b = 0; b < 52; b++) t += S.cur[b];
  return t;
}

// offset k: the eight signed bytes travel in one 64-bit kernel argument, byte k = sf_offsets[k]
__device__ __forceinline__ int offset_of(unsigned long long packed, int k) { return (int)(int8_t)(packed >> (8 * (k & 7))); }

__global__ __launch_bounds__(C1_WAVE * kMmWaves) void k_measured_modes_masked(
    C1EncodeLaunch L, const float *__restrict__ coefs_short, const uint8_t *__restrict__ side_short, const uint8_t *__restrict__ trial,
    int64_t trial_stride, C1ModeCandidates cand, int n_cand_arg, int has_long, int has_short, int finalize, unsigned long long offsets,
    int n_offsets_arg, const double *__restrict__ mask, int has_spread, uint8_t *__restrict__ choice, uint8_t *__restrict__ modes_out,
    uint8_t *__restrict__ taken, int8_t *__restrict__ shifts, double *__restrict__ distortion, double *__restrict__ energy,
    double *__restrict__ weights) {
  __shared__ MeasuredModesLds lds[kMmWaves];
  TablesPtr T = C1_TABLES(L.tables);
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  MeasuredModesLds &S = lds[wave];
  int slot_b[8];
#pragma unroll
  for (int m = 0; m < 8; m++) slot_b[m] = bfu_of_slot(8 * lane + m);
  const int band_shift = lane < 16 ? 0 : (lane < 32 ? 2 : 4);                 // the lane's slots (and its 8 coefficients)
  const int bl = lane < 52 ? lane : 51;                        // lanes 52..63 shadow BFU 51 and never take part
  const int my_first = kBfuFirst[bl], my_size = kSpecs[bl];
  const int bfu_shift = bl < 20 ? 0 : (bl < 36 ? 2 : 4);
  const double w_short = bl < 36 ? 0.25 : 0.5;
  const int dq_step = T->dq_step, dq_fast = T->dq_fast;
  const int n_cand = n_cand_arg < 1 ? 1 : (n_cand_arg > C1_MAX_MODE_CANDIDATES ? C1_MAX_MODE_CANDIDATES : n_cand_arg);
  const int n_off = n_offsets_arg < 1 ? 1 : (n_offsets_arg > 8 ? 8 : n_offsets_arg);
  const int64_t units_total = L.frames * L.channels;
  const int64_t stride = (int64_t)gridDim.x * kMmWaves;
  for (int64_t unit = (int64_t)blockIdx.x * kMmWaves + wave; unit < units_total; unit += stride) {
    // ---- both analyses of the unit, once ----
    int sfi_long = 0, sfi_short = 0;
    float xl[8], xs[8];
#pragma unroll
    for (int m = 0; m < 8; m++) xl[m] = xs[m] = 0.0f;
    {                                                          // the all-long coefficients always: the weights come from them
      const float4 *c4 = reinterpret_cast<const float4 *>(L.coefs + (unit << 9));
      const float4 a = c4[2 * lane], c = c4[2 * lane + 1];
      xl[0] = a.x; xl[1] = a.y; xl[2] = a.z; xl[3] = a.w; xl[4] = c.x; xl[5] = c.y; xl[6] = c.z; xl[7] = c.w;
    }
    if (has_long) {
      const uint32_t *side = reinterpret_cast<const uint32_t *>(L.side + unit * kSideBytes);
      if (lane < 52) sfi_long = (int)((side[lane >> 2] >> ((lane & 3) * 8)) & 63);
    }
    if (has_short) {
      const uint32_t *side = reinterpret_cast<const uint32_t *>(side_short + unit * kSideBytes);
      if (lane < 52) sfi_short = (int)((side[lane >> 2] >> ((lane & 3) * 8)) & 63);
      const float *cs = coefs_short + (unit << 9);
#pragma unroll
      for (int m = 0; m < 8; m++) {
        const int p = 8 * lane + m;
        xs[m] = cs[kStartShort[slot_b[m]] + (p - kBfuFirst[slot_b[m]])];
      }
    }
    // ---- the weights: E_b over the all-long coefficients into the table's first row, M_b, P_b ----
#pragma unroll
    for (int m = 0; m < 8; m++) {
      const double t = (double)xl[m];
      S.terms[8 * lane + m] = t * t;
    }
    wave_fence();
    if (lane < 52) {
      double acc = 0.0;                                        // ascending slot order, as every table row below
      for (int j = 0; j < my_size; j += 4) {
        const double t0 = S.terms[my_first + j], t1 = S.terms[my_first + j + 1], t2 = S.terms[my_first + j + 2],
                     t3 = S.terms[my_first + j + 3];
        acc += t0;
        acc += j + 1 < my_size ? t1 : 0.0;
        acc += j + 2 < my_size ? t2 : 0.0;
        acc += j + 3 < my_size ? t3 : 0.0;
      }
      S.table[lane] = acc;                                     // W = 1
    }
    wave_fence();
    double M = 0.0;
    if (has_spread) {                                          // wave-uniform (a kernel argument)
#pragma unroll 4
      for (int c = 0; c < 52; c++) {                           // the transposed matrix follows the floor
        const double prod = mask[52u * (unsigned)(c + 1) + (unsigned)bl] * S.table[c];
        M += prod;
      }
    }
    const double my_floor = mask[(unsigned)bl];                // floor[b], read per unit
    const double thr = M > my_floor ? M : my_floor;             // a NaN M_b falls to the floor
    const double P = 1.0 / thr;
    if (weights && lane < 52) weights[unit * 52 + lane] = P;
    wave_fence();                                              // every lane has read the row; the first candidate rewrites the block

    // ---- the best candidate so far: the final error, and what lane b has to write for its BFU ----
    double win_t = 0.0;
    int win_k = 0, win_wl = 0, win_a = 0, win_offset = 0, win_sfi = 0;
    bool win_take = false, have_win = false;

    for (int kc = 0; kc < n_cand; kc++) {                      // wave-uniform (a kernel argument)
      const int modes = mode_in_domain(cand.byte[kc]);
      const bool lane_short = ((modes >> band_shift) & 3) != 0;
      const bool bfu_short = ((modes >> bfu_shift) & 3) != 0;
      float x[8];
#pragma unroll
      for (int m = 0; m < 8; m++) x[m] = lane_short ? xs[m] : xl[m];
      const int sfi = lane < 52 ? (bfu_short ? sfi_short : sfi_long) : 0;
      const double W = bfu_short ? w_short : 1.0;              // BFU `lane`'s weight

      // ---- the reference's record under this candidate: the word length whose e_0 lane b has to keep ----
      const uint32_t *al = reinterpret_cast<const uint32_t *>(trial + (int64_t)kc * trial_stride + unit * kAllocBytes);
      const uint32_t a7 = al[7];                               // amount index, fallback flag
      const bool ref_fallback = (a7 >> 27) & 1;
      const int ref_n = bfu_amount((int)(a7 >> 28) & 7);
      const int wl_ref = (lane < 52 && lane < ref_n && !ref_fallback) ? (int)((al[lane >> 3] >> ((lane & 7) * 4)) & 15) : 0;

      // ---- the table ----
      unsigned long long pick = 0ull;                          // 3 bits per coded level: offset index of e(b, w) at bits 3 (w - 1) ..
      double e_ref = 0.0;                                      // e_0(b, wl_ref)
      for (int w = 0; w < 16; w++) {                           // wave-uniform
        const int passes = w == 0 ? 1 : n_off;                 // e(b, 0) has no index in it
        const double yy = T->inv_range[w];
        for (int k = 0; k < passes; k++) {                     // wave-uniform
          const int sk = sfi + offset_of(offsets, k);
          const bool valid = sfi != 0 && sk >= 1 && sk <= 63;  // k = 0: offset 0, valid wherever the BFU codes anything
          const int at = valid ? sk : 0;                       // range-checked before it indexes a table
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
            const double xn = (double)x[m] * S.norm[b];
            const double v = xn + (xn >= 0 ? 0.5 : -0.5);      // round half away from zero ...
            int32_t q = (int32_t)v;                            // ... then `| 0`: truncation; exact wrap below
            if (__builtin_expect(!(fabs(v) < 2147483648.0), 0)) q = to_int32(v);
            q = q > range ? range : (q < -range ? -range : q); // range 0 (nothing coded): 0
            const double sfv = S.sf[b];
            float d;
            if (range == 0) d = 0.0f;
            else if (dq_step) d = f32((double)q * sfv);        // == Float32((q * SF) / range) for every input (checked on the host)
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
            const double e = P * (W * acc);                    // the finished e_k(b, w), then the weight
            if (k == 0) {
              S.table[w * kTableStride + lane] = e;
              if (w == wl_ref) e_ref = e;
            } else if (valid && e < S.table[w * kTableStride + lane]) {   // strictly smaller: the first offset of least error stays
              S.table[w * kTableStride + lane] = e;
              const int sh = 3 * (w - 1);
              pick = (pick & ~(7ull << sh)) | ((unsigned long long)k << sh);
            }
          }
          wave_fence();                                        // the next pass rewrites the block
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
      for (int a = 0; a < 8; a++) {                            // wave-uniform
        const int n = bfu_amount(a);
        int rem = 1696 - 40 - 10 * n;
        const bool mine = lane < n;                             // n <= 52
        int wl = 0;
        unsigned long long key = S.key[bl];
        int cost = 2 * my_size;                                // (bits(1) - bits(0)) * size
        for (int step = 0; step < kMaxSteps; step++) {
          const bool eligible = mine && cost <= rem && key != 0ull;          // word length 15: the key is 0
          const uint32_t hi = eligible ? (uint32_t)(key >> 32) : 0u, top_hi = wave_umax32(hi);
          unsigned long long holders = __ballot(eligible && hi == top_hi);
          if (holders == 0ull) break;                          // wave-uniform
          if (holders & (holders - 1)) {                       // wave-uniform and rare: the high words tie, the low words decide
            const bool tied = eligible && hi == top_hi;
            const uint32_t lo = tied ? (uint32_t)key : 0u, top_lo = wave_umax32(lo);
            holders = __ballot(tied && lo == top_lo);
          }
          const int winner = __builtin_ctzll(holders);         // the smallest BFU on a tie
          rem -= __builtin_amdgcn_readlane(cost, winner);
          if (lane == winner) {
            wl++;
            cost = my_size;                                    // (bits(w + 1) - bits(w)) * size, w >= 1
            key = wl < 15 ? S.key[wl * kTableStride + bl] : 0ull;
          }
        }
        const double e_cur = S.table[wl * kTableStride + bl];
        if (lane < 52) S.cur[lane] = lane < n ? e_cur : S.table[lane];
        wave_fence();
        const double t = total_in_bfu_order(S);
        wave_fence();
        if (a == 0) best_t = t;                                // all NaN: the first amount's total is reported, and nothing is taken
        if (t == t && (!have || t < best_t)) { best_t = t; best_wl = wl; best_a = a; have = true; }
      }
      const bool take = have && best_t < t_ref;

      // the offset written for BFU `lane`: the pick of its final level where it is coded in a taken unit, else 0
      const int nb = bfu_amount(best_a);
      const bool shifted = take && lane < nb && best_wl > 0;   // nb <= 52
      const int my_offset = shifted ? offset_of(offsets, (int)((pick >> (3 * ((best_wl > 0 ? best_wl : 1) - 1))) & 7)) : 0;

      if (lane == 0) {
        if (distortion) { distortion[(unit * n_cand + kc) * 2] = t_ref; distortion[(unit * n_cand + kc) * 2 + 1] = best_t; }
        if (energy) energy[unit * n_cand + kc] = e_unit;
      }

      // ---- the candidate of least final error so far (wave-uniform: every lane holds the same totals) ----
      const double t_final = take ? best_t : t_ref;
      if (kc == 0 || (t_final == t_final && (!have_win || t_final < win_t))) {
        win_t = t_final; win_k = kc; win_take = take; win_wl = best_wl; win_a = best_a; win_offset = my_offset; win_sfi = sfi;
        have_win = t_final == t_final;
      }
      wave_fence();                                            // the next candidate rewrites the block
    }

    const int win = mode_in_domain(cand.byte[win_k]);
    if (finalize) {
      // the lane id once more, opaque to the compiler: the addresses below are formed here, per unit, not kept in registers across
      // the whole unit loop (c1_device.h)
      const int fl = lane_for_this_frame(lane);
      // what k_measured_sf leaves of a taken unit and the plain chain of any other, in the layout k_choose_modes hands to packing.
      // win_offset belongs to an offset that was valid for this BFU: the index stays within 1 .. 63 (masked all the same)
      const int nb = bfu_amount(win_a);
      if (fl < 56) S.wl[fl] = fl < 52 ? ((win_take && fl < nb) ? ((uint32_t)win_wl & 15u) : 0u) | ((uint32_t)((win_sfi + win_offset) & 63) << 8) : 0u;
      wave_fence();
      if (fl < 8) {
        uint32_t word;
        if (win_take) {
          word = (uint32_t)win_a << 28;
          if (fl < 7) {
            word = 0u;
#pragma unroll
            for (int k = 0; k < 8; k++) word |= (S.wl[8 * fl + k] & 15u) << (4 * k);
          }
        } else word = reinterpret_cast<const uint32_t *>(trial + (int64_t)win_k * trial_stride + unit * kAllocBytes)[fl];
        reinterpret_cast<uint32_t *>(L.alloc + unit * kAllocBytes)[fl] = word;
      }
      if (fl < 16) {                                         // the 52 scale-factor bytes, the mode byte where k_mdct_bands keeps it, padding
        uint32_t word = fl == 13 ? (uint32_t)win : 0u;
        if (fl < 13) {
#pragma unroll
          for (int k = 0; k < 4; k++) word |= ((S.wl[4 * fl + k] >> 8) & 63u) << (8 * k);
        }
        reinterpret_cast<uint32_t *>(L.side + unit * kSideBytes)[fl] = word;
      }
      if ((win >> band_shift) & 3) {                           // a lane overwrites only the 8 long coefficients it loaded itself
        const float4 *src = reinterpret_cast<const float4 *>(coefs_short + (unit << 9));
        float4 *dst = reinterpret_cast<float4 *>(L.coefs + (unit << 9));
        const float4 a = src[2 * fl], c = src[2 * fl + 1];
        dst[2 * fl] = a;
        dst[2 * fl + 1] = c;
      }
      wave_fence();                                            // the next unit rewrites the block
    }
    if (shifts && lane < 52) shifts[unit * 52 + lane] = (int8_t)win_offset;
    if (lane == 0) {
      if (choice) choice[unit] = (uint8_t)win_k;
      if (modes_out) modes_out[unit] = (uint8_t)win;
      if (taken) taken[unit] = win_take ? 1 : 0;
    }
  }
}

}  // namespace

void c1k_launch_measured_modes_masked(const C1EncodeLaunch &L, const float *coefs_short, const uint8_t *side_short, const uint8_t *trial,
                                      int64_t trial_stride, const uint8_t *cand, int n_cand, const int8_t *sf_offsets, int n_offsets,
                                      const double *mask, bool has_spread, bool finalize, uint8_t *choice, uint8_t *modes_out,
                                      uint8_t *taken, int8_t *shifts, double *distortion, double *energy, double *weights,
                                      hipStream_t stream) {
  const int64_t units = L.frames * L.channels;
  if (units <= 0 || n_cand <= 0 || n_cand > C1_MAX_MODE_CANDIDATES || n_offsets <= 0 || n_offsets > 8 || !mask) return;
  C1ModeCandidates c;
  int has_long = 0, has_short = 0;
  for (int k = 0; k < C1_MAX_MODE_CANDIDATES; k++) {
    c.byte[k] = k < n_cand ? cand[k] : 0;
    if (k >= n_cand) continue;
    if ((cand[k] & 0x3f) != 0x3a) has_long = 1;               // some band long (bytes are in the domain here)
    if ((cand[k] & 0x3f) != 0) has_short = 1;
  }
  unsigned long long packed = 0ull;
  for (int k = 0; k < n_offsets; k++) packed |= (unsigned long long)(uint8_t)sf_offsets[k] << (8 * k);
  const dim3 grid((unsigned)std::min<int64_t>(kMmBlocks, (units + kMmWaves - 1) / kMmWaves)), block(C1_WAVE * kMmWaves);
  hipLaunchKernelGGL(k_measured_modes_masked, grid, block, 0, stream, L, coefs_short, side_short, trial, trial_stride, c, n_cand, has_long,
                     has_short, finalize ? 1 : 0, packed, n_offsets, mask, has_spread ? 1 : 0, choice, modes_out, taken, shifts, distortion,
                     energy, weights);
}
