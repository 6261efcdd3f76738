// c1_k_measured_modes_masked_wide.hip -- the weighted mode search of c1_k_measured_modes_masked.hip for a launch of few units (a
// streaming push, a frame closure): a workgroup of eight waves per unit instead of one wave, as c1_k_measured_modes_wide.hip is to
// c1_k_measured_modes.hip.  Both planes of tables are multiplied by the unit's one weight per BFU.  Every output is bit for bit what
// k_measured_modes_masked gives: no floating-point operation is reordered or fused, only handed to another wave
#include "c1_device.h"

namespace {

// the domain of a mode byte is what blockSelectorStage writes (encoder.js:143): 0 or 2 in the low and mid fields, 0 or 3 in
// the high one.  Every candidate byte is brought into it before anything selects with its fields
__device__ __forceinline__ int mode_in_domain(int b) { return (b & 0x02) | (b & 0x08) | ((b & 0x30) == 0x30 ? 0x30 : 0); }

// =====================================================================================================
// k_measured_modes_masked_wide : k_measured_modes_masked's unit function, a workgroup per unit
// =====================================================================================================
// The helpers and the structure of c1_k_measured_modes_wide.hip are repeated here so that its code stays as it is; the arguments
// and the workspace are k_measured_modes_masked's, the definition is include/carta1_hip.h's.  A BFU's e(b, w) and pick(b, w) depend on the
// candidate only through the mode of the BFU's own band (its coefficients, its scale-factor index and its weight W_b all follow
// that one field), so two planes of tables serve every candidate: plane 0 from the all-long analysis with W = 1, plane 1 from the
// all-short one with W = w_short, both times P_b.  In the kernel's terms, where it differs from k_measured_modes_masked:
//   weights   Every wave forms E, M and P for itself, in its own terms and cur rows, with that kernel's statements: 52 lanes, 8
//             squares, at most 20 additions and 52 products, about a fifth of one table row of five offsets, and no fourth barrier
//             in front of the tables (one wave working in front of a barrier would leave seven waiting for the same time).  The
//             all-long coefficients are always read.
//   table     The 2 x 16 rows are dealt over the waves (wave v: rows v, v + 8 of plane 0, then of plane 1), each wave in a norm /
//             range / sf / terms block of its own; the rows of a plane no candidate needs are skipped.  All offsets of one
//             (plane, b, w) stay in one wave, in offset order, with the strictly-smaller rule.  pick goes to LDS, a byte per
//             entry.  A lane carries the trial word length of its BFU under every candidate (4 bits each) and which plane each
//             candidate selects for it (a bit each): the wave that owns (plane, w) leaves e_0 for every candidate that selects the
//             plane and whose trial record has w there.  Barrier.
//   gains     The 2 x 15 rows of the keys, one row per wave in turn; wave v adds T_ref and the energy of candidate v in BFU
//             order over the composed rows meanwhile.  Barrier.
//   greedy    Wave v runs amount (v + k) & 7 for candidate k = 0 .. n_cand - 1: every wave gets each amount once per eight
//             candidates, so the 52-BFU chain is not one wave's alone.  The key and the table entry of BFU b under candidate k
//             are those of the plane k's mode of b's band selects; the step is k_measured_modes' unchanged.  A chain writes only
//             its own T(k, a) and 52 word lengths: no barrier between the candidates.  Barrier.
//   the rest  Wave 0 walks the candidates in order with that kernel's statements (the first amount of least non-NaN T, take,
//             T_final, the first least T_final; a NaN never wins, all NaN selects candidate 0), then its finalisation and stores.
// Every barrier is outside any branch and outside any loop: all eight waves reach each of the three, and a workgroup past the unit
// count (none is launched) would reach them on the last unit and store nothing.  Any bytes in the side and trial records and any
// candidate bytes are memory-safe here: indices are masked (sfi & 63, wl & 15, amount & 7), s0 + offset is range-checked before it
// indexes a table, a candidate byte passes mode_in_domain first, and the only loop bounds that are not constants are n_cand (1 ..
// C1_MAX_MODE_CANDIDATES, clamped) and n_offsets (1 .. 8, clamped).  The grid is the unit count: no wave strides
constexpr int kWideWaves = 8;
constexpr int kMaxCand = C1_MAX_MODE_CANDIDATES;
constexpr int kTableStride = 52;         // doubles between the rows (word lengths) of the tables
constexpr int kPlaneTable = 16 * kTableStride, kPlaneKey = 15 * kTableStride;
constexpr int kMaxSteps = 52 * 15;
static_assert(kMaxCand == 8, "a lane keeps 8 trial word lengths in 32 bits, and a wave owns one candidate's totals");

struct C1ModeCandidates {
  uint8_t byte[C1_MAX_MODE_CANDIDATES];
};

struct alignas(16) ModesWideWaveLds {  // a wave's own block
  double terms[512];                   // one pass' squared differences, BFU-major slot order
  double norm[52];                     // quantRange / SCALE_FACTORS[sfi]; 0 when the BFU codes nothing
  double sf[52];                       // dq_step: SCALE_FACTORS[sfi] * RN(1 / range); else SCALE_FACTORS[sfi]
  double cur[52];                      // the BFUs' errors under one allocation, for the total
  int32_t range[52];                   // 2^(bits - 1) - 1; 0 when the BFU codes nothing
};

struct alignas(16) ModesWideLds {      // 80 160 bytes: two workgroups per CU
  double table[2 * kPlaneTable];                 // e(b, w) of plane p at [p * kPlaneTable + w * kTableStride + b]
  unsigned long long key[2 * kPlaneKey];         // the gain of raising BFU b from w, as an ordered key, at [p * kPlaneKey + w * kTableStride + b]
  double e_ref[kMaxCand * 52];                   // e_0(b, wl_ref_k[b]) at [k * 52 + b]
  double t[kMaxCand * kWideWaves];               // T(k, a) at [k * 8 + a]
  double t_ref[kMaxCand], e_unit[kMaxCand];
  uint32_t win[56];                              // the winner's word lengths (bits 0-3) and written scale-factor indices (bits 8-13)
  uint8_t pick[2 * kPlaneTable];                 // the offset index of e(b, w)
  uint8_t wl[kMaxCand * kWideWaves * 64];        // chain (k, a)'s word lengths at [(k * 8 + a) * 64 + b]
  ModesWideWaveLds w[kWideWaves];
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

// offset k: the eight signed bytes travel in one 64-bit kernel argument, byte k = sf_offsets[k]
__device__ __forceinline__ int offset_of(unsigned long long packed, int k) { return (int)(int8_t)(packed >> (8 * (k & 7))); }

__global__ __launch_bounds__(C1_WAVE * kWideWaves) void k_measured_modes_masked_wide(
    C1EncodeLaunch L, const float *__restrict__ coefs_short, const uint8_t *__restrict__ side_short, const uint8_t *__restrict__ trial,
    int64_t trial_stride, C1ModeCandidates cand, int n_cand_arg, int has_long, int has_short, int finalize, unsigned long long offsets,
    int n_offsets_arg, const double *__restrict__ mask, int has_spread, uint8_t *__restrict__ choice, uint8_t *__restrict__ modes_out,
    uint8_t *__restrict__ taken, int8_t *__restrict__ shifts, double *__restrict__ distortion, double *__restrict__ energy,
    double *__restrict__ weights) {
  __shared__ ModesWideLds S;
  TablesPtr T = C1_TABLES(L.tables);
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) & (kWideWaves - 1);
  ModesWideWaveLds &V = S.w[wave];
  int slot_b[8];
#pragma unroll
  for (int m = 0; m < 8; m++) slot_b[m] = bfu_of_slot(8 * lane + m);
  const int band_shift = lane < 16 ? 0 : (lane < 32 ? 2 : 4);                 // the lane's slots (and its 8 coefficients)
  const int bl = lane < 52 ? lane : 51;                        // lanes 52..63 shadow BFU 51 and never take part
  const int my_first = kBfuFirst[bl], my_size = kSpecs[bl];
  const int bfu_shift = bl < 20 ? 0 : (bl < 36 ? 2 : 4);
  const double w_short = bl < 36 ? 0.25 : 0.5;
  const int dq_step = T->dq_step, dq_fast = T->dq_fast;
  const int n_cand = n_cand_arg < 1 ? 1 : (n_cand_arg > kMaxCand ? kMaxCand : n_cand_arg);
  const int n_off = n_offsets_arg < 1 ? 1 : (n_offsets_arg > 8 ? 8 : n_offsets_arg);
  const double my_floor = mask[bl];                            // floor[b]; the transposed matrix follows at mask + 52
  const double *my_spread = mask + 52 + bl;
  const int64_t units_total = L.frames * L.channels;
  // the grid is the unit count; a workgroup past it (none is launched) would still reach every barrier, on the last unit, and
  // store nothing
  const bool in_range = (int64_t)blockIdx.x < units_total;
  const int64_t unit = in_range ? (int64_t)blockIdx.x : units_total - 1;

  // ---- both analyses of the unit, in every wave ----
  int sfi_long = 0, sfi_short = 0;
  float xl[8], xs[8];
#pragma unroll
  for (int m = 0; m < 8; m++) xl[m] = xs[m] = 0.0f;
  {                                                            // the all-long coefficients always: the weights come from them
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

  // ---- the weights, in every wave: E_b over the all-long coefficients into the wave's cur row, M_b, P_b ----
#pragma unroll
  for (int m = 0; m < 8; m++) {
    const double t = (double)xl[m];
    V.terms[8 * lane + m] = t * t;
  }
  wave_fence();
  if (lane < 52) {
    double acc = 0.0;                                          // ascending slot order, as every table row below
    for (int j = 0; j < my_size; j += 4) {
      const double t0 = V.terms[my_first + j], t1 = V.terms[my_first + j + 1], t2 = V.terms[my_first + j + 2],
                   t3 = V.terms[my_first + j + 3];
      acc += t0;
      acc += j + 1 < my_size ? t1 : 0.0;
      acc += j + 2 < my_size ? t2 : 0.0;
      acc += j + 3 < my_size ? t3 : 0.0;
    }
    V.cur[lane] = acc;                                         // W = 1
  }
  wave_fence();
  double M = 0.0;
  if (has_spread) {                                            // workgroup-uniform (a kernel argument)
#pragma unroll 4
    for (int c = 0; c < 52; c++) {
      const double prod = my_spread[52 * c] * V.cur[c];
      M += prod;
    }
  }
  const double thr = M > my_floor ? M : my_floor;               // a NaN M_b falls to the floor
  const double P = 1.0 / thr;
  wave_fence();                                                // every lane has read the rows; the first table pass rewrites the block

  // ---- per candidate: the plane BFU `lane` takes (a bit), and the reference's word length whose e_0 has to be kept (4 bits) ----
  uint32_t short_of = 0u, wl_refs = 0u;
  for (int kc = 0; kc < n_cand; kc++) {                        // workgroup-uniform (a kernel argument)
    const int modes = mode_in_domain(cand.byte[kc]);
    if (((modes >> bfu_shift) & 3) != 0) short_of |= 1u << kc;
    const uint32_t *al = reinterpret_cast<const uint32_t *>(trial + (int64_t)kc * trial_stride + unit * kAllocBytes);
    const uint32_t a7 = al[7];                                 // amount index, fallback flag
    const bool ref_fallback = (a7 >> 27) & 1;
    const int ref_n = bfu_amount((int)(a7 >> 28) & 7);
    const int wl_ref = (lane < 52 && lane < ref_n && !ref_fallback) ? (int)((al[lane >> 3] >> ((lane & 7) * 4)) & 15) : 0;
    wl_refs |= (uint32_t)wl_ref << (4 * kc);
  }

  // ---- the tables: rows wave, wave + 8 of plane 0, then of plane 1 ----
  for (int i = 0; i < 4; i++) {                                // wave-uniform; no barrier inside this loop
    const int plane = i >> 1, w = wave + 8 * (i & 1);
    if (!(plane ? has_short : has_long)) continue;             // no candidate reads this plane
    float x[8];
#pragma unroll
    for (int m = 0; m < 8; m++) x[m] = plane ? xs[m] : xl[m];
    const int sfi = plane ? sfi_short : sfi_long;              // 0 in lanes 52..63
    const double W = plane ? w_short : 1.0;                    // BFU `lane`'s weight
    const int passes = w == 0 ? 1 : n_off;                     // e(b, 0) has no index in it
    const double yy = T->inv_range[w];
    double best = 0.0;                                         // e(b, w) so far, and its offset index
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
        const double xn = (double)x[m] * V.norm[b];
        const double v = xn + (xn >= 0 ? 0.5 : -0.5);          // round half away from zero ...
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
        const double e = P * (W * acc);                        // the finished e_k(b, w), then the weight
        if (k == 0) {
          best = e;
          // this wave owns (plane, w): one writer per (candidate, BFU)
          for (int kc = 0; kc < n_cand; kc++)
            if ((int)((short_of >> kc) & 1u) == plane && (int)((wl_refs >> (4 * kc)) & 15u) == w) S.e_ref[kc * 52 + lane] = e;
        } else if (valid && e < best) {                        // strictly smaller: the first offset of least error stays
          best = e;
          best_k = k;
        }
      }
      wave_fence();                                            // the next pass rewrites the block
    }
    if (lane < 52) {
      S.table[plane * kPlaneTable + w * kTableStride + lane] = best;
      S.pick[plane * kPlaneTable + w * kTableStride + lane] = (uint8_t)best_k;
    }
  }
  __syncthreads();

  // ---- the gains, a row per wave in turn; candidate `wave`'s T_ref and energy over its composed rows meanwhile ----
  for (int r = wave; r < 30; r += kWideWaves) {                // wave-uniform
    const int plane = r >= 15 ? 1 : 0, w = r - 15 * plane;
    if (!(plane ? has_short : has_long)) continue;
    if (lane < 52) {
      const int sfi = plane ? sfi_short : sfi_long;
      const double e0 = S.table[plane * kPlaneTable + w * kTableStride + lane], e1 = S.table[plane * kPlaneTable + (w + 1) * kTableStride + lane];
      const double gain = (e0 - e1) / (double)((w == 0 ? 2 : 1) * my_size);   // cost = (bits(w + 1) - bits(w)) * size
      S.key[plane * kPlaneKey + w * kTableStride + lane] = (sfi != 0 && gain > 0.0) ? (unsigned long long)__double_as_longlong(gain) : 0ull;
    }
  }
  if (wave < n_cand) {                                         // wave-uniform
    const double t_ref = total_in_bfu_order(S.e_ref + wave * 52);
    if (lane < 52) V.cur[lane] = S.table[((short_of >> wave) & 1u) * kPlaneTable + lane];
    wave_fence();
    const double e_unit = total_in_bfu_order(V.cur);
    wave_fence();                                              // the greedy rewrites the row
    if (lane == 0) { S.t_ref[wave] = t_ref; S.e_unit[wave] = e_unit; }
  }
  __syncthreads();

  // ---- the greedy allocation: amount (wave + k) & 7 of candidate k ----
  for (int kc = 0; kc < n_cand; kc++) {                        // workgroup-uniform; no barrier inside this loop
    const int a = (wave + kc) & 7;
    const int plane = (int)((short_of >> kc) & 1u);            // BFU `lane`'s
    const double *table = S.table + plane * kPlaneTable;
    const unsigned long long *keys = S.key + plane * kPlaneKey;
    const int n = bfu_amount(a);
    int rem = 1696 - 40 - 10 * n;
    const bool mine = lane < n;                                // n <= 52
    int wl = 0;
    unsigned long long key = keys[bl];
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
        key = wl < 15 ? keys[wl * kTableStride + bl] : 0ull;
      }
    }
    const double e_cur = table[(wl & 15) * kTableStride + bl];
    if (lane < 52) V.cur[lane] = lane < n ? e_cur : table[lane];
    wave_fence();
    const double t = total_in_bfu_order(V.cur);
    wave_fence();                                              // the next candidate rewrites the row
    S.wl[(kc * kWideWaves + a) * 64 + lane] = (uint8_t)wl;
    if (lane == 0) S.t[kc * kWideWaves + a] = t;
  }
  __syncthreads();
  if (wave != 0 || !in_range) return;                          // no barrier follows

  // ---- wave 0: the candidates in order, k_measured_modes' statements over what the chains left ----
  double win_t = 0.0;
  int win_k = 0, win_a = 0;
  bool win_take = false, have_win = false;
  for (int kc = 0; kc < n_cand; kc++) {                        // wave-uniform
    const double t_ref = S.t_ref[kc], e_unit = S.e_unit[kc];
    double best_t = 0.0;
    int best_a = 0;
    bool have = false;
    for (int a = 0; a < 8; a++) {
      const double t = S.t[kc * kWideWaves + a];
      if (a == 0) best_t = t;                                  // all NaN: the first amount's total is reported, and nothing is taken
      if (t == t && (!have || t < best_t)) { best_t = t; best_a = a; have = true; }
    }
    const bool take = have && best_t < t_ref;
    if (lane == 0) {
      if (distortion) { distortion[(unit * n_cand + kc) * 2] = t_ref; distortion[(unit * n_cand + kc) * 2 + 1] = best_t; }
      if (energy) energy[unit * n_cand + kc] = e_unit;
    }
    // the candidate of least final error so far (wave-uniform: every lane holds the same totals)
    const double t_final = take ? best_t : t_ref;
    if (kc == 0 || (t_final == t_final && (!have_win || t_final < win_t))) {
      win_t = t_final; win_k = kc; win_take = take; win_a = have ? best_a : 0;
      have_win = t_final == t_final;
    }
  }
  win_k &= kMaxCand - 1;
  win_a &= 7;

  // what lane b has to write for its BFU under the winner: the word length, the offset of its final level where it is coded in a
  // taken unit (else 0), and the composed index
  const int win = mode_in_domain(cand.byte[win_k]);
  const int win_plane = (int)((short_of >> win_k) & 1u);
  const int win_sfi = win_plane ? sfi_short : sfi_long;
  const int win_wl = (int)(S.wl[(win_k * kWideWaves + win_a) * 64 + bl] & 15u);
  const int nb = bfu_amount(win_a);
  const bool shifted = win_take && lane < nb && win_wl > 0;    // nb <= 52
  const int win_offset = shifted ? offset_of(offsets, (int)(S.pick[win_plane * kPlaneTable + win_wl * kTableStride + bl] & 7)) : 0;

  if (finalize) {
    // what k_measured_sf leaves of a taken unit and the plain chain of any other, in the layout k_choose_modes hands to packing.
    // win_offset belongs to an offset that was valid for this BFU: the index stays within 1 .. 63 (masked all the same)
    if (lane < 56) S.win[lane] = lane < 52 ? ((win_take && lane < nb) ? ((uint32_t)win_wl & 15u) : 0u) | ((uint32_t)((win_sfi + win_offset) & 63) << 8) : 0u;
    wave_fence();
    if (lane < 8) {
      uint32_t word;
      if (win_take) {
        word = (uint32_t)win_a << 28;
        if (lane < 7) {
          word = 0u;
#pragma unroll
          for (int k = 0; k < 8; k++) word |= (S.win[8 * lane + k] & 15u) << (4 * k);
        }
      } else word = reinterpret_cast<const uint32_t *>(trial + (int64_t)win_k * trial_stride + unit * kAllocBytes)[lane];
      reinterpret_cast<uint32_t *>(L.alloc + unit * kAllocBytes)[lane] = word;
    }
    if (lane < 16) {                                           // the 52 scale-factor bytes, the mode byte where k_mdct_bands keeps it, padding
      uint32_t word = lane == 13 ? (uint32_t)win : 0u;
      if (lane < 13) {
#pragma unroll
        for (int k = 0; k < 4; k++) word |= ((S.win[4 * lane + k] >> 8) & 63u) << (8 * k);
      }
      reinterpret_cast<uint32_t *>(L.side + unit * kSideBytes)[lane] = word;
    }
    if ((win >> band_shift) & 3) {                             // every wave has read the long plane before the first barrier
      const float4 *src = reinterpret_cast<const float4 *>(coefs_short + (unit << 9));
      float4 *dst = reinterpret_cast<float4 *>(L.coefs + (unit << 9));
      const float4 a = src[2 * lane], c = src[2 * lane + 1];
      dst[2 * lane] = a;
      dst[2 * lane + 1] = c;
    }
  }
  if (shifts && lane < 52) shifts[unit * 52 + lane] = (int8_t)win_offset;
  if (weights && lane < 52) weights[unit * 52 + lane] = P;
  if (lane == 0) {
    if (choice) choice[unit] = (uint8_t)win_k;
    if (modes_out) modes_out[unit] = (uint8_t)win;
    if (taken) taken[unit] = win_take ? 1 : 0;
  }
}

}  // namespace

void c1k_launch_measured_modes_masked_wide(const C1EncodeLaunch &L, const float *coefs_short, const uint8_t *side_short,
                                           const uint8_t *trial, int64_t trial_stride, const uint8_t *cand, int n_cand,
                                           const int8_t *sf_offsets, int n_offsets, const double *mask, bool has_spread, bool finalize,
                                           uint8_t *choice, uint8_t *modes_out, uint8_t *taken, int8_t *shifts, double *distortion,
                                           double *energy, double *weights, hipStream_t stream) {
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
  const dim3 grid((unsigned)units), block(C1_WAVE * kWideWaves);   // a chunk holds fewer than 2^29 units
  hipLaunchKernelGGL(k_measured_modes_masked_wide, grid, block, 0, stream, L, coefs_short, side_short, trial, trial_stride, c, n_cand,
                     has_long, has_short, finalize ? 1 : 0, packed, n_offsets, mask, has_spread ? 1 : 0, choice, modes_out, taken, shifts,
                     distortion, energy, weights);
}
