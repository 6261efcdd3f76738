// c1_k_measure_units_shared.hip -- the coding error of given sound units against their PCM, scored under the masking threshold
// of the all-long spectrum (c1_measure_units_shared_device): k_measure_units' noise and signal, read back from the unit's 212
// bytes against the analysis under the unit's own modes, and in place of its weights those of k_measured_modes_masked, which
// come from the all-long analysis of the same frame and so do not depend on the unit's bytes
#include "c1_device.h"

namespace {

// the domain of a mode byte is what blockSelectorStage writes (encoder.js:143): 0 or 2 in the low and mid fields, 0 or 3 in
// the high one.  Every mode byte is brought into it before anything selects with its fields
__device__ __forceinline__ int mode_in_domain(int b) { return (b & 0x02) | (b & 0x08) | ((b & 0x30) == 0x30 ? 0x30 : 0); }

// low | mid << 2 | high << 4 of the block modes deserializeFrame reports (serialization.js:120-124); header = the unit's first
// 16 bits.  A field the encoder never writes gives a negative mode: mode_in_domain reads bits 1, 3, 4 and 5 alone
__device__ __forceinline__ int unit_mode_byte(uint32_t header) {
  const int low = 2 - (int)((header >> 14) & 3), mid = 2 - (int)((header >> 12) & 3), high = 3 - (int)((header >> 10) & 3);
  return low | (mid * 4) | (high * 16);
}

// unpackBits (bitstream.js:49-70) over the unit's words, most significant bit first: stops at the end of the 212-byte buffer
// and returns what it has.  words: 53 words of the unit and one of padding (a read may touch word w + 1 <= 53).  nbits <= 16
__device__ __forceinline__ uint32_t unit_bits(const uint32_t *words, int pos, int nbits) {
  const int avail = C1_UNIT_BYTES * 8 - pos;
  if (avail <= 0 || nbits == 0) return 0u;
  const int nb = nbits < avail ? nbits : avail;
  const int w = pos >> 5, o = pos & 31;
  const uint32_t hi = words[w], lo = words[w + 1];
  const uint32_t window = o == 0 ? hi : __builtin_amdgcn_alignbit(hi, lo, (uint32_t)(32 - o));
  return window >> (32 - nb);
}

// a wave-uniform address as the scalar registers hold it: the loads and stores below then take it as their scalar base with the
// lane's 32-bit offset, where the compiler would otherwise keep a 64-bit address per lane and array alive over the whole loop
template <typename P> __device__ __forceinline__ P *uniform_ptr(P *p) {
  const uint64_t a = reinterpret_cast<uint64_t>(p);
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)a), hi = __builtin_amdgcn_readfirstlane((uint32_t)(a >> 32));
  return reinterpret_cast<P *>(((uint64_t)hi << 32) | lo);
}

// =====================================================================================================
// k_measure_units_shared : noise[b] and signal[b] of k_measure_units, P_b of k_measured_modes_masked, the two totals
// =====================================================================================================
// k_measure_units (c1_k_measure_units.hip) with a second coefficient plane and another weight phase; launch shape, fields,
// dequantization, the two sums, the totals and the order of stores and prefetch are that kernel's, statement for statement.
// What differs:
//   loads     two more 16-byte loads per lane and unit, of the all-long plane, requested with the rest a unit ahead.
//   E         first in the unit, while the terms block is free: every lane squares its 8 all-long coefficients in binary64 into
//             the block (all long, coefficient order is slot order: no gather) and lane b adds BFU b's in ascending slot order, W
//             = 1, into a row of its own: k_measured_modes_masked's statement.  The plane's 8 registers are free from there on.
//   weights   M_b = sum_c spread[b][c] * E_c, c ascending, each product rounded before it is added, E_c a broadcast read of LDS,
//             the matrix transposed behind the floor in the context's buffer, the one lane-varying global read in the loop; P_b =
//             1 / max(M_b, floor[b]).
//   registers 4 waves per SIMD leave 128: the finished unit's totals wait in LDS (lane 0 reads them back where it stores), and the
//             wave-uniform bases of loads and stores go through uniform_ptr, which keeps 64-bit addresses per lane out of the loop.
// mask is never null here (the host requires the floor).  No fused operation.  All stores are plain vector stores.
constexpr int kMeterWaves = 4;
constexpr int kMeterBlocks = 2048;       // as k_measure_units: past 8 192 units the waves stride

// 9 888 bytes a wave (k_measure_units' 9 456, E's row and the held totals): four workgroups of four waves on a CU, 160 768 bytes
// of its 160 KB with the workgroups' tables
struct alignas(16) SharedMeterLds {
  union {
    float coef[512];                     // the own-mode coefficients of a unit with a short band, on their way to slot order
    double2 terms[512];                  // {(x - d)^2, x^2} of slot p
    double sq[512];                      // where the unit begins: x0^2 of slot p, the all-long plane
    double2 cur[52];                     // after the sums: {P_b noise_b, P_b signal_b}
  };
  double sf[52];                         // SCALE_FACTORS[sfi]; 0 when the BFU codes nothing
  double e[52];                          // E_c, from where the unit begins to its weights
  double step[52];                       // SCALE_FACTORS[sfi] * RN(1 / range) (dq_step)
  uint32_t words[56];                    // the unit, byte-swapped, and zero padding
  uint32_t desc[52];                     // per BFU: mantissa bits (0: codes nothing) | bit offset of its first mantissa << 5
  double2 held_totals;                   // the finished unit's totals, until lane 0 stores them
};

__global__ __launch_bounds__(C1_WAVE * kMeterWaves) __attribute__((amdgpu_waves_per_eu(4))) void k_measure_units_shared(
    const C1DevTables *tables, const float *__restrict__ coefs, const float *__restrict__ coefs_long, const uint8_t *__restrict__ units,
    int64_t units_total, const double *__restrict__ mask, int has_spread, double *__restrict__ noise, double *__restrict__ signal,
    double *__restrict__ totals, double *__restrict__ weights) {
  __shared__ SharedMeterLds lds[kMeterWaves];
  __shared__ double sf_tab[64], inv_tab[16];                   // SCALE_FACTORS and RN(1 / range): a lane-varying table read inside
  TablesPtr T = C1_TABLES(tables);                             // the loop would be a global load in front of the prefetch
  if (threadIdx.x < 64) sf_tab[threadIdx.x] = T->scale_factors[threadIdx.x];
  else if (threadIdx.x < 80) inv_tab[threadIdx.x - 64] = T->inv_range[threadIdx.x - 64];
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  SharedMeterLds &S = lds[wave];
  // the geometry of the lane's 8 slots, one register each: coefficient index long (9 bits) | short << 9 | j << 18 | BFU << 23
  uint32_t geo[8];
#pragma unroll
  for (int m = 0; m < 8; m++) {
    const int p = 8 * lane + m, b = bfu_of_slot(p), j = p - kBfuFirst[b];
    geo[m] = (uint32_t)(kStartLong[b] + j) | ((uint32_t)(kStartShort[b] + j) << 9) | ((uint32_t)j << 18) | ((uint32_t)b << 23);
  }
  const int bl = lane < 52 ? lane : 51;                        // lanes 52..63 shadow BFU 51 and never store
  int my_first = kBfuFirst[bl], my_size = kSpecs[bl];
  const int bfu_shift = bl < 20 ? 0 : (bl < 36 ? 2 : 4);
  const double w_short = bl < 36 ? 0.25 : 0.5;
  const int dq_step = T->dq_step;
  double my_floor = mask[bl];                                  // floor[b]; the transposed matrix follows at mask + 52
  // delivered before the loop: a table value still pending at the loop's entry makes the compiler wait for it inside the loop,
  // every unit, and a wait for it (vmcnt is in order) is a wait for the prefetch
  asm volatile("" : "+v"(my_first), "+v"(my_size), "+v"(my_floor));
#pragma unroll
  for (int m = 0; m < 8; m++) asm volatile("" : "+v"(geo[m]));
  if (lane >= 53 && lane < 56) S.words[lane] = 0u;             // the padding stays zero for every unit of the wave
  const int64_t stride = (int64_t)gridDim.x * kMeterWaves;
  const int wl_lane = lane < 53 ? lane : 52;                   // the word of the unit a lane reads (lanes 53..63: word 52 again)
  int64_t unit = (int64_t)blockIdx.x * kMeterWaves + wave;
  // the next unit's bytes and both of its planes are requested a whole unit ahead (wave-uniform branches)
  float4 next_a = make_float4(0.0f, 0.0f, 0.0f, 0.0f), next_b = next_a, next_la = next_a, next_lb = next_a;
  uint32_t next_word = 0u;
  if (unit < units_total) {
    const float4 *c4 = uniform_ptr(reinterpret_cast<const float4 *>(coefs + (unit << 9)));
    const float4 *l4 = uniform_ptr(reinterpret_cast<const float4 *>(coefs_long + (unit << 9)));
    next_a = c4[2u * (unsigned)lane];
    next_b = c4[2u * (unsigned)lane + 1u];
    next_la = l4[2u * (unsigned)lane];
    next_lb = l4[2u * (unsigned)lane + 1u];
    next_word = uniform_ptr(reinterpret_cast<const uint32_t *>(units + unit * C1_UNIT_BYTES))[(unsigned)wl_lane];
  }
  // The results of a unit are stored where the next unit begins, in front of that unit's prefetch: stores count on the counter
  // of the loads, so behind the prefetch they would be waited for, just issued, where the next unit takes delivery of it
  int64_t held = -1;
  double held_noise = 0.0, held_signal = 0.0, held_P = 0.0;    // the totals wait in LDS: four registers a lane fewer
  auto store_held = [&]() {
    if (held < 0) return;                                      // wave-uniform
    if (lane < 52) {
      if (noise) (noise + held * 52)[(unsigned)lane] = held_noise;       // a uniform base and the lane: no address held per lane
      if (signal) (signal + held * 52)[(unsigned)lane] = held_signal;
      if (weights) (weights + held * 52)[(unsigned)lane] = held_P;
    }
    if (totals && lane == 0) {
      const double2 t = S.held_totals;
      totals[2 * held] = t.x;
      totals[2 * held + 1] = t.y;
    }
  };
  for (; unit < units_total; unit += stride) {
    const float4 ca = next_a, cb = next_b, la = next_la, lb = next_lb;
    if (lane < 53) S.words[lane] = __builtin_bswap32(next_word);
    store_held();
    if (unit + stride < units_total) {
      const float4 *c4 = uniform_ptr(reinterpret_cast<const float4 *>(coefs + ((unit + stride) << 9)));
      const float4 *l4 = uniform_ptr(reinterpret_cast<const float4 *>(coefs_long + ((unit + stride) << 9)));
      next_a = c4[2u * (unsigned)lane];
      next_b = c4[2u * (unsigned)lane + 1u];
      next_la = l4[2u * (unsigned)lane];
      next_lb = l4[2u * (unsigned)lane + 1u];
      next_word = uniform_ptr(reinterpret_cast<const uint32_t *>(units + (unit + stride) * C1_UNIT_BYTES))[(unsigned)wl_lane];
    }
    // ---- E_b over the all-long coefficients, first: the block is free and the plane's 8 registers are given back ----
#pragma unroll
    for (int m = 0; m < 8; m++) {
      const double t = (double)(m == 0 ? la.x : m == 1 ? la.y : m == 2 ? la.z : m == 3 ? la.w : m == 4 ? lb.x : m == 5 ? lb.y : m == 6 ? lb.z : lb.w);
      S.sq[8 * lane + m] = t * t;
    }
    wave_fence();                                              // the squares and the unit's words are written
    {
      double acc = 0.0;                                        // ascending slot order, W = 1
      for (int j = 0; j < my_size; j += 4) {                   // my_first + j + 3 <= 511: the reads stay inside the block
        const double t0 = S.sq[my_first + j], t1 = S.sq[my_first + j + 1], t2 = S.sq[my_first + j + 2], t3 = S.sq[my_first + j + 3];
        acc += t0;
        acc += j + 1 < my_size ? t1 : 0.0;
        acc += j + 2 < my_size ? t2 : 0.0;
        acc += j + 3 < my_size ? t3 : 0.0;
      }
      if (lane < 52) S.e[lane] = acc;                          // lanes 52..63 repeated BFU 51's
    }
    wave_fence();                                              // every lane has read its squares: the block is free again

    // ---- the fields ----
    const uint32_t header = S.words[0] >> 16;
    const int n = bfu_amount((int)(header >> 5) & 7);          // 20 .. 52
    const int modes = mode_in_domain(unit_mode_byte(header));
    const int m0 = modes & 3, m1 = (modes >> 2) & 3, m2 = (modes >> 4) & 3;
    int wl = 0, sfi = 0;
    if (lane < n) {
      wl = (int)unit_bits(S.words, 16 + 4 * lane, 4);
      sfi = (int)unit_bits(S.words, 16 + 4 * n + 6 * lane, 6);
    }
    const int bits = wl_bits(wl);
    const int mybits = lane < 52 ? bits * my_size : 0;
    const int scan = wave_inclusive_scan(mybits);
    if (lane < 52) {
      const bool coded = bits != 0 && sfi != 0;                // lane >= n: both are 0
      const double sfv = coded ? sf_tab[sfi] : 0.0;
      S.desc[lane] = (uint32_t)(coded ? bits : 0) | ((uint32_t)(16 + 10 * n + scan - mybits) << 5);
      S.sf[lane] = sfv;
      S.step[lane] = coded ? sfv * inv_tab[wl] : 0.0;
    }

    // ---- the own-mode coefficients in slot order ----
    float x[8];
    if (modes == 0) {                                          // wave-uniform; all long: coefficient order == slot order
      x[0] = ca.x; x[1] = ca.y; x[2] = ca.z; x[3] = ca.w; x[4] = cb.x; x[5] = cb.y; x[6] = cb.z; x[7] = cb.w;
    } else {
      reinterpret_cast<float4 *>(S.coef)[2 * lane] = ca;
      reinterpret_cast<float4 *>(S.coef)[2 * lane + 1] = cb;
      wave_fence();
#pragma unroll
      for (int m = 0; m < 8; m++) {
        const int b = (int)(geo[m] >> 23), mode = b >= 36 ? m2 : (b >= 20 ? m1 : m0);
        x[m] = S.coef[mode == 0 ? geo[m] & 511u : (geo[m] >> 9) & 511u];
      }
    }
    wave_fence();                                              // the fields are written, the coefficients read

    // ---- mantissas, dequantized values, terms ----
#pragma unroll
    for (int m = 0; m < 8; m++) {
      const int b = (int)(geo[m] >> 23), slot_j = (int)((geo[m] >> 18) & 31u);
      const uint32_t d = S.desc[b];
      const int qbits = (int)(d & 31u);
      float dq = 0.0f;
      if (qbits != 0) {
        // unpackSignedBits (bitstream.js:78-82), past the unit's end as unpackBits reads it
        const uint32_t raw = unit_bits(S.words, (int)(d >> 5) + slot_j * qbits, qbits);
        const int32_t q = raw >= (1u << (qbits - 1)) ? (int32_t)raw - (1 << qbits) : (int32_t)raw;
        const int32_t range = (1 << (qbits - 1)) - 1;          // qbits >= 2: range >= 1
        if (dq_step && q >= -range) dq = f32((double)q * S.step[b]);   // == the division for these mantissas (checked on the host)
        else dq = f32(((double)q * S.sf[b]) / (double)range);
      }
      const double xd = (double)x[m], t = xd - (double)dq;
      S.terms[8 * lane + m] = make_double2(t * t, xd * xd);
    }
    wave_fence();

    // ---- the two sums of BFU `lane`, j ascending ----
    double acc_n = 0.0, acc_s = 0.0;
    for (int j = 0; j < my_size; j += 4) {                     // my_first + j + 3 <= 511: the reads stay inside the block
      const double2 t0 = S.terms[my_first + j], t1 = S.terms[my_first + j + 1], t2 = S.terms[my_first + j + 2],
                    t3 = S.terms[my_first + j + 3];
      const bool in1 = j + 1 < my_size, in2 = j + 2 < my_size, in3 = j + 3 < my_size;
      acc_n += t0.x;              acc_s += t0.y;
      acc_n += in1 ? t1.x : 0.0;  acc_s += in1 ? t1.y : 0.0;
      acc_n += in2 ? t2.x : 0.0;  acc_s += in2 ? t2.y : 0.0;
      acc_n += in3 ? t3.x : 0.0;  acc_s += in3 ? t3.y : 0.0;
    }
    const double W = ((modes >> bfu_shift) & 3) != 0 ? w_short : 1.0;
    const double my_noise = W * acc_n, my_signal = W * acc_s;
    wave_fence();                                              // every lane has read its terms: the block is free for the pairs below

    // ---- the weights: M_b over the E_c formed where the unit began, P_b ----
    double M = 0.0;
    if (has_spread) {                                          // wave-uniform (a kernel argument)
#pragma unroll 4
      for (int c = 0; c < 52; c++) {
        const double prod = mask[52u * (unsigned)(c + 1) + (unsigned)bl] * S.e[c];   // c, bl < 52: inside 52 + 52 * 52 doubles
        M += prod;
      }
    }
    const double thr = M > my_floor ? M : my_floor;             // a NaN M_b falls to the floor
    const double P = 1.0 / thr;

    // ---- the totals, in BFU order ----
    if (lane < 52) S.cur[lane] = make_double2(P * my_noise, P * my_signal);
    wave_fence();
    double tot_n = 0.0, tot_s = 0.0;
#pragma unroll 4
    for (int b = 0; b < 52; b++) {
      const double2 c = S.cur[b];
      tot_n += c.x;
      tot_s += c.y;
    }
    held = unit;
    held_noise = my_noise; held_signal = my_signal; held_P = P;
    if (lane == 0) S.held_totals = make_double2(tot_n, tot_s);
    wave_fence();                                              // the next unit rewrites the block
  }
  store_held();
}

}  // namespace

void c1k_launch_measure_units_shared(const C1DevTables *tables, const float *coefs, const float *coefs_long, const uint8_t *units,
                                     int64_t n, const double *mask, bool has_spread, double *noise, double *signal, double *totals,
                                     double *weights, hipStream_t stream) {
  if (n <= 0) return;
  // C1_METER_BLOCKS (experiments, tests): another bound on the grid, so that a few units already make the waves stride
  const char *env = getenv("C1_METER_BLOCKS");
  const int64_t bound = env && atoi(env) > 0 ? atoi(env) : kMeterBlocks;
  const dim3 grid((unsigned)std::min<int64_t>(bound, (n + kMeterWaves - 1) / kMeterWaves)), block(C1_WAVE * kMeterWaves);
  hipLaunchKernelGGL(k_measure_units_shared, grid, block, 0, stream, tables, coefs, coefs_long, units, n, mask, has_spread ? 1 : 0, noise,
                     signal, totals, weights);
}
