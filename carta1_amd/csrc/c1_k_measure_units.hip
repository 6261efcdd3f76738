// c1_k_measure_units.hip -- the coding error of given sound units against their PCM (c1_measure_units_device): the mode byte
// of every unit for the exact analysis under given modes, and the meter itself, which reads a unit's 212 bytes back, dequantizes
// them and forms the W-weighted noise and signal of every BFU against the coefficients of that analysis
#include "c1_device.h"

namespace {

// the domain of a mode byte is what blockSelectorStage writes (encoder.js:143): 0 or 2 in the low and mid fields, 0 or 3 in
// the high one.  Every mode byte is brought into it before anything selects with its fields
__device__ __forceinline__ int mode_in_domain(int b) { return (b & 0x02) | (b & 0x08) | ((b & 0x30) == 0x30 ? 0x30 : 0); }

// low | mid << 2 | high << 4 of the block modes deserializeFrame reports (serialization.js:120-124: 2 - field, 2 - field,
// 3 - field of the header's first six bits); header = the unit's first 16 bits.  A field the encoder never writes gives a
// negative mode, and the byte is then whatever two's complement makes of it: mode_in_domain reads bits 1, 3, 4 and 5 alone
__device__ __forceinline__ int unit_mode_byte(uint32_t header) {
  const int low = 2 - (int)((header >> 14) & 3), mid = 2 - (int)((header >> 12) & 3), high = 3 - (int)((header >> 10) & 3);
  return low | (mid * 4) | (high * 16);
}

// unpackBits (bitstream.js:49-70) over the unit's words, most significant bit first: stops at the end of the 212-byte buffer
// and returns what it has.  words: 53 words of the unit and one of padding (a read may touch word w + 1 <= 53).  nbits <= 16:
// the field lies in the 32-bit window that starts at bit pos, one funnel shift over two words
__device__ __forceinline__ uint32_t unit_bits(const uint32_t *words, int pos, int nbits) {
  const int avail = C1_UNIT_BYTES * 8 - pos;
  if (avail <= 0 || nbits == 0) return 0u;
  const int nb = nbits < avail ? nbits : avail;
  const int w = pos >> 5, o = pos & 31;
  const uint32_t hi = words[w], lo = words[w + 1];
  const uint32_t window = o == 0 ? hi : __builtin_amdgcn_alignbit(hi, lo, (uint32_t)(32 - o));
  return window >> (32 - nb);
}

// =====================================================================================================
// k_unit_mode_bytes : the mode byte of every unit, where k_modes_lists (c1_k_modes.hip) reads the caller's
// =====================================================================================================
// One lane per unit, two byte reads (any alignment).  The byte is stored as it is; k_modes_lists brings it into the domain.
__global__ __launch_bounds__(256) void k_unit_mode_bytes(const uint8_t *__restrict__ units, int64_t n, uint8_t *__restrict__ modes) {
  const int64_t unit = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (unit >= n) return;
  const uint8_t *u = units + unit * C1_UNIT_BYTES;
  modes[unit] = (uint8_t)unit_mode_byte(((uint32_t)u[0] << 8) | (uint32_t)u[1]);
}

// =====================================================================================================
// k_measure_units : noise[b] = W_b sum_j (x_b[j] - d_b[j])^2, signal[b] = W_b sum_j x_b[j]^2, P_b, the two totals
// =====================================================================================================
// One wave per sound unit, kMeterWaves independent waves per workgroup, a bounded grid whose waves stride over the units: the
// shape of k_measured_masked, of which this is the measuring half run on the record the bytes hold instead of a search.  A
// streaming pass: per unit 2 048 bytes of coefficients and 212 of the unit in, 16 to 1 264 bytes out.
//   loads     a wave requests its next unit's word and coefficients before it works on the present one.  SCALE_FACTORS and RN(1 /
//             range) are copied into LDS once per workgroup (the one barrier, in front of the loop): read from global memory per
//             unit they were loads behind the prefetch, and a wait for them (vmcnt is in order) a wait for the prefetch too.
//   bytes     lanes 0..52 read one word each, byte-swapped into LDS (MSB-first bit order); three zero words follow.
//   fields    deserializeFrame as k_unpack_units reads it: nBfu from the header's amount index, lane b < nBfu its word length
//             (4 bits) and scale-factor index (6 bits), a wave scan of bits(wl) * size for the mantissas' bit offsets.  Every
//             index is a masked bit field (amount 3 bits, wl 4, sfi 6) and unit_bits never reads past the padded words, so no
//             byte pattern leaves the buffers.
//   x         the unit's 512 coefficients in two 16-byte loads per lane.  All long: coefficient order is slot order and the
//             values stay in registers; otherwise they pass through LDS and a lane gathers its 8 BFU-major slots at
//             BFU_START_LONG / BFU_START_SHORT of the unit's (in-domain) modes.
//   d         a lane sign-extends the mantissas of its 8 slots and dequantizes: Float32((q * SF) / range), zero where the BFU is
//             at or above nBfu or has word length or index 0.  With dq_step (C1DevTables: the host has checked Float32(q * RN(SF
//             * RN(1 / range))) against the division for every mantissa within +-range) the product form is taken for those
//             mantissas; -range - 1, which sign extension admits and quantize never writes, always divides.
//   sums      the terms (x - d)^2 and x^2 go to LDS as pairs in slot order; lane b adds its BFU's in ascending j, four pairs per
//             wait (a slot past the BFU's last adds +0.0, which leaves a sum of squares as it is), then multiplies by W_b.
//   weights   as k_measured_masked: E_c = signal[c] broadcast from LDS, the transposed matrix from the context's buffer, c
//             ascending, P_b = 1 / max(M_b, floor[b]); without tables P_b = 1.0 and no table is read.
//   totals    P_b noise_b and P_b signal_b as pairs in LDS, added in BFU order by every lane alike.
//   stores    a unit's results stay in registers until the next unit begins and are stored in front of that unit's prefetch
//             (stores count on the loads' counter); the slot geometry is packed into one register a slot to make room for them.
// No fused operation (the unit is built without contraction).  All stores are plain vector stores.
constexpr int kMeterWaves = 4;
constexpr int kMeterBlocks = 2048;       // as the measured kernels: past 8 192 units the waves stride

// 9 456 bytes a wave: four workgroups of four waves on a CU (154 KB of its 160 KB with the workgroups' tables)
struct alignas(16) MeterLds {
  union {
    float coef[512];                     // the coefficients of a unit with a short band, on their way to slot order
    double2 terms[512];                  // {(x - d)^2, x^2} of slot p
    double2 cur[52];                     // after the sums: {P_b noise_b, P_b signal_b}
  };
  union {
    double sf[52];                       // SCALE_FACTORS[sfi]; 0 when the BFU codes nothing
    double sig[52];                      // after the terms: E_c
  };
  double step[52];                       // SCALE_FACTORS[sfi] * RN(1 / range) (dq_step)
  uint32_t words[56];                    // the unit, byte-swapped, and zero padding
  uint32_t desc[52];                     // per BFU: mantissa bits (0: codes nothing) | bit offset of its first mantissa << 5
};

__global__ __launch_bounds__(C1_WAVE * kMeterWaves) void k_measure_units(const C1DevTables *tables, const float *__restrict__ coefs,
                                                                         const uint8_t *__restrict__ units, int64_t units_total,
                                                                         const double *__restrict__ mask, int has_spread,
                                                                         double *__restrict__ noise, double *__restrict__ signal,
                                                                         double *__restrict__ totals, double *__restrict__ weights) {
  __shared__ MeterLds lds[kMeterWaves];
  __shared__ double sf_tab[64], inv_tab[16];                   // SCALE_FACTORS and RN(1 / range): a lane-varying table read inside
  TablesPtr T = C1_TABLES(tables);                             // the loop would be a global load in front of the prefetch
  if (threadIdx.x < 64) sf_tab[threadIdx.x] = T->scale_factors[threadIdx.x];
  else if (threadIdx.x < 80) inv_tab[threadIdx.x - 64] = T->inv_range[threadIdx.x - 64];
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  MeterLds &S = lds[wave];
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
  double my_floor = mask ? mask[bl] : 1.0;                     // floor[b]; the transposed matrix follows at mask + 52
  // delivered before the loop: a table value still pending at the loop's entry makes the compiler wait for it inside the loop,
  // every unit, and a wait for it (vmcnt is in order) is a wait for the prefetch
  asm volatile("" : "+v"(my_first), "+v"(my_size), "+v"(my_floor));
#pragma unroll
  for (int m = 0; m < 8; m++) asm volatile("" : "+v"(geo[m]));
  const double *my_spread = mask ? mask + 52 + bl : nullptr;
  if (lane >= 53 && lane < 56) S.words[lane] = 0u;             // the padding stays zero for every unit of the wave
  const int64_t stride = (int64_t)gridDim.x * kMeterWaves;
  const int wl_lane = lane < 53 ? lane : 52;                   // the word of the unit a lane reads (lanes 53..63: word 52 again)
  int64_t unit = (int64_t)blockIdx.x * kMeterWaves + wave;
  // the next unit's bytes and coefficients are requested a whole unit ahead (wave-uniform branches); nothing else in the
  // loop of a call without tables is a load, so the only wait for them is where the unit begins
  float4 next_a = make_float4(0.0f, 0.0f, 0.0f, 0.0f), next_b = next_a;
  uint32_t next_word = 0u;
  if (unit < units_total) {
    const float4 *c4 = reinterpret_cast<const float4 *>(coefs + (unit << 9));
    next_a = c4[2 * lane];
    next_b = c4[2 * lane + 1];
    next_word = reinterpret_cast<const uint32_t *>(units + unit * C1_UNIT_BYTES)[wl_lane];
  }
  // The results of a unit are stored where the next unit begins, in front of that unit's prefetch: stores count on the counter
  // of the loads, so behind the prefetch they would be waited for, just issued, where the next unit takes delivery of it
  int64_t held = -1;
  double held_noise = 0.0, held_signal = 0.0, held_P = 0.0, held_tn = 0.0, held_ts = 0.0;
  auto store_held = [&]() {
    if (held < 0) return;                                      // wave-uniform
    if (lane < 52) {
      if (noise) noise[held * 52 + lane] = held_noise;
      if (signal) signal[held * 52 + lane] = held_signal;
      if (weights) weights[held * 52 + lane] = held_P;
    }
    if (totals && lane == 0) {
      totals[2 * held] = held_tn;
      totals[2 * held + 1] = held_ts;
    }
  };
  for (; unit < units_total; unit += stride) {
    const float4 ca = next_a, cb = next_b;
    if (lane < 53) S.words[lane] = __builtin_bswap32(next_word);
    store_held();
    if (unit + stride < units_total) {
      const float4 *c4 = reinterpret_cast<const float4 *>(coefs + ((unit + stride) << 9));
      next_a = c4[2 * lane];
      next_b = c4[2 * lane + 1];
      next_word = reinterpret_cast<const uint32_t *>(units + (unit + stride) * C1_UNIT_BYTES)[wl_lane];
    }
    wave_fence();

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

    // ---- the coefficients in slot order ----
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

    // ---- the weights ----
    double P = 1.0;
    if (mask) {                                                // wave-uniform (a kernel argument)
      if (lane < 52) S.sig[lane] = my_signal;
      wave_fence();
      double M = 0.0;
      if (has_spread) {
#pragma unroll 4
        for (int c = 0; c < 52; c++) {
          const double prod = my_spread[52 * c] * S.sig[c];
          M += prod;
        }
      }
      const double thr = M > my_floor ? M : my_floor;           // a NaN M_b falls to the floor
      P = 1.0 / thr;
    }

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
    held_noise = my_noise; held_signal = my_signal; held_P = P; held_tn = tot_n; held_ts = tot_s;
    wave_fence();                                              // the next unit rewrites the block
  }
  store_held();
}

}  // namespace

void c1k_launch_unit_mode_bytes(const uint8_t *units, int64_t n, uint8_t *modes, hipStream_t stream) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_unit_mode_bytes, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, units, n, modes);
}

void c1k_launch_measure_units(const C1DevTables *tables, const float *coefs, const uint8_t *units, int64_t n, const double *mask,
                              bool has_spread, double *noise, double *signal, double *totals, double *weights, hipStream_t stream) {
  if (n <= 0) return;
  // C1_METER_BLOCKS (experiments, tests): another bound on the grid, so that a few units already make the waves stride
  const char *env = getenv("C1_METER_BLOCKS");
  const int64_t bound = env && atoi(env) > 0 ? atoi(env) : kMeterBlocks;
  const dim3 grid((unsigned)std::min<int64_t>(bound, (n + kMeterWaves - 1) / kMeterWaves)), block(C1_WAVE * kMeterWaves);
  hipLaunchKernelGGL(k_measure_units, grid, block, 0, stream, tables, coefs, units, n, mask, has_spread ? 1 : 0, noise, signal, totals,
                     weights);
}
