// c1_k_decision.hip -- the encoder's decision functions as the reference exports them from codec/analysis/transient.js
// (performFFT, detectTransient) and codec/coding/bitallocation.js (findScaleFactor, allocateBits), batched over independent
// problems of any shape.  The encoder makes these decisions inside k_detect and k_alloc_* at the codec's fixed shapes; these
// kernels are not the hot path.  They serve applications that import those names and build their own pipeline stages, and
// they restate the reference's loops directly: binary64 operations in its index order, binary32 at every typed-array
// store, no fused multiply-add.
#include "c1_detect_core.h"

namespace {

// e_log2.c as V8 carries it (src/base/ieee754.cc log2, k_log1p of k_log.h inlined): Math.log2 of findScaleFactor
// (bitallocation.js:297).  Like the four functions of c1_detect_core.h it is not correctly rounded, so the algorithm is
// restated operation for operation; tests pin it against V8's outputs through c1_libm_device (fn 4).
__device__ double js_log2(double x) {
  constexpr double ivln2hi = 1.44269504072144627571e+00, ivln2lo = 1.67517131648865118353e-10;
  constexpr double Lg1 = 6.666666666666735130e-01, Lg2 = 3.999999999940941908e-01, Lg3 = 2.857142874366239149e-01,
                   Lg4 = 2.222219843214978396e-01, Lg5 = 1.818357216161805012e-01, Lg6 = 1.531383769920937332e-01,
                   Lg7 = 1.479819860511658591e-01;
  int hx = __double2hiint(x), k = 0;
  const uint32_t lx = (uint32_t)__double2loint(x);
  if (hx < 0x00100000) {
    if (((hx & 0x7fffffff) | lx) == 0) return -__builtin_huge_val();
    if (hx < 0) return __builtin_nan("");
    k = -54; x *= kTwo54; hx = __double2hiint(x);
  }
  if (hx >= 0x7ff00000) return x + x;
  if (hx == 0x3ff00000 && lx == 0) return 0.0;
  k += (hx >> 20) - 1023;
  hx &= 0x000fffff;
  const int i = (hx + 0x95f64) & 0x100000;
  x = js_with_hi(x, hx | (i ^ 0x3ff00000));
  k += (i >> 20);
  const double y = (double)k;
  const double f = x - 1.0;
  const double hfsq = 0.5 * f * f;
  const double s = f / (2.0 + f), z = s * s, w = z * z;
  const double t1 = w * (Lg2 + w * (Lg4 + w * Lg6));
  const double t2 = z * (Lg1 + w * (Lg3 + w * (Lg5 + w * Lg7)));
  const double r = s * (hfsq + (t2 + t1));
  const double hi = __hiloint2double(__double2hiint(f - hfsq), 0);
  const double lo = (f - hi) - hfsq + r;
  const double val_hi = hi * ivln2hi;
  double val_lo = (lo + hi) * ivln2lo + lo * ivln2hi;
  const double sum = y + val_hi;
  val_lo += (y - sum) + val_hi;
  return val_lo + sum;
}

__global__ void k_log2_tap(const double *__restrict__ in, double *__restrict__ out, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  out[i] = js_log2(in[i]);
}

// findScaleFactor (bitallocation.js:290-299) over v[0..n): the caller has cut `length` to the values that exist (reads past
// the array are undefined, and a NaN amplitude never raises the maximum)
__device__ int find_scale_factor(const double *v, int64_t n) {
  double m = 0.0;
  for (int64_t i = 0; i < n; i++) {
    const double a = fabs(v[i]);
    if (a > m) m = a;
  }
  if (m == 0.0) return 0;
  const double index = ceil(3.0 * (js_log2(m) + 21.0));    // +Inf for m = +Inf
  return index > 63.0 ? 63 : (index < 0.0 ? 0 : (int)index);
}

__global__ void k_find_scale_factors(const double *__restrict__ values, const int64_t *__restrict__ offsets,
                                     const int64_t *__restrict__ counts, int64_t problems, int32_t *__restrict__ out) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= problems) return;
  out[p] = find_scale_factor(values + offsets[p], counts[p]);
}

// ---- performFFT (transient.js:17-35) ---------------------------------------------------------------------------------
// the twiddle recurrence of FFT.fft (fft.js:44-64) from the host's (cos, sin)(-2 pi / stride), one thread per stage:
// tw[h - 1 + k] = the twiddle of butterfly k in the stage of half-stride h, the same in every start block
__global__ void k_fft_twiddles(const double *__restrict__ w, int stages, double2 *__restrict__ tw) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= stages) return;
  const int half = 1 << s;
  const double wr = w[2 * s], wi = w[2 * s + 1];
  double tr = 1.0, ti = 0.0;
  for (int k = 0; k < half; k++) {
    tw[half - 1 + k] = make_double2(tr, ti);
    const double nr = tr * wr - ti * wi;
    ti = tr * wi + ti * wr;
    tr = nr;
  }
}

// one workgroup per problem: real.set of the first min(length, n) samples (Float32 rounding) into the bit-reversed
// positions (the swaps of fft.js:21-32 are that permutation), the stages of k_fft_reference on re / im (n floats each,
// the problem's own), then Float32(Math.sqrt(re*re + im*im)) of the n / 2 positive frequencies
__global__ __launch_bounds__(256) void k_perform_fft(const double *__restrict__ samples, const int64_t *__restrict__ offsets, int n,
                                                     int bits, const double2 *__restrict__ tw, float *re_all, float *im_all,
                                                     float *__restrict__ mag) {
  const int tid = threadIdx.x;
  const int64_t p = blockIdx.x;
  float *re = re_all + p * n, *im = im_all + p * n;
  const int64_t off = offsets[p], len = offsets[p + 1] - off;
  const int copy = len < n ? (int)len : n;
  for (int j = tid; j < n; j += 256) {
    const int src = (int)(__brev((unsigned)j) >> (32 - bits));
    re[j] = src < copy ? f32(samples[off + src]) : 0.0f;
    im[j] = 0.0f;
  }
  __threadfence_block();
  __syncthreads();
  for (int half = 1; half < n; half <<= 1) {
    const int stride = half << 1;
    for (int b = tid; b < n / 2; b += 256) {
      const int k = b & (half - 1), e = (b / half) * stride + k, o = e + half;
      const double er = re[e], ei = im[e], orr = re[o], oi = im[o];
      const double2 t = tw[half - 1 + k];
      const double xr = orr * t.x - oi * t.y;
      const double xi = orr * t.y + oi * t.x;
      re[e] = f32(er + xr);
      im[e] = f32(ei + xi);
      re[o] = f32(er - xr);
      im[o] = f32(ei - xi);
    }
    __threadfence_block();
    __syncthreads();
  }
  float *out = mag + p * (n / 2);
  for (int i = tid; i < n / 2; i += 256) {
    const double r = re[i], q = im[i];
    out[i] = f32(sqrt(r * r + q * q));
  }
}

// ---- detectTransient (transient.js:44-226) ----------------------------------------------------------------------------
// one problem per thread, each feature summed in the reference's index order.  cur = currentCoeffs[0..n); prev =
// prevCoeffs[0..m): a read at or past m is undefined, NaN in every arithmetic use (transient.js:97, :178)
__device__ double spectral_flatness(const double *c, int64_t n) {   // :120-141
  double sum_log = 0.0, sum_lin = 0.0;
  int64_t valid = 0;
  for (int64_t i = 0; i < n; i++) {
    const double mag = fabs(c[i]);
    if (mag > 1e-10) {
      sum_log += js_log(mag);
      sum_lin += mag;
      valid++;
    }
  }
  if (valid == 0) return 0.0;
  const double gm = js_exp(sum_log / (double)valid), am = sum_lin / (double)valid;
  return am > 1e-10 ? gm / am : 0.0;
}

__device__ double high_frequency_ratio(const double *c, int64_t n) {   // :149-164
  const int64_t mid = n / 2;
  double lo = 0.0, hi = 0.0;
  for (int64_t i = 0; i < mid; i++) lo += c[i] * c[i];
  for (int64_t i = mid; i < n; i++) hi += c[i] * c[i];
  const double tot = lo + hi;
  return tot > 0 ? hi / tot : 0.0;
}

__device__ double transient_score(const double *cur, int64_t n, const double *prev, int64_t m, double log1p10) {
  const double nan = __builtin_nan("");
  // calculateSpectralFlux :92-112.  Its energy sum (|c|^2) is bit for bit calculateEnergyChange's (c^2) :176-179
  double flux = 0.0, ce = 0.0, pe = 0.0;
  for (int64_t i = 0; i < n; i++) {
    const double cm = fabs(cur[i]), pv = i < m ? prev[i] : nan;
    const double diff = cm - fabs(pv);
    if (diff > 0) flux += diff;
    ce += cm * cm;
    pe += pv * pv;
  }
  double norm = sqrt(ce);
  if (!(norm != 0.0)) norm = 1e-6;                          // `Math.sqrt(e) || 1e-6`: 0 and NaN
  flux = flux / norm;
  const double flat_change = fabs(spectral_flatness(cur, n) - spectral_flatness(prev, m));
  const double hf_change = fabs(high_frequency_ratio(cur, n) - high_frequency_ratio(prev, m));
  // Math.max / Math.min propagate NaN (:181-188, :215)
  ce = ce > 1e-10 ? ce : (ce != ce ? ce : 1e-10);
  pe = pe > 1e-10 ? pe : (pe != pe ? pe : 1e-10);
  const double db = 10.0 * js_log10(ce / pe);
  const double e_change = db > 0 ? db : (db != db ? db : 0.0);
  const double flat_c = sqrt(flat_change);                  // calculateTransientScore :197-226
  const double hf_c = js_log1p(hf_change * 10.0) / log1p10;
  const double e_c = e_change / 30.0 < 1.0 ? e_change / 30.0 : (e_change != e_change ? e_change : 1.0);
  return (flux + flat_c + hf_c + e_c) / 4.0;
}

__global__ void k_detect_transients(const double *__restrict__ cur, const int64_t *__restrict__ cur_off, const double *__restrict__ prev,
                                    const int64_t *__restrict__ prev_off, const uint8_t *__restrict__ has_prev,
                                    const double *__restrict__ thresholds, int64_t problems, const C1DevTables *tables,
                                    uint8_t *__restrict__ transient, double *__restrict__ scores) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= problems) return;
  if (has_prev && !has_prev[p]) {                          // `if (!prevCoeffs) return false` (:46)
    transient[p] = 0;
    scores[p] = __builtin_nan("");
    return;
  }
  const double score = transient_score(cur + cur_off[p], cur_off[p + 1] - cur_off[p], prev + prev_off[p],
                                       prev_off[p + 1] - prev_off[p], tables->log1p10);
  transient[p] = score > thresholds[p] ? 1 : 0;
  scores[p] = score;
}

// ---- allocateBits (bitallocation.js:74-288) ---------------------------------------------------------------------------
// one problem per thread, every candidate BFU count in full (no pruning).  Per-problem state lives in private memory.
constexpr int kBfuAmounts[8] = {20, 28, 32, 36, 40, 44, 48, 52};
__device__ __forceinline__ int word_length_bits(int wl) { return wl == 0 ? 0 : wl + 1; }         // WORD_LENGTH_BITS, wl 0..15
__device__ __forceinline__ int word_length_delta_bits(int wl) { return wl == 0 ? 2 : 1; }        // WORD_LENGTH_DELTA_BITS, wl 0..14
__device__ __forceinline__ double distortion_delta_factor(int wl) {                               // DISTORTION_DELTA_FACTORS, wl 0..14
  return wl == 0 ? 1.75 : ldexp(1.0, -(wl + 2));
}

// siftDown (:313-340): a child replaces the parent only when strictly greater, the right child only when strictly greater
// than the left one's priority (or the parent's)
__device__ void sift_down(int *idx, float *pri, int i, int size) {
  const int iv = idx[i];
  const float pv = pri[i];
  while (true) {
    const int l = (i << 1) + 1, r = l + 1;
    int max_i = i;
    float max_p = pv;
    if (l < size && pri[l] > max_p) { max_i = l; max_p = pri[l]; }
    if (r < size && pri[r] > max_p) max_i = r;
    if (max_i == i) break;
    idx[i] = idx[max_i];
    pri[i] = pri[max_i];
    i = max_i;
  }
  idx[i] = iv;
  pri[i] = pv;
}

__global__ __launch_bounds__(64) void k_allocate_bits(const double *__restrict__ data, const int64_t *__restrict__ bfu_off,
                                                      const int32_t *__restrict__ bfu_len, const int32_t *__restrict__ bfu_sizes,
                                                      const int32_t *__restrict__ max_bfus, int64_t problems,
                                                      const double *__restrict__ bsf, int32_t *__restrict__ out_count,
                                                      int32_t *__restrict__ out_wl, int32_t *__restrict__ out_sfi,
                                                      uint8_t *__restrict__ out_fallback) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= problems) return;
  const int mb = max_bfus[p];
  int sz[52], sfi[52], wl[52], best_wl[52], heap_idx[52];
  float zero_bit[52], heap_pri[52];
  for (int i = 0; i < 52; i++) {                            // :75-88
    sz[i] = i < mb ? bfu_sizes[52 * p + i] : 0;
    sfi[i] = 0;
    zero_bit[i] = 0.0f;
    best_wl[i] = 0;
    if (sz[i] == 0) continue;
    const int64_t len = bfu_len[52 * p + i];
    sfi[i] = find_scale_factor(data + bfu_off[52 * p + i], sz[i] < len ? sz[i] : len);   // sz < 0 reads nothing
    if (sfi[i] > 0) zero_bit[i] = f32(bsf[sfi[i]] * 2.0 * (double)sz[i]);
  }
  int best = -1;
  double min_total = __builtin_huge_val();
  for (int c = 0; c < 8; c++) {                             // :93-129
    const int cand = kBfuAmounts[c];
    if (cand > mb) continue;
    int remaining = 1696 - 40 - cand * 10;                  // FRAME_BITS - FRAME_OVERHEAD_BITS - n * BITS_PER_BFU_METADATA, >= 1136
    // distributeBitsRDO (:203-288)
    int size = 0;
    for (int b = 0; b < cand; b++) {
      wl[b] = 0;
      if (sz[b] == 0 || sfi[b] == 0) continue;
      heap_idx[size] = b;
      heap_pri[size] = f32((bsf[sfi[b]] * distortion_delta_factor(0)) / (double)word_length_delta_bits(0));
      size++;
    }
    for (int i = (size >> 1) - 1; i >= 0; i--) sift_down(heap_idx, heap_pri, i, size);
    while (remaining > 0 && size > 0) {
      const int b = heap_idx[0], cur = wl[b];
      const int64_t cost = (int64_t)word_length_delta_bits(cur) * sz[b];
      bool pop = cost > remaining || cost <= 0;
      if (!pop) {
        remaining -= (int)cost;
        const int nxt = cur + 1;
        wl[b] = nxt;
        if (nxt < 15) {                                     // MAX_WORD_LENGTH_INDEX; WORD_LENGTH_DELTA_BITS[nxt] > 0 there
          heap_pri[0] = f32((bsf[sfi[b]] * distortion_delta_factor(nxt)) / (double)word_length_delta_bits(nxt));
          sift_down(heap_idx, heap_pri, 0, size);
        } else {
          pop = true;
        }
      }
      if (pop) {
        size--;
        heap_idx[0] = heap_idx[size];
        heap_pri[0] = heap_pri[size];
        if (size > 0) sift_down(heap_idx, heap_pri, 0, size);
      }
    }
    // calculateTotalDistortion (:157-190)
    double total = 0.0;
    for (int i = 0; i < cand; i++) {
      const int bits = word_length_bits(wl[i]);
      if (bits == 0) { total += (double)zero_bit[i]; continue; }
      if (sfi[i] == 0) continue;
      total += bsf[sfi[i]] * ldexp(1.0, -bits) * (double)sz[i];
    }
    for (int i = cand; i < mb; i++) total += (double)zero_bit[i];
    if (total < min_total) {                                // first strict minimum; NaN and +Inf are never chosen
      min_total = total;
      best = cand;
      for (int i = 0; i < cand; i++) best_wl[i] = wl[i];
    }
  }
  const bool fallback = best < 0;                           // :132-139
  out_count[p] = fallback ? kBfuAmounts[0] : best;
  out_fallback[p] = fallback ? 1 : 0;
  for (int i = 0; i < 52; i++) {
    out_wl[52 * p + i] = fallback ? 0 : best_wl[i];
    out_sfi[52 * p + i] = fallback ? 0 : sfi[i];
  }
}

}  // namespace

void c1k_launch_js_log2(const double *in, double *out, int64_t n, hipStream_t stream) {
  if (n > 0) hipLaunchKernelGGL(k_log2_tap, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, in, out, n);
}
void c1k_launch_find_scale_factors(const double *values, const int64_t *offsets, const int64_t *counts, int64_t problems, int32_t *out,
                                   hipStream_t stream) {
  hipLaunchKernelGGL(k_find_scale_factors, dim3((unsigned)((problems + 255) / 256)), dim3(256), 0, stream, values, offsets, counts,
                     problems, out);
}
void c1k_launch_perform_fft(const double *samples, const int64_t *offsets, int64_t problems, int n, const double *w, double *tw,
                            float *re, float *im, float *mag, hipStream_t stream) {
  int bits = 0;
  while ((1 << bits) < n) bits++;
  hipLaunchKernelGGL(k_fft_twiddles, dim3(1), dim3(32), 0, stream, w, bits, reinterpret_cast<double2 *>(tw));
  hipLaunchKernelGGL(k_perform_fft, dim3((unsigned)problems), dim3(256), 0, stream, samples, offsets, n, bits,
                     reinterpret_cast<const double2 *>(tw), re, im, mag);
}
void c1k_launch_detect_transients(const double *cur, const int64_t *cur_off, const double *prev, const int64_t *prev_off,
                                  const uint8_t *has_prev, const double *thresholds, int64_t problems, const C1DevTables *tables,
                                  uint8_t *transient, double *scores, hipStream_t stream) {
  hipLaunchKernelGGL(k_detect_transients, dim3((unsigned)((problems + 63) / 64)), dim3(64), 0, stream, cur, cur_off, prev, prev_off,
                     has_prev, thresholds, problems, tables, transient, scores);
}
void c1k_launch_allocate_bits(const double *data, const int64_t *bfu_off, const int32_t *bfu_len, const int32_t *bfu_sizes,
                              const int32_t *max_bfus, int64_t problems, const double *bsf, int32_t *count, int32_t *wl, int32_t *sfi,
                              uint8_t *fallback, hipStream_t stream) {
  hipLaunchKernelGGL(k_allocate_bits, dim3((unsigned)((problems + 63) / 64)), dim3(64), 0, stream, data, bfu_off, bfu_len, bfu_sizes,
                     max_bfus, problems, bsf, count, wl, sfi, fallback);
}
