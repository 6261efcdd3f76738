// c1_api.hip -- host side of libcarta1_hip.so: the C ABI of include/carta1_hip.h.
// Contexts, table upload, workspace, chunking of large batches, stateful streams, profiling events.
// Compiled with -ffp-contract=off: the twiddle recurrence and the normalisation table below are part
// of the reference's numerics (codec/transforms/fft.js:62-64, codec/coding/quantization.js:42-44).
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <map>
#include <memory>
#include <atomic>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "c1_internal.h"
#include "c1_detect_bound.h"

#pragma clang fp contract(off)

namespace {

#include "c1_default_tables.inc"

thread_local std::string g_error;
int fail(int code, const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_error = buf;
  return code;
}
#define HIP_TRY(expr)                                                                        \
  do {                                                                                       \
    hipError_t e_ = (expr);                                                                  \
    if (e_ != hipSuccess) return fail(C1_ERR_HIP, "%s: %s", #expr, hipGetErrorString(e_)); \
  } while (0)

std::mutex g_tables_mutex;
bool g_tables_custom = false;
std::atomic<uint64_t> g_tables_gen{0};        // bumped by every c1_set_tables(): pooled contexts made before it are retired
c1_tables g_tables;

void default_tables(c1_tables *t) {
  memcpy(t->scale_factors, C1D_SCALE_FACTORS, sizeof t->scale_factors);
  memcpy(t->window_short, C1D_WINDOW_SHORT, sizeof t->window_short);
  memcpy(t->mdct_fwd64, C1D_MDCT_FWD64, sizeof t->mdct_fwd64);
  memcpy(t->mdct_fwd256, C1D_MDCT_FWD256, sizeof t->mdct_fwd256);
  memcpy(t->mdct_fwd512, C1D_MDCT_FWD512, sizeof t->mdct_fwd512);
  memcpy(t->mdct_inv64, C1D_MDCT_INV64, sizeof t->mdct_inv64);
  memcpy(t->mdct_inv256, C1D_MDCT_INV256, sizeof t->mdct_inv256);
  memcpy(t->mdct_inv512, C1D_MDCT_INV512, sizeof t->mdct_inv512);
  memcpy(t->fft_w, C1D_FFT_W, sizeof t->fft_w);
  t->log1p_10 = C1D_LOG1P_10;
}

// QMF prototype (codec/core/constants.js:74-107): `new Float32Array([...])` rounds the decimal
// literals decimal -> double -> float; the 48-tap window is 2 * prototype, mirrored; EVEN = window[2j].
void qmf_even_taps(double out[24]) {
  static const double proto[24] = {
      -0.00001461907, -0.00009205479, -0.000056157569, 0.00030117269, 0.0002422519, -0.00085293897,
      -0.0005205574,  0.0020340169,   0.00078333891,   -0.0042153862, -0.00075614988, 0.0078402944,
      -0.000061169922, -0.01344162,   0.0024626821,    0.021736089,   -0.007801671,  -0.034090221,
      0.01880949,     0.054326009,    -0.043596379,    -0.099384367,  0.13207909,    0.46424159};
  float window[48];
  for (int i = 0; i < 24; i++) {
    const float c = (float)proto[i];
    window[i] = (float)((double)c * 2.0);
    window[47 - i] = window[i];
  }
  for (int j = 0; j < 24; j++) out[j] = (double)window[2 * j];
}

// ---- speculative binary32 path (c1_k_spec.hip): rounded tables and the coefficients of its error bound -------------
// DESIGN.md 3b derives   eps_b = u (1 + theta) [ KA_b sigma sqrt(n_b) Z_b + sigma^2 sqrt(2 n_b) (D_b + 3 T_b) ] + eabs
// with u = 2^-24, Z_b the measured norm of the band's pre-twiddled points, W / L the measured norms of the PCM and of
// the first-stage low band over the two frames a unit depends on, and
//   D_2 = (2 gH + gQ) W,  T_2 = gH W;   D_0 = D_1 = gH (2 L + gQ W) + (2 gH + gQ) L,  T_0 = T_1 = gH L.
// gH bounds the l2 gain of one QMF branch (sqrt(|E|^2 + |O|^2) of the polyphase responses), gQ the accumulated
// rounding of the two-chain binary32 convolution in units of u * |input|; both depend only on the QMF prototype, which
// is compiled in (tools/spec_constants.py recomputes them from the taps; tests/test_spec_bound.py checks these are >=).
constexpr double kSpecGH = 1.4160, kSpecGQ = 4.80;
// KA = post-twiddle (1 + 2 sqrt 2) + 1  |  FFT rounds  |  pre-twiddle (1 + 3 sqrt 2) + 1      (reference's share + ours)
constexpr double kSpecKAPost = 4.83, kSpecKAPre = 6.25;
constexpr double kSpecKARoundA = 4.0, kSpecKARound4 = 7.0, kSpecKARound2 = 5.0;
constexpr double kSpecTheta = 1.01;
float round_up_f32(double x) {
  float f = (float)x;
  if ((double)f < x) f = std::nextafterf(f, INFINITY);
  return f;
}
void build_spec_tables(const c1_tables &t, C1DevTables *d) {
  for (int j = 0; j < 24; j++) d->tap32[j] = (float)d->tap_e[j];
  for (int j = 0; j < 24; j++) { d->tap_pair[j][0] = d->tap32[23 - j]; d->tap_pair[j][1] = d->tap32[j]; }
  d->tap_pair[24][0] = 0.0f; d->tap_pair[24][1] = d->tap32[11];
  d->tap_pair[25][0] = d->tap32[11]; d->tap_pair[25][1] = 0.0f;
  bool ok = d->sf_fast != 0;
  for (int i = 0; i < 32; i++) {
    d->win32[i] = (float)t.window_short[i];
    if (!(t.window_short[i] >= 0.0 && t.window_short[i] <= 1.0)) ok = false;
  }
  for (int i = 0; i < 16; i++) { d->pre32_64[i][0] = (float)t.mdct_fwd64[2 * i]; d->pre32_64[i][1] = (float)t.mdct_fwd64[2 * i + 1]; }
  for (int i = 0; i < 64; i++) { d->pre32_256[i][0] = (float)t.mdct_fwd256[2 * i]; d->pre32_256[i][1] = (float)t.mdct_fwd256[2 * i + 1]; }
  for (int i = 0; i < 128; i++) { d->pre32_512[i][0] = (float)t.mdct_fwd512[2 * i]; d->pre32_512[i][1] = (float)t.mdct_fwd512[2 * i + 1]; }
  // every (cos, sin) pair of an MDCT table has the same modulus sigma = sqrt(scale / N) (mdct.js:27-36)
  auto sigma2 = [&](const double *tab, int pairs, double want) {
    double mx = 0;
    for (int i = 0; i < pairs; i++) {
      const double m = tab[2 * i] * tab[2 * i] + tab[2 * i + 1] * tab[2 * i + 1];
      if (!(std::fabs(m - want) <= 1e-9 * want)) ok = false;
      mx = std::max(mx, m);
    }
    return mx;
  };
  const double s64 = sigma2(t.mdct_fwd64, 16, 0.5 / 64), s256 = sigma2(t.mdct_fwd256, 64, 0.5 / 256), s512 = sigma2(t.mdct_fwd512, 128, 1.0 / 512);
  // the FFT twiddles must be the unit-modulus roots the radix-4 regrouping assumes (to 1e-12; the bound's theta absorbs that)
  const double (*tw)[2] = d->fft_tw;
  for (int h = 1; h <= 128; h <<= 1)
    for (int k = 0; k < h; k++) {
      const double ang = -M_PI * (double)k / (double)h;
      if (std::fabs(tw[h - 1 + k][0] - std::cos(ang)) > 1e-12 || std::fabs(tw[h - 1 + k][1] - std::sin(ang)) > 1e-12) ok = false;
    }
  for (int r = 0; r < 2; r++) {
    const int h = r == 0 ? 4 : 16;
    for (int k = 0; k < h; k++) {
      const double *a = tw[h - 1 + k], *b = tw[2 * h - 1 + k];
      float (*dst)[2] = r == 0 ? d->r4b[k] : d->r4c[k];
      dst[0][0] = (float)a[0]; dst[0][1] = (float)a[1];
      dst[1][0] = (float)b[0]; dst[1][1] = (float)b[1];
      dst[2][0] = (float)(a[0] * b[0] - a[1] * b[1]);
      dst[2][1] = (float)(a[0] * b[1] + a[1] * b[0]);
    }
  }
  for (int k = 0; k < 64; k++) { d->r2d[k][0] = (float)tw[63 + k][0]; d->r2d[k][1] = (float)tw[63 + k][1]; }
  for (int i = 0; i < 64 * 16; i++) d->norm32[i] = (float)d->norm[i];
  for (int i = 0; i < 16; i++) { d->inv32_64[i][0] = (float)t.mdct_inv64[2 * i]; d->inv32_64[i][1] = (float)t.mdct_inv64[2 * i + 1]; }
  for (int i = 0; i < 64; i++) { d->inv32_256[i][0] = (float)t.mdct_inv256[2 * i]; d->inv32_256[i][1] = (float)t.mdct_inv256[2 * i + 1]; }
  for (int i = 0; i < 128; i++) { d->inv32_512[i][0] = (float)t.mdct_inv512[2 * i]; d->inv32_512[i][1] = (float)t.mdct_inv512[2 * i + 1]; }
  for (int i = 0; i < 256; i++) { d->tw32[i][0] = (float)tw[i][0]; d->tw32[i][1] = (float)tw[i][1]; }
  const double u = std::ldexp(1.0, -24) * kSpecTheta;
  const double ka64 = kSpecKAPost + kSpecKARoundA + 2 * kSpecKARound4 + kSpecKAPre;
  const double ka128 = ka64 + kSpecKARound2;
  const double ka16 = kSpecKAPost + kSpecKARoundA + kSpecKARound4 + kSpecKAPre;
  for (int b = 0; b < 3; b++) {
    const double n = b == 2 ? 128 : 64, sg2 = b == 2 ? s512 : s256;
    d->spec_cz[b] = round_up_f32(u * (b == 2 ? ka128 : ka64) * std::sqrt(sg2 * n));
    const double gb = u * sg2 * std::sqrt(2 * n);
    if (b == 2) { d->spec_cw[b] = round_up_f32(gb * (5 * kSpecGH + kSpecGQ)); d->spec_cl[b] = 0.0f; }
    else { d->spec_cw[b] = round_up_f32(gb * kSpecGH * kSpecGQ); d->spec_cl[b] = round_up_f32(gb * (7 * kSpecGH + kSpecGQ)); }
    d->spec_cz_short[b] = round_up_f32(u * ka16 * std::sqrt(s64 * 16));
    const double gs = u * s64 * std::sqrt(2.0 * 16);
    if (b == 2) { d->spec_cw_short[b] = round_up_f32(gs * (5 * kSpecGH + kSpecGQ)); d->spec_cl_short[b] = 0.0f; }
    else { d->spec_cw_short[b] = round_up_f32(gs * kSpecGH * kSpecGQ); d->spec_cl_short[b] = round_up_f32(gs * (7 * kSpecGH + kSpecGQ)); }
  }
  d->spec_cz[3] = d->spec_cw[3] = d->spec_cl[3] = d->spec_cz_short[3] = d->spec_cw_short[3] = d->spec_cl_short[3] = 0.0f;
  d->spec_eabs = (float)std::ldexp(1.0, -70);
  // speculative transient detector (c1_detect_bound.h): Delta_b = K u theta sqrt(n) ||band samples|| + eabs
  for (int b = 0; b < 3; b++)
    d->det_ck[b] = round_up_f32(std::ldexp(1.0, -24) * C1_DET_THETA * (b == 2 ? C1_DET_K256 * 16.0 : C1_DET_K128 * std::sqrt(128.0)));
  d->det_ck[3] = 0.0f;
  d->det_eabs = round_up_f32(C1_DET_EABS);
  d->spec_ok = ok ? 1 : 0;
}

void build_device_tables(const c1_tables &t, C1DevTables *d) {
  memset(d, 0, sizeof *d);
  qmf_even_taps(d->tap_e);
  for (int j = 0; j < 24; j++) d->tap_o[j] = d->tap_e[23 - j];
  memcpy(d->window, t.window_short, sizeof d->window);
  memcpy(d->mdct_fwd64, t.mdct_fwd64, sizeof d->mdct_fwd64);
  memcpy(d->mdct_fwd256, t.mdct_fwd256, sizeof d->mdct_fwd256);
  memcpy(d->mdct_fwd512, t.mdct_fwd512, sizeof d->mdct_fwd512);
  memcpy(d->mdct_inv64, t.mdct_inv64, sizeof d->mdct_inv64);
  memcpy(d->mdct_inv256, t.mdct_inv256, sizeof d->mdct_inv256);
  memcpy(d->mdct_inv512, t.mdct_inv512, sizeof d->mdct_inv512);
  // twiddle recurrence of FFT.fft (fft.js:44-64): starts at (1,0), advanced by a complex multiply in
  // double, unfused; it does not depend on the data, so it is tabulated once per stride
  int stage = 0;
  for (int h = 1; h <= 128; h <<= 1, stage++) {
    const double wr = t.fft_w[stage][0], wi = t.fft_w[stage][1];
    double tr = 1.0, ti = 0.0;
    for (int k = 0; k < h; k++) {
      d->fft_tw[h - 1 + k][0] = tr;
      d->fft_tw[h - 1 + k][1] = ti;
      const double nr = tr * wr - ti * wi;
      ti = tr * wi + ti * wr;
      tr = nr;
    }
  }
  memcpy(d->scale_factors, t.scale_factors, sizeof d->scale_factors);
  for (int s = 0; s < 64; s++)
    for (int wl = 0; wl < 16; wl++) {
      const int bits = wl == 0 ? 0 : wl + 1;
      const int range = bits ? (1 << (bits - 1)) - 1 : 0;
      d->norm[s * 16 + wl] = (double)range / t.scale_factors[s];  // quantization.js:42-44
    }
  d->log1p10 = t.log1p_10;
  // Float32 thresholds of findScaleFactor: for a binary32 m, m > B[i] <=> m > floor_f32(B[i]).  The reference computes
  // ceil(3 (log2 m + 21)) and never reads SCALE_FACTORS there, so the boundaries B are the powers 2^(i/3-21) whatever table
  // is installed: the default table, whose compare tests/golden/find_scale_factor.json pins to the log2 form.  Every
  // octave of B has the same two fraction patterns, so the kernels always read the index off the bit pattern.  sf_fast asks
  // the installed table for that structure too: the speculative paths require it (build_spec_tables).
  auto floor_f32_bits = [](double x) -> uint32_t {
    float f = (float)x;
    if ((double)f > x) f = std::nextafterf(f, 0.0f);
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
  };
  d->sf_m1 = floor_f32_bits(C1D_SCALE_FACTORS[1]) & 0x7fffffu;
  d->sf_m2 = floor_f32_bits(C1D_SCALE_FACTORS[2]) & 0x7fffffu;
  d->sf_fast = 1;
  const uint32_t tm1 = floor_f32_bits(t.scale_factors[1]) & 0x7fffffu, tm2 = floor_f32_bits(t.scale_factors[2]) & 0x7fffffu;
  for (int i = 0; i < 64; i++) {
    const uint32_t u = floor_f32_bits(t.scale_factors[i]);
    const int e = (int)(u >> 23) - 127, want_e = i / 3 - 21;
    const uint32_t frac = u & 0x7fffffu, want = i % 3 == 0 ? 0u : (i % 3 == 1 ? tm1 : tm2);
    const bool exact_pow2 = i % 3 != 0 || (double)std::ldexp(1.0f, want_e) == t.scale_factors[i];
    if (e != want_e || frac != want || !exact_pow2) d->sf_fast = 0;
  }
  // dequantize (quantization.js:65-78): Float32((q * SF) / range).  One correctly rounded reciprocal, a multiply
  // and two FMAs give the correctly rounded quotient (Markstein); rather than rely on the theorem's side
  // conditions, compare against the division for every input the decoder can meet with this table.
  d->dq_fast = 1;
  d->dq_step = 1;
  for (int wl = 1; wl < 16 && d->dq_fast; wl++) {
    const int bits = wl + 1;
    const double range = (double)((1 << (bits - 1)) - 1), y = 1.0 / range;
    d->inv_range[wl] = y;
    for (int s = 1; s < 64 && d->dq_fast; s++) {
      const double sf = t.scale_factors[s];
      for (int q = -(1 << (bits - 1)); q < (1 << (bits - 1)); q++) {
        const double a = (double)q * sf;
        const double q0 = a * y, r = std::fma(-q0, range, a), fast = std::fma(r, y, q0), exact = a / range;
        if (!(fast == exact) || std::signbit(fast) != std::signbit(exact)) { d->dq_fast = 0; break; }
        // after the store to the Float32 array even the plain product with one rounded step per BFU is the same value
        const float f_exact = (float)exact, f_step = (float)((double)q * (sf * y));
        if (!(f_step == f_exact) || std::signbit(f_step) != std::signbit(f_exact)) d->dq_step = 0;
      }
    }
  }
  if (!d->dq_fast || getenv("C1_NO_DQ_STEP")) d->dq_step = 0;      // the variable: tests of the reciprocal form, which the step form shadows
  build_spec_tables(t, d);
}

// rank table of the Float32 heap priorities (bitallocation.js:226-231, 267-269)
// C1DevEncOpts = the fields of this call (threshold, block modes: fill_call_fields, run on every call) + what derives from
// the biased scale-factor table alone (the table itself, its log2 line, the rank tables and their integer form:
// build_table_fields).  The search for an integer form costs ~30 M host operations when there is none, so the last few
// table-derived parts are kept; nothing that depends on another option may live in that cache.
int fill_call_fields(const c1_encode_options &o, C1DevEncOpts *d) {
  if (std::isnan(o.transient_threshold)) return fail(C1_ERR_ARG, "transient_threshold is NaN");
  d->threshold = o.transient_threshold;
  const bool detect = o.fixed_block_modes[0] < 0;
  for (int b = 0; b < 3; b++) {
    const int m = o.fixed_block_modes[b];
    if (detect) { d->modes[b] = -1; continue; }
    if (m < 0 || m > (b == 2 ? 3 : 2))
      return fail(C1_ERR_ARG, "fixed_block_modes[%d] = %d is outside 0..%d", b, m, b == 2 ? 3 : 2);
    d->modes[b] = m;
  }
  static const int no_tonal = getenv("C1_ALLOC_NO_TONAL") ? atoi(getenv("C1_ALLOC_NO_TONAL")) : 0;
  d->alloc_no_tonal = no_tonal;                          // experiments: 1 = always run the 52-BFU candidate first
  return C1_OK;
}

int build_table_fields(const c1_encode_options &o, C1DevEncOpts *d);

int build_encode_opts(const c1_encode_options &o, C1DevEncOpts *d) {
  struct Entry { double biased[64]; C1DevEncOpts table_part; };
  static std::mutex mu;
  static std::vector<Entry> cache;
  bool hit = false;
  {
    std::lock_guard<std::mutex> lock(mu);
    for (const Entry &e : cache)
      if (memcmp(e.biased, o.biased_scale_factors, sizeof e.biased) == 0) { *d = e.table_part; hit = true; break; }
  }
  if (!hit) {
    const int rc = build_table_fields(o, d);
    if (rc) return rc;
    std::lock_guard<std::mutex> lock(mu);
    if (cache.size() >= 8) cache.erase(cache.begin());
    Entry e;
    memcpy(e.biased, o.biased_scale_factors, sizeof e.biased);
    e.table_part = *d;
    cache.push_back(e);
  }
  return fill_call_fields(o, d);
}

int build_table_fields(const c1_encode_options &o, C1DevEncOpts *d) {
  memset(d, 0, sizeof *d);
  for (int i = 0; i < 64; i++) {
    if (!std::isfinite(o.biased_scale_factors[i]) || o.biased_scale_factors[i] < 0)
      return fail(C1_ERR_ARG, "biased_scale_factors[%d] is not a finite non-negative number", i);
    d->biased[i] = o.biased_scale_factors[i];
  }
  {
    // log2 of the biased table as a line in the index (exact for pow(2^(s/3-21), bias)); see C1DevEncOpts
    const double l1 = std::log2(d->biased[1]), l63 = std::log2(d->biased[63]);
    const double slope = (l63 - l1) / 62.0;
    d->la_slope = (std::isfinite(slope) && std::isfinite(l1)) ? (float)slope : 0.0f;
    d->la_off = (std::isfinite(slope) && std::isfinite(l1)) ? (float)(l1 - slope) : 0.0f;
  }
  float pri[64 * 15];
  std::vector<float> uniq;
  for (int s = 1; s < 64; s++)
    for (int wl = 0; wl < 15; wl++) {
      const int b0 = wl == 0 ? 0 : wl + 1, b1 = wl + 2;
      const double ddf = wl == 0 ? 2.0 - std::ldexp(1.0, -b1) : std::ldexp(1.0, -b0) - std::ldexp(1.0, -b1);
      const double dbits = (double)(b1 - b0);
      pri[s * 15 + wl] = (float)(d->biased[s] * ddf / dbits);
      uniq.push_back(pri[s * 15 + wl]);
    }
  std::sort(uniq.begin(), uniq.end());
  uniq.erase(std::unique(uniq.begin(), uniq.end()), uniq.end());
  for (int s = 1; s < 64; s++)
    for (int wl = 0; wl < 15; wl++) {
      const auto it = std::lower_bound(uniq.begin(), uniq.end(), pri[s * 15 + wl]);
      d->rank[s * 16 + wl] = (uint16_t)(1 + (it - uniq.begin()));
    }
  // Is the order of the ranks the order of an integer form?  (bias 1: priority = 2^(s/3-21) * {0.875 | 2^-(wl+2)}
  // -> 2s-1 for wl = 0 and 2s - 6wl - 12 for wl >= 1, i.e. A = 2, B = 6, C = 5 in the form below: the wl = 0 term
  // sits above the wl = 1 term of the same sfi, so C is searched on both sides of zero.)  Search small coefficients;
  // ties must match too.
  d->rank_affine = 0;
  {
    std::vector<int> order;                       // (s, wl) pairs sorted by rank
    for (int s = 1; s < 64; s++)
      for (int wl = 0; wl < 15; wl++) order.push_back(s * 16 + wl);
    std::sort(order.begin(), order.end(), [&](int x, int y) { return d->rank[x] < d->rank[y]; });
    for (int A = 1; A <= 12 && !d->rank_affine; A++)
      for (int B = 1; B <= 36 && !d->rank_affine; B++)
        for (int C = -2 * B; C <= 2 * B && !d->rank_affine; C++) {
          auto key = [&](int idx) { const int s = idx >> 4, wl = idx & 15; return wl == 0 ? A * s + C : A * s - B * wl - B; };
          bool ok = true;
          int lo = key(order[0]), hi = lo;
          for (size_t i = 1; i < order.size() && ok; i++) {
            const int k0 = key(order[i - 1]), k1 = key(order[i]);
            const bool req = d->rank[order[i]] == d->rank[order[i - 1]];
            if (req ? (k1 != k0) : !(k1 > k0)) ok = false;
            lo = std::min(lo, k1); hi = std::max(hi, k1);
          }
          if (ok && hi - lo + 1 < 1023) {
            d->rank_affine = 1; d->rank_a = A; d->rank_b = B; d->rank_c = C; d->rank_off = 1 - lo;
          }
        }
  }
  // With the integer form, a successful step of the spending loop is one addition to the root's heap entry
  // (rank(10) | size(5) | sfi(6) | wl(4) | bfu(6), c1_k_allocate.hip): word length + 1, rank - B (from word length 0:
  // rank - 2B - C).  Walk every (sfi, wl) with the two steps; anything out of line and the kernels read the table.
  if (d->rank_affine) {
    const int A = d->rank_a, B = d->rank_b, C = d->rank_c, off = d->rank_off;
    auto rk = [&](int s, int wl) { return wl == 0 ? A * s + C + off : A * s + off - B * (wl + 1); };
    auto entry = [&](int s, int wl) { return ((uint32_t)rk(s, wl) << 21) | ((uint32_t)s << 10) | ((uint32_t)wl << 6); };
    d->rank_step0 = (1u << 6) + ((uint32_t)(-2 * B - C) << 21);
    d->rank_step = (1u << 6) - ((uint32_t)B << 21);
    bool ok = true;
    for (int s = 1; s < 64 && ok; s++)
      for (int wl = 0; wl < 15 && ok; wl++) {
        if (rk(s, wl) < 1 || rk(s, wl) > 1022) ok = false;
        if (wl < 14 && entry(s, wl) + (wl == 0 ? d->rank_step0 : d->rank_step) != entry(s, wl + 1)) ok = false;
      }
    if (!ok) { d->rank_affine = 0; d->rank_step0 = d->rank_step = 0; }
  }
  // The terms of calculateTotalDistortion (bitallocation.js:157-190) per BFU size and sfi: see C1DevEncOpts::dist.
  // (b * 2^-k) * n == (b * n) * 2^-k as long as neither side leaves the normal range, and then multiplying by 2^-k is
  // subtracting k from the exponent field; the installed table may hold anything, so every case is tried here.
  {
    bool ok = true;
    for (int c = 0; c < 8; c++) {
      const double size = (double)kDistSizes[c];
      for (int s = 0; s < 64; s++) {
        const double bs = d->biased[s];
        const double zb = s != 0 ? (double)(float)(bs * 2.0 * size) : 0.0;     // zeroBitDistortions (:76, 87-89)
        const double cs = bs * size;
        d->dist[c][s][0] = zb;
        d->dist[c][s][1] = cs;
        if (s == 0) continue;
        if (!(zb >= (double)std::numeric_limits<float>::min())) ok = false;   // a binary32 subnormal: leave it to the device's own conversion
        uint64_t u;
        memcpy(&u, &cs, sizeof u);
        for (int wl = 1; wl <= 15; wl++) {
          const int bits = wl + 1;
          const double want = bs * std::ldexp(1.0, -bits) * size;               // (:183-187): biased * INV_POWER_OF_TWO[bits] * size
          if ((int)((u >> 52) & 0x7ff) <= bits || (int)((u >> 52) & 0x7ff) == 0x7ff) { ok = false; continue; }
          const uint64_t v = u - ((uint64_t)bits << 52);
          if (memcmp(&v, &want, sizeof v) != 0) ok = false;
        }
      }
    }
    d->dist_tables = (ok && !getenv("C1_NO_DIST_TABLES")) ? 1 : 0;
  }
  return C1_OK;
}

constexpr int kTotals = 8;                             // running totals of a context (c1_ctx::d_spec_totals)
constexpr int64_t kSpecMinUnits = 64;                  // default mode: calls below this many sound units use the exact kernels only
constexpr int kListHead = 8;                           // uint32 counters in front of the speculative path's lists
constexpr int64_t kMaxModesBatchFrames = (int64_t)1 << 22;   // c1_encode_modes_batch: one staging buffer for the whole call
constexpr int64_t kMaxChunkFrames = (int64_t)1 << 27;   // x 2 channels = 2^28 units per chunk < 2^29
constexpr bool kSignalStartsFused = false;             // c1_encode_signals_measured*'s default route; C1_SIGNAL_STARTS overrides

struct Timing {
  hipEvent_t start, stop;
  int kind;
};
enum { K_ANALYSIS = 0, K_ALLOCATE, K_PACK, K_DECODE, K_REDO, K_PACK_UNITS, K_DECODE_FIELDS, K_FROM_STATE, K_SIGNAL_STARTS, K_CHOOSE, K_MEASURE, K_METER, K_METER_PCM, K_KINDS };
const char *const kKindNames[K_KINDS] = {"analysis", "allocate", "pack", "decode", "redo", "pack_units", "decode_fields", "from_state", "signal_starts", "choose", "measure", "meter", "meter_pcm"};

}  // namespace

struct c1_ctx {
  // Every public entry point that touches the context holds this for its whole duration: calls on one context are
  // serialised on the host (workspace, staging buffers, option cache and timings are per context), as the GPU side
  // already is by the context's stream.  Recursive because entry points call each other (batch -> device, ...).
  std::recursive_mutex mu;
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  C1DevTables *d_tables = nullptr;
  C1DevEncOpts *d_opts = nullptr;
  c1_encode_options last_opts;
  bool have_opts = false;
  // workspace: two chunk-sized sets, so chunk i+1's analysis overlaps chunk i's allocation and packing
  int64_t ws_units = 0;
  float *d_coefs[2] = {nullptr, nullptr};
  uint8_t *d_side[2] = {nullptr, nullptr};
  uint8_t *d_alloc[2] = {nullptr, nullptr};
  uint8_t *d_cand[2] = {nullptr, nullptr};
  uint32_t *d_work[2] = {nullptr, nullptr};      // [0] = count, list from [4]
  // speculative binary32 path: per-unit error bounds, redo list ([0] = count, list from [4]), running totals
  float *d_eps[2] = {nullptr, nullptr};
  uint32_t *d_redo[2] = {nullptr, nullptr};
  // running totals on the device: [0] units that stayed with the speculative analysis, [1] units among them redone exactly,
  // [2] units of exact coefficients quantized in binary32, [3] units among them packed again, [4] units the speculative
  // detector decided, [5] units among them rechecked, [6] units the speculative analysis handed to the exact kernels.
  // Statistics only (c1_ctx_*_stats): no decision of the encode path reads them.
  unsigned long long *d_spec_totals = nullptr;
  int spec_mode = 1;                             // 0 exact only, 1 material-local (default), 2 always speculate
  float spec_defer = 1.0f;                       // mode 1: predicted open decisions per unit past which a run goes to the exact kernels
  bool decode_binary32 = false;                  // c1_ctx_set_decode_precision: opt-in binary32 decoder
  int decode_model = C1_DECODE_EXACT;            // c1_ctx_set_decode_model; decode_binary32 == (decode_model != C1_DECODE_EXACT)
  bool spec_tables_ok = false;
  // transient-detection workspace (allocated on first use): band samples, feature sums, block modes
  int64_t det_units = 0;
  float *d_bands[2] = {nullptr, nullptr};
  double *d_feat[2] = {nullptr, nullptr};
  uint8_t *d_modes[2] = {nullptr, nullptr};
  uint32_t *d_lists[2] = {nullptr, nullptr};
  // allocation bias per unit (c1_encode_biases_device): the palette's tables in device form, the tables uploaded last, and the
  // unit lists of one chunk ([0, 8) counts, then one list per entry); all allocated on first use
  C1DevEncOpts *d_palette = nullptr;
  // the masking tables of c1_encode_measured_masked_device, uploaded by every such call: floor[52], then the spreading matrix
  // transposed; a page-locked staging copy and the event of the last upload from it.  Allocated on first use
  double *d_mask = nullptr, *h_mask = nullptr;
  hipEvent_t ev_mask = nullptr;
  double pal_tables[C1_MAX_BIAS_PALETTE][64];
  int pal_n = 0;
  uint32_t *d_pal_lists = nullptr;
  int64_t pal_entries = 0;
  // the bias chosen per unit (c1_encode_best_bias_device): one allocation record per unit and palette entry of one chunk, entry
  // k's records at d_trial + k * trial_units * kAllocBytes; allocated on first use
  uint8_t *d_trial = nullptr;
  int64_t trial_units = 0, trial_n = 0;
  // the block modes chosen per unit (c1_encode_best_modes_device): the coefficients and side records of one chunk's second
  // (all-short) analysis and the side records composed for one candidate at a time; allocated on first use
  float *d_bm_coefs = nullptr;
  uint8_t *d_bm_side = nullptr, *d_bm_cand_side = nullptr;
  int64_t bm_units = 0;
  // Tail overlap: the exact redo of a speculative chunk -- short lists, latency-bound launches -- runs on
  // s_tail while the next chunk's (or, on a context that owns its stream, the next call's) main kernels run on the
  // context's stream; the two chunks work on different halves of the workspace.  ev_main[p] / ev_tail[p]: main part /
  // tail of the chunk that last used half p.  tail_pending: a tail is in flight that the context's stream has not
  // been made to wait for yet (join_tail); every entry point but the device encode joins before it does anything.
  bool overlap = false;
  hipStream_t s_tail = nullptr;
  hipEvent_t ev_main[2] = {nullptr, nullptr}, ev_tail[2] = {nullptr, nullptr};
  bool tail_used[2] = {false, false};
  bool tail_pending = false;
  int ws_next = 0;
  int64_t chunk_frames = 0;
  bool pipeline = true;
  int measured_wide = -1;                         // C1_MEASURED_WIDE: -1 unset (the threshold decides), 0 never, 1 always
  bool signal_starts_fused = false;               // C1_SIGNAL_STARTS: the route of c1_encode_signals_measured*'s signal starts
  hipStream_t s_ana = nullptr, s_rest = nullptr;  // internal streams of the two pipeline halves
  hipEvent_t ev_in = nullptr, ev_ana[2] = {nullptr, nullptr}, ev_free[2] = {nullptr, nullptr}, ev_end[2] = {nullptr, nullptr};
  // profiling
  int timing_depth = 0;                          // > 0 inside a multi-chunk host call: the per-chunk device calls keep the timings
  bool profiling = false;
  std::vector<Timing> timings;
  std::vector<hipEvent_t> event_pool;
  double ms[K_KINDS] = {};
  int launches[K_KINDS] = {};
  // scratch for host-resident calls
  void *d_io = nullptr;
  size_t d_io_bytes = 0;
  // the signals entry points: device scratch of one call (index lists, states in flight, rows of units or frame fields) and
  // the page-locked image the index lists are uploaded from; ev_rows: that upload is through, the image may be rewritten
  void *d_sig = nullptr;
  size_t d_sig_bytes = 0;
  uint32_t *h_rows = nullptr;
  size_t h_rows_bytes = 0;
  hipEvent_t ev_rows = nullptr;
  bool rows_pending = false;
  // streamed host path (pinned buffers): copy streams, two chunk-sized staging sets and their events
  hipStream_t s_up = nullptr, s_down = nullptr;
  void *d_ring = nullptr;
  size_t d_ring_bytes = 0;
  hipEvent_t ev_up[2] = {nullptr, nullptr}, ev_run[2] = {nullptr, nullptr}, ev_down[2] = {nullptr, nullptr};
};

namespace {

#define CTX_GUARD(c)                                   \
  std::unique_lock<std::recursive_mutex> ctx_guard_;   \
  if (c) ctx_guard_ = std::unique_lock<std::recursive_mutex>((c)->mu)

// the context's stream waits for every tail in flight: from here on it sees the finished results of all earlier calls
int join_tail(c1_ctx *ctx) {
  if (!ctx->tail_pending) return C1_OK;
  for (int p = 0; p < 2; p++)
    if (ctx->tail_used[p]) HIP_TRY(hipStreamWaitEvent(ctx->stream, ctx->ev_tail[p], 0));
  ctx->tail_pending = false;
  return C1_OK;
}

int ctx_bind(c1_ctx *ctx, bool join = true) {
  if (!ctx) return fail(C1_ERR_ARG, "context is NULL");
  HIP_TRY(hipSetDevice(ctx->device));
  if (join) return join_tail(ctx);
  return C1_OK;
}

void free_workspace(c1_ctx *ctx) {
  for (int p = 0; p < 2; p++) {
    if (ctx->d_coefs[p]) (void)hipFree(ctx->d_coefs[p]);
    if (ctx->d_side[p]) (void)hipFree(ctx->d_side[p]);
    if (ctx->d_alloc[p]) (void)hipFree(ctx->d_alloc[p]);
    if (ctx->d_cand[p]) (void)hipFree(ctx->d_cand[p]);
    if (ctx->d_work[p]) (void)hipFree(ctx->d_work[p]);
    if (ctx->d_eps[p]) (void)hipFree(ctx->d_eps[p]);
    if (ctx->d_redo[p]) (void)hipFree(ctx->d_redo[p]);
    ctx->d_coefs[p] = nullptr; ctx->d_side[p] = nullptr; ctx->d_alloc[p] = nullptr; ctx->d_cand[p] = nullptr; ctx->d_work[p] = nullptr;
    ctx->d_eps[p] = nullptr; ctx->d_redo[p] = nullptr;
  }
  ctx->ws_units = 0;
  for (int p = 0; p < 2; p++) {
    if (ctx->d_bands[p]) (void)hipFree(ctx->d_bands[p]);
    if (ctx->d_feat[p]) (void)hipFree(ctx->d_feat[p]);
    if (ctx->d_modes[p]) (void)hipFree(ctx->d_modes[p]);
    if (ctx->d_lists[p]) (void)hipFree(ctx->d_lists[p]);
    ctx->d_bands[p] = nullptr; ctx->d_feat[p] = nullptr; ctx->d_modes[p] = nullptr; ctx->d_lists[p] = nullptr;
  }
  ctx->det_units = 0;
  if (ctx->d_pal_lists) (void)hipFree(ctx->d_pal_lists);
  ctx->d_pal_lists = nullptr;
  ctx->pal_entries = 0;
  if (ctx->d_trial) (void)hipFree(ctx->d_trial);
  ctx->d_trial = nullptr;
  ctx->trial_units = ctx->trial_n = 0;
  if (ctx->d_bm_coefs) (void)hipFree(ctx->d_bm_coefs);
  if (ctx->d_bm_side) (void)hipFree(ctx->d_bm_side);
  if (ctx->d_bm_cand_side) (void)hipFree(ctx->d_bm_cand_side);
  ctx->d_bm_coefs = nullptr; ctx->d_bm_side = nullptr; ctx->d_bm_cand_side = nullptr;
  ctx->bm_units = 0;
}

int ensure_detect_workspace(c1_ctx *ctx, int64_t units) {
  if (units <= ctx->det_units) return C1_OK;
  HIP_TRY(hipDeviceSynchronize());
  for (int p = 0; p < (ctx->pipeline ? 2 : 1); p++) {
    if (ctx->d_bands[p]) (void)hipFree(ctx->d_bands[p]);
    if (ctx->d_feat[p]) (void)hipFree(ctx->d_feat[p]);
    if (ctx->d_modes[p]) (void)hipFree(ctx->d_modes[p]);
    if (ctx->d_lists[p]) (void)hipFree(ctx->d_lists[p]);
    ctx->d_bands[p] = nullptr; ctx->d_feat[p] = nullptr; ctx->d_modes[p] = nullptr; ctx->d_lists[p] = nullptr;
    // one extra row of slots in front: frame -1 of the batch (c1_internal.h)
    HIP_TRY(hipMalloc(&ctx->d_bands[p], (size_t)(units + C1_MAX_CHANNELS) * 512 * sizeof(float)));
    HIP_TRY(hipMalloc(&ctx->d_feat[p], (size_t)(units + C1_MAX_CHANNELS) * kFeatureWsDoubles * sizeof(double)));
    HIP_TRY(hipMalloc(&ctx->d_modes[p], (size_t)units));
    HIP_TRY(hipMalloc(&ctx->d_lists[p], ((size_t)units * 3 + 4) * sizeof(uint32_t)));
  }
  ctx->det_units = units;
  return C1_OK;
}

int ensure_workspace(c1_ctx *ctx, int64_t units) {
  if (units <= ctx->ws_units) return C1_OK;
  HIP_TRY(hipDeviceSynchronize());
  free_workspace(ctx);
  ctx->tail_used[0] = ctx->tail_used[1] = false;
  ctx->tail_pending = false;
  for (int p = 0; p < ((ctx->pipeline || ctx->overlap) ? 2 : 1); p++) {
    HIP_TRY(hipMalloc(&ctx->d_coefs[p], (size_t)units * 512 * sizeof(float)));
    HIP_TRY(hipMalloc(&ctx->d_side[p], (size_t)units * kSideBytes));
    HIP_TRY(hipMalloc(&ctx->d_alloc[p], (size_t)units * kAllocBytes));
    HIP_TRY(hipMalloc(&ctx->d_cand[p], (size_t)units * kCandidateBytes));
    HIP_TRY(hipMalloc(&ctx->d_work[p], ((size_t)units * 8 + 4) * sizeof(uint32_t)));
    HIP_TRY(hipMalloc(&ctx->d_eps[p], (size_t)units * kEpsFloats * sizeof(float)));
    HIP_TRY(hipMalloc(&ctx->d_redo[p], ((size_t)units * 4 + kListHead + 64) * sizeof(uint32_t)));   // counts, then four lists (bind_lists) + slack for the masks of tiny batches
  }
  ctx->ws_units = units;
  return C1_OK;
}

// Frames per chunk of an encode call.  Every kernel of the chain ends in a tail of draining workgroups and the allocation's
// later rounds are bound by the latency of one heap run whatever their list's length, so a batch is best kept in ONE chunk
// (BASELINE configs[3]'s share of 12.5 M stereo frames: 130.7 M frames/s in chunks of 1 M, 138.9 M in chunks of 4 M, 144.7 M
// in one) -- the workspace costs 2.6 KB per unit (4.8 KB with transient detection) and this part has 288 GB.  The configured
// chunk (C1_CHUNK_FRAMES, default 2^24 frames) is cut down to what the device can hold right now next to the caller's
// buffers; a workspace that is already large enough is used as it is.
constexpr size_t kWsBytesPerUnit = 512 * sizeof(float) + kSideBytes + kAllocBytes + kCandidateBytes + 8 * sizeof(uint32_t) + kEpsFloats * sizeof(float) + 4 * sizeof(uint32_t);
constexpr size_t kDetectWsBytesPerUnit = 512 * sizeof(float) + kFeatureWsDoubles * sizeof(double) + 1 + 3 * sizeof(uint32_t);
// trial_n > 0 (c1_encode_best_bias_device): that many trial allocation records per unit on top (one set: only the second half
// of the pipeline touches them)
// best_modes (c1_encode_best_modes_device): the second analysis' coefficients and side records and one candidate's side records
// on top (one set: such a call is not pipelined)
constexpr size_t kBestModesWsBytesPerUnit = 512 * sizeof(float) + 2 * kSideBytes;
int64_t chunk_for_call(c1_ctx *ctx, int64_t frames, int channels, bool detect, int trial_n = 0, bool best_modes = false) {
  const int64_t want = std::min(frames, ctx->chunk_frames);
  const bool trial_fits = trial_n == 0 || (want * channels <= ctx->trial_units && trial_n <= ctx->trial_n);
  if (want * channels <= ctx->ws_units && (!detect || want * channels <= ctx->det_units) && trial_fits &&
      (!best_modes || want * channels <= ctx->bm_units)) return want;
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void)hipGetLastError(); return std::min<int64_t>(want, 1048576); }
  const size_t sets = (ctx->pipeline || ctx->overlap) ? 2 : 1, det_sets = ctx->pipeline ? 2 : 1;
  size_t avail = free_b + (size_t)ctx->ws_units * kWsBytesPerUnit * sets;          // the present workspace is freed before it grows
  size_t per_unit = kWsBytesPerUnit * sets;
  if (detect) { avail += (size_t)ctx->det_units * kDetectWsBytesPerUnit * det_sets; per_unit += kDetectWsBytesPerUnit * det_sets; }
  if (trial_n > 0) { avail += (size_t)ctx->trial_units * ctx->trial_n * kAllocBytes; per_unit += (size_t)trial_n * kAllocBytes; }
  if (best_modes) { avail += (size_t)ctx->bm_units * kBestModesWsBytesPerUnit; per_unit += kBestModesWsBytesPerUnit; }
  const int64_t fit = (int64_t)((double)avail * 0.9 / (double)per_unit) / channels;
  return std::max<int64_t>(16, std::min(want, fit));
}

// the lists of the speculative path in workspace half p: counts at [0, kListHead), then the redo, reallocation,
// re-analysis and deferred-run lists, ws_units entries each
void bind_lists(c1_ctx *ctx, int p, C1EncodeLaunch *L) {
  uint32_t *base = ctx->d_redo[p];
  const size_t u = (size_t)ctx->ws_units;
  L->redo_count = base;
  L->realloc_count = base + 1;
  L->reana_count = base + 2;
  L->redo_list = base + kListHead;
  L->realloc_list = base + kListHead + u;
  L->reana_list = base + kListHead + 2 * u;
}
void bind_defer(c1_ctx *ctx, int p, C1EncodeLaunch *L) {
  L->defer_list = ctx->d_redo[p] + kListHead + 3 * (size_t)ctx->ws_units;   // one slot per run and channel (<= units)
}

int ensure_io(c1_ctx *ctx, size_t bytes) {
  if (bytes <= ctx->d_io_bytes) return C1_OK;
  if (ctx->d_io) hipFree(ctx->d_io);
  ctx->d_io = nullptr; ctx->d_io_bytes = 0;
  HIP_TRY(hipMalloc(&ctx->d_io, bytes));
  ctx->d_io_bytes = bytes;
  return C1_OK;
}

int upload_opts(c1_ctx *ctx, const c1_encode_options *opts) {
  if (!opts) return fail(C1_ERR_ARG, "options are NULL");
  if (ctx->have_opts && memcmp(&ctx->last_opts, opts, sizeof *opts) == 0) return C1_OK;
  C1DevEncOpts h;
  const int rc = build_encode_opts(*opts, &h);
  if (rc) return rc;
  // the previous options may still be in use by kernels queued on the stream (or on the tail stream)
  int jr = join_tail(ctx);
  if (jr) return jr;
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  HIP_TRY(hipMemcpy(ctx->d_opts, &h, sizeof h, hipMemcpyHostToDevice));
  ctx->last_opts = *opts;
  ctx->have_opts = true;
  return C1_OK;
}

// One call's palette (c1_encode_biases_*): entries on the device, the index bytes of the call's units (device memory)
struct PaletteCall {
  int n;
  const uint8_t *index;
};

// The palette's tables in device form.  Of an entry only what derives from its biased scale factors reaches a kernel (the
// allocation chain reads nothing else), so only the tables are compared with what was uploaded last; a change waits for the
// kernels that may still read the old ones, as upload_opts does.  An invalid table: C1_ERR_ARG naming the entry
// host only: the size, every entry's table, and -- call_fields: the entries' threshold and block modes decide (a batch call
// without given modes) -- those fields of every entry, which must then agree (threshold bit for bit)
int check_palette(const char *what, const c1_encode_options *palette, int n, bool call_fields) {
  if (n < 1 || n > C1_MAX_BIAS_PALETTE) return fail(C1_ERR_ARG, "%s: n_palette = %d is outside 1..%d", what, n, C1_MAX_BIAS_PALETTE);
  if (!palette) return fail(C1_ERR_ARG, "%s: palette is NULL", what);
  std::unique_ptr<C1DevEncOpts> d(new C1DevEncOpts);
  for (int k = 0; k < n; k++) {
    c1_encode_options o = palette[k];
    if (!call_fields) {
      o.transient_threshold = 1.0;
      o.fixed_block_modes[0] = o.fixed_block_modes[1] = o.fixed_block_modes[2] = -1;
    }
    const int rc = build_encode_opts(o, d.get());
    if (rc) { const std::string inner = g_error; return fail(rc, "%s: palette entry %d: %s", what, k, inner.c_str()); }
    if (call_fields && k > 0) {
      if (memcmp(&palette[k].transient_threshold, &palette[0].transient_threshold, sizeof(double)) != 0)
        return fail(C1_ERR_ARG, "%s: palette entry %d: transient_threshold differs from entry 0's, and no modes are given", what, k);
      if (memcmp(palette[k].fixed_block_modes, palette[0].fixed_block_modes, sizeof palette[0].fixed_block_modes) != 0)
        return fail(C1_ERR_ARG, "%s: palette entry %d: fixed_block_modes differ from entry 0's, and no modes are given", what, k);
    }
  }
  return C1_OK;
}

// host only: the options of a measured-allocation call, as upload_opts will judge them (call_fields false: modes are given, and
// neither the threshold nor the fixed modes are read)
int check_measured_opts(const char *what, const c1_encode_options *opts, bool call_fields) {
  if (!opts) return fail(C1_ERR_ARG, "%s: options are NULL", what);
  std::unique_ptr<C1DevEncOpts> d(new C1DevEncOpts);
  c1_encode_options o = *opts;
  if (!call_fields) {
    o.transient_threshold = 1.0;
    o.fixed_block_modes[0] = o.fixed_block_modes[1] = o.fixed_block_modes[2] = -1;
  }
  const int rc = build_encode_opts(o, d.get());
  if (rc) { const std::string inner = g_error; return fail(rc, "%s: %s", what, inner.c_str()); }
  return C1_OK;
}

int upload_palette(c1_ctx *ctx, const char *what, const c1_encode_options *palette, int n) {
  bool same = ctx->d_palette && ctx->pal_n >= n;
  for (int k = 0; k < n && same; k++) same = memcmp(ctx->pal_tables[k], palette[k].biased_scale_factors, sizeof ctx->pal_tables[k]) == 0;
  if (same) return C1_OK;
  std::unique_ptr<C1DevEncOpts[]> h(new C1DevEncOpts[C1_MAX_BIAS_PALETTE]);
  for (int k = 0; k < n; k++) {
    c1_encode_options o = palette[k];
    o.transient_threshold = 1.0;                           // the call fields of an entry never reach a kernel
    o.fixed_block_modes[0] = o.fixed_block_modes[1] = o.fixed_block_modes[2] = -1;
    const int rc = build_encode_opts(o, &h[k]);
    if (rc) { const std::string inner = g_error; return fail(rc, "%s: palette entry %d: %s", what, k, inner.c_str()); }
  }
  int jr = join_tail(ctx);
  if (jr) return jr;
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  if (!ctx->d_palette) HIP_TRY(hipMalloc(&ctx->d_palette, C1_MAX_BIAS_PALETTE * sizeof(C1DevEncOpts)));
  ctx->pal_n = 0;
  HIP_TRY(hipMemcpy(ctx->d_palette, h.get(), (size_t)n * sizeof(C1DevEncOpts), hipMemcpyHostToDevice));
  for (int k = 0; k < n; k++) memcpy(ctx->pal_tables[k], palette[k].biased_scale_factors, sizeof ctx->pal_tables[k]);
  ctx->pal_n = n;
  return C1_OK;
}

// unit lists of one chunk: 8 counts, then n lists of `units` entries
int ensure_palette_lists(c1_ctx *ctx, int64_t units, int n) {
  const int64_t entries = units * n;
  if (entries <= ctx->pal_entries) return C1_OK;
  HIP_TRY(hipDeviceSynchronize());
  if (ctx->d_pal_lists) (void)hipFree(ctx->d_pal_lists);
  ctx->d_pal_lists = nullptr; ctx->pal_entries = 0;
  HIP_TRY(hipMalloc(&ctx->d_pal_lists, ((size_t)entries + 8) * sizeof(uint32_t)));
  ctx->pal_entries = entries;
  return C1_OK;
}

// trial allocation records of one chunk: n planes of `units` records
int ensure_trial_allocs(c1_ctx *ctx, int64_t units, int n) {
  if (units <= ctx->trial_units && n <= ctx->trial_n) return C1_OK;
  HIP_TRY(hipDeviceSynchronize());
  if (ctx->d_trial) (void)hipFree(ctx->d_trial);
  ctx->d_trial = nullptr; ctx->trial_units = ctx->trial_n = 0;
  const int64_t u = std::max(units, ctx->trial_units), planes = std::max<int64_t>(n, ctx->trial_n);
  HIP_TRY(hipMalloc(&ctx->d_trial, (size_t)u * planes * kAllocBytes));
  ctx->trial_units = u; ctx->trial_n = planes;
  return C1_OK;
}

// the second analysis' planes and one candidate's side records of one chunk (c1_encode_best_modes_device)
int ensure_best_modes_planes(c1_ctx *ctx, int64_t units) {
  if (units <= ctx->bm_units) return C1_OK;
  HIP_TRY(hipDeviceSynchronize());
  if (ctx->d_bm_coefs) (void)hipFree(ctx->d_bm_coefs);
  if (ctx->d_bm_side) (void)hipFree(ctx->d_bm_side);
  if (ctx->d_bm_cand_side) (void)hipFree(ctx->d_bm_cand_side);
  ctx->d_bm_coefs = nullptr; ctx->d_bm_side = nullptr; ctx->d_bm_cand_side = nullptr; ctx->bm_units = 0;
  HIP_TRY(hipMalloc(&ctx->d_bm_coefs, (size_t)units * 512 * sizeof(float)));
  HIP_TRY(hipMalloc(&ctx->d_bm_side, (size_t)units * kSideBytes));
  HIP_TRY(hipMalloc(&ctx->d_bm_cand_side, (size_t)units * kSideBytes));
  ctx->bm_units = units;
  return C1_OK;
}

// One call of c1_encode_best_modes_device: the candidates (host memory, in the domain, distinct) and the call's outputs (device
// memory, each may be null)
struct BestModesCall {
  int n;
  const uint8_t *cand;
  uint8_t *choice, *modes_out;
  double *distortion, *energy;
  // c1_encode_measured_modes_device: the candidates are judged by the measured allocation's final error (k_measured_modes in
  // k_choose_modes' place); the offsets (host memory, validated) and the winner's outputs.  distortion then holds two values per
  // (unit, candidate)
  const int8_t *sf_offsets = nullptr;
  int n_offsets = 0;
  uint8_t *taken = nullptr;
  int8_t *shifts = nullptr;
  // c1_encode_measured_modes_masked_device: the uploaded tables (c1_ctx::d_mask; null for the calls above) and its output.  The
  // front end then always makes the all-long analysis: the weights come from it
  const double *mask = nullptr;
  bool has_spread = false;
  double *weights = nullptr;
};

// One call of c1_encode_best_bias_device: the palette's size and the call's outputs (device memory, each may be null)
struct BestBiasCall {
  int n;
  uint8_t *choice;
  double *distortion, *energy;
};

// One call of c1_encode_measured_device: the call's outputs (device memory, each may be null)
struct MeasuredCall {
  uint8_t *taken;
  double *distortion, *energy;
  // c1_encode_measured_sf_device: the candidate offsets (host memory, validated; null for c1_encode_measured_device) and its output
  const int8_t *sf_offsets = nullptr;
  int n_offsets = 0;
  int8_t *shifts = nullptr;
  // c1_encode_measured_masked_device: the uploaded tables (c1_ctx::d_mask; null for the calls above) and its output
  const double *mask = nullptr;
  bool has_spread = false;
  double *weights = nullptr;
};

// the first index byte that is not below n: C1_ERR_ARG naming frame and channel (of two)
int check_index_bytes(const char *what, const uint8_t *index, int64_t frames, int channels, int n) {
  for (int64_t i = 0; i < frames * channels; i++) {
    if (index[i] < n) continue;
    if (channels == 2) return fail(C1_ERR_ARG, "%s: frame %lld, channel %d: bias index %d is not below n_palette = %d", what, (long long)(i / 2), (int)(i & 1), (int)index[i], n);
    return fail(C1_ERR_ARG, "%s: frame %lld: bias index %d is not below n_palette = %d", what, (long long)i, (int)index[i], n);
  }
  return C1_OK;
}

hipEvent_t take_event(c1_ctx *ctx) {
  if (!ctx->event_pool.empty()) {
    hipEvent_t e = ctx->event_pool.back();
    ctx->event_pool.pop_back();
    return e;
  }
  hipEvent_t e;
  // timing marks only: nobody reads memory behind them, so no system-scope release (a cache write-back per record, ~5 us of
  // idle stream each; tools/prof_cost.py)
  hipEventCreateWithFlags(&e, hipEventDisableSystemFence);
  return e;
}
struct ScopedTiming {
  c1_ctx *ctx;
  Timing t;
  bool on;
  hipStream_t stream;
  ScopedTiming(c1_ctx *c, int kind, hipStream_t s = nullptr) : ctx(c), on(c->profiling), stream(s ? s : c->stream) {
    if (!on) return;
    t.kind = kind;
    t.start = take_event(ctx);
    t.stop = take_event(ctx);
    (void)hipEventRecord(t.start, stream);
  }
  ~ScopedTiming() {
    if (!on) return;
    (void)hipEventRecord(t.stop, stream);
    ctx->timings.push_back(t);
  }
};
void reset_timings(c1_ctx *ctx) {
  for (auto &t : ctx->timings) { ctx->event_pool.push_back(t.start); ctx->event_pool.push_back(t.stop); }
  ctx->timings.clear();
  for (int k = 0; k < K_KINDS; k++) { ctx->ms[k] = 0; ctx->launches[k] = 0; }
}
int collect_timings(c1_ctx *ctx) {
  if (ctx->timings.empty()) return C1_OK;
  int jr = join_tail(ctx);
  if (jr) return jr;
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  for (auto &t : ctx->timings) {
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, t.start, t.stop));
    ctx->ms[t.kind] += ms;
    ctx->launches[t.kind]++;
    ctx->event_pool.push_back(t.start);
    ctx->event_pool.push_back(t.stop);
  }
  ctx->timings.clear();
  return C1_OK;
}

// The measured step of one launch, between the allocation chain and packing: L.coefs / L.side / L.alloc hold the launch's units,
// whose outputs start at unit `at` of the call's.  A taken unit's record in L.alloc and the scale-factor bytes of its side record
// are rewritten when the launch packs (L.units), where every packing kernel reads them.  Which kernel: by the call's arguments
// (tables: c1_encode_measured_masked_device; offsets alone: _sf_; neither: c1_encode_measured_device), and the workgroup-per-unit
// kernel (c1_k_measured_wide.hip, the same outputs bit for bit) for a launch of at most kMeasuredWideUnits units
void launch_measured(c1_ctx *ctx, const C1EncodeLaunch &L, bool all_long, const MeasuredCall *mc, int64_t at, hipStream_t stream) {
  ScopedTiming t(ctx, K_MEASURE, stream);
  uint8_t *taken = mc->taken ? mc->taken + at : nullptr;
  int8_t *shifts = mc->shifts ? mc->shifts + at * 52 : nullptr;
  double *distortion = mc->distortion ? mc->distortion + at * 2 : nullptr, *energy = mc->energy ? mc->energy + at : nullptr;
  double *weights = mc->weights ? mc->weights + at * 52 : nullptr;
  const bool finalize = L.units != nullptr;
  const int64_t units = L.frames * L.channels;
  const bool wide = ctx->measured_wide < 0 ? units <= kMeasuredWideUnits : ctx->measured_wide != 0;
  if (wide) {
    static const int8_t kNoOffset[1] = {0};
    c1k_launch_measured_wide(L, all_long, finalize, mc->sf_offsets ? mc->sf_offsets : kNoOffset, mc->sf_offsets ? mc->n_offsets : 1, mc->mask,
                             mc->has_spread, taken, mc->sf_offsets ? shifts : nullptr, distortion, energy, weights, stream);
  } else if (mc->mask) {
    // the same over e' = P_b * e, P_b from the unit's own level-0 errors and the tables
    c1k_launch_measured_masked(L, all_long, finalize, mc->sf_offsets, mc->n_offsets, mc->mask, mc->has_spread, taken, shifts, distortion,
                               energy, weights, stream);
  } else if (mc->sf_offsets) {
    // the same over the least error of the candidate scale-factor indices
    c1k_launch_measured_sf(L, all_long, finalize, mc->sf_offsets, mc->n_offsets, taken, shifts, distortion, energy, stream);
  } else {
    c1k_launch_measured_alloc(L, all_long, finalize, taken, distortion, energy, stream);
  }
}

// The mode search of one launch, in k_choose_modes' place: L.coefs / L.side hold the all-long analysis, d_bm_coefs / d_bm_side the
// all-short one, trial record k the reference's allocation under candidate k; bm's outputs start at unit `at` of the call's.  The
// workgroup-per-unit kernel (c1_k_measured_modes_wide.hip, the same outputs bit for bit) for a launch of at most
// kMeasuredModesWideUnits units; C1_MEASURED_WIDE overrides as in launch_measured
void launch_measured_modes(c1_ctx *ctx, const C1EncodeLaunch &L, const uint8_t *trial, int64_t trial_stride, const BestModesCall *bm,
                           int64_t at, hipStream_t stream) {
  ScopedTiming t(ctx, K_MEASURE, stream);
  const int64_t units = L.frames * L.channels;
  const bool wide = ctx->measured_wide < 0 ? units <= kMeasuredModesWideUnits : ctx->measured_wide != 0;
  if (bm->mask) {
    // the same over e' = P_b * e, P_b from the unit's all-long plane and the tables (c1_encode_measured_modes_masked_device)
    (wide ? c1k_launch_measured_modes_masked_wide : c1k_launch_measured_modes_masked)(
        L, ctx->d_bm_coefs, ctx->d_bm_side, trial, trial_stride, bm->cand, bm->n, bm->sf_offsets, bm->n_offsets, bm->mask, bm->has_spread,
        L.units != nullptr, bm->choice ? bm->choice + at : nullptr, bm->modes_out ? bm->modes_out + at : nullptr,
        bm->taken ? bm->taken + at : nullptr, bm->shifts ? bm->shifts + at * 52 : nullptr,
        bm->distortion ? bm->distortion + at * bm->n * 2 : nullptr, bm->energy ? bm->energy + at * bm->n : nullptr,
        bm->weights ? bm->weights + at * 52 : nullptr, stream);
    return;
  }
  (wide ? c1k_launch_measured_modes_wide : c1k_launch_measured_modes)(
      L, ctx->d_bm_coefs, ctx->d_bm_side, trial, trial_stride, bm->cand, bm->n, bm->sf_offsets, bm->n_offsets, L.units != nullptr,
      bm->choice ? bm->choice + at : nullptr, bm->modes_out ? bm->modes_out + at : nullptr, bm->taken ? bm->taken + at : nullptr,
      bm->shifts ? bm->shifts + at * 52 : nullptr, bm->distortion ? bm->distortion + at * bm->n * 2 : nullptr,
      bm->energy ? bm->energy + at * bm->n : nullptr, stream);
}

int check_channels(int channels) {
  if (channels != 1 && channels != 2) return fail(C1_ERR_ARG, "channels must be 1 or 2, got %d", channels);
  return C1_OK;
}

// The domain of a mode byte is what blockSelectorStage writes (encoder.js:143): low and mid fields 0 or 2, high field 0 or 3,
// bits 6-7 clear.  The first byte outside it: C1_ERR_ARG naming frame, channel (of two) and field
int check_mode_bytes(const char *what, const uint8_t *modes, int64_t frames, int channels) {
  static const char *const kField[3] = {"low", "mid", "high"};
  for (int64_t i = 0; i < frames * channels; i++) {
    const int b = modes[i];
    if ((b & ~0x3a) == 0 && ((b & 0x30) == 0 || (b & 0x30) == 0x30)) continue;
    char where[64];
    if (channels == 2) snprintf(where, sizeof where, "frame %lld, channel %d", (long long)(i / 2), (int)(i & 1));
    else snprintf(where, sizeof where, "frame %lld", (long long)i);
    for (int k = 0; k < 3; k++) {
      const int m = (b >> (2 * k)) & 3, other = k == 2 ? 3 : 2;
      if (m != 0 && m != other)
        return fail(C1_ERR_ARG, "%s: %s: %s field of mode byte 0x%02x is %d, not 0 or %d", what, where, kField[k], b, m, other);
    }
    return fail(C1_ERR_ARG, "%s: %s: bits 6-7 of mode byte 0x%02x are set", what, where, b);
  }
  return C1_OK;
}

// lazy: the call may return with its last tail still unjoined (c1_encode_device on a context that owns its stream: nobody
// else can enqueue on that stream, and every other entry point joins first)
int encode_device_impl(c1_ctx *ctx, const float *const *pcm, int channels, int64_t frames, int halo_frames,
                       const c1_encode_options *opts, uint8_t *units, float *bands, float *coefs_tap,
                       uint8_t *side_tap, uint8_t *alloc_tap, bool lazy = false, const uint8_t *given_modes = nullptr,
                       const PaletteCall *pal = nullptr, const BestBiasCall *best = nullptr, const BestModesCall *bm = nullptr,
                       const MeasuredCall *mc = nullptr) {
  CTX_GUARD(ctx);
  int rc = ctx_bind(ctx, false);
  if (rc) return rc;
  if ((rc = check_channels(channels))) return rc;
  if (frames < 0) return fail(C1_ERR_ARG, "frames must be >= 0");
  if (halo_frames < 0 || halo_frames > 2) return fail(C1_ERR_ARG, "halo_frames must be 0, 1 or 2");
  if (!pcm) return fail(C1_ERR_ARG, "pcm is NULL");
  for (int c = 0; c < channels; c++) {
    if (!pcm[c] && frames > 0) return fail(C1_ERR_ARG, "pcm[%d] is NULL", c);
    if ((uintptr_t)pcm[c] & 15) return fail(C1_ERR_ARG, "pcm[%d] must be 16-byte aligned on the device", c);
  }
  if ((rc = upload_opts(ctx, opts))) return rc;
  if (ctx->profiling && ctx->timing_depth == 0) reset_timings(ctx);
  if (frames == 0) return C1_OK;
  // given_modes (c1_encode_modes_device): one mode byte per unit on the device instead of the detector's decision.  The call
  // is laid out like a detection call (bands, mode bytes and unit lists in the detection workspace); of `opts` only the
  // biased scale factors reach a kernel that runs
  const bool detect = given_modes || bm || opts->fixed_block_modes[0] < 0;
  const bool taps = coefs_tap || side_tap || alloc_tap;
  const int64_t chunk = taps ? ctx->chunk_frames : chunk_for_call(ctx, frames, channels, detect, best ? best->n : (bm ? bm->n : 0), bm != nullptr);
  if ((rc = ensure_workspace(ctx, (taps ? frames : std::min(frames, chunk)) * channels))) return rc;
  if (detect && (rc = ensure_detect_workspace(ctx, (taps ? frames : std::min(frames, chunk)) * channels))) return rc;
  // pal (c1_encode_biases_device): the allocation of every chunk runs once per palette entry over that entry's units, from
  // the tables upload_palette left in d_palette; analysis and packing do not read the bias and run as without it
  if (pal && (rc = ensure_palette_lists(ctx, std::min(frames, chunk) * channels, pal->n))) return rc;
  // best (c1_encode_best_bias_device): the allocation of every chunk runs once per palette entry over ALL its units into that
  // entry's trial records; k_choose_bias measures every (unit, entry) and leaves the winner's record where packing reads it
  if (best && (rc = ensure_trial_allocs(ctx, std::min(frames, chunk) * channels, best->n))) return rc;
  // bm (c1_encode_best_modes_device): the front end of given_modes under a constant byte, at most twice (all long into the
  // chunk's workspace, all short into planes of its own); per candidate its side record composed from the two and the allocation
  // run over all units into the candidate's trial records; k_choose_modes measures every (unit, candidate) and leaves the
  // winner's coefficients, side record and allocation where packing reads them.  One workspace half: not pipelined.  With
  // offsets (c1_encode_measured_modes_device) k_measured_modes stands in k_choose_modes' place, on the same workspace
  if (bm && (rc = ensure_trial_allocs(ctx, std::min(frames, chunk) * channels, bm->n))) return rc;
  if (bm && (rc = ensure_best_modes_planes(ctx, std::min(frames, chunk) * channels))) return rc;
  bool bm_long = false, bm_short = false;                     // some candidate codes a band long / short
  for (int k = 0; bm && k < bm->n; k++) {
    if ((bm->cand[k] & 0x3f) != 0x3a) bm_long = true;
    if ((bm->cand[k] & 0x3f) != 0) bm_short = true;
  }
  if (bm && bm->mask) bm_long = true;                          // the weights come from the all-long analysis, whatever the candidates
  if (taps && (!coefs_tap || !side_tap || !alloc_tap)) return fail(C1_ERR_ARG, "coefs, side and alloc taps must be given together");
  if (taps && frames > kMaxChunkFrames) return fail(C1_ERR_ARG, "stage taps are not chunked: at most %lld frames per call", (long long)kMaxChunkFrames);
  // Two-stage software pipeline over chunks: the analysis of chunk i+1 (fp64-VALU bound) runs on one
  // stream while allocation + packing of chunk i (latency bound) run on another, each chunk on its own
  // half of the workspace.  Everything is ordered after the caller's stream and joined back into it.
  const bool all_long_modes = !detect && opts->fixed_block_modes[0] == 0 && opts->fixed_block_modes[1] == 0 &&
                              opts->fixed_block_modes[2] == 0 && !getenv("C1_NO_FAST_LONG");
  const bool all_short_modes = !detect && opts->fixed_block_modes[0] != 0 && opts->fixed_block_modes[1] != 0 &&
                               opts->fixed_block_modes[2] != 0;
  bool speculate = (all_long_modes || all_short_modes) && !taps && !pal && !best && !bm && !mc && units && ctx->spec_tables_ok && ctx->spec_mode != 0;
  bool quantize32 = !taps && units && ctx->spec_tables_ok && ctx->spec_mode != 0;   // exact coefficients, binary32 quantization with the guard (below)
  static const bool det_spec_env_off = getenv("C1_DETECT_SPEC") && atoi(getenv("C1_DETECT_SPEC")) == 0;   // experiments: exact detector, the rest as usual
  bool detect_spec = detect && !given_modes && !bm && !taps && ctx->spec_tables_ok && ctx->spec_mode != 0 && !det_spec_env_off;   // binary32 transient detector with a score interval
  // A call of a few frames (a frame closure, a short streaming push) is bound by the number of launches behind it, and
  // every speculative shortcut adds some (the redo chain, the recheck, the second packing pass): in the default mode such
  // calls take the exact kernels (one mono frame: 159 against 185 us, tools/latency_probe.py).  A rule on the size of
  // this call alone; mode 2 still speculates on anything.
  if (ctx->spec_mode == 1 && frames * channels < kSpecMinUnits) speculate = quantize32 = detect_spec = false;
  // Both shortcuts of the exact paths (binary32 quantization of exact coefficients, binary32 transient detector) are
  // taken whenever speculation is on; nothing is carried from call to call.  What they hand back to the exact arithmetic
  // is listed unit by unit inside the call: 0.07 % (noise) to 4 % (stationary partials) of the units packed again, 0.02 to
  // 0.3 % rechecked (tools/adaptive_probe.py) -- round 2's per-context switches at 10 % and 20 % never fired on any
  // material tried and made throughput depend on what a context had encoded before.  c1_ctx_set_speculation(ctx, 0)
  // turns every shortcut off for a stream that is known to defeat them; the bytes are the same either way.
  const bool overlap = speculate && ctx->overlap && ctx->s_tail != nullptr;
  if (!overlap && (rc = join_tail(ctx))) return rc;       // every other path works on the context's stream alone
  const bool piped = ctx->pipeline && !taps && frames > chunk && !speculate && !bm;
  hipStream_t sA = piped ? ctx->s_ana : ctx->stream, sB = piped ? ctx->s_rest : ctx->stream;
  if (piped) {
    HIP_TRY(hipEventRecord(ctx->ev_in, ctx->stream));
    HIP_TRY(hipStreamWaitEvent(sA, ctx->ev_in, 0));
    HIP_TRY(hipStreamWaitEvent(sB, ctx->ev_in, 0));
  }
  int64_t index = 0;
  for (int64_t f0 = 0, n = 0; f0 < frames; f0 += n, ++index) {
    n = taps ? frames : std::min(chunk, frames - f0);
    int p = piped ? (int)(index & 1) : 0;
    if (overlap) { p = ctx->ws_next; ctx->ws_next ^= 1; }
    C1EncodeLaunch L;
    memset(&L, 0, sizeof L);
    for (int c = 0; c < channels; c++) L.pcm[c] = pcm[c] + f0 * 512;
    L.channels = channels;
    L.frames = n;
    L.halo_frames = (int)std::min<int64_t>(2, f0 + halo_frames);
    L.tables = ctx->d_tables;
    L.opts = ctx->d_opts;
    L.coefs = taps ? coefs_tap : ctx->d_coefs[p];
    L.side = taps ? side_tap : ctx->d_side[p];
    L.alloc = taps ? alloc_tap : ctx->d_alloc[p];
    L.cand = ctx->d_cand[p];
    L.work_count = ctx->d_work[p];
    L.work_list = ctx->d_work[p] + 4;
    L.sel_list = ctx->d_work[p] + 4 + (size_t)ctx->ws_units * 7;
    L.bands = bands ? bands + f0 * channels * 512 : nullptr;
    L.units = units ? units + f0 * channels * C1_UNIT_BYTES : nullptr;
    const bool all_long = all_long_modes;
    if (piped && index >= 2) HIP_TRY(hipStreamWaitEvent(sA, ctx->ev_free[p], 0));   // workspace half p is free again
    if (speculate) {
      // Speculative pass in binary32 (c1_k_spec.hip): coefficients with a proven error bound; allocation works on the
      // scale-factor indices; the packing kernel accepts a unit only when every decision is certain within the bound
      // and lists the others.  Then the exact kernels redo the listed units in place.
      // Material-local: every 16 frames of a run the speculative kernel estimates from the scale-factor indices and its
      // bound how many decisions of a unit will stay open; past spec_defer it hands the rest of the run to the exact
      // kernels (run list), whose units are then quantized in binary32 behind a bound of zero like the exact paths'.
      L.eps = ctx->d_eps[p];
      bind_lists(ctx, p, &L);
      if (ctx->spec_mode == 1) { bind_defer(ctx, p, &L); L.spec_defer = ctx->spec_defer; }
      // masks of the units with an open scale factor: behind the deferred runs' slots (one per run and channel, at most a
      // quarter of the units: a run is at least 4 frames), two words per run; only with runs of at most 64 frames
      if (c1k_pick_run(n, channels, 0) <= 64 && !getenv("C1_NO_SF_PREPASS"))
        L.open_masks = reinterpret_cast<unsigned long long *>((reinterpret_cast<uintptr_t>(ctx->d_redo[p] + kListHead + 3 * (size_t)ctx->ws_units + (size_t)ctx->ws_units / 4 + 4) + 7) & ~(uintptr_t)7);
      // this half of the workspace is free once the tail of the chunk that used it last is through
      if (overlap && ctx->tail_used[p]) HIP_TRY(hipStreamWaitEvent(sA, ctx->ev_tail[p], 0));
      HIP_TRY(hipMemsetAsync(ctx->d_redo[p], 0, kListHead * sizeof(uint32_t), sA));
      {
        ScopedTiming t(ctx, K_ANALYSIS, sA);
        c1k_launch_analysis_spec(L, all_short_modes, sA);
        if (L.defer_list) {
          C1EncodeLaunch D = L;
          uint32_t *dense = ctx->d_redo[p] + kListHead + 2 * (size_t)ctx->ws_units;   // the re-analysis list's space: that list is filled
          c1k_launch_defer_compact(L, dense, ctx->d_redo[p] + 3, sA);                 // by the packing kernel, after this pass is done
          D.unit_list = dense;
          D.unit_count = ctx->d_redo[p] + 3;
          D.list_runs = 1;
          D.defer_list = nullptr;
          if (all_long_modes) c1k_launch_analysis_long(D, sA); else c1k_launch_analysis(D, false, sA);
        }
      }
      if (L.open_masks) {
        ScopedTiming t(ctx, K_REDO, sA);                       // exact work on uncertain units: timed with the redo, wherever it runs
        {
          // the units whose scale-factor guard stayed open (1.8 % of white noise) are re-analysed exactly HERE, in front of the
          // allocation: it then sees the reference's indices the first time, and the redo behind the packing pass has no
          // allocation chain of its own (five launches, one of them a lone heap run long: 0.13 ms per 2 M units)
          C1EncodeLaunch X = L;
          uint32_t *open_list = ctx->d_redo[p] + kListHead + 2 * (size_t)ctx->ws_units;   // the re-analysis list's space again (the
          c1k_launch_open_compact(L, open_list, ctx->d_redo[p] + 5, sA);                  // deferred runs' list above is consumed)
          X.unit_list = open_list;
          X.unit_count = ctx->d_redo[p] + 5;
          X.list_runs = 0;
          X.list_zero_eps = 1;
          X.defer_list = nullptr;
          X.open_masks = nullptr;
          if (all_long_modes) c1k_launch_analysis_long(X, sA); else c1k_launch_analysis(X, false, sA);
        }
      }
      { ScopedTiming t(ctx, K_ALLOCATE, sA); c1k_launch_allocate(L, sA); }
      // The previous chunk's tail repacks units of ITS output range; when a caller reuses one output buffer call after
      // call that range is this chunk's: the tail's stores must have landed before this chunk packs (in practice it
      // finished long ago: it has had the whole analysis and allocation of this chunk to run beside)
      if (overlap && ctx->tail_used[p ^ 1]) HIP_TRY(hipStreamWaitEvent(sA, ctx->ev_tail[p ^ 1], 0));
      { ScopedTiming t(ctx, K_PACK, sA); c1k_launch_pack_spec(L, all_long_modes, sA); }
      hipStream_t sT = sA;
      if (overlap) {
        sT = ctx->s_tail;
        HIP_TRY(hipEventRecord(ctx->ev_main[p], sA));
        HIP_TRY(hipStreamWaitEvent(sT, ctx->ev_main[p], 0));
      }
      {
        ScopedTiming t(ctx, K_REDO, sT);
        hipStream_t sA = sT;                                   // the exact redo of the listed units: on the tail stream
        C1EncodeLaunch R = L;
        R.defer_list = nullptr;
        R.unit_list = L.reana_list;
        R.unit_count = L.reana_count;
        if (all_long_modes) c1k_launch_analysis_long(R, sA); else c1k_launch_analysis(R, false, sA);
        if (!L.open_masks) {                                   // with the pre-pass above no unit reaches the packing pass with an open scale factor
          C1EncodeLaunch A = R;
          A.unit_list = L.realloc_list;
          A.unit_count = L.realloc_count;
          c1k_launch_allocate(A, sA);
        }
        R.unit_list = L.redo_list;
        R.unit_count = L.redo_count;
        c1k_launch_pack(R, all_long_modes, sA);
        c1k_launch_spec_totals(ctx->d_spec_totals, (uint64_t)(n * channels), ctx->d_redo[p], 0, sA);
      }
      if (overlap) {
        HIP_TRY(hipEventRecord(ctx->ev_tail[p], sT));
        ctx->tail_used[p] = true;
        ctx->tail_pending = true;
      }
      continue;
    }
    {
      ScopedTiming t(ctx, K_ANALYSIS, sA);
      if (all_long) c1k_launch_analysis_long(L, sA);
      else if (bm) {
        // the band samples once; the all-long analysis into the chunk's planes and the all-short one into the call's own.  The
        // constant bytes of the front end's input lie in the candidate side plane, which is composed only after this
        C1EncodeLaunch S2 = L;
        S2.coefs = ctx->d_bm_coefs;
        S2.side = ctx->d_bm_side;
        HIP_TRY(hipMemsetAsync(ctx->d_bm_cand_side, bm_long ? 0 : 0x3a, (size_t)n * channels, sA));
        c1k_launch_modes_front(L, ctx->d_bm_cand_side, ctx->d_bands[p], ctx->d_modes[p], ctx->d_lists[p], sA);
        c1k_launch_mdct_bands(bm_long ? L : S2, ctx->d_bands[p], ctx->d_modes[p], ctx->d_lists[p], sA);
        if (bm_long && bm_short) {
          c1k_launch_const_mode_lists(0x3a, n * channels, ctx->d_modes[p], ctx->d_lists[p], sA);
          c1k_launch_mdct_bands(S2, ctx->d_bands[p], ctx->d_modes[p], ctx->d_lists[p], sA);
        }
      } else if (given_modes) {
        c1k_launch_modes_front(L, given_modes + f0 * channels, ctx->d_bands[p], ctx->d_modes[p], ctx->d_lists[p], sA);
        c1k_launch_mdct_bands(L, ctx->d_bands[p], ctx->d_modes[p], ctx->d_lists[p], sA);
      } else if (detect) {
        c1k_launch_detect(L, ctx->d_bands[p], ctx->d_feat[p], ctx->d_modes[p], ctx->d_lists[p], detect_spec, nullptr, sA);
        if (detect_spec) c1k_launch_spec_totals(ctx->d_spec_totals, (uint64_t)(n * channels), ctx->d_lists[p] + 2, 2, sA);
        if (L.bands) HIP_TRY(hipMemcpyAsync(L.bands, ctx->d_bands[p] + (size_t)channels * 512, (size_t)n * channels * 512 * sizeof(float),
                                            hipMemcpyDeviceToDevice, sA));
      } else c1k_launch_analysis(L, false, sA);
    }
    if (piped) {
      HIP_TRY(hipEventRecord(ctx->ev_ana[p], sA));
      HIP_TRY(hipStreamWaitEvent(sB, ctx->ev_ana[p], 0));
    }
    if (bm) {
      const int64_t trial_stride = ctx->trial_units * kAllocBytes;
      for (int k = 0; k < bm->n; k++) {                          // one chain after the other: they share the side plane and the scratch
        { ScopedTiming t(ctx, K_ANALYSIS, sB); c1k_launch_compose_side(L.side, ctx->d_bm_side, n * channels, bm->cand[k], ctx->d_bm_cand_side, sB); }
        ScopedTiming t(ctx, K_ALLOCATE, sB);
        C1EncodeLaunch A = L;
        A.side = ctx->d_bm_cand_side;
        A.alloc = ctx->d_trial + (size_t)k * trial_stride;
        c1k_launch_allocate(A, sB);
      }
      if (bm->sf_offsets) {
        launch_measured_modes(ctx, L, ctx->d_trial, trial_stride, bm, f0 * channels, sB);
      } else {
        ScopedTiming t(ctx, K_CHOOSE, sB);
        c1k_launch_choose_modes(L, ctx->d_bm_coefs, ctx->d_bm_side, ctx->d_trial, trial_stride, bm->cand, bm->n, L.units != nullptr,
                                bm->choice ? bm->choice + f0 * channels : nullptr, bm->modes_out ? bm->modes_out + f0 * channels : nullptr,
                                bm->distortion ? bm->distortion + f0 * channels * bm->n : nullptr,
                                bm->energy ? bm->energy + f0 * channels * bm->n : nullptr, sB);
      }
    } else if (best) {
      const int64_t trial_stride = ctx->trial_units * kAllocBytes;
      {
        ScopedTiming t(ctx, K_ALLOCATE, sB);
        for (int k = 0; k < best->n; k++) {                      // one chain after the other: they share the candidate and work-list scratch
          C1EncodeLaunch A = L;
          A.opts = ctx->d_palette + k;
          A.alloc = ctx->d_trial + (size_t)k * trial_stride;
          c1k_launch_allocate(A, sB);
        }
      }
      ScopedTiming t(ctx, K_CHOOSE, sB);
      c1k_launch_choose_bias(L, ctx->d_trial, trial_stride, best->n, all_long, best->choice ? best->choice + f0 * channels : nullptr,
                             best->distortion ? best->distortion + f0 * channels * best->n : nullptr,
                             best->energy ? best->energy + f0 * channels : nullptr, sB);
    } else if (pal) {
      ScopedTiming t(ctx, K_ALLOCATE, sB);
      c1k_launch_allocate_palette(L, ctx->d_palette, pal->n, pal->index + f0 * channels, ctx->d_pal_lists, ctx->d_pal_lists + 8, n * channels, sB);
    } else { ScopedTiming t(ctx, K_ALLOCATE, sB); c1k_launch_allocate(L, sB); }
    // mc (c1_encode_measured_device): the allocation chain above left the reference's record of every unit; the measured kernel
    // builds the unit's error table, allocates greedily by it, and replaces the record where that codes with less error
    if (mc) launch_measured(ctx, L, all_long, mc, f0 * channels, sB);
    if (L.units && quantize32) {
      // The coefficients are the reference's, and still the quantization need not be done in binary64: the packing
      // kernel of the speculative path with a bound of zero forms |x| norm + 0.5 in binary32 and accepts a mantissa only
      // when no value within the roundings of that (norm32 against norm, the fused operation, the reference's own
      // two) truncates differently; the few units it lists (and anything not finite) are packed again by the exact kernel.
      ScopedTiming t(ctx, K_PACK, sB);
      L.eps = ctx->d_eps[p];
      bind_lists(ctx, p, &L);                                  // the reallocation and re-analysis lists stay empty: with bounds of zero no
                                                               // scale-factor index is open and every coefficient is the exact kernels'
      HIP_TRY(hipMemsetAsync(L.eps, 0, (size_t)n * channels * kEpsFloats * sizeof(float), sB));
      HIP_TRY(hipMemsetAsync(ctx->d_redo[p], 0, kListHead * sizeof(uint32_t), sB));
      c1k_launch_pack_spec(L, all_long, sB);
      C1EncodeLaunch R = L;
      R.unit_list = L.redo_list;
      R.unit_count = L.redo_count;
      c1k_launch_pack(R, all_long, sB);
      c1k_launch_spec_totals(ctx->d_spec_totals, (uint64_t)(n * channels), L.redo_count, 1, sB);
    } else if (L.units) { ScopedTiming t(ctx, K_PACK, sB); c1k_launch_pack(L, all_long, sB); }
    if (piped) HIP_TRY(hipEventRecord(ctx->ev_free[p], sB));
  }
  if (piped) {
    HIP_TRY(hipEventRecord(ctx->ev_end[0], sA));
    HIP_TRY(hipEventRecord(ctx->ev_end[1], sB));
    HIP_TRY(hipStreamWaitEvent(ctx->stream, ctx->ev_end[0], 0));
    HIP_TRY(hipStreamWaitEvent(ctx->stream, ctx->ev_end[1], 0));
  }
  if (overlap && !lazy && (rc = join_tail(ctx))) return rc;
  HIP_TRY(hipGetLastError());
  return C1_OK;
}

// xorshift32 as a GF(2) linear map: column form of T^n, used to jump the generator
struct XsMatrix {
  uint32_t col[32];
  uint32_t apply(uint32_t s) const {
    uint32_t r = 0;
    for (int b = 0; b < 32; b++) if ((s >> b) & 1u) r ^= col[b];
    return r;
  }
};
uint32_t xs_step(uint32_t s) { s ^= s << 13; s ^= s >> 17; s ^= s << 5; return s; }
XsMatrix xs_power(uint64_t n) {
  XsMatrix result, base;
  for (int b = 0; b < 32; b++) { result.col[b] = 1u << b; base.col[b] = xs_step(1u << b); }
  while (n) {
    if (n & 1) { XsMatrix r; for (int b = 0; b < 32; b++) r.col[b] = base.apply(result.col[b]); result = r; }
    XsMatrix sq;
    for (int b = 0; b < 32; b++) sq.col[b] = base.apply(base.col[b]);
    base = sq;
    n >>= 1;
  }
  return result;
}

}  // namespace

// ------------------------------------------------------------------------------------------------------
namespace {
struct DeviceScratch {       // a few small device buffers for one call, freed on every path
  std::vector<void *> ptrs;
  ~DeviceScratch() { for (void *p : ptrs) (void)hipFree(p); }
  template <class T> int alloc(T **out, size_t count) {
    void *p = nullptr;
    if (hipMalloc(&p, std::max<size_t>(count, 1) * sizeof(T)) != hipSuccess) return fail(C1_ERR_HIP, "device allocation of %zu bytes failed", count * sizeof(T));
    ptrs.push_back(p);
    *out = static_cast<T *>(p);
    return C1_OK;
  }
};
}  // namespace

extern "C" {

int c1_abi_version(void) { return C1_ABI_VERSION; }
const char *c1_last_error(void) { return g_error.c_str(); }

int c1_device_count(int *count) {
  if (!count) return fail(C1_ERR_ARG, "count is NULL");
  int n = 0;
  const hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) {
    *count = 0;
    return fail(C1_ERR_NO_DEVICE, "hipGetDeviceCount: %s", hipGetErrorString(e));
  }
  *count = n;
  return C1_OK;
}

int c1_get_default_tables(c1_tables *out) {
  if (!out) return fail(C1_ERR_ARG, "out is NULL");
  default_tables(out);
  return C1_OK;
}

int c1_set_tables(const c1_tables *tables) {
  std::lock_guard<std::mutex> lock(g_tables_mutex);
  if (!tables) { g_tables_custom = false; g_tables_gen++; return C1_OK; }
  const double *p = reinterpret_cast<const double *>(tables);
  for (size_t i = 0; i < sizeof(c1_tables) / sizeof(double); i++)
    if (!std::isfinite(p[i])) return fail(C1_ERR_ARG, "table entry %zu is not finite", i);
  g_tables = *tables;
  g_tables_custom = true;
  g_tables_gen++;
  return C1_OK;
}

int c1_table_fast_paths(int *scale_factor_bits, int *dequant_reciprocal) {
  c1_tables t;
  {
    std::lock_guard<std::mutex> lock(g_tables_mutex);
    if (g_tables_custom) t = g_tables; else default_tables(&t);
  }
  std::unique_ptr<C1DevTables> d(new C1DevTables);
  build_device_tables(t, d.get());
  if (scale_factor_bits) *scale_factor_bits = d->sf_fast;
  if (dequant_reciprocal) *dequant_reciprocal = d->dq_fast + d->dq_step;
  return C1_OK;
}

int c1_alloc_rank_form(const c1_encode_options *opts, int *affine, int *coef) {
  if (!opts) return fail(C1_ERR_ARG, "opts is NULL");
  std::unique_ptr<C1DevEncOpts> d(new C1DevEncOpts);
  const int rc = build_table_fields(*opts, d.get());
  if (rc) return rc;
  if (affine) *affine = d->rank_affine;
  if (coef) { coef[0] = d->rank_a; coef[1] = d->rank_b; coef[2] = d->rank_c; coef[3] = d->rank_off; }
  return C1_OK;
}

int c1_alloc_tables(const c1_encode_options *opts, int *affine, uint32_t *steps, uint16_t *rank, int *dist_ok, double *dist) {
  if (!opts) return fail(C1_ERR_ARG, "opts is NULL");
  std::unique_ptr<C1DevEncOpts> d(new C1DevEncOpts);
  const int rc = build_table_fields(*opts, d.get());
  if (rc) return rc;
  if (affine) *affine = d->rank_affine;
  if (steps) { steps[0] = d->rank_step0; steps[1] = d->rank_step; }
  if (rank) {
    // the rank field of the heap entries the kernels build for (sfi, wl): the integer form where there is one
    for (int s = 0; s < 64; s++)
      for (int wl = 0; wl < 16; wl++)
        rank[s * 16 + wl] = !d->rank_affine ? d->rank[s * 16 + wl]
                            : (uint16_t)(wl == 0 ? d->rank_a * s + d->rank_c + d->rank_off : d->rank_a * s + d->rank_off - d->rank_b * (wl + 1));
  }
  if (dist_ok) *dist_ok = d->dist_tables;
  if (dist) memcpy(dist, d->dist, sizeof d->dist);
  return C1_OK;
}

int c1_default_encode_options(c1_encode_options *out) {
  if (!out) return fail(C1_ERR_ARG, "out is NULL");
  memset(out, 0, sizeof *out);
  c1_tables t;
  {
    std::lock_guard<std::mutex> lock(g_tables_mutex);
    if (g_tables_custom) t = g_tables; else default_tables(&t);
  }
  memcpy(out->biased_scale_factors, t.scale_factors, sizeof out->biased_scale_factors);
  out->transient_threshold = 1.0;
  out->fixed_block_modes[0] = out->fixed_block_modes[1] = out->fixed_block_modes[2] = -1;
  return C1_OK;
}

int c1_ctx_create(int device, void *hip_stream, c1_ctx **out) {
  if (!out) return fail(C1_ERR_ARG, "out is NULL");
  *out = nullptr;
  int n = 0;
  const hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n == 0)
    return fail(C1_ERR_NO_DEVICE, "no HIP device available (%s); this library has no CPU path",
                e != hipSuccess ? hipGetErrorString(e) : "device count is 0");
  if (device < 0 || device >= n) return fail(C1_ERR_ARG, "device %d out of range (0..%d)", device, n - 1);
  HIP_TRY(hipSetDevice(device));
  c1_ctx *ctx = new c1_ctx();
  ctx->device = device;
  if (hip_stream) ctx->stream = (hipStream_t)hip_stream;
  else {
    const hipError_t se = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking);
    if (se != hipSuccess) { delete ctx; return fail(C1_ERR_HIP, "hipStreamCreate: %s", hipGetErrorString(se)); }
    ctx->own_stream = true;
  }
  c1_tables t;
  {
    std::lock_guard<std::mutex> lock(g_tables_mutex);
    if (g_tables_custom) t = g_tables; else default_tables(&t);
  }
  C1DevTables *h = new C1DevTables();
  build_device_tables(t, h);
  hipError_t me = hipMalloc(&ctx->d_tables, sizeof(C1DevTables));
  if (me == hipSuccess) me = hipMalloc(&ctx->d_opts, sizeof(C1DevEncOpts));
  if (me == hipSuccess) me = hipMemcpy(ctx->d_tables, h, sizeof *h, hipMemcpyHostToDevice);
  if (me == hipSuccess) me = hipMalloc(&ctx->d_spec_totals, kTotals * sizeof(unsigned long long));
  if (me == hipSuccess) me = hipMemset(ctx->d_spec_totals, 0, kTotals * sizeof(unsigned long long));
  ctx->spec_tables_ok = h->spec_ok != 0;
  {
    const char *sp = getenv("C1_SPEC");       // 0 exact only, 1 material-local (default), 2 always speculate
    ctx->spec_mode = sp ? atoi(sp) : 1;
    if (ctx->spec_mode < 0 || ctx->spec_mode > 2) ctx->spec_mode = 1;
    const char *sd = getenv("C1_SPEC_DEFER");   // experiments: the predictor's threshold (open decisions per unit)
    if (sd && atof(sd) > 0) ctx->spec_defer = (float)atof(sd);
  }
  delete h;
  if (me != hipSuccess) { c1_ctx_destroy(ctx); return fail(C1_ERR_HIP, "table upload: %s", hipGetErrorString(me)); }
  {
    hipError_t pe = hipStreamCreateWithFlags(&ctx->s_ana, hipStreamNonBlocking);
    if (pe == hipSuccess) pe = hipStreamCreateWithFlags(&ctx->s_rest, hipStreamNonBlocking);
    if (pe == hipSuccess) pe = hipEventCreateWithFlags(&ctx->ev_in, hipEventDisableTiming);
    for (int p = 0; p < 2 && pe == hipSuccess; p++) {
      pe = hipEventCreateWithFlags(&ctx->ev_ana[p], hipEventDisableTiming);
      if (pe == hipSuccess) pe = hipEventCreateWithFlags(&ctx->ev_free[p], hipEventDisableTiming);
      if (pe == hipSuccess) pe = hipEventCreateWithFlags(&ctx->ev_end[p], hipEventDisableTiming);
    }
    if (pe != hipSuccess) { c1_ctx_destroy(ctx); return fail(C1_ERR_HIP, "pipeline streams: %s", hipGetErrorString(pe)); }
    if (pe == hipSuccess) pe = hipStreamCreateWithFlags(&ctx->s_tail, hipStreamNonBlocking);
    for (int p = 0; p < 2 && pe == hipSuccess; p++) {
      pe = hipEventCreateWithFlags(&ctx->ev_main[p], hipEventDisableTiming);
      if (pe == hipSuccess) pe = hipEventCreateWithFlags(&ctx->ev_tail[p], hipEventDisableTiming);
    }
    if (pe != hipSuccess) { c1_ctx_destroy(ctx); return fail(C1_ERR_HIP, "tail stream: %s", hipGetErrorString(pe)); }
    // C1_OVERLAP=1: the exact redo of a chunk on the tail stream, beside the next chunk's (or call's) analysis.  Off by default:
    // measured +1.3 % (white noise) to +2.7 % (mixed corpus) -- the redo is mostly real work that the analysis beside it pays
    // for -- at the price of per-kernel times that include each other
    const char *ov = getenv("C1_OVERLAP");
    ctx->overlap = ov ? atoi(ov) != 0 : false;
    const char *pl = getenv("C1_PIPELINE");
    ctx->pipeline = pl ? atoi(pl) != 0 : false;   // measured: no gain while one kernel's grid already owns every CU's LDS
  }
  // C1_MEASURED_WIDE: 0 never takes the workgroup-per-unit measured kernel, 1 always; unset: launches of at most
  // kMeasuredWideUnits units take it; the mode search's kernels likewise, by kMeasuredModesWideUnits (6q).  The
  // outputs are the same bits either way
  const char *mw = getenv("C1_MEASURED_WIDE");
  ctx->measured_wide = mw ? (atoi(mw) != 0 ? 1 : 0) : -1;
  // C1_SIGNAL_STARTS: how c1_encode_signals_measured* redoes the first two frames of every signal: 0 in two passes of the row
  // kernel, 1 in one pass of k_encode_signal_starts; unset: kSignalStartsFused.  The outputs are the same bits
  const char *ss = getenv("C1_SIGNAL_STARTS");
  ctx->signal_starts_fused = ss ? atoi(ss) != 0 : kSignalStartsFused;
  const char *env = getenv("C1_CHUNK_FRAMES");
  ctx->chunk_frames = env ? atoll(env) : (int64_t)1 << 24;   // chunk_for_call() cuts it down to what fits
  if (ctx->chunk_frames < 16) ctx->chunk_frames = 16;
  // the allocation work list packs (unit << 3 | candidate) into 32 bits and unit lists are 32-bit: a chunk holds
  // fewer than 2^29 units, with room to spare
  if (ctx->chunk_frames > kMaxChunkFrames) ctx->chunk_frames = kMaxChunkFrames;
  *out = ctx;
  return C1_OK;
}

int c1_ctx_destroy(c1_ctx *ctx) {
  if (!ctx) return C1_OK;
  hipSetDevice(ctx->device);
  if (ctx->s_tail) hipStreamSynchronize(ctx->s_tail);
  if (ctx->stream) hipStreamSynchronize(ctx->stream);
  for (auto &t : ctx->timings) { hipEventDestroy(t.start); hipEventDestroy(t.stop); }
  for (auto e : ctx->event_pool) hipEventDestroy(e);
  if (ctx->d_tables) hipFree(ctx->d_tables);
  if (ctx->d_opts) hipFree(ctx->d_opts);
  if (ctx->d_palette) hipFree(ctx->d_palette);
  if (ctx->d_mask) hipFree(ctx->d_mask);
  if (ctx->h_mask) hipHostFree(ctx->h_mask);
  if (ctx->ev_mask) hipEventDestroy(ctx->ev_mask);
  if (ctx->d_spec_totals) hipFree(ctx->d_spec_totals);
  (void)hipDeviceSynchronize();
  free_workspace(ctx);
  if (ctx->s_tail) (void)hipStreamDestroy(ctx->s_tail);
  for (int p = 0; p < 2; p++) {
    if (ctx->ev_main[p]) (void)hipEventDestroy(ctx->ev_main[p]);
    if (ctx->ev_tail[p]) (void)hipEventDestroy(ctx->ev_tail[p]);
  }
  if (ctx->s_ana) (void)hipStreamDestroy(ctx->s_ana);
  if (ctx->s_rest) (void)hipStreamDestroy(ctx->s_rest);
  if (ctx->ev_in) (void)hipEventDestroy(ctx->ev_in);
  for (int p = 0; p < 2; p++) {
    if (ctx->ev_ana[p]) (void)hipEventDestroy(ctx->ev_ana[p]);
    if (ctx->ev_free[p]) (void)hipEventDestroy(ctx->ev_free[p]);
    if (ctx->ev_end[p]) (void)hipEventDestroy(ctx->ev_end[p]);
  }
  if (ctx->d_io) hipFree(ctx->d_io);
  if (ctx->d_sig) (void)hipFree(ctx->d_sig);
  if (ctx->h_rows) (void)hipHostFree(ctx->h_rows);
  if (ctx->ev_rows) (void)hipEventDestroy(ctx->ev_rows);
  if (ctx->d_ring) (void)hipFree(ctx->d_ring);
  if (ctx->s_up) (void)hipStreamDestroy(ctx->s_up);
  if (ctx->s_down) (void)hipStreamDestroy(ctx->s_down);
  for (int p = 0; p < 2; p++) {
    if (ctx->ev_up[p]) (void)hipEventDestroy(ctx->ev_up[p]);
    if (ctx->ev_run[p]) (void)hipEventDestroy(ctx->ev_run[p]);
    if (ctx->ev_down[p]) (void)hipEventDestroy(ctx->ev_down[p]);
  }
  if (ctx->own_stream && ctx->stream) hipStreamDestroy(ctx->stream);
  delete ctx;
  return C1_OK;
}

int c1_ctx_synchronize(c1_ctx *ctx) {
  CTX_GUARD(ctx);
  int rc = ctx_bind(ctx);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return C1_OK;
}

int c1_ctx_set_profiling(c1_ctx *ctx, int enabled) {
  if (!ctx) return fail(C1_ERR_ARG, "context is NULL");
  CTX_GUARD(ctx);
  ctx->profiling = enabled != 0;
  return C1_OK;
}

int c1_ctx_set_speculation(c1_ctx *ctx, int mode) {
  if (!ctx) return fail(C1_ERR_ARG, "context is NULL");
  if (mode < 0 || mode > 2) return fail(C1_ERR_ARG, "speculation mode must be 0, 1 or 2, got %d", mode);
  CTX_GUARD(ctx);
  ctx->spec_mode = mode;
  return C1_OK;
}

int c1_ctx_set_decode_model(c1_ctx *ctx, int model) {
  if (!ctx) return fail(C1_ERR_ARG, "context is NULL");
  if (model != C1_DECODE_EXACT && model != C1_DECODE_BINARY32_BULK && model != C1_DECODE_BINARY32)
    return fail(C1_ERR_ARG, "decode model must be 0, 1 or 2, got %d", model);
  CTX_GUARD(ctx);
  ctx->decode_model = model;
  ctx->decode_binary32 = model != C1_DECODE_EXACT;
  return C1_OK;
}

int c1_ctx_get_decode_model(c1_ctx *ctx, int *model) {
  if (!ctx) return fail(C1_ERR_ARG, "context is NULL");
  if (!model) return fail(C1_ERR_ARG, "model is NULL");
  CTX_GUARD(ctx);
  *model = ctx->decode_model;
  return C1_OK;
}

int c1_ctx_set_decode_precision(c1_ctx *ctx, int binary32) {
  return c1_ctx_set_decode_model(ctx, binary32 ? C1_DECODE_BINARY32_BULK : C1_DECODE_EXACT);
}

int c1_ctx_speculation_stats(c1_ctx *ctx, uint64_t *units, uint64_t *redone, int reset) {
  CTX_GUARD(ctx);
  int rc = ctx_bind(ctx);
  if (rc) return rc;
  unsigned long long tot[2] = {0, 0};
  HIP_TRY(hipMemcpyAsync(tot, ctx->d_spec_totals, sizeof tot, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  if (units) *units = tot[0];
  if (redone) *redone = tot[1];
  if (reset) {
    HIP_TRY(hipMemsetAsync(ctx->d_spec_totals, 0, kTotals * sizeof(unsigned long long), ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
  }
  return C1_OK;
}

int c1_ctx_speculation_deferred(c1_ctx *ctx, uint64_t *units) {
  CTX_GUARD(ctx);
  int rc = ctx_bind(ctx);
  if (rc) return rc;
  unsigned long long tot[kTotals];
  HIP_TRY(hipMemcpyAsync(tot, ctx->d_spec_totals, sizeof tot, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  if (units) *units = tot[6];
  return C1_OK;
}

int c1_ctx_quantization_stats(c1_ctx *ctx, uint64_t *units, uint64_t *repacked) {
  CTX_GUARD(ctx);
  int rc = ctx_bind(ctx);
  if (rc) return rc;
  unsigned long long tot[4] = {0, 0, 0, 0};
  HIP_TRY(hipMemcpyAsync(tot, ctx->d_spec_totals, sizeof tot, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  if (units) *units = tot[2];
  if (repacked) *repacked = tot[3];
  return C1_OK;
}

int c1_ctx_detection_stats(c1_ctx *ctx, uint64_t *units, uint64_t *rechecked) {
  CTX_GUARD(ctx);
  int rc = ctx_bind(ctx);
  if (rc) return rc;
  unsigned long long tot[6] = {0, 0, 0, 0, 0, 0};
  HIP_TRY(hipMemcpyAsync(tot, ctx->d_spec_totals, sizeof tot, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  if (units) *units = tot[4];
  if (rechecked) *rechecked = tot[5];
  return C1_OK;
}

int c1_ctx_kernel_ms(c1_ctx *ctx, const char *name, double *ms, int *launches) {
  CTX_GUARD(ctx);
  int rc = ctx_bind(ctx);
  if (rc) return rc;
  if (!name || !ms) return fail(C1_ERR_ARG, "name or ms is NULL");
  if ((rc = collect_timings(ctx))) return rc;
  double total = 0;
  int count = 0;
  for (int k = 0; k < K_KINDS; k++) {
    if (!strcmp(name, kKindNames[k])) {
      *ms = ctx->ms[k];
      if (launches) *launches = ctx->launches[k];
      return C1_OK;
    }
    total += ctx->ms[k];
    count += ctx->launches[k];
  }
  if (!strcmp(name, "total")) {
    *ms = total;
    if (launches) *launches = count;
    return C1_OK;
  }
  return fail(C1_ERR_ARG, "unknown kernel name '%s'", name);
}

int c1_encode_device(c1_ctx *ctx, const float *const *pcm, int channels, int64_t frames, int halo_frames,
                     const c1_encode_options *opts, uint8_t *units) {
  if (!units && frames > 0) return fail(C1_ERR_ARG, "units is NULL");
  // On a context that owns its stream the last chunk's exact redo may still be running on the tail stream when the call
  // returns: it overlaps the next call's analysis.  c1_ctx_synchronize and every other entry point wait for it.
  return encode_device_impl(ctx, pcm, channels, frames, halo_frames, opts, units, nullptr, nullptr, nullptr, nullptr, ctx && ctx->own_stream);
}
// for the host-resident entry points below: ordered like any other work on the context's stream
static int encode_device_joined(c1_ctx *ctx, const float *const *pcm, int channels, int64_t frames, int halo_frames,
                                const c1_encode_options *opts, uint8_t *units) {
  if (!units && frames > 0) return fail(C1_ERR_ARG, "units is NULL");
  return encode_device_impl(ctx, pcm, channels, frames, halo_frames, opts, units, nullptr, nullptr, nullptr, nullptr, false);
}

int c1_encode_modes_device(c1_ctx *ctx, const float *const *pcm, int channels, int64_t frames, int halo_frames,
                           const c1_encode_options *opts, const uint8_t *modes, uint8_t *units) {
  if (frames > 0 && (!modes || !units)) return fail(C1_ERR_ARG, "modes or units is NULL");
  if (frames > kMaxChunkFrames) return fail(C1_ERR_ARG, "at most %lld frames per call", (long long)kMaxChunkFrames);
  return encode_device_impl(ctx, pcm, channels, frames, halo_frames, opts, units, nullptr, nullptr, nullptr, nullptr, false, frames > 0 ? modes : nullptr);
}

int c1_encode_stages_device(c1_ctx *ctx, const float *const *pcm, int channels, int64_t frames, int halo_frames,
                            const c1_encode_options *opts, float *bands, float *coefs, uint8_t *side,
                            uint8_t *alloc) {
  return encode_device_impl(ctx, pcm, channels, frames, halo_frames, opts, nullptr, bands, coefs, side, alloc);
}

int c1_detect_stages_device(c1_ctx *ctx, const float *const *pcm, int channels, int64_t frames, int halo_frames,
                            const c1_encode_options *opts, float *mags, uint8_t *modes) {
  CTX_GUARD(ctx);
  int rc = ctx_bind(ctx);
  if (rc) return rc;
  if ((rc = check_channels(channels))) return rc;
  if (frames < 0 || halo_frames < 0 || halo_frames > 2) return fail(C1_ERR_ARG, "bad frames / halo_frames");
  if (!pcm || !opts) return fail(C1_ERR_ARG, "NULL argument");
  if (opts->fixed_block_modes[0] >= 0) return fail(C1_ERR_ARG, "the detector taps need transient detection (fixed_block_modes -1)");
  if (frames > kMaxChunkFrames) return fail(C1_ERR_ARG, "stage taps are not chunked: at most %lld frames per call", (long long)kMaxChunkFrames);
  for (int c = 0; c < channels; c++)
    if (!pcm[c] || ((uintptr_t)pcm[c] & 15)) return fail(C1_ERR_ARG, "pcm[%d] must be a 16-byte aligned device pointer", c);
  if ((rc = upload_opts(ctx, opts))) return rc;
  if (frames == 0) return C1_OK;
  const int64_t units = frames * channels;
  if ((rc = ensure_workspace(ctx, units))) return rc;
  if ((rc = ensure_detect_workspace(ctx, units))) return rc;
  C1EncodeLaunch L;
  memset(&L, 0, sizeof L);
  for (int c = 0; c < channels; c++) L.pcm[c] = pcm[c];
  L.channels = channels; L.frames = frames; L.halo_frames = halo_frames;
  L.tables = ctx->d_tables; L.opts = ctx->d_opts;
  L.coefs = ctx->d_coefs[0]; L.side = ctx->d_side[0]; L.alloc = ctx->d_alloc[0]; L.cand = ctx->d_cand[0];
  L.work_count = ctx->d_work[0]; L.work_list = ctx->d_work[0] + 4; L.sel_list = ctx->d_work[0] + 4 + (size_t)ctx->ws_units * 7;
  L.mags = mags;
  c1k_launch_detect(L, ctx->d_bands[0], ctx->d_feat[0], ctx->d_modes[0], ctx->d_lists[0], false, nullptr, ctx->stream);
  if (modes) HIP_TRY(hipMemcpyAsync(modes, ctx->d_modes[0], (size_t)units, hipMemcpyDeviceToDevice, ctx->stream));
  HIP_TRY(hipGetLastError());
  return C1_OK;
}

int c1_detect_scores_device(c1_ctx *ctx, const float *const *pcm, int channels, int64_t frames, int halo_frames,
                            const c1_encode_options *opts, int speculative, double *scores, uint8_t *modes, uint32_t *open_units) {
  CTX_GUARD(ctx);
  int rc = ctx_bind(ctx);
  if (rc) return rc;
  if ((rc = check_channels(channels))) return rc;
  if (frames < 0 || halo_frames < 0 || halo_frames > 2) return fail(C1_ERR_ARG, "bad frames / halo_frames");
  if (!pcm || !opts) return fail(C1_ERR_ARG, "NULL argument");
  if (opts->fixed_block_modes[0] >= 0) return fail(C1_ERR_ARG, "the detector taps need transient detection (fixed_block_modes -1)");
  if (frames > kMaxChunkFrames) return fail(C1_ERR_ARG, "stage taps are not chunked: at most %lld frames per call", (long long)kMaxChunkFrames);
  if (speculative && !ctx->spec_tables_ok) return fail(C1_ERR_ARG, "the installed tables do not admit the speculative paths");
  for (int c = 0; c < channels; c++)
    if (!pcm[c] || ((uintptr_t)pcm[c] & 15)) return fail(C1_ERR_ARG, "pcm[%d] must be a 16-byte aligned device pointer", c);
  if ((rc = upload_opts(ctx, opts))) return rc;
  if (frames == 0) return C1_OK;
  const int64_t units = frames * channels;
  if ((rc = ensure_detect_workspace(ctx, units))) return rc;
  C1EncodeLaunch L;
  memset(&L, 0, sizeof L);
  for (int c = 0; c < channels; c++) L.pcm[c] = pcm[c];
  L.channels = channels; L.frames = frames; L.halo_frames = halo_frames;
  L.tables = ctx->d_tables; L.opts = ctx->d_opts;
  c1k_launch_detect(L, ctx->d_bands[0], ctx->d_feat[0], ctx->d_modes[0], ctx->d_lists[0], speculative != 0, scores, ctx->stream);
  if (modes) HIP_TRY(hipMemcpyAsync(modes, ctx->d_modes[0], (size_t)units, hipMemcpyDeviceToDevice, ctx->stream));
  if (open_units) HIP_TRY(hipMemcpyAsync(open_units, ctx->d_lists[0] + 2, sizeof(uint32_t), hipMemcpyDeviceToDevice, ctx->stream));
  HIP_TRY(hipGetLastError());
  return C1_OK;
}

int c1_detect_spec_mags_device(c1_ctx *ctx, const float *const *pcm, int channels, int64_t frames, int halo_frames,
                               float *mags, float *bounds) {
  CTX_GUARD(ctx);
  int rc = ctx_bind(ctx);
  if (rc) return rc;
  if ((rc = check_channels(channels))) return rc;
  if (frames < 0 || halo_frames < 0 || halo_frames > 2) return fail(C1_ERR_ARG, "bad frames / halo_frames");
  if (!pcm || !mags || !bounds) return fail(C1_ERR_ARG, "NULL argument");
  if (frames > kMaxChunkFrames) return fail(C1_ERR_ARG, "stage taps are not chunked: at most %lld frames per call", (long long)kMaxChunkFrames);
  if (!ctx->spec_tables_ok) return fail(C1_ERR_ARG, "the installed tables do not admit the speculative paths");
  for (int c = 0; c < channels; c++)
    if (!pcm[c] || ((uintptr_t)pcm[c] & 15)) return fail(C1_ERR_ARG, "pcm[%d] must be a 16-byte aligned device pointer", c);
  if (frames == 0) return C1_OK;
  if ((rc = ensure_detect_workspace(ctx, frames * channels))) return rc;
  C1EncodeLaunch L;
  memset(&L, 0, sizeof L);
  for (int c = 0; c < channels; c++) L.pcm[c] = pcm[c];
  L.channels = channels; L.frames = frames; L.halo_frames = halo_frames;
  L.tables = ctx->d_tables; L.opts = ctx->d_opts;
  L.mags = mags; L.mag_bounds = bounds;
  c1k_launch_detect_spec_tap(L, ctx->d_bands[0], ctx->d_feat[0], ctx->stream);
  HIP_TRY(hipGetLastError());
  return C1_OK;
}

int c1_log2f_error_device(c1_ctx *ctx, uint32_t first_bits, uint64_t count, double *out_host) {
  CTX_GUARD(ctx);
  int rc = ctx_bind(ctx);
  if (rc) return rc;
  if (!out_host) return fail(C1_ERR_ARG, "out is NULL");
  if (first_bits < 0x00800000u || (uint64_t)first_bits + count > 0x7f800000ull) return fail(C1_ERR_ARG, "range must stay within the normal positive binary32 numbers");
  if ((rc = ensure_io(ctx, 16))) return rc;
  c1k_launch_log2f_error(first_bits, count, reinterpret_cast<unsigned long long *>(ctx->d_io), ctx->stream);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(out_host, ctx->d_io, 16, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return C1_OK;
}

int c1_alloc_bounds_device(c1_ctx *ctx, const uint8_t *side, int64_t units, const c1_encode_options *opts, double *out) {
  CTX_GUARD(ctx);
  int rc = ctx_bind(ctx);
  if (rc) return rc;
  if (units < 0 || units > ((int64_t)1 << 24) || (units > 0 && (!side || !out))) return fail(C1_ERR_ARG, "bad units / NULL argument");
  if ((rc = upload_opts(ctx, opts))) return rc;
  if (units == 0) return C1_OK;
  if ((rc = ensure_workspace(ctx, units * 2))) return rc;        // the tap lists all eight candidates of every unit: 9 list entries per unit
  C1EncodeLaunch L;
  memset(&L, 0, sizeof L);
  L.channels = 1;
  L.frames = units;
  L.tables = ctx->d_tables;
  L.opts = ctx->d_opts;
  L.side = const_cast<uint8_t *>(side);
  L.alloc = ctx->d_alloc[0];
  L.cand = ctx->d_cand[0];
  L.work_count = ctx->d_work[0];
  L.work_list = ctx->d_work[0] + 4;
  L.sel_list = ctx->d_work[0] + 4 + (size_t)ctx->ws_units * 7;
  c1k_launch_alloc_tap(L, out, ctx->stream);
  HIP_TRY(hipGetLastError());
  return C1_OK;
}

int c1_libm_device(c1_ctx *ctx, int fn, const double *in, double *out, int64_t n) {
  CTX_GUARD(ctx);
  int rc = ctx_bind(ctx);
  if (rc) return rc;
  if (fn < 0 || fn > 4 || n < 0 || (n > 0 && (!in || !out))) return fail(C1_ERR_ARG, "bad fn / n / NULL argument");
  if (fn == 4) c1k_launch_js_log2(in, out, n, ctx->stream);
  else c1k_launch_libm(fn, in, out, n, ctx->stream);
  HIP_TRY(hipGetLastError());
  return C1_OK;
}

int c1_spec_stages_device(c1_ctx *ctx, const float *const *pcm, int channels, int64_t frames, int halo_frames,
                          const c1_encode_options *opts, float *coefs, float *eps, uint8_t *side) {
  CTX_GUARD(ctx);
  int rc = ctx_bind(ctx);
  if (rc) return rc;
  if ((rc = check_channels(channels))) return rc;
  if (frames < 0 || halo_frames < 0 || halo_frames > 2) return fail(C1_ERR_ARG, "bad frames / halo_frames");
  if (!pcm || !opts || !coefs || !eps || !side) return fail(C1_ERR_ARG, "NULL argument");
  const bool sp_long = opts->fixed_block_modes[0] == 0 && opts->fixed_block_modes[1] == 0 && opts->fixed_block_modes[2] == 0;
  const bool sp_short = opts->fixed_block_modes[0] > 0 && opts->fixed_block_modes[1] > 0 && opts->fixed_block_modes[2] > 0;
  if (!sp_long && !sp_short)
    return fail(C1_ERR_ARG, "the speculative analysis covers fixed block modes with all bands long or all bands short");
  if (!ctx->spec_tables_ok) return fail(C1_ERR_STATE, "the installed tables fail the checks the error bound relies on");
  for (int c = 0; c < channels; c++)
    if (!pcm[c] || ((uintptr_t)pcm[c] & 15)) return fail(C1_ERR_ARG, "pcm[%d] must be a 16-byte aligned device pointer", c);
  if ((rc = upload_opts(ctx, opts))) return rc;
  if (frames == 0) return C1_OK;
  C1EncodeLaunch L;
  memset(&L, 0, sizeof L);
  for (int c = 0; c < channels; c++) L.pcm[c] = pcm[c];
  L.channels = channels; L.frames = frames; L.halo_frames = halo_frames;
  L.tables = ctx->d_tables; L.opts = ctx->d_opts;
  L.coefs = coefs; L.eps = eps; L.side = side;
  c1k_launch_analysis_spec(L, sp_short, ctx->stream);
  HIP_TRY(hipGetLastError());
  return C1_OK;
}

// ---- the single-stage functions of the reference's export surface (codec/index.js:30-35,42), host-resident ----------

int c1_quantize(c1_ctx *ctx, const float *coefficients, int n, int scale_factor_index, int bits_per_sample, int32_t *out) {
  CTX_GUARD(ctx);
  int rc = ctx_bind(ctx);
  if (rc) return rc;
  if (n < 0 || (n > 0 && (!coefficients || !out))) return fail(C1_ERR_ARG, "quantize: bad arguments");
  if (scale_factor_index < 0 || scale_factor_index > 63) return fail(C1_ERR_ARG, "quantize: scaleFactorIndex %d outside SCALE_FACTORS", scale_factor_index);
  if (n == 0) return C1_OK;
  DeviceScratch ds;
  float *dx; int32_t *dq;
  if ((rc = ds.alloc(&dx, (size_t)n)) || (rc = ds.alloc(&dq, (size_t)n))) return rc;
  HIP_TRY(hipMemcpyAsync(dx, coefficients, (size_t)n * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  c1k_launch_quantize_one(ctx->d_tables, dx, n, scale_factor_index, bits_per_sample, dq, ctx->stream);
  HIP_TRY(hipMemcpyAsync(out, dq, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return C1_OK;
}

int c1_dequantize(c1_ctx *ctx, const int32_t *quantized, int n, int scale_factor_index, int bits_per_sample, float *out) {
  CTX_GUARD(ctx);
  int rc = ctx_bind(ctx);
  if (rc) return rc;
  if (n < 0 || (n > 0 && (!quantized || !out))) return fail(C1_ERR_ARG, "dequantize: bad arguments");
  if (scale_factor_index < 0 || scale_factor_index > 63) return fail(C1_ERR_ARG, "dequantize: scaleFactorIndex %d outside SCALE_FACTORS", scale_factor_index);
  if (n == 0) return C1_OK;
  DeviceScratch ds;
  int32_t *dq; float *dx;
  if ((rc = ds.alloc(&dq, (size_t)n)) || (rc = ds.alloc(&dx, (size_t)n))) return rc;
  HIP_TRY(hipMemcpyAsync(dq, quantized, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
  c1k_launch_dequantize_one(ctx->d_tables, dq, n, scale_factor_index, bits_per_sample, dx, ctx->stream);
  HIP_TRY(hipMemcpyAsync(out, dx, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return C1_OK;
}

int c1_fft(c1_ctx *ctx, float *real, float *imag, int n, const double *w) {
  CTX_GUARD(ctx);
  int rc = ctx_bind(ctx);
  if (rc) return rc;
  if (n < 1 || (n & (n - 1)) || n > (1 << 22)) return fail(C1_ERR_ARG, "fft: size must be a power of two <= 2^22, got %d", n);
  if (!real || !imag || (n > 1 && !w)) return fail(C1_ERR_ARG, "fft: NULL argument");
  if (n == 1) return C1_OK;                                  // fft.js:16
  int stages = 0;
  while ((1 << stages) < n) stages++;
  DeviceScratch ds;
  float *dr, *di; double *dw, *dtw;
  if ((rc = ds.alloc(&dr, (size_t)n)) || (rc = ds.alloc(&di, (size_t)n)) || (rc = ds.alloc(&dw, (size_t)2 * stages)) || (rc = ds.alloc(&dtw, (size_t)n))) return rc;
  HIP_TRY(hipMemcpyAsync(dr, real, (size_t)n * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(hipMemcpyAsync(di, imag, (size_t)n * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(hipMemcpyAsync(dw, w, (size_t)2 * stages * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  c1k_launch_fft_reference(dr, di, n, dw, dtw, ctx->stream);
  HIP_TRY(hipMemcpyAsync(real, dr, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipMemcpyAsync(imag, di, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return C1_OK;
}

int c1_qmf_analysis_batch(c1_ctx *ctx, const float *pcm, int64_t frames, int halo_frames, float *bands) {
  CTX_GUARD(ctx);
  int rc = ctx_bind(ctx);
  if (rc) return rc;
  if (frames < 0 || halo_frames < 0 || halo_frames > 2) return fail(C1_ERR_ARG, "qmf analysis: bad frames / halo_frames");
  if (frames == 0) return C1_OK;
  if (!pcm || !bands) return fail(C1_ERR_ARG, "qmf analysis: NULL argument");
  if (frames > (1 << 20)) return fail(C1_ERR_ARG, "qmf analysis: at most 2^20 frames per call");
  DeviceScratch ds;
  float *dp, *db, *dc; uint8_t *dside, *dalloc;
  const size_t total = (size_t)(frames + halo_frames) * 512;
  if ((rc = ds.alloc(&dp, total)) || (rc = ds.alloc(&db, (size_t)frames * 512)) || (rc = ds.alloc(&dc, (size_t)frames * 512)) ||
      (rc = ds.alloc(&dside, (size_t)frames * kSideBytes)) || (rc = ds.alloc(&dalloc, (size_t)frames * kAllocBytes))) return rc;
  HIP_TRY(hipMemcpyAsync(dp, pcm, total * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  c1_encode_options o;
  c1_default_encode_options(&o);
  o.fixed_block_modes[0] = o.fixed_block_modes[1] = o.fixed_block_modes[2] = 0;   // the bands do not depend on the block modes
  const float *chan[1] = {dp + (size_t)halo_frames * 512};
  if ((rc = encode_device_impl(ctx, chan, 1, frames, halo_frames, &o, nullptr, db, dc, dside, dalloc))) return rc;
  HIP_TRY(hipMemcpyAsync(bands, db, (size_t)frames * 512 * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return C1_OK;
}

int c1_mdct_batch(c1_ctx *ctx, const float *bands, int64_t frames, int halo_frames, const int32_t *block_modes, float *coefs,
                  float *bands_windowed) {
  CTX_GUARD(ctx);
  int rc = ctx_bind(ctx);
  if (rc) return rc;
  if (frames < 0 || halo_frames < 0 || halo_frames > 1) return fail(C1_ERR_ARG, "mdct: halo_frames must be 0 or 1");
  if (frames == 0) return C1_OK;
  if (!bands || !block_modes || !coefs) return fail(C1_ERR_ARG, "mdct: NULL argument");
  if (frames > (1 << 20)) return fail(C1_ERR_ARG, "mdct: at most 2^20 frames per call");
  // any non-zero mode is a short band (encoder.js:196); the unit header's values are 2, 2, 3
  std::vector<uint8_t> modes((size_t)frames);
  std::vector<uint32_t> lists(4 + 2 * (size_t)frames, 0u);
  for (int64_t f = 0; f < frames; f++) {
    const int m0 = block_modes[3 * f] ? 2 : 0, m1 = block_modes[3 * f + 1] ? 2 : 0, m2 = block_modes[3 * f + 2] ? 3 : 0;
    modes[(size_t)f] = (uint8_t)(m0 | (m1 << 2) | (m2 << 4));
    if (modes[(size_t)f] == 0) lists[4 + lists[0]++] = (uint32_t)f;
    else lists[4 + (size_t)frames + lists[1]++] = (uint32_t)f;
  }
  DeviceScratch ds;
  float *db, *dc, *dw = nullptr; uint8_t *dm, *dside; uint32_t *dl;
  if ((rc = ds.alloc(&db, (size_t)(frames + 1) * 512)) || (rc = ds.alloc(&dc, (size_t)frames * 512)) || (rc = ds.alloc(&dm, (size_t)frames)) ||
      (rc = ds.alloc(&dside, (size_t)frames * kSideBytes)) || (rc = ds.alloc(&dl, lists.size()))) return rc;
  if (bands_windowed && (rc = ds.alloc(&dw, (size_t)frames * 512))) return rc;
  // slot row 0 = frame -1: the halo frame, or nothing (a fresh BufferPool's zero overlap, buffers.js:44-48)
  if (!halo_frames) HIP_TRY(hipMemsetAsync(db, 0, 512 * sizeof(float), ctx->stream));
  HIP_TRY(hipMemcpyAsync(db + (halo_frames ? 0 : 512), bands, (size_t)(frames + halo_frames) * 512 * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(hipMemcpyAsync(dm, modes.data(), modes.size(), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(hipMemcpyAsync(dl, lists.data(), lists.size() * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
  C1EncodeLaunch L;
  memset(&L, 0, sizeof L);
  L.channels = 1; L.frames = frames; L.halo_frames = halo_frames;
  L.tables = ctx->d_tables; L.opts = ctx->d_opts;
  L.coefs = dc; L.side = dside;
  c1k_launch_mdct_bands(L, db, dm, dl, ctx->stream);
  if (dw) c1k_launch_window_bands(db + 512, dm, frames, ctx->d_tables, dw, ctx->stream);
  HIP_TRY(hipMemcpyAsync(coefs, dc, (size_t)frames * 512 * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  if (dw) HIP_TRY(hipMemcpyAsync(bands_windowed, dw, (size_t)frames * 512 * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));       // also: the host vectors above outlive the copies
  HIP_TRY(hipGetLastError());
  return C1_OK;
}

// ---- the decoder's pipeline stages on their own (codec/pipeline/decoder.js:52-389, serialization.js:111-176), host-resident ----

namespace {
constexpr int64_t kMaxStageFrames = (int64_t)1 << 20;

// The indices the reference reads (BFUs below nBfu) must name table entries: BFU_START_*, WORD_LENGTH_BITS, SCALE_FACTORS.
// units = frames * channels frame fields, unit u = frame (first_frame + u / channels) of channel u % channels.
int check_field_domain(const char *what, int64_t units, int channels, int64_t first_frame, const int32_t *nbfu, const int32_t *sfi,
                       const int32_t *wl) {
  auto where = [&](int64_t u) {
    char at[64];
    if (channels == 1) snprintf(at, sizeof at, "frame %lld", (long long)(first_frame + u));
    else snprintf(at, sizeof at, "frame %lld channel %d", (long long)(first_frame + u / channels), (int)(u % channels));
    return std::string(at);
  };
  for (int64_t u = 0; u < units; u++) {
    const int32_t n = nbfu[u];
    if (n < 0 || n > 52) return fail(C1_ERR_ARG, "%s: %s: nBfu %d outside 0..52", what, where(u).c_str(), n);
    for (int b = 0; b < n; b++) {
      const int32_t w = wl[52 * u + b], s = sfi[52 * u + b];
      if (w < 0 || w > 15) return fail(C1_ERR_ARG, "%s: %s BFU %d: word length index %d outside 0..15", what, where(u).c_str(), b, w);
      if (s < 0 || s > 63) return fail(C1_ERR_ARG, "%s: %s BFU %d: scale factor index %d outside 0..63", what, where(u).c_str(), b, s);
    }
  }
  return C1_OK;
}

// the five field arrays of `units` frame fields packed in one allocation, in this order (one copy moves them all; q stays
// 16-byte aligned: it starts 432 * units bytes in)
constexpr int64_t kFieldInts = 1 + 3 + 52 + 52 + 512;
C1FieldPtrs field_layout(const int32_t *base, int64_t units) {
  return C1FieldPtrs{base, base + units, base + 4 * units, base + 56 * units, base + 108 * units};
}
C1FieldPtrs field_unit(const C1FieldPtrs &p, int64_t u) {
  return C1FieldPtrs{p.nbfu + u, p.modes + 3 * u, p.sfi + 52 * u, p.wl + 52 * u, p.q + 512 * u};
}
}  // namespace

int c1_unpack_units(c1_ctx *ctx, const uint8_t *units, int64_t frames, int32_t *nbfu, int32_t *block_modes, int32_t *sfi,
                    int32_t *wl, int32_t *quantized) {
  CTX_GUARD(ctx);
  int rc = ctx_bind(ctx);
  if (rc) return rc;
  if (frames < 0 || frames > kMaxStageFrames) return fail(C1_ERR_ARG, "unpack: frames must be 0 .. 2^20, got %lld", (long long)frames);
  if (frames == 0) return C1_OK;
  if (!units || !nbfu || !block_modes || !sfi || !wl || !quantized) return fail(C1_ERR_ARG, "unpack: NULL argument");
  DeviceScratch ds;
  uint8_t *du; int32_t *dn, *dm, *ds_, *dw, *dq;
  const size_t n = (size_t)frames;
  if ((rc = ds.alloc(&du, n * C1_UNIT_BYTES)) || (rc = ds.alloc(&dn, n)) || (rc = ds.alloc(&dm, 3 * n)) || (rc = ds.alloc(&ds_, 52 * n)) ||
      (rc = ds.alloc(&dw, 52 * n)) || (rc = ds.alloc(&dq, 512 * n))) return rc;
  HIP_TRY(hipMemcpyAsync(du, units, n * C1_UNIT_BYTES, hipMemcpyHostToDevice, ctx->stream));
  c1k_launch_unpack_units(du, frames, dn, dm, ds_, dw, dq, ctx->stream);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(nbfu, dn, n * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipMemcpyAsync(block_modes, dm, 3 * n * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipMemcpyAsync(sfi, ds_, 52 * n * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipMemcpyAsync(wl, dw, 52 * n * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipMemcpyAsync(quantized, dq, 512 * n * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return C1_OK;
}

int c1_dequantize_frames(c1_ctx *ctx, int64_t frames, const int32_t *nbfu, const int32_t *block_modes, const int32_t *sfi,
                         const int32_t *wl, const int32_t *quantized, float *coefs) {
  CTX_GUARD(ctx);
  int rc = ctx_bind(ctx);
  if (rc) return rc;
  if (frames < 0 || frames > kMaxStageFrames) return fail(C1_ERR_ARG, "dequantize frames: frames must be 0 .. 2^20, got %lld", (long long)frames);
  if (frames == 0) return C1_OK;
  if (!nbfu || !block_modes || !sfi || !wl || !quantized || !coefs) return fail(C1_ERR_ARG, "dequantize frames: NULL argument");
  if ((rc = check_field_domain("dequantize frames", frames, 1, 0, nbfu, sfi, wl))) return rc;
  DeviceScratch ds;
  int32_t *dn, *dm, *ds_, *dw, *dq; float *dc;
  const size_t n = (size_t)frames;
  if ((rc = ds.alloc(&dn, n)) || (rc = ds.alloc(&dm, 3 * n)) || (rc = ds.alloc(&ds_, 52 * n)) || (rc = ds.alloc(&dw, 52 * n)) ||
      (rc = ds.alloc(&dq, 512 * n)) || (rc = ds.alloc(&dc, 512 * n))) return rc;
  HIP_TRY(hipMemcpyAsync(dn, nbfu, n * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(hipMemcpyAsync(dm, block_modes, 3 * n * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(hipMemcpyAsync(ds_, sfi, 52 * n * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(hipMemcpyAsync(dw, wl, 52 * n * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(hipMemcpyAsync(dq, quantized, 512 * n * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
  c1k_launch_dequantize_frames(ctx->d_tables, dn, dm, ds_, dw, dq, frames, dc, ctx->stream);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(coefs, dc, 512 * n * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return C1_OK;
}

int c1_imdct_batch(c1_ctx *ctx, const float *coefs, int64_t frames, int halo_frames, const int32_t *block_modes, float *bands) {
  CTX_GUARD(ctx);
  int rc = ctx_bind(ctx);
  if (rc) return rc;
  if (halo_frames < 0 || halo_frames > 1) return fail(C1_ERR_ARG, "imdct: halo_frames must be 0 or 1, got %d", halo_frames);
  if (frames < 0 || frames > kMaxStageFrames) return fail(C1_ERR_ARG, "imdct: frames must be 0 .. 2^20, got %lld", (long long)frames);
  if (frames == 0) return C1_OK;
  if (!coefs || !block_modes || !bands) return fail(C1_ERR_ARG, "imdct: NULL argument");
  DeviceScratch ds;
  float *dc, *db; int32_t *dm;
  const size_t n = (size_t)frames, all = (size_t)(frames + halo_frames);
  if ((rc = ds.alloc(&dc, 512 * all)) || (rc = ds.alloc(&dm, 3 * all)) || (rc = ds.alloc(&db, 512 * n))) return rc;
  HIP_TRY(hipMemcpyAsync(dc, coefs, 512 * all * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(hipMemcpyAsync(dm, block_modes, 3 * all * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
  c1k_launch_imdct_frames(ctx->d_tables, dc, dm, frames, halo_frames, db, ctx->stream);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(bands, db, 512 * n * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return C1_OK;
}

int c1_qmf_synthesis_batch(c1_ctx *ctx, const float *bands, int64_t frames, int halo_frames, float *pcm) {
  CTX_GUARD(ctx);
  int rc = ctx_bind(ctx);
  if (rc) return rc;
  if (halo_frames < 0 || halo_frames > 1) return fail(C1_ERR_ARG, "qmf synthesis: halo_frames must be 0 or 1, got %d", halo_frames);
  if (frames < 0 || frames > kMaxStageFrames) return fail(C1_ERR_ARG, "qmf synthesis: frames must be 0 .. 2^20, got %lld", (long long)frames);
  if (frames == 0) return C1_OK;
  if (!bands || !pcm) return fail(C1_ERR_ARG, "qmf synthesis: NULL argument");
  DeviceScratch ds;
  float *db, *dp;
  const size_t n = (size_t)frames, all = (size_t)(frames + halo_frames);
  if ((rc = ds.alloc(&db, 512 * all)) || (rc = ds.alloc(&dp, 512 * n))) return rc;
  HIP_TRY(hipMemcpyAsync(db, bands, 512 * all * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  c1k_launch_qmf_synthesis_frames(ctx->d_tables, db, frames, halo_frames, dp, ctx->stream);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(pcm, dp, 512 * n * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return C1_OK;
}

// ---- the encoder's block selection, quantization and serialization stages on their own (encoder.js:111-152, :365-418,
// serialization.js:41-98) ----

int c1_select_block_modes(c1_ctx *ctx, const float *bands, int64_t frames, int halo_frames, double threshold, int32_t *block_modes) {
  CTX_GUARD(ctx);
  int rc = ctx_bind(ctx);
  if (rc) return rc;
  if (halo_frames < 0 || halo_frames > 1) return fail(C1_ERR_ARG, "select block modes: halo_frames must be 0 or 1, got %d", halo_frames);
  if (frames < 0 || frames > kMaxStageFrames) return fail(C1_ERR_ARG, "select block modes: frames must be 0 .. 2^20, got %lld", (long long)frames);
  if (frames == 0) return C1_OK;
  if (!bands || !block_modes) return fail(C1_ERR_ARG, "select block modes: NULL argument");
  DeviceScratch ds;
  float *db, *dm; int32_t *dmodes;
  const size_t n = (size_t)frames, all = (size_t)(frames + halo_frames);
  if ((rc = ds.alloc(&db, 512 * all)) || (rc = ds.alloc(&dm, 256 * all)) || (rc = ds.alloc(&dmodes, 3 * n))) return rc;
  HIP_TRY(hipMemcpyAsync(db, bands, 512 * all * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  c1k_launch_block_modes_from_bands(ctx->d_tables, db, frames, halo_frames, threshold, dm, dmodes, ctx->stream);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(block_modes, dmodes, 3 * n * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return C1_OK;
}

int c1_quantize_frames(c1_ctx *ctx, const float *coefs, int64_t frames, const int32_t *block_modes, const c1_encode_options *opts,
                       int32_t *nbfu, int32_t *sfi, int32_t *wl, int32_t *quantized) {
  CTX_GUARD(ctx);
  int rc = ctx_bind(ctx);
  if (rc) return rc;
  if (!opts) return fail(C1_ERR_ARG, "quantize frames: options are NULL");
  if (frames < 0 || frames > kMaxStageFrames) return fail(C1_ERR_ARG, "quantize frames: frames must be 0 .. 2^20, got %lld", (long long)frames);
  if (frames == 0) return C1_OK;
  if (!coefs || !block_modes || !nbfu || !sfi || !wl || !quantized) return fail(C1_ERR_ARG, "quantize frames: NULL argument");
  // the stage reads allocationBias alone: the threshold and the fixed modes of `opts` are not looked at
  c1_encode_options o = *opts;
  o.transient_threshold = 1.0;
  o.fixed_block_modes[0] = o.fixed_block_modes[1] = o.fixed_block_modes[2] = -1;
  if ((rc = upload_opts(ctx, &o))) return rc;
  DeviceScratch ds;
  float *dc; int32_t *dmodes, *dn, *ds_, *dw, *dq; uint8_t *dside, *dalloc, *dcand; uint32_t *dwork;
  const size_t n = (size_t)frames;
  if ((rc = ds.alloc(&dc, 512 * n)) || (rc = ds.alloc(&dmodes, 3 * n)) || (rc = ds.alloc(&dside, kSideBytes * n)) ||
      (rc = ds.alloc(&dalloc, kAllocBytes * n)) || (rc = ds.alloc(&dcand, (size_t)kCandidateBytes * n)) ||
      (rc = ds.alloc(&dwork, 4 + 8 * n)) || (rc = ds.alloc(&dn, n)) || (rc = ds.alloc(&ds_, 52 * n)) || (rc = ds.alloc(&dw, 52 * n)) ||
      (rc = ds.alloc(&dq, 512 * n))) return rc;
  HIP_TRY(hipMemcpyAsync(dc, coefs, 512 * n * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(hipMemcpyAsync(dmodes, block_modes, 3 * n * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
  c1k_launch_stage_scale_factors(ctx->d_tables, dc, dmodes, frames, dside, ctx->stream);
  // allocateBits as the encoder runs it (c1k_launch_allocate), on per-call scratch: counts, then 7 work-list entries and one
  // selection-list entry per frame (the layout c1_alloc_bounds_device gives the context's workspace)
  C1EncodeLaunch L;
  memset(&L, 0, sizeof L);
  L.channels = 1;
  L.frames = frames;
  L.tables = ctx->d_tables;
  L.opts = ctx->d_opts;
  L.side = dside;
  L.alloc = dalloc;
  L.cand = dcand;
  L.work_count = dwork;
  L.work_list = dwork + 4;
  L.sel_list = dwork + 4 + 7 * n;
  c1k_launch_allocate(L, ctx->stream);
  c1k_launch_stage_fields(ctx->d_tables, dc, dmodes, dside, dalloc, frames, dn, ds_, dw, dq, ctx->stream);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(nbfu, dn, n * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipMemcpyAsync(sfi, ds_, 52 * n * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipMemcpyAsync(wl, dw, 52 * n * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipMemcpyAsync(quantized, dq, 512 * n * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return C1_OK;
}

int c1_pack_units(c1_ctx *ctx, int64_t frames, const int32_t *nbfu, const int32_t *block_modes, const int32_t *sfi, const int32_t *wl,
                  const int32_t *quantized, uint8_t *units) {
  CTX_GUARD(ctx);
  int rc = ctx_bind(ctx);
  if (rc) return rc;
  if (frames < 0 || frames > kMaxStageFrames) return fail(C1_ERR_ARG, "pack units: frames must be 0 .. 2^20, got %lld", (long long)frames);
  if (frames == 0) return C1_OK;
  if (!nbfu || !block_modes || !sfi || !wl || !quantized || !units) return fail(C1_ERR_ARG, "pack units: NULL argument");
  // the field layout holds 52 BFUs; every other value takes the reference's meaning (include/carta1_hip.h)
  for (int64_t f = 0; f < frames; f++)
    if (nbfu[f] < 0 || nbfu[f] > 52) return fail(C1_ERR_ARG, "pack units: frame %lld: nBfu %d outside 0..52", (long long)f, nbfu[f]);
  DeviceScratch ds;
  int32_t *dn, *dm, *ds_, *dw, *dq; uint8_t *du;
  const size_t n = (size_t)frames;
  if ((rc = ds.alloc(&dn, n)) || (rc = ds.alloc(&dm, 3 * n)) || (rc = ds.alloc(&ds_, 52 * n)) || (rc = ds.alloc(&dw, 52 * n)) ||
      (rc = ds.alloc(&dq, 512 * n)) || (rc = ds.alloc(&du, n * C1_UNIT_BYTES))) return rc;
  HIP_TRY(hipMemcpyAsync(dn, nbfu, n * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(hipMemcpyAsync(dm, block_modes, 3 * n * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(hipMemcpyAsync(ds_, sfi, 52 * n * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(hipMemcpyAsync(dw, wl, 52 * n * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(hipMemcpyAsync(dq, quantized, 512 * n * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
  if (ctx->profiling && ctx->timing_depth == 0) reset_timings(ctx);
  { ScopedTiming t(ctx, K_PACK_UNITS); c1k_launch_pack_units(dn, dm, ds_, dw, dq, frames, du, ctx->stream); }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(units, du, n * C1_UNIT_BYTES, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return C1_OK;
}

// ---- the decision functions of analysis/transient.js and coding/bitallocation.js over batches of problems ----
namespace {
constexpr int64_t kMaxDecisionProblems = (int64_t)1 << 20;
constexpr int64_t kMaxDecisionValues = (int64_t)1 << 28;      // doubles of input per call (2 GiB)

// offsets[0..problems]: non-decreasing from 0; *total = offsets[problems]
int check_csr(const char *what, const int64_t *offsets, int64_t problems, int64_t *total) {
  if (offsets[0] != 0) return fail(C1_ERR_ARG, "%s: offsets[0] must be 0", what);
  for (int64_t p = 0; p < problems; p++)
    if (offsets[p + 1] < offsets[p]) return fail(C1_ERR_ARG, "%s: offsets decrease at problem %lld", what, (long long)p);
  if (offsets[problems] > kMaxDecisionValues) return fail(C1_ERR_ARG, "%s: more than 2^28 values", what);
  *total = offsets[problems];
  return C1_OK;
}
}  // namespace

int c1_perform_fft(c1_ctx *ctx, const double *samples, const int64_t *offsets, int64_t problems, int fft_size, const double *w,
                   float *magnitudes) {
  CTX_GUARD(ctx);
  int rc = ctx_bind(ctx);
  if (rc) return rc;
  if (fft_size < 1 || (fft_size & (fft_size - 1)) || fft_size > (1 << 22))
    return fail(C1_ERR_ARG, "perform fft: fftSize must be a power of two <= 2^22, got %d", fft_size);
  if (problems < 0 || problems > kMaxDecisionProblems) return fail(C1_ERR_ARG, "perform fft: problems must be 0 .. 2^20, got %lld", (long long)problems);
  if (problems == 0 || fft_size == 1) return C1_OK;          // fft.js:16; Float32Array(1 / 2) is empty
  if (!offsets || !w || !magnitudes) return fail(C1_ERR_ARG, "perform fft: NULL argument");
  if (problems * fft_size > ((int64_t)1 << 26)) return fail(C1_ERR_ARG, "perform fft: problems * fftSize above 2^26");
  int64_t total = 0;
  if ((rc = check_csr("perform fft", offsets, problems, &total))) return rc;
  if (total > 0 && !samples) return fail(C1_ERR_ARG, "perform fft: NULL argument");
  int stages = 0;
  while ((1 << stages) < fft_size) stages++;
  const size_t n = (size_t)fft_size, np = (size_t)problems;
  DeviceScratch ds;
  double *dsamp, *dw, *dtw; int64_t *doff; float *dre, *dim, *dmag;
  if ((rc = ds.alloc(&dsamp, (size_t)total)) || (rc = ds.alloc(&doff, np + 1)) || (rc = ds.alloc(&dw, 2 * (size_t)stages)) ||
      (rc = ds.alloc(&dtw, 2 * n)) || (rc = ds.alloc(&dre, np * n)) || (rc = ds.alloc(&dim, np * n)) || (rc = ds.alloc(&dmag, np * n / 2))) return rc;
  if (total > 0) HIP_TRY(hipMemcpyAsync(dsamp, samples, (size_t)total * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(hipMemcpyAsync(doff, offsets, (np + 1) * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(hipMemcpyAsync(dw, w, 2 * (size_t)stages * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  c1k_launch_perform_fft(dsamp, doff, problems, fft_size, dw, dtw, dre, dim, dmag, ctx->stream);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(magnitudes, dmag, np * n / 2 * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return C1_OK;
}

int c1_detect_transients(c1_ctx *ctx, const double *cur, const int64_t *cur_offsets, const double *prev, const int64_t *prev_offsets,
                         const uint8_t *has_prev, const double *thresholds, int64_t problems, uint8_t *transient, double *scores) {
  CTX_GUARD(ctx);
  int rc = ctx_bind(ctx);
  if (rc) return rc;
  if (problems < 0 || problems > kMaxDecisionProblems) return fail(C1_ERR_ARG, "detect transients: problems must be 0 .. 2^20, got %lld", (long long)problems);
  if (problems == 0) return C1_OK;
  if (!cur_offsets || !prev_offsets || !thresholds || !transient || !scores) return fail(C1_ERR_ARG, "detect transients: NULL argument");
  int64_t nc = 0, np_ = 0;
  if ((rc = check_csr("detect transients (current)", cur_offsets, problems, &nc)) ||
      (rc = check_csr("detect transients (previous)", prev_offsets, problems, &np_))) return rc;
  if ((nc > 0 && !cur) || (np_ > 0 && !prev)) return fail(C1_ERR_ARG, "detect transients: NULL argument");
  const size_t n = (size_t)problems;
  DeviceScratch ds;
  double *dc, *dp, *dthr, *dscore; int64_t *dco, *dpo; uint8_t *dhas = nullptr, *dout;
  if ((rc = ds.alloc(&dc, (size_t)nc)) || (rc = ds.alloc(&dp, (size_t)np_)) || (rc = ds.alloc(&dco, n + 1)) || (rc = ds.alloc(&dpo, n + 1)) ||
      (rc = ds.alloc(&dthr, n)) || (rc = ds.alloc(&dscore, n)) || (rc = ds.alloc(&dout, n)) || (has_prev && (rc = ds.alloc(&dhas, n)))) return rc;
  if (nc > 0) HIP_TRY(hipMemcpyAsync(dc, cur, (size_t)nc * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  if (np_ > 0) HIP_TRY(hipMemcpyAsync(dp, prev, (size_t)np_ * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(hipMemcpyAsync(dco, cur_offsets, (n + 1) * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(hipMemcpyAsync(dpo, prev_offsets, (n + 1) * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(hipMemcpyAsync(dthr, thresholds, n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  if (has_prev) HIP_TRY(hipMemcpyAsync(dhas, has_prev, n, hipMemcpyHostToDevice, ctx->stream));
  c1k_launch_detect_transients(dc, dco, dp, dpo, dhas, dthr, problems, ctx->d_tables, dout, dscore, ctx->stream);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(transient, dout, n, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipMemcpyAsync(scores, dscore, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return C1_OK;
}

int c1_find_scale_factors(c1_ctx *ctx, const double *values, const int64_t *offsets, const int64_t *lengths, int64_t problems,
                          int32_t *indices) {
  CTX_GUARD(ctx);
  int rc = ctx_bind(ctx);
  if (rc) return rc;
  if (problems < 0 || problems > kMaxDecisionProblems) return fail(C1_ERR_ARG, "find scale factors: problems must be 0 .. 2^20, got %lld", (long long)problems);
  if (problems == 0) return C1_OK;
  if (!offsets || !lengths || !indices) return fail(C1_ERR_ARG, "find scale factors: NULL argument");
  int64_t total = 0;
  if ((rc = check_csr("find scale factors", offsets, problems, &total))) return rc;
  if (total > 0 && !values) return fail(C1_ERR_ARG, "find scale factors: NULL argument");
  // `length` past the array reads undefined, which never raises the maximum: read min(length, array length), none for length <= 0
  const size_t n = (size_t)problems;
  std::vector<int64_t> counts(n);
  for (size_t p = 0; p < n; p++) counts[p] = std::max<int64_t>(0, std::min(lengths[p], offsets[p + 1] - offsets[p]));
  DeviceScratch ds;
  double *dv; int64_t *doff, *dcnt; int32_t *dout;
  if ((rc = ds.alloc(&dv, (size_t)total)) || (rc = ds.alloc(&doff, n + 1)) || (rc = ds.alloc(&dcnt, n)) || (rc = ds.alloc(&dout, n))) return rc;
  if (total > 0) HIP_TRY(hipMemcpyAsync(dv, values, (size_t)total * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(hipMemcpyAsync(doff, offsets, (n + 1) * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(hipMemcpyAsync(dcnt, counts.data(), n * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
  c1k_launch_find_scale_factors(dv, doff, dcnt, problems, dout, ctx->stream);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(indices, dout, n * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return C1_OK;
}

int c1_allocate_bits(c1_ctx *ctx, const double *data, int64_t data_len, const int64_t *bfu_offsets, const int32_t *bfu_lengths,
                     const int32_t *bfu_sizes, const int32_t *max_bfu_counts, int64_t problems, const double *biased_scale_factors,
                     int32_t *bfu_count, int32_t *allocation, int32_t *scale_factor_indices, uint8_t *fallback) {
  CTX_GUARD(ctx);
  int rc = ctx_bind(ctx);
  if (rc) return rc;
  if (problems < 0 || problems > kMaxDecisionProblems) return fail(C1_ERR_ARG, "allocate bits: problems must be 0 .. 2^20, got %lld", (long long)problems);
  if (problems == 0) return C1_OK;
  if (!bfu_offsets || !bfu_lengths || !bfu_sizes || !max_bfu_counts || !biased_scale_factors || !bfu_count || !allocation ||
      !scale_factor_indices || !fallback) return fail(C1_ERR_ARG, "allocate bits: NULL argument");
  if (data_len < 0 || data_len > kMaxDecisionValues || (data_len > 0 && !data)) return fail(C1_ERR_ARG, "allocate bits: bad data length");
  const size_t n = (size_t)problems;
  for (size_t p = 0; p < n; p++) {
    const int mb = max_bfu_counts[p];
    if (mb < 0 || mb > 52) return fail(C1_ERR_ARG, "allocate bits: problem %zu: maxBfuCount %d outside 0..52", p, mb);
    for (int i = 0; i < mb; i++) {
      const int64_t off = bfu_offsets[52 * p + i], len = bfu_lengths[52 * p + i];
      if (bfu_sizes[52 * p + i] != 0 && (off < 0 || len < 0 || off > data_len || len > data_len - off))
        return fail(C1_ERR_ARG, "allocate bits: problem %zu: BFU %d's values lie outside the data", p, i);
    }
  }
  DeviceScratch ds;
  double *dd, *dbsf; int64_t *doff; int32_t *dlen, *dsz, *dmb, *dcount, *dwl, *dsfi; uint8_t *dfb;
  if ((rc = ds.alloc(&dd, (size_t)data_len)) || (rc = ds.alloc(&dbsf, 64)) || (rc = ds.alloc(&doff, 52 * n)) || (rc = ds.alloc(&dlen, 52 * n)) ||
      (rc = ds.alloc(&dsz, 52 * n)) || (rc = ds.alloc(&dmb, n)) || (rc = ds.alloc(&dcount, n)) || (rc = ds.alloc(&dwl, 52 * n)) ||
      (rc = ds.alloc(&dsfi, 52 * n)) || (rc = ds.alloc(&dfb, n))) return rc;
  if (data_len > 0) HIP_TRY(hipMemcpyAsync(dd, data, (size_t)data_len * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(hipMemcpyAsync(dbsf, biased_scale_factors, 64 * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(hipMemcpyAsync(doff, bfu_offsets, 52 * n * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(hipMemcpyAsync(dlen, bfu_lengths, 52 * n * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(hipMemcpyAsync(dsz, bfu_sizes, 52 * n * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(hipMemcpyAsync(dmb, max_bfu_counts, n * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
  c1k_launch_allocate_bits(dd, doff, dlen, dsz, dmb, problems, dbsf, dcount, dwl, dsfi, dfb, ctx->stream);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(bfu_count, dcount, n * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipMemcpyAsync(allocation, dwl, 52 * n * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipMemcpyAsync(scale_factor_indices, dsfi, 52 * n * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipMemcpyAsync(fallback, dfb, n, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return C1_OK;
}

int c1_pack_spec_tap_device(c1_ctx *ctx, const float *coefs, const float *eps, const uint8_t *side, const uint8_t *alloc,
                            int64_t units, int all_long, uint8_t *units_out, uint32_t *lists) {
  CTX_GUARD(ctx);
  int rc = ctx_bind(ctx);
  if (rc) return rc;
  if (units < 0 || units > kMaxChunkFrames) return fail(C1_ERR_ARG, "bad unit count");
  if (!coefs || !eps || !side || !alloc || !units_out || !lists) return fail(C1_ERR_ARG, "NULL argument");
  if (((uintptr_t)coefs | (uintptr_t)eps) & 15) return fail(C1_ERR_ARG, "coefs and eps must be 16-byte aligned device pointers");
  if (!ctx->spec_tables_ok) return fail(C1_ERR_STATE, "the installed tables fail the checks the error bound relies on");
  HIP_TRY(hipMemsetAsync(lists, 0, kListHead * sizeof(uint32_t), ctx->stream));
  if (units == 0) return C1_OK;
  C1EncodeLaunch L;
  memset(&L, 0, sizeof L);
  L.channels = 1; L.frames = units;
  L.tables = ctx->d_tables; L.opts = ctx->d_opts;
  L.coefs = const_cast<float *>(coefs); L.eps = const_cast<float *>(eps);
  L.side = const_cast<uint8_t *>(side); L.alloc = const_cast<uint8_t *>(alloc);
  L.units = units_out;
  L.redo_count = lists; L.realloc_count = lists + 1; L.reana_count = lists + 2;
  L.redo_list = lists + kListHead; L.realloc_list = lists + kListHead + units; L.reana_list = lists + kListHead + 2 * units;
  c1k_launch_pack_spec(L, all_long != 0, ctx->stream);
  HIP_TRY(hipGetLastError());
  return C1_OK;
}

// ---- streamed host path --------------------------------------------------------------------------------------
namespace {
constexpr int64_t kStreamChunkFrames = 32768;   // frames per channel per chunk of the streamed host path

int ensure_ring(c1_ctx *ctx, size_t bytes) {
  if (!ctx->s_up) {
    HIP_TRY(hipStreamCreateWithFlags(&ctx->s_up, hipStreamNonBlocking));
    HIP_TRY(hipStreamCreateWithFlags(&ctx->s_down, hipStreamNonBlocking));
    for (int p = 0; p < 2; p++) {
      HIP_TRY(hipEventCreateWithFlags(&ctx->ev_up[p], hipEventDisableTiming));
      HIP_TRY(hipEventCreateWithFlags(&ctx->ev_run[p], hipEventDisableTiming));
      HIP_TRY(hipEventCreateWithFlags(&ctx->ev_down[p], hipEventDisableTiming));
    }
  }
  if (bytes <= ctx->d_ring_bytes) return C1_OK;
  HIP_TRY(hipDeviceSynchronize());
  if (ctx->d_ring) (void)hipFree(ctx->d_ring);
  ctx->d_ring = nullptr; ctx->d_ring_bytes = 0;
  HIP_TRY(hipMalloc(&ctx->d_ring, bytes));
  ctx->d_ring_bytes = bytes;
  return C1_OK;
}

// Leaves no copy in flight into or out of the caller's host memory, whichever way the function returns.  While it
// lives, the per-chunk device calls add to the context's kernel timings instead of restarting them.
struct StreamDrain {
  c1_ctx *ctx;
  explicit StreamDrain(c1_ctx *c) : ctx(c) {
    if (ctx->profiling && ctx->timing_depth == 0) reset_timings(ctx);
    ctx->timing_depth++;
  }
  ~StreamDrain() {
    ctx->timing_depth--;
    if (ctx->s_up) (void)hipStreamSynchronize(ctx->s_up);
    (void)hipStreamSynchronize(ctx->stream);
    if (ctx->s_down) (void)hipStreamSynchronize(ctx->s_down);
  }
};

// upload of chunk i+1 | kernels of chunk i | download of chunk i-1, two staging sets.  The download of chunk i-1 is
// queued after the upload and the kernels of chunk i, so a download into pageable memory (which blocks the host
// until it is done) still leaves the other two stages of the next chunk in flight.
int encode_batch_streamed(c1_ctx *ctx, const float *const *pcm, int channels, int64_t frames, int halo_frames,
                          const c1_encode_options *opts, uint8_t *units) {
  const int64_t chunk = kStreamChunkFrames;
  const size_t in_bytes = (size_t)(chunk + 2) * 512 * sizeof(float);            // per channel, with the 2-frame halo
  const size_t out_bytes = ((size_t)chunk * channels * C1_UNIT_BYTES + 255) & ~(size_t)255;
  const size_t set_bytes = in_bytes * channels + out_bytes;
  int rc = ensure_ring(ctx, 2 * set_bytes);
  if (rc) return rc;
  StreamDrain drain(ctx);
  auto download = [&](int64_t index) -> int {
    const int p = (int)(index & 1);
    const int64_t f0 = index * chunk, n = std::min(chunk, frames - f0);
    const uint8_t *d_units = reinterpret_cast<const uint8_t *>((char *)ctx->d_ring + (size_t)p * set_bytes + in_bytes * channels);
    HIP_TRY(hipStreamWaitEvent(ctx->s_down, ctx->ev_run[p], 0));
    HIP_TRY(hipMemcpyAsync(units + (size_t)f0 * channels * C1_UNIT_BYTES, d_units, (size_t)n * channels * C1_UNIT_BYTES,
                           hipMemcpyDeviceToHost, ctx->s_down));
    HIP_TRY(hipEventRecord(ctx->ev_down[p], ctx->s_down));
    return C1_OK;
  };
  int64_t index = 0;
  for (int64_t f0 = 0; f0 < frames; f0 += chunk, ++index) {
    const int p = (int)(index & 1);
    const int64_t n = std::min(chunk, frames - f0);
    const int h = (int)std::min<int64_t>(2, f0 + halo_frames);
    char *set = (char *)ctx->d_ring + (size_t)p * set_bytes;
    if (index >= 2) {                                           // staging set p is free again
      HIP_TRY(hipStreamWaitEvent(ctx->s_up, ctx->ev_run[p], 0));
      HIP_TRY(hipStreamWaitEvent(ctx->s_up, ctx->ev_down[p], 0));
      HIP_TRY(hipStreamWaitEvent(ctx->stream, ctx->ev_down[p], 0));
    }
    const float *dptr[C1_MAX_CHANNELS] = {nullptr, nullptr};
    for (int c = 0; c < channels; c++) {
      float *d = reinterpret_cast<float *>(set + in_bytes * c);
      HIP_TRY(hipMemcpyAsync(d, pcm[c] + (f0 - h) * 512, (size_t)(n + h) * 512 * sizeof(float), hipMemcpyHostToDevice, ctx->s_up));
      dptr[c] = d + (size_t)h * 512;
    }
    HIP_TRY(hipEventRecord(ctx->ev_up[p], ctx->s_up));
    HIP_TRY(hipStreamWaitEvent(ctx->stream, ctx->ev_up[p], 0));
    uint8_t *d_units = reinterpret_cast<uint8_t *>(set + in_bytes * channels);
    if ((rc = encode_device_joined(ctx, dptr, channels, n, h, opts, d_units))) return rc;
    HIP_TRY(hipEventRecord(ctx->ev_run[p], ctx->stream));
    if (index >= 1 && (rc = download(index - 1))) return rc;
  }
  if ((rc = download(index - 1))) return rc;
  HIP_TRY(hipStreamSynchronize(ctx->s_down));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return C1_OK;
}

int decode_batch_streamed(c1_ctx *ctx, const uint8_t *units, int channels, int64_t frames, int halo_units, float *const *pcm) {
  const int64_t chunk = kStreamChunkFrames;
  const size_t in_bytes = ((size_t)(chunk + 1) * channels * C1_UNIT_BYTES + 255) & ~(size_t)255;
  const size_t out_bytes = (size_t)chunk * 512 * sizeof(float);                // per channel
  const size_t set_bytes = in_bytes + out_bytes * channels;
  int rc = ensure_ring(ctx, 2 * set_bytes);
  if (rc) return rc;
  StreamDrain drain(ctx);
  auto download = [&](int64_t index) -> int {
    const int p = (int)(index & 1);
    const int64_t f0 = index * chunk, n = std::min(chunk, frames - f0);
    char *set = (char *)ctx->d_ring + (size_t)p * set_bytes;
    HIP_TRY(hipStreamWaitEvent(ctx->s_down, ctx->ev_run[p], 0));
    for (int c = 0; c < channels; c++)
      HIP_TRY(hipMemcpyAsync(pcm[c] + f0 * 512, set + in_bytes + out_bytes * c, (size_t)n * 512 * sizeof(float), hipMemcpyDeviceToHost, ctx->s_down));
    HIP_TRY(hipEventRecord(ctx->ev_down[p], ctx->s_down));
    return C1_OK;
  };
  int64_t index = 0;
  for (int64_t f0 = 0; f0 < frames; f0 += chunk, ++index) {
    const int p = (int)(index & 1);
    const int64_t n = std::min(chunk, frames - f0);
    const int h = (int)std::min<int64_t>(1, f0 + halo_units);
    char *set = (char *)ctx->d_ring + (size_t)p * set_bytes;
    if (index >= 2) {
      HIP_TRY(hipStreamWaitEvent(ctx->s_up, ctx->ev_run[p], 0));
      HIP_TRY(hipStreamWaitEvent(ctx->s_up, ctx->ev_down[p], 0));
      HIP_TRY(hipStreamWaitEvent(ctx->stream, ctx->ev_down[p], 0));
    }
    const size_t hb = (size_t)h * channels * C1_UNIT_BYTES;
    HIP_TRY(hipMemcpyAsync(set, units + (size_t)f0 * channels * C1_UNIT_BYTES - hb, (size_t)n * channels * C1_UNIT_BYTES + hb,
                           hipMemcpyHostToDevice, ctx->s_up));
    HIP_TRY(hipEventRecord(ctx->ev_up[p], ctx->s_up));
    HIP_TRY(hipStreamWaitEvent(ctx->stream, ctx->ev_up[p], 0));
    float *dptr[C1_MAX_CHANNELS] = {nullptr, nullptr};
    for (int c = 0; c < channels; c++) dptr[c] = reinterpret_cast<float *>(set + in_bytes + out_bytes * c);
    if ((rc = c1_decode_device(ctx, (const uint8_t *)set + hb, channels, n, h, dptr))) return rc;
    HIP_TRY(hipEventRecord(ctx->ev_run[p], ctx->stream));
    if (index >= 1 && (rc = download(index - 1))) return rc;
  }
  if ((rc = download(index - 1))) return rc;
  HIP_TRY(hipStreamSynchronize(ctx->s_down));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return C1_OK;
}
}  // namespace

int c1_host_alloc(size_t bytes, void **out) {
  if (!out) return fail(C1_ERR_ARG, "out is NULL");
  *out = nullptr;
  if (bytes == 0) return C1_OK;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count == 0) { (void)hipGetLastError(); return fail(C1_ERR_NO_DEVICE, "no HIP device: page-locked memory needs the HIP runtime"); }
  HIP_TRY(hipHostMalloc(out, bytes, hipHostMallocDefault));
  return C1_OK;
}

int c1_host_free(void *p) {
  if (!p) return C1_OK;
  HIP_TRY(hipHostFree(p));
  return C1_OK;
}

int c1_encode_batch(c1_ctx *ctx, const float *const *pcm, int channels, int64_t frames, int halo_frames,
                    const c1_encode_options *opts, uint8_t *units) {
  CTX_GUARD(ctx);
  int rc = ctx_bind(ctx);
  if (rc) return rc;
  if ((rc = check_channels(channels))) return rc;
  if (frames < 0 || halo_frames < 0 || halo_frames > 2) return fail(C1_ERR_ARG, "bad frames / halo_frames");
  if (frames == 0) return C1_OK;
  if (!pcm || !units) return fail(C1_ERR_ARG, "pcm or units is NULL");
  if (frames > 2 * kStreamChunkFrames) {
    // large batches are streamed in chunks (upload | kernels | download on three streams), from page-locked memory at the
    // link's rate (12.9 M stereo frames/s), from pageable memory nearly so (11.8 M: the runtime stages those copies, but the
    // chunks keep the stages of the pipeline busy; copy - compute - copy in one piece managed 8.1 M)
    for (int c = 0; c < channels; c++) if (!pcm[c]) return fail(C1_ERR_ARG, "pcm[%d] is NULL", c);
    return encode_batch_streamed(ctx, pcm, channels, frames, halo_frames, opts, units);
  }
  const size_t ch_bytes = (size_t)(frames + halo_frames) * 512 * sizeof(float);
  const size_t unit_bytes = (size_t)frames * channels * C1_UNIT_BYTES;
  const size_t unit_off = (ch_bytes * channels + 255) & ~(size_t)255;
  if ((rc = ensure_io(ctx, unit_off + unit_bytes))) return rc;
  const float *dptr[C1_MAX_CHANNELS] = {nullptr, nullptr};
  for (int c = 0; c < channels; c++) {
    if (!pcm[c]) return fail(C1_ERR_ARG, "pcm[%d] is NULL", c);
    float *d = reinterpret_cast<float *>((char *)ctx->d_io + ch_bytes * c);
    HIP_TRY(hipMemcpyAsync(d, pcm[c] - (size_t)halo_frames * 512, ch_bytes, hipMemcpyHostToDevice, ctx->stream));
    dptr[c] = d + (size_t)halo_frames * 512;
  }
  uint8_t *d_units = (uint8_t *)ctx->d_io + unit_off;
  if ((rc = encode_device_joined(ctx, dptr, channels, frames, halo_frames, opts, d_units))) return rc;
  HIP_TRY(hipMemcpyAsync(units, d_units, unit_bytes, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return C1_OK;
}

int c1_encode_modes_batch(c1_ctx *ctx, const float *const *pcm, int channels, int64_t frames, int halo_frames,
                          const c1_encode_options *opts, const uint8_t *modes, uint8_t *units) {
  CTX_GUARD(ctx);
  int rc = ctx_bind(ctx);
  if (rc) return rc;
  if ((rc = check_channels(channels))) return rc;
  if (frames < 0 || halo_frames < 0 || halo_frames > 2) return fail(C1_ERR_ARG, "bad frames / halo_frames");
  if (frames > kMaxModesBatchFrames) return fail(C1_ERR_ARG, "at most %lld frames per call", (long long)kMaxModesBatchFrames);
  if (frames == 0) return C1_OK;
  if (!pcm || !units || !modes) return fail(C1_ERR_ARG, "pcm, modes or units is NULL");
  for (int c = 0; c < channels; c++) if (!pcm[c]) return fail(C1_ERR_ARG, "pcm[%d] is NULL", c);
  if ((rc = check_mode_bytes("c1_encode_modes_batch", modes, frames, channels))) return rc;   // before any device work
  // one copy in, the device call, one copy out
  const size_t ch_bytes = (size_t)(frames + halo_frames) * 512 * sizeof(float);
  const size_t unit_bytes = (size_t)frames * channels * C1_UNIT_BYTES, mode_bytes = (size_t)frames * channels;
  const size_t unit_off = (ch_bytes * channels + 255) & ~(size_t)255, mode_off = (unit_off + unit_bytes + 255) & ~(size_t)255;
  if ((rc = ensure_io(ctx, mode_off + mode_bytes))) return rc;
  const float *dptr[C1_MAX_CHANNELS] = {nullptr, nullptr};
  for (int c = 0; c < channels; c++) {
    float *d = reinterpret_cast<float *>((char *)ctx->d_io + ch_bytes * c);
    HIP_TRY(hipMemcpyAsync(d, pcm[c] - (size_t)halo_frames * 512, ch_bytes, hipMemcpyHostToDevice, ctx->stream));
    dptr[c] = d + (size_t)halo_frames * 512;
  }
  uint8_t *d_units = (uint8_t *)ctx->d_io + unit_off, *d_modes = (uint8_t *)ctx->d_io + mode_off;
  HIP_TRY(hipMemcpyAsync(d_modes, modes, mode_bytes, hipMemcpyHostToDevice, ctx->stream));
  if ((rc = c1_encode_modes_device(ctx, dptr, channels, frames, halo_frames, opts, d_modes, d_units))) return rc;
  HIP_TRY(hipMemcpyAsync(units, d_units, unit_bytes, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return C1_OK;
}

int c1_encode_biases_device(c1_ctx *ctx, const float *const *pcm, int channels, int64_t frames, int halo_frames,
                            const c1_encode_options *palette, int n_palette, const uint8_t *bias_index, const uint8_t *modes,
                            uint8_t *units) {
  CTX_GUARD(ctx);
  int rc = ctx_bind(ctx);
  if (rc) return rc;
  if ((rc = check_channels(channels))) return rc;
  if (frames < 0 || halo_frames < 0 || halo_frames > 2) return fail(C1_ERR_ARG, "bad frames / halo_frames");
  if (frames > kMaxChunkFrames) return fail(C1_ERR_ARG, "at most %lld frames per call", (long long)kMaxChunkFrames);
  if ((rc = check_palette("c1_encode_biases_device", palette, n_palette, modes == nullptr))) return rc;
  if (frames > 0 && (!bias_index || !units)) return fail(C1_ERR_ARG, "bias_index or units is NULL");
  if ((rc = upload_palette(ctx, "c1_encode_biases_device", palette, n_palette))) return rc;
  // what analysis and packing read of the options: entry 0's (with given modes neither threshold nor fixed modes are read)
  c1_encode_options base = palette[0];
  if (modes) {
    base.transient_threshold = 1.0;
    base.fixed_block_modes[0] = base.fixed_block_modes[1] = base.fixed_block_modes[2] = -1;
  }
  const PaletteCall pc = {n_palette, bias_index};
  return encode_device_impl(ctx, pcm, channels, frames, halo_frames, &base, units, nullptr, nullptr, nullptr, nullptr, false,
                            frames > 0 ? modes : nullptr, &pc);
}

int c1_encode_biases_batch(c1_ctx *ctx, const float *const *pcm, int channels, int64_t frames, int halo_frames,
                           const c1_encode_options *palette, int n_palette, const uint8_t *bias_index, const uint8_t *modes,
                           uint8_t *units) {
  CTX_GUARD(ctx);
  int rc = ctx_bind(ctx);
  if (rc) return rc;
  if ((rc = check_channels(channels))) return rc;
  if (frames < 0 || halo_frames < 0 || halo_frames > 2) return fail(C1_ERR_ARG, "bad frames / halo_frames");
  if (frames > kMaxModesBatchFrames) return fail(C1_ERR_ARG, "at most %lld frames per call", (long long)kMaxModesBatchFrames);
  if ((rc = check_palette("c1_encode_biases_batch", palette, n_palette, modes == nullptr))) return rc;
  if (frames == 0) return C1_OK;
  if (!pcm || !units || !bias_index) return fail(C1_ERR_ARG, "pcm, bias_index or units is NULL");
  for (int c = 0; c < channels; c++) if (!pcm[c]) return fail(C1_ERR_ARG, "pcm[%d] is NULL", c);
  if ((rc = check_index_bytes("c1_encode_biases_batch", bias_index, frames, channels, n_palette))) return rc;   // before any device work
  if (modes && (rc = check_mode_bytes("c1_encode_biases_batch", modes, frames, channels))) return rc;
  // one copy in, the device call, one copy out
  const size_t ch_bytes = (size_t)(frames + halo_frames) * 512 * sizeof(float);
  const size_t unit_bytes = (size_t)frames * channels * C1_UNIT_BYTES, byte_bytes = (size_t)frames * channels;
  const size_t unit_off = (ch_bytes * channels + 255) & ~(size_t)255, index_off = (unit_off + unit_bytes + 255) & ~(size_t)255,
               mode_off = (index_off + byte_bytes + 255) & ~(size_t)255;
  if ((rc = ensure_io(ctx, mode_off + byte_bytes))) return rc;
  const float *dptr[C1_MAX_CHANNELS] = {nullptr, nullptr};
  for (int c = 0; c < channels; c++) {
    float *d = reinterpret_cast<float *>((char *)ctx->d_io + ch_bytes * c);
    HIP_TRY(hipMemcpyAsync(d, pcm[c] - (size_t)halo_frames * 512, ch_bytes, hipMemcpyHostToDevice, ctx->stream));
    dptr[c] = d + (size_t)halo_frames * 512;
  }
  uint8_t *d_units = (uint8_t *)ctx->d_io + unit_off, *d_index = (uint8_t *)ctx->d_io + index_off, *d_modes = (uint8_t *)ctx->d_io + mode_off;
  HIP_TRY(hipMemcpyAsync(d_index, bias_index, byte_bytes, hipMemcpyHostToDevice, ctx->stream));
  if (modes) HIP_TRY(hipMemcpyAsync(d_modes, modes, byte_bytes, hipMemcpyHostToDevice, ctx->stream));
  if ((rc = c1_encode_biases_device(ctx, dptr, channels, frames, halo_frames, palette, n_palette, d_index, modes ? d_modes : nullptr, d_units))) return rc;
  HIP_TRY(hipMemcpyAsync(units, d_units, unit_bytes, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return C1_OK;
}

int c1_encode_best_bias_device(c1_ctx *ctx, const float *const *pcm, int channels, int64_t frames, int halo_frames,
                               const c1_encode_options *palette, int n_palette, const uint8_t *modes, uint8_t *units,
                               uint8_t *choice, double *distortion, double *energy) {
  CTX_GUARD(ctx);
  int rc = ctx_bind(ctx);
  if (rc) return rc;
  if ((rc = check_channels(channels))) return rc;
  if (frames < 0 || halo_frames < 0 || halo_frames > 2) return fail(C1_ERR_ARG, "bad frames / halo_frames");
  if (frames > kMaxChunkFrames) return fail(C1_ERR_ARG, "at most %lld frames per call", (long long)kMaxChunkFrames);
  if ((rc = check_palette("c1_encode_best_bias_device", palette, n_palette, modes == nullptr))) return rc;
  if (!units && !choice && !distortion && !energy) return fail(C1_ERR_ARG, "c1_encode_best_bias_device: units, choice, distortion and energy are all NULL");
  if ((rc = upload_palette(ctx, "c1_encode_best_bias_device", palette, n_palette))) return rc;
  // what analysis and packing read of the options: entry 0's (with given modes neither threshold nor fixed modes are read)
  c1_encode_options base = palette[0];
  if (modes) {
    base.transient_threshold = 1.0;
    base.fixed_block_modes[0] = base.fixed_block_modes[1] = base.fixed_block_modes[2] = -1;
  }
  const BestBiasCall bc = {n_palette, choice, distortion, energy};
  return encode_device_impl(ctx, pcm, channels, frames, halo_frames, &base, units, nullptr, nullptr, nullptr, nullptr, false,
                            frames > 0 ? modes : nullptr, nullptr, &bc);
}

int c1_encode_best_bias_batch(c1_ctx *ctx, const float *const *pcm, int channels, int64_t frames, int halo_frames,
                              const c1_encode_options *palette, int n_palette, const uint8_t *modes, uint8_t *units,
                              uint8_t *choice, double *distortion, double *energy) {
  // everything the arguments alone decide comes first and needs neither a context nor a device
  int rc = check_channels(channels);
  if (rc) return rc;
  if (frames < 0 || halo_frames < 0 || halo_frames > 2) return fail(C1_ERR_ARG, "bad frames / halo_frames");
  if (frames > kMaxModesBatchFrames) return fail(C1_ERR_ARG, "at most %lld frames per call", (long long)kMaxModesBatchFrames);
  if ((rc = check_palette("c1_encode_best_bias_batch", palette, n_palette, modes == nullptr))) return rc;
  if (!units && !choice && !distortion && !energy) return fail(C1_ERR_ARG, "c1_encode_best_bias_batch: units, choice, distortion and energy are all NULL");
  if (frames > 0) {
    if (!pcm) return fail(C1_ERR_ARG, "pcm is NULL");
    for (int c = 0; c < channels; c++) if (!pcm[c]) return fail(C1_ERR_ARG, "pcm[%d] is NULL", c);
    if (modes && (rc = check_mode_bytes("c1_encode_best_bias_batch", modes, frames, channels))) return rc;
  }
  if (!ctx) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count == 0) { (void)hipGetLastError(); return fail(C1_ERR_NO_DEVICE, "c1_encode_best_bias_batch: no HIP device available; this library has no CPU path"); }
    return fail(C1_ERR_ARG, "context is NULL");
  }
  CTX_GUARD(ctx);
  if ((rc = ctx_bind(ctx))) return rc;
  if (frames == 0) return C1_OK;
  // one copy in, the device call, one copy out per output
  const size_t n_units = (size_t)frames * channels;
  const size_t ch_bytes = (size_t)(frames + halo_frames) * 512 * sizeof(float);
  auto up256 = [](size_t x) { return (x + 255) & ~(size_t)255; };
  const size_t unit_off = up256(ch_bytes * channels), mode_off = up256(unit_off + n_units * C1_UNIT_BYTES), choice_off = up256(mode_off + n_units),
               dist_off = up256(choice_off + n_units), energy_off = up256(dist_off + n_units * n_palette * sizeof(double));
  if ((rc = ensure_io(ctx, energy_off + n_units * sizeof(double)))) return rc;
  const float *dptr[C1_MAX_CHANNELS] = {nullptr, nullptr};
  for (int c = 0; c < channels; c++) {
    float *d = reinterpret_cast<float *>((char *)ctx->d_io + ch_bytes * c);
    HIP_TRY(hipMemcpyAsync(d, pcm[c] - (size_t)halo_frames * 512, ch_bytes, hipMemcpyHostToDevice, ctx->stream));
    dptr[c] = d + (size_t)halo_frames * 512;
  }
  uint8_t *d_units = (uint8_t *)ctx->d_io + unit_off, *d_modes = (uint8_t *)ctx->d_io + mode_off, *d_choice = (uint8_t *)ctx->d_io + choice_off;
  double *d_dist = reinterpret_cast<double *>((char *)ctx->d_io + dist_off), *d_energy = reinterpret_cast<double *>((char *)ctx->d_io + energy_off);
  if (modes) HIP_TRY(hipMemcpyAsync(d_modes, modes, n_units, hipMemcpyHostToDevice, ctx->stream));
  if ((rc = c1_encode_best_bias_device(ctx, dptr, channels, frames, halo_frames, palette, n_palette, modes ? d_modes : nullptr,
                                       units ? d_units : nullptr, choice ? d_choice : nullptr, distortion ? d_dist : nullptr,
                                       energy ? d_energy : nullptr))) return rc;
  if (units) HIP_TRY(hipMemcpyAsync(units, d_units, n_units * C1_UNIT_BYTES, hipMemcpyDeviceToHost, ctx->stream));
  if (choice) HIP_TRY(hipMemcpyAsync(choice, d_choice, n_units, hipMemcpyDeviceToHost, ctx->stream));
  if (distortion) HIP_TRY(hipMemcpyAsync(distortion, d_dist, n_units * n_palette * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  if (energy) HIP_TRY(hipMemcpyAsync(energy, d_energy, n_units * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return C1_OK;
}

int c1_encode_measured_device(c1_ctx *ctx, const float *const *pcm, int channels, int64_t frames, int halo_frames,
                              const c1_encode_options *opts, const uint8_t *modes, uint8_t *units, uint8_t *taken,
                              double *distortion, double *energy) {
  CTX_GUARD(ctx);
  int rc = ctx_bind(ctx);
  if (rc) return rc;
  if ((rc = check_channels(channels))) return rc;
  if (frames < 0 || halo_frames < 0 || halo_frames > 2) return fail(C1_ERR_ARG, "bad frames / halo_frames");
  if (frames > kMaxChunkFrames) return fail(C1_ERR_ARG, "at most %lld frames per call", (long long)kMaxChunkFrames);
  if ((rc = check_measured_opts("c1_encode_measured_device", opts, modes == nullptr))) return rc;
  if (!units && !taken && !distortion && !energy) return fail(C1_ERR_ARG, "c1_encode_measured_device: units, taken, distortion and energy are all NULL");
  // with given modes neither threshold nor fixed modes are read
  c1_encode_options base = *opts;
  if (modes) {
    base.transient_threshold = 1.0;
    base.fixed_block_modes[0] = base.fixed_block_modes[1] = base.fixed_block_modes[2] = -1;
  }
  const MeasuredCall mc = {taken, distortion, energy};
  return encode_device_impl(ctx, pcm, channels, frames, halo_frames, &base, units, nullptr, nullptr, nullptr, nullptr, false,
                            frames > 0 ? modes : nullptr, nullptr, nullptr, nullptr, &mc);
}

int c1_encode_measured_batch(c1_ctx *ctx, const float *const *pcm, int channels, int64_t frames, int halo_frames,
                             const c1_encode_options *opts, const uint8_t *modes, uint8_t *units, uint8_t *taken,
                             double *distortion, double *energy) {
  // everything the arguments alone decide comes first and needs neither a context nor a device
  int rc = check_channels(channels);
  if (rc) return rc;
  if (frames < 0 || halo_frames < 0 || halo_frames > 2) return fail(C1_ERR_ARG, "bad frames / halo_frames");
  if (frames > kMaxModesBatchFrames) return fail(C1_ERR_ARG, "at most %lld frames per call", (long long)kMaxModesBatchFrames);
  if ((rc = check_measured_opts("c1_encode_measured_batch", opts, modes == nullptr))) return rc;
  if (!units && !taken && !distortion && !energy) return fail(C1_ERR_ARG, "c1_encode_measured_batch: units, taken, distortion and energy are all NULL");
  if (frames > 0) {
    if (!pcm) return fail(C1_ERR_ARG, "pcm is NULL");
    for (int c = 0; c < channels; c++) if (!pcm[c]) return fail(C1_ERR_ARG, "pcm[%d] is NULL", c);
    if (modes && (rc = check_mode_bytes("c1_encode_measured_batch", modes, frames, channels))) return rc;
  }
  if (!ctx) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count == 0) { (void)hipGetLastError(); return fail(C1_ERR_NO_DEVICE, "c1_encode_measured_batch: no HIP device available; this library has no CPU path"); }
    return fail(C1_ERR_ARG, "context is NULL");
  }
  CTX_GUARD(ctx);
  if ((rc = ctx_bind(ctx))) return rc;
  if (frames == 0) return C1_OK;
  // one copy in, the device call, one copy out per output
  const size_t n_units = (size_t)frames * channels;
  const size_t ch_bytes = (size_t)(frames + halo_frames) * 512 * sizeof(float);
  auto up256 = [](size_t x) { return (x + 255) & ~(size_t)255; };
  const size_t unit_off = up256(ch_bytes * channels), mode_off = up256(unit_off + n_units * C1_UNIT_BYTES), taken_off = up256(mode_off + n_units),
               dist_off = up256(taken_off + n_units), energy_off = up256(dist_off + n_units * 2 * sizeof(double));
  if ((rc = ensure_io(ctx, energy_off + n_units * sizeof(double)))) return rc;
  const float *dptr[C1_MAX_CHANNELS] = {nullptr, nullptr};
  for (int c = 0; c < channels; c++) {
    float *d = reinterpret_cast<float *>((char *)ctx->d_io + ch_bytes * c);
    HIP_TRY(hipMemcpyAsync(d, pcm[c] - (size_t)halo_frames * 512, ch_bytes, hipMemcpyHostToDevice, ctx->stream));
    dptr[c] = d + (size_t)halo_frames * 512;
  }
  uint8_t *d_units = (uint8_t *)ctx->d_io + unit_off, *d_modes = (uint8_t *)ctx->d_io + mode_off, *d_taken = (uint8_t *)ctx->d_io + taken_off;
  double *d_dist = reinterpret_cast<double *>((char *)ctx->d_io + dist_off), *d_energy = reinterpret_cast<double *>((char *)ctx->d_io + energy_off);
  if (modes) HIP_TRY(hipMemcpyAsync(d_modes, modes, n_units, hipMemcpyHostToDevice, ctx->stream));
  if ((rc = c1_encode_measured_device(ctx, dptr, channels, frames, halo_frames, opts, modes ? d_modes : nullptr, units ? d_units : nullptr,
                                      taken ? d_taken : nullptr, distortion ? d_dist : nullptr, energy ? d_energy : nullptr))) return rc;
  if (units) HIP_TRY(hipMemcpyAsync(units, d_units, n_units * C1_UNIT_BYTES, hipMemcpyDeviceToHost, ctx->stream));
  if (taken) HIP_TRY(hipMemcpyAsync(taken, d_taken, n_units, hipMemcpyDeviceToHost, ctx->stream));
  if (distortion) HIP_TRY(hipMemcpyAsync(distortion, d_dist, n_units * 2 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  if (energy) HIP_TRY(hipMemcpyAsync(energy, d_energy, n_units * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return C1_OK;
}

// host only: 1 to 8 distinct offsets within -8 .. 8, the first of them 0
static int check_sf_offsets(const char *what, const int8_t *sf_offsets, int n) {
  if (n < 1 || n > C1_MAX_SF_OFFSETS) return fail(C1_ERR_ARG, "%s: n_offsets = %d is outside 1..%d", what, n, C1_MAX_SF_OFFSETS);
  if (!sf_offsets) return fail(C1_ERR_ARG, "%s: sf_offsets is NULL", what);
  for (int k = 0; k < n; k++) {
    if (sf_offsets[k] < -8 || sf_offsets[k] > 8) return fail(C1_ERR_ARG, "%s: sf_offsets[%d] = %d is outside -8..8", what, k, (int)sf_offsets[k]);
    for (int j = 0; j < k; j++) if (sf_offsets[j] == sf_offsets[k]) return fail(C1_ERR_ARG, "%s: sf_offsets[%d] repeats sf_offsets[%d] = %d", what, k, j, (int)sf_offsets[k]);
  }
  if (sf_offsets[0] != 0) return fail(C1_ERR_ARG, "%s: sf_offsets[0] = %d, not 0 (the reference's own index comes first)", what, (int)sf_offsets[0]);
  return C1_OK;
}

int c1_encode_measured_sf_device(c1_ctx *ctx, const float *const *pcm, int channels, int64_t frames, int halo_frames,
                                 const c1_encode_options *opts, const uint8_t *modes, const int8_t *sf_offsets, int n_offsets,
                                 uint8_t *units, uint8_t *taken, int8_t *shifts, double *distortion, double *energy) {
  CTX_GUARD(ctx);
  int rc = ctx_bind(ctx);
  if (rc) return rc;
  if ((rc = check_channels(channels))) return rc;
  if (frames < 0 || halo_frames < 0 || halo_frames > 2) return fail(C1_ERR_ARG, "bad frames / halo_frames");
  if (frames > kMaxChunkFrames) return fail(C1_ERR_ARG, "at most %lld frames per call", (long long)kMaxChunkFrames);
  if ((rc = check_measured_opts("c1_encode_measured_sf_device", opts, modes == nullptr))) return rc;
  if ((rc = check_sf_offsets("c1_encode_measured_sf_device", sf_offsets, n_offsets))) return rc;
  if (!units && !taken && !shifts && !distortion && !energy) return fail(C1_ERR_ARG, "c1_encode_measured_sf_device: units, taken, shifts, distortion and energy are all NULL");
  // with given modes neither threshold nor fixed modes are read
  c1_encode_options base = *opts;
  if (modes) {
    base.transient_threshold = 1.0;
    base.fixed_block_modes[0] = base.fixed_block_modes[1] = base.fixed_block_modes[2] = -1;
  }
  MeasuredCall mc = {taken, distortion, energy};
  mc.sf_offsets = sf_offsets;                                   // they travel to the kernel as an argument of every launch
  mc.n_offsets = n_offsets;
  mc.shifts = shifts;
  return encode_device_impl(ctx, pcm, channels, frames, halo_frames, &base, units, nullptr, nullptr, nullptr, nullptr, false,
                            frames > 0 ? modes : nullptr, nullptr, nullptr, nullptr, &mc);
}

int c1_encode_measured_sf_batch(c1_ctx *ctx, const float *const *pcm, int channels, int64_t frames, int halo_frames,
                                const c1_encode_options *opts, const uint8_t *modes, const int8_t *sf_offsets, int n_offsets,
                                uint8_t *units, uint8_t *taken, int8_t *shifts, double *distortion, double *energy) {
  // everything the arguments alone decide comes first and needs neither a context nor a device
  int rc = check_channels(channels);
  if (rc) return rc;
  if (frames < 0 || halo_frames < 0 || halo_frames > 2) return fail(C1_ERR_ARG, "bad frames / halo_frames");
  if (frames > kMaxModesBatchFrames) return fail(C1_ERR_ARG, "at most %lld frames per call", (long long)kMaxModesBatchFrames);
  if ((rc = check_measured_opts("c1_encode_measured_sf_batch", opts, modes == nullptr))) return rc;
  if ((rc = check_sf_offsets("c1_encode_measured_sf_batch", sf_offsets, n_offsets))) return rc;
  if (!units && !taken && !shifts && !distortion && !energy) return fail(C1_ERR_ARG, "c1_encode_measured_sf_batch: units, taken, shifts, distortion and energy are all NULL");
  if (frames > 0) {
    if (!pcm) return fail(C1_ERR_ARG, "pcm is NULL");
    for (int c = 0; c < channels; c++) if (!pcm[c]) return fail(C1_ERR_ARG, "pcm[%d] is NULL", c);
    if (modes && (rc = check_mode_bytes("c1_encode_measured_sf_batch", modes, frames, channels))) return rc;
  }
  if (!ctx) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count == 0) { (void)hipGetLastError(); return fail(C1_ERR_NO_DEVICE, "c1_encode_measured_sf_batch: no HIP device available; this library has no CPU path"); }
    return fail(C1_ERR_ARG, "context is NULL");
  }
  CTX_GUARD(ctx);
  if ((rc = ctx_bind(ctx))) return rc;
  if (frames == 0) return C1_OK;
  // one copy in, the device call, one copy out per output
  const size_t n_units = (size_t)frames * channels;
  const size_t ch_bytes = (size_t)(frames + halo_frames) * 512 * sizeof(float);
  auto up256 = [](size_t x) { return (x + 255) & ~(size_t)255; };
  const size_t unit_off = up256(ch_bytes * channels), mode_off = up256(unit_off + n_units * C1_UNIT_BYTES), taken_off = up256(mode_off + n_units),
               shift_off = up256(taken_off + n_units), dist_off = up256(shift_off + n_units * 52),
               energy_off = up256(dist_off + n_units * 2 * sizeof(double));
  if ((rc = ensure_io(ctx, energy_off + n_units * sizeof(double)))) return rc;
  const float *dptr[C1_MAX_CHANNELS] = {nullptr, nullptr};
  for (int c = 0; c < channels; c++) {
    float *d = reinterpret_cast<float *>((char *)ctx->d_io + ch_bytes * c);
    HIP_TRY(hipMemcpyAsync(d, pcm[c] - (size_t)halo_frames * 512, ch_bytes, hipMemcpyHostToDevice, ctx->stream));
    dptr[c] = d + (size_t)halo_frames * 512;
  }
  uint8_t *d_units = (uint8_t *)ctx->d_io + unit_off, *d_modes = (uint8_t *)ctx->d_io + mode_off, *d_taken = (uint8_t *)ctx->d_io + taken_off;
  int8_t *d_shifts = reinterpret_cast<int8_t *>((char *)ctx->d_io + shift_off);
  double *d_dist = reinterpret_cast<double *>((char *)ctx->d_io + dist_off), *d_energy = reinterpret_cast<double *>((char *)ctx->d_io + energy_off);
  if (modes) HIP_TRY(hipMemcpyAsync(d_modes, modes, n_units, hipMemcpyHostToDevice, ctx->stream));
  if ((rc = c1_encode_measured_sf_device(ctx, dptr, channels, frames, halo_frames, opts, modes ? d_modes : nullptr, sf_offsets, n_offsets,
                                         units ? d_units : nullptr, taken ? d_taken : nullptr, shifts ? d_shifts : nullptr,
                                         distortion ? d_dist : nullptr, energy ? d_energy : nullptr))) return rc;
  if (units) HIP_TRY(hipMemcpyAsync(units, d_units, n_units * C1_UNIT_BYTES, hipMemcpyDeviceToHost, ctx->stream));
  if (taken) HIP_TRY(hipMemcpyAsync(taken, d_taken, n_units, hipMemcpyDeviceToHost, ctx->stream));
  if (shifts) HIP_TRY(hipMemcpyAsync(shifts, d_shifts, n_units * 52, hipMemcpyDeviceToHost, ctx->stream));
  if (distortion) HIP_TRY(hipMemcpyAsync(distortion, d_dist, n_units * 2 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  if (energy) HIP_TRY(hipMemcpyAsync(energy, d_energy, n_units * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return C1_OK;
}

// host only: every floor finite and within [1e-60, 1e60], every spread entry finite and within [0, 1e60]
static int check_masking(const char *what, const double *mask_floor, const double *mask_spread) {
  if (!mask_floor) return fail(C1_ERR_ARG, "%s: mask_floor is NULL", what);
  for (int b = 0; b < 52; b++)
    if (!(mask_floor[b] >= 1e-60 && mask_floor[b] <= 1e60)) return fail(C1_ERR_ARG, "%s: mask_floor[%d] = %g is outside [1e-60, 1e60]", what, b, mask_floor[b]);
  for (int i = 0; mask_spread && i < 52 * 52; i++)
    if (!(mask_spread[i] >= 0.0 && mask_spread[i] <= 1e60)) return fail(C1_ERR_ARG, "%s: mask_spread[%d] = %g (masker %d onto BFU %d) is outside [0, 1e60]", what, i, mask_spread[i], i % 52, i / 52);
  return C1_OK;
}

constexpr size_t kMaskDoubles = 52 + 52 * 52;                  // 22 048 bytes

// the tables of one call into c1_ctx::d_mask, ordered on the context's stream like the call's kernels: behind the kernels of every
// earlier call, in front of this one's.  The staging copy is rewritten only once the upload before has left it
static int upload_masking(c1_ctx *ctx, const double *mask_floor, const double *mask_spread) {
  if (!ctx->d_mask) {
    HIP_TRY(hipMalloc(&ctx->d_mask, kMaskDoubles * sizeof(double)));
    HIP_TRY(hipHostMalloc((void **)&ctx->h_mask, kMaskDoubles * sizeof(double), hipHostMallocDefault));
    HIP_TRY(hipEventCreateWithFlags(&ctx->ev_mask, hipEventDisableTiming));
  } else {
    HIP_TRY(hipEventSynchronize(ctx->ev_mask));
  }
  for (int b = 0; b < 52; b++) ctx->h_mask[b] = mask_floor[b];
  for (int b = 0; b < 52; b++)
    for (int c = 0; c < 52; c++) ctx->h_mask[52 + 52 * c + b] = mask_spread ? mask_spread[52 * b + c] : 0.0;
  HIP_TRY(hipMemcpyAsync(ctx->d_mask, ctx->h_mask, kMaskDoubles * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(hipEventRecord(ctx->ev_mask, ctx->stream));
  return C1_OK;
}

int c1_encode_measured_masked_device(c1_ctx *ctx, const float *const *pcm, int channels, int64_t frames, int halo_frames,
                                     const c1_encode_options *opts, const uint8_t *modes, const int8_t *sf_offsets, int n_offsets,
                                     const double *mask_floor, const double *mask_spread, uint8_t *units, uint8_t *taken,
                                     int8_t *shifts, double *distortion, double *energy, double *weights) {
  CTX_GUARD(ctx);
  int rc = ctx_bind(ctx);
  if (rc) return rc;
  if ((rc = check_channels(channels))) return rc;
  if (frames < 0 || halo_frames < 0 || halo_frames > 2) return fail(C1_ERR_ARG, "bad frames / halo_frames");
  if (frames > kMaxChunkFrames) return fail(C1_ERR_ARG, "at most %lld frames per call", (long long)kMaxChunkFrames);
  if ((rc = check_measured_opts("c1_encode_measured_masked_device", opts, modes == nullptr))) return rc;
  if ((rc = check_sf_offsets("c1_encode_measured_masked_device", sf_offsets, n_offsets))) return rc;
  if ((rc = check_masking("c1_encode_measured_masked_device", mask_floor, mask_spread))) return rc;
  if (!units && !taken && !shifts && !distortion && !energy && !weights) return fail(C1_ERR_ARG, "c1_encode_measured_masked_device: units, taken, shifts, distortion, energy and weights are all NULL");
  // with given modes neither threshold nor fixed modes are read
  c1_encode_options base = *opts;
  if (modes) {
    base.transient_threshold = 1.0;
    base.fixed_block_modes[0] = base.fixed_block_modes[1] = base.fixed_block_modes[2] = -1;
  }
  if (frames > 0) {
    // the tail of an earlier speculative encode may still run beside the context's stream: it reads none of this
    if ((rc = upload_masking(ctx, mask_floor, mask_spread))) return rc;
  }
  MeasuredCall mc = {taken, distortion, energy};
  mc.sf_offsets = sf_offsets;
  mc.n_offsets = n_offsets;
  mc.shifts = shifts;
  mc.mask = ctx->d_mask;
  mc.has_spread = mask_spread != nullptr;
  mc.weights = weights;
  return encode_device_impl(ctx, pcm, channels, frames, halo_frames, &base, units, nullptr, nullptr, nullptr, nullptr, false,
                            frames > 0 ? modes : nullptr, nullptr, nullptr, nullptr, frames > 0 ? &mc : nullptr);
}

int c1_encode_measured_masked_batch(c1_ctx *ctx, const float *const *pcm, int channels, int64_t frames, int halo_frames,
                                    const c1_encode_options *opts, const uint8_t *modes, const int8_t *sf_offsets, int n_offsets,
                                    const double *mask_floor, const double *mask_spread, uint8_t *units, uint8_t *taken,
                                    int8_t *shifts, double *distortion, double *energy, double *weights) {
  // everything the arguments alone decide comes first and needs neither a context nor a device
  const char *const what = "c1_encode_measured_masked_batch";
  int rc = check_channels(channels);
  if (rc) return rc;
  if (frames < 0 || halo_frames < 0 || halo_frames > 2) return fail(C1_ERR_ARG, "bad frames / halo_frames");
  if (frames > kMaxModesBatchFrames) return fail(C1_ERR_ARG, "at most %lld frames per call", (long long)kMaxModesBatchFrames);
  if ((rc = check_measured_opts(what, opts, modes == nullptr))) return rc;
  if ((rc = check_sf_offsets(what, sf_offsets, n_offsets))) return rc;
  if ((rc = check_masking(what, mask_floor, mask_spread))) return rc;
  if (!units && !taken && !shifts && !distortion && !energy && !weights) return fail(C1_ERR_ARG, "%s: units, taken, shifts, distortion, energy and weights are all NULL", what);
  if (frames > 0) {
    if (!pcm) return fail(C1_ERR_ARG, "pcm is NULL");
    for (int c = 0; c < channels; c++) if (!pcm[c]) return fail(C1_ERR_ARG, "pcm[%d] is NULL", c);
    if (modes && (rc = check_mode_bytes(what, modes, frames, channels))) return rc;
  }
  if (!ctx) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count == 0) { (void)hipGetLastError(); return fail(C1_ERR_NO_DEVICE, "%s: no HIP device available; this library has no CPU path", what); }
    return fail(C1_ERR_ARG, "context is NULL");
  }
  CTX_GUARD(ctx);
  if ((rc = ctx_bind(ctx))) return rc;
  if (frames == 0) return C1_OK;
  // one copy in, the device call, one copy out per output
  const size_t n_units = (size_t)frames * channels;
  const size_t ch_bytes = (size_t)(frames + halo_frames) * 512 * sizeof(float);
  auto up256 = [](size_t x) { return (x + 255) & ~(size_t)255; };
  const size_t unit_off = up256(ch_bytes * channels), mode_off = up256(unit_off + n_units * C1_UNIT_BYTES), taken_off = up256(mode_off + n_units),
               shift_off = up256(taken_off + n_units), dist_off = up256(shift_off + n_units * 52),
               energy_off = up256(dist_off + n_units * 2 * sizeof(double)), weight_off = up256(energy_off + n_units * sizeof(double));
  if ((rc = ensure_io(ctx, weight_off + n_units * 52 * sizeof(double)))) return rc;
  const float *dptr[C1_MAX_CHANNELS] = {nullptr, nullptr};
  for (int c = 0; c < channels; c++) {
    float *d = reinterpret_cast<float *>((char *)ctx->d_io + ch_bytes * c);
    HIP_TRY(hipMemcpyAsync(d, pcm[c] - (size_t)halo_frames * 512, ch_bytes, hipMemcpyHostToDevice, ctx->stream));
    dptr[c] = d + (size_t)halo_frames * 512;
  }
  uint8_t *d_units = (uint8_t *)ctx->d_io + unit_off, *d_modes = (uint8_t *)ctx->d_io + mode_off, *d_taken = (uint8_t *)ctx->d_io + taken_off;
  int8_t *d_shifts = reinterpret_cast<int8_t *>((char *)ctx->d_io + shift_off);
  double *d_dist = reinterpret_cast<double *>((char *)ctx->d_io + dist_off), *d_energy = reinterpret_cast<double *>((char *)ctx->d_io + energy_off),
         *d_weights = reinterpret_cast<double *>((char *)ctx->d_io + weight_off);
  if (modes) HIP_TRY(hipMemcpyAsync(d_modes, modes, n_units, hipMemcpyHostToDevice, ctx->stream));
  if ((rc = c1_encode_measured_masked_device(ctx, dptr, channels, frames, halo_frames, opts, modes ? d_modes : nullptr, sf_offsets, n_offsets,
                                             mask_floor, mask_spread, units ? d_units : nullptr, taken ? d_taken : nullptr,
                                             shifts ? d_shifts : nullptr, distortion ? d_dist : nullptr, energy ? d_energy : nullptr,
                                             weights ? d_weights : nullptr))) return rc;
  if (units) HIP_TRY(hipMemcpyAsync(units, d_units, n_units * C1_UNIT_BYTES, hipMemcpyDeviceToHost, ctx->stream));
  if (taken) HIP_TRY(hipMemcpyAsync(taken, d_taken, n_units, hipMemcpyDeviceToHost, ctx->stream));
  if (shifts) HIP_TRY(hipMemcpyAsync(shifts, d_shifts, n_units * 52, hipMemcpyDeviceToHost, ctx->stream));
  if (distortion) HIP_TRY(hipMemcpyAsync(distortion, d_dist, n_units * 2 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  if (energy) HIP_TRY(hipMemcpyAsync(energy, d_energy, n_units * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  if (weights) HIP_TRY(hipMemcpyAsync(weights, d_weights, n_units * 52 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return C1_OK;
}

// ---- the coding error of given sound units (c1_measure_units_*) --------------------------------------------------------------
// what the arguments of both calls decide alone: the tables (host memory in both), which outputs go with which tables
static int check_measure_args(const char *what, const double *mask_floor, const double *mask_spread, const double *noise,
                              const double *signal, const double *totals, const double *weights) {
  if (!noise && !signal && !totals && !weights) return fail(C1_ERR_ARG, "%s: noise, signal, totals and weights are all NULL", what);
  if (mask_spread && !mask_floor) return fail(C1_ERR_ARG, "%s: mask_spread needs mask_floor", what);
  if (weights && !mask_floor) return fail(C1_ERR_ARG, "%s: weights needs mask_floor", what);
  if (mask_floor) return check_masking(what, mask_floor, mask_spread);
  return C1_OK;
}

// host only: the block modes deserializeFrame reports for every unit (2 - field, 2 - field, 3 - field of the first six bits)
// must form a mode byte of the domain of c1_encode_modes_*.  The first that does not: C1_ERR_ARG naming frame, channel and field
static int check_unit_modes(const char *what, const uint8_t *units, int64_t frames, int channels) {
  static const char *const kField[3] = {"low", "mid", "high"};
  for (int64_t i = 0; i < frames * channels; i++) {
    const int first = units[i * C1_UNIT_BYTES];
    const int m[3] = {2 - ((first >> 6) & 3), 2 - ((first >> 4) & 3), 3 - ((first >> 2) & 3)};
    for (int k = 0; k < 3; k++) {
      const int other = k == 2 ? 3 : 2;
      if (m[k] == 0 || m[k] == other) continue;
      char where[64];
      if (channels == 2) snprintf(where, sizeof where, "frame %lld, channel %d", (long long)(i / 2), (int)(i & 1));
      else snprintf(where, sizeof where, "frame %lld", (long long)i);
      return fail(C1_ERR_ARG, "%s: %s: %s block mode of the unit is %d, not 0 or %d", what, where, kField[k], m[k], other);
    }
  }
  return C1_OK;
}

int c1_measure_units_device(c1_ctx *ctx, const float *const *pcm, int channels, int64_t frames, int halo_frames, const uint8_t *units,
                            const double *mask_floor, const double *mask_spread, double *noise, double *signal, double *totals,
                            double *weights) {
  const char *const what = "c1_measure_units_device";
  CTX_GUARD(ctx);
  int rc = ctx_bind(ctx);
  if (rc) return rc;
  if ((rc = check_channels(channels))) return rc;
  if (frames < 0 || halo_frames < 0 || halo_frames > 2) return fail(C1_ERR_ARG, "bad frames / halo_frames");
  if (frames > kMaxChunkFrames) return fail(C1_ERR_ARG, "at most %lld frames per call", (long long)kMaxChunkFrames);
  if ((rc = check_measure_args(what, mask_floor, mask_spread, noise, signal, totals, weights))) return rc;
  if (!pcm) return fail(C1_ERR_ARG, "pcm is NULL");
  for (int c = 0; c < channels; c++) {
    if (!pcm[c] && frames > 0) return fail(C1_ERR_ARG, "pcm[%d] is NULL", c);
    if ((uintptr_t)pcm[c] & 15) return fail(C1_ERR_ARG, "pcm[%d] must be 16-byte aligned on the device", c);
  }
  if (!units && frames > 0) return fail(C1_ERR_ARG, "%s: units is NULL", what);
  if ((uintptr_t)units & 3) return fail(C1_ERR_ARG, "%s: units must be 4-byte aligned on the device", what);
  if (ctx->profiling && ctx->timing_depth == 0) reset_timings(ctx);
  if (frames == 0) return C1_OK;
  // the tail of an earlier speculative encode was joined above: this call works on the context's stream alone
  if (mask_floor && (rc = upload_masking(ctx, mask_floor, mask_spread))) return rc;
  const int64_t chunk = chunk_for_call(ctx, frames, channels, true);
  if ((rc = ensure_workspace(ctx, std::min(frames, chunk) * channels))) return rc;
  if ((rc = ensure_detect_workspace(ctx, std::min(frames, chunk) * channels))) return rc;
  // Per chunk, on workspace half 0: the units' mode bytes into the allocation plane (no allocation runs here), the front end of
  // c1_encode_modes_device under them as far as the coefficients, then the meter.  A frame's coefficients do not depend on the
  // modes of the frames before it, so a chunk needs the PCM history alone
  for (int64_t f0 = 0, n = 0; f0 < frames; f0 += n) {
    n = std::min(chunk, frames - f0);
    C1EncodeLaunch L;
    memset(&L, 0, sizeof L);
    for (int c = 0; c < channels; c++) L.pcm[c] = pcm[c] + f0 * 512;
    L.channels = channels;
    L.frames = n;
    L.halo_frames = (int)std::min<int64_t>(2, f0 + halo_frames);
    L.tables = ctx->d_tables;
    L.opts = ctx->d_opts;
    L.coefs = ctx->d_coefs[0];
    L.side = ctx->d_side[0];
    const uint8_t *chunk_units = units + f0 * channels * C1_UNIT_BYTES;
    uint8_t *mode_bytes = ctx->d_alloc[0];
    const int64_t at = f0 * channels;
    {
      ScopedTiming t(ctx, K_ANALYSIS);
      c1k_launch_unit_mode_bytes(chunk_units, n * channels, mode_bytes, ctx->stream);
      c1k_launch_modes_front(L, mode_bytes, ctx->d_bands[0], ctx->d_modes[0], ctx->d_lists[0], ctx->stream);
      c1k_launch_mdct_bands(L, ctx->d_bands[0], ctx->d_modes[0], ctx->d_lists[0], ctx->stream);
    }
    ScopedTiming t(ctx, K_METER);
    c1k_launch_measure_units(ctx->d_tables, L.coefs, chunk_units, n * channels, mask_floor ? ctx->d_mask : nullptr, mask_spread != nullptr,
                             noise ? noise + at * 52 : nullptr, signal ? signal + at * 52 : nullptr, totals ? totals + at * 2 : nullptr,
                             weights ? weights + at * 52 : nullptr, ctx->stream);
  }
  HIP_TRY(hipGetLastError());
  return C1_OK;
}

int c1_measure_units_batch(c1_ctx *ctx, const float *const *pcm, int channels, int64_t frames, int halo_frames, const uint8_t *units,
                           const double *mask_floor, const double *mask_spread, double *noise, double *signal, double *totals,
                           double *weights) {
  // everything the arguments alone decide comes first and needs neither a context nor a device
  const char *const what = "c1_measure_units_batch";
  int rc = check_channels(channels);
  if (rc) return rc;
  if (frames < 0 || halo_frames < 0 || halo_frames > 2) return fail(C1_ERR_ARG, "bad frames / halo_frames");
  if (frames > kMaxModesBatchFrames) return fail(C1_ERR_ARG, "at most %lld frames per call", (long long)kMaxModesBatchFrames);
  if ((rc = check_measure_args(what, mask_floor, mask_spread, noise, signal, totals, weights))) return rc;
  if (frames > 0) {
    if (!pcm) return fail(C1_ERR_ARG, "pcm is NULL");
    for (int c = 0; c < channels; c++) if (!pcm[c]) return fail(C1_ERR_ARG, "pcm[%d] is NULL", c);
    if (!units) return fail(C1_ERR_ARG, "%s: units is NULL", what);
    if ((rc = check_unit_modes(what, units, frames, channels))) return rc;
  }
  if (!ctx) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count == 0) { (void)hipGetLastError(); return fail(C1_ERR_NO_DEVICE, "%s: no HIP device available; this library has no CPU path", what); }
    return fail(C1_ERR_ARG, "context is NULL");
  }
  CTX_GUARD(ctx);
  if ((rc = ctx_bind(ctx))) return rc;
  if (frames == 0) return C1_OK;
  // one copy in, the device call, one copy out per output
  const size_t n_units = (size_t)frames * channels;
  const size_t ch_bytes = (size_t)(frames + halo_frames) * 512 * sizeof(float);
  auto up256 = [](size_t x) { return (x + 255) & ~(size_t)255; };
  const size_t unit_off = up256(ch_bytes * channels), noise_off = up256(unit_off + n_units * C1_UNIT_BYTES),
               signal_off = up256(noise_off + n_units * 52 * sizeof(double)), totals_off = up256(signal_off + n_units * 52 * sizeof(double)),
               weight_off = up256(totals_off + n_units * 2 * sizeof(double));
  if ((rc = ensure_io(ctx, weight_off + n_units * 52 * sizeof(double)))) return rc;
  const float *dptr[C1_MAX_CHANNELS] = {nullptr, nullptr};
  for (int c = 0; c < channels; c++) {
    float *d = reinterpret_cast<float *>((char *)ctx->d_io + ch_bytes * c);
    HIP_TRY(hipMemcpyAsync(d, pcm[c] - (size_t)halo_frames * 512, ch_bytes, hipMemcpyHostToDevice, ctx->stream));
    dptr[c] = d + (size_t)halo_frames * 512;
  }
  uint8_t *d_units = (uint8_t *)ctx->d_io + unit_off;
  double *d_noise = reinterpret_cast<double *>((char *)ctx->d_io + noise_off), *d_signal = reinterpret_cast<double *>((char *)ctx->d_io + signal_off),
         *d_totals = reinterpret_cast<double *>((char *)ctx->d_io + totals_off), *d_weights = reinterpret_cast<double *>((char *)ctx->d_io + weight_off);
  HIP_TRY(hipMemcpyAsync(d_units, units, n_units * C1_UNIT_BYTES, hipMemcpyHostToDevice, ctx->stream));
  if ((rc = c1_measure_units_device(ctx, dptr, channels, frames, halo_frames, d_units, mask_floor, mask_spread, noise ? d_noise : nullptr,
                                    signal ? d_signal : nullptr, totals ? d_totals : nullptr, weights ? d_weights : nullptr))) return rc;
  if (noise) HIP_TRY(hipMemcpyAsync(noise, d_noise, n_units * 52 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  if (signal) HIP_TRY(hipMemcpyAsync(signal, d_signal, n_units * 52 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  if (totals) HIP_TRY(hipMemcpyAsync(totals, d_totals, n_units * 2 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  if (weights) HIP_TRY(hipMemcpyAsync(weights, d_weights, n_units * 52 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return C1_OK;
}

// ---- the same under the all-long threshold (c1_measure_units_shared_*) -------------------------------------------------------
// what the arguments of both calls decide alone: c1_measure_units_*' rules, and the floor is required
static int check_measure_shared_args(const char *what, const double *mask_floor, const double *mask_spread, const double *noise,
                                     const double *signal, const double *totals, const double *weights) {
  if (!noise && !signal && !totals && !weights) return fail(C1_ERR_ARG, "%s: noise, signal, totals and weights are all NULL", what);
  if (mask_spread && !mask_floor) return fail(C1_ERR_ARG, "%s: mask_spread needs mask_floor", what);
  if (!mask_floor) return fail(C1_ERR_ARG, "%s: mask_floor is NULL: the all-long threshold needs the tables", what);
  return check_masking(what, mask_floor, mask_spread);
}

int c1_measure_units_shared_device(c1_ctx *ctx, const float *const *pcm, int channels, int64_t frames, int halo_frames,
                                   const uint8_t *units, const double *mask_floor, const double *mask_spread, double *noise,
                                   double *signal, double *totals, double *weights) {
  // everything the arguments alone decide comes first and needs neither a context nor a device
  const char *const what = "c1_measure_units_shared_device";
  int rc = check_channels(channels);
  if (rc) return rc;
  if (frames < 0 || halo_frames < 0 || halo_frames > 2) return fail(C1_ERR_ARG, "bad frames / halo_frames");
  if (frames > kMaxChunkFrames) return fail(C1_ERR_ARG, "at most %lld frames per call", (long long)kMaxChunkFrames);
  if ((rc = check_measure_shared_args(what, mask_floor, mask_spread, noise, signal, totals, weights))) return rc;
  if (!pcm) return fail(C1_ERR_ARG, "pcm is NULL");
  for (int c = 0; c < channels; c++) {
    if (!pcm[c] && frames > 0) return fail(C1_ERR_ARG, "pcm[%d] is NULL", c);
    if ((uintptr_t)pcm[c] & 15) return fail(C1_ERR_ARG, "pcm[%d] must be 16-byte aligned on the device", c);
  }
  if (!units && frames > 0) return fail(C1_ERR_ARG, "%s: units is NULL", what);
  if ((uintptr_t)units & 3) return fail(C1_ERR_ARG, "%s: units must be 4-byte aligned on the device", what);
  CTX_GUARD(ctx);
  if ((rc = ctx_bind(ctx))) return rc;
  if (ctx->profiling && ctx->timing_depth == 0) reset_timings(ctx);
  if (frames == 0) return C1_OK;
  // the tail of an earlier speculative encode was joined above: this call works on the context's stream alone
  if ((rc = upload_masking(ctx, mask_floor, mask_spread))) return rc;
  const int64_t chunk = chunk_for_call(ctx, frames, channels, true, 0, true);
  if ((rc = ensure_workspace(ctx, std::min(frames, chunk) * channels))) return rc;
  if ((rc = ensure_detect_workspace(ctx, std::min(frames, chunk) * channels))) return rc;
  if ((rc = ensure_best_modes_planes(ctx, std::min(frames, chunk) * channels))) return rc;
  // Per chunk, on workspace half 0: c1_measure_units_device's front end into the chunk's plane under the units' modes, then, from
  // the same band samples, the all-long analysis into the mode search's second plane (encode_device_impl's idiom), then the meter.
  // A frame's coefficients do not depend on the modes of the frames before it, so a chunk needs the PCM history alone
  for (int64_t f0 = 0, n = 0; f0 < frames; f0 += n) {
    n = std::min(chunk, frames - f0);
    C1EncodeLaunch L;
    memset(&L, 0, sizeof L);
    for (int c = 0; c < channels; c++) L.pcm[c] = pcm[c] + f0 * 512;
    L.channels = channels;
    L.frames = n;
    L.halo_frames = (int)std::min<int64_t>(2, f0 + halo_frames);
    L.tables = ctx->d_tables;
    L.opts = ctx->d_opts;
    L.coefs = ctx->d_coefs[0];
    L.side = ctx->d_side[0];
    C1EncodeLaunch L0 = L;                                     // the all-long analysis: its side records are not read
    L0.coefs = ctx->d_bm_coefs;
    L0.side = ctx->d_bm_side;
    const uint8_t *chunk_units = units + f0 * channels * C1_UNIT_BYTES;
    uint8_t *mode_bytes = ctx->d_alloc[0];
    const int64_t at = f0 * channels;
    {
      ScopedTiming t(ctx, K_ANALYSIS);
      c1k_launch_unit_mode_bytes(chunk_units, n * channels, mode_bytes, ctx->stream);
      c1k_launch_modes_front(L, mode_bytes, ctx->d_bands[0], ctx->d_modes[0], ctx->d_lists[0], ctx->stream);
      c1k_launch_mdct_bands(L, ctx->d_bands[0], ctx->d_modes[0], ctx->d_lists[0], ctx->stream);
      c1k_launch_const_mode_lists(0, n * channels, ctx->d_modes[0], ctx->d_lists[0], ctx->stream);
      c1k_launch_mdct_bands(L0, ctx->d_bands[0], ctx->d_modes[0], ctx->d_lists[0], ctx->stream);
    }
    ScopedTiming t(ctx, K_METER);
    c1k_launch_measure_units_shared(ctx->d_tables, L.coefs, L0.coefs, chunk_units, n * channels, ctx->d_mask, mask_spread != nullptr,
                                    noise ? noise + at * 52 : nullptr, signal ? signal + at * 52 : nullptr,
                                    totals ? totals + at * 2 : nullptr, weights ? weights + at * 52 : nullptr, ctx->stream);
  }
  HIP_TRY(hipGetLastError());
  return C1_OK;
}

int c1_measure_units_shared_batch(c1_ctx *ctx, const float *const *pcm, int channels, int64_t frames, int halo_frames,
                                  const uint8_t *units, const double *mask_floor, const double *mask_spread, double *noise,
                                  double *signal, double *totals, double *weights) {
  // everything the arguments alone decide comes first and needs neither a context nor a device
  const char *const what = "c1_measure_units_shared_batch";
  int rc = check_channels(channels);
  if (rc) return rc;
  if (frames < 0 || halo_frames < 0 || halo_frames > 2) return fail(C1_ERR_ARG, "bad frames / halo_frames");
  if (frames > kMaxModesBatchFrames) return fail(C1_ERR_ARG, "at most %lld frames per call", (long long)kMaxModesBatchFrames);
  if ((rc = check_measure_shared_args(what, mask_floor, mask_spread, noise, signal, totals, weights))) return rc;
  if (frames > 0) {
    if (!pcm) return fail(C1_ERR_ARG, "pcm is NULL");
    for (int c = 0; c < channels; c++) if (!pcm[c]) return fail(C1_ERR_ARG, "pcm[%d] is NULL", c);
    if (!units) return fail(C1_ERR_ARG, "%s: units is NULL", what);
    if ((rc = check_unit_modes(what, units, frames, channels))) return rc;
  }
  if (!ctx) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count == 0) { (void)hipGetLastError(); return fail(C1_ERR_NO_DEVICE, "%s: no HIP device available; this library has no CPU path", what); }
    return fail(C1_ERR_ARG, "context is NULL");
  }
  CTX_GUARD(ctx);
  if ((rc = ctx_bind(ctx))) return rc;
  if (frames == 0) return C1_OK;
  // one copy in, the device call, one copy out per output
  const size_t n_units = (size_t)frames * channels;
  const size_t ch_bytes = (size_t)(frames + halo_frames) * 512 * sizeof(float);
  auto up256 = [](size_t x) { return (x + 255) & ~(size_t)255; };
  const size_t unit_off = up256(ch_bytes * channels), noise_off = up256(unit_off + n_units * C1_UNIT_BYTES),
               signal_off = up256(noise_off + n_units * 52 * sizeof(double)), totals_off = up256(signal_off + n_units * 52 * sizeof(double)),
               weight_off = up256(totals_off + n_units * 2 * sizeof(double));
  if ((rc = ensure_io(ctx, weight_off + n_units * 52 * sizeof(double)))) return rc;
  const float *dptr[C1_MAX_CHANNELS] = {nullptr, nullptr};
  for (int c = 0; c < channels; c++) {
    float *d = reinterpret_cast<float *>((char *)ctx->d_io + ch_bytes * c);
    HIP_TRY(hipMemcpyAsync(d, pcm[c] - (size_t)halo_frames * 512, ch_bytes, hipMemcpyHostToDevice, ctx->stream));
    dptr[c] = d + (size_t)halo_frames * 512;
  }
  uint8_t *d_units = (uint8_t *)ctx->d_io + unit_off;
  double *d_noise = reinterpret_cast<double *>((char *)ctx->d_io + noise_off), *d_signal = reinterpret_cast<double *>((char *)ctx->d_io + signal_off),
         *d_totals = reinterpret_cast<double *>((char *)ctx->d_io + totals_off), *d_weights = reinterpret_cast<double *>((char *)ctx->d_io + weight_off);
  HIP_TRY(hipMemcpyAsync(d_units, units, n_units * C1_UNIT_BYTES, hipMemcpyHostToDevice, ctx->stream));
  if ((rc = c1_measure_units_shared_device(ctx, dptr, channels, frames, halo_frames, d_units, mask_floor, mask_spread,
                                           noise ? d_noise : nullptr, signal ? d_signal : nullptr, totals ? d_totals : nullptr,
                                           weights ? d_weights : nullptr))) return rc;
  if (noise) HIP_TRY(hipMemcpyAsync(noise, d_noise, n_units * 52 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  if (signal) HIP_TRY(hipMemcpyAsync(signal, d_signal, n_units * 52 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  if (totals) HIP_TRY(hipMemcpyAsync(totals, d_totals, n_units * 2 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  if (weights) HIP_TRY(hipMemcpyAsync(weights, d_weights, n_units * 52 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return C1_OK;
}

// ---- the decoded PCM error of given sound units (c1_measure_pcm_*) ----------------------------------------------------------
// what the arguments of both calls decide alone, before a context is looked at
static int check_measure_pcm_args(const char *what, const float *const *pcm, int channels, int64_t frames, int halo_frames,
                                  const uint8_t *units, int halo_units, const double *noise, const double *signal, const double *totals) {
  int rc = check_channels(channels);
  if (rc) return rc;
  if (frames < 0 || frames > kMaxModesBatchFrames) return fail(C1_ERR_ARG, "%s: frames must be 0 .. 2^22, got %lld", what, (long long)frames);
  if (halo_frames < 0 || halo_frames > 2) return fail(C1_ERR_ARG, "%s: halo_frames must be 0 .. 2, got %d", what, halo_frames);
  if (halo_units < 0 || halo_units > 1) return fail(C1_ERR_ARG, "%s: halo_units must be 0 or 1, got %d", what, halo_units);
  if (!noise && !signal && !totals) return fail(C1_ERR_ARG, "%s: noise, signal and totals are all NULL", what);
  if (frames > 0) {
    if (!pcm) return fail(C1_ERR_ARG, "%s: pcm is NULL", what);
    for (int c = 0; c < channels; c++) if (!pcm[c]) return fail(C1_ERR_ARG, "%s: pcm[%d] is NULL", what, c);
    if (!units) return fail(C1_ERR_ARG, "%s: units is NULL", what);
  }
  return C1_OK;
}

int c1_measure_pcm_device(c1_ctx *ctx, const float *const *pcm, int channels, int64_t frames, int halo_frames, const uint8_t *units,
                          int halo_units, double *noise, double *signal, double *totals) {
  const char *const what = "c1_measure_pcm_device";
  int rc = check_measure_pcm_args(what, pcm, channels, frames, halo_frames, units, halo_units, noise, signal, totals);
  if (rc) return rc;
  for (int c = 0; c < channels && frames > 0; c++)
    if ((uintptr_t)pcm[c] & 15) return fail(C1_ERR_ARG, "%s: pcm[%d] must be 16-byte aligned on the device", what, c);
  if ((uintptr_t)units & 3) return fail(C1_ERR_ARG, "%s: units must be 4-byte aligned on the device", what);
  CTX_GUARD(ctx);
  if ((rc = ctx_bind(ctx))) return rc;
  if (ctx->profiling && ctx->timing_depth == 0) reset_timings(ctx);
  if (frames == 0) return C1_OK;
  C1MeasurePcmLaunch L;
  memset(&L, 0, sizeof L);
  L.units = units;
  L.channels = channels;
  L.frames = frames;
  L.halo_units = halo_units;
  L.halo_frames = halo_frames;
  L.tables = ctx->d_tables;
  for (int c = 0; c < channels; c++) L.pcm[c] = pcm[c];
  L.noise = noise;
  L.signal = signal;
  L.totals = totals;
  { ScopedTiming t(ctx, K_METER_PCM); c1k_launch_measure_pcm(L, ctx->stream); }
  HIP_TRY(hipGetLastError());
  return C1_OK;
}

int c1_measure_pcm_batch(c1_ctx *ctx, const float *const *pcm, int channels, int64_t frames, int halo_frames, const uint8_t *units,
                         int halo_units, double *noise, double *signal, double *totals) {
  // everything the arguments alone decide comes first and needs neither a context nor a device
  const char *const what = "c1_measure_pcm_batch";
  int rc = check_measure_pcm_args(what, pcm, channels, frames, halo_frames, units, halo_units, noise, signal, totals);
  if (rc) return rc;
  if (!ctx) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count == 0) { (void)hipGetLastError(); return fail(C1_ERR_NO_DEVICE, "%s: no HIP device available; this library has no CPU path", what); }
    return fail(C1_ERR_ARG, "context is NULL");
  }
  CTX_GUARD(ctx);
  if ((rc = ctx_bind(ctx))) return rc;
  if (frames == 0) return C1_OK;
  // Chunks of the context's chunk length (C1_CHUNK_FRAMES), each with its halos from the batch itself: one frame of PCM covers
  // the 266 samples of history, one unit rebuilds the decoder's state.  Per chunk one copy in, the device call, one copy out per
  // output; the kernel's time adds up over the chunks
  const int64_t chunk = std::max<int64_t>(1, std::min(ctx->chunk_frames, kMaxModesBatchFrames));
  const int64_t cf = std::min(frames, chunk);
  const size_t ch_bytes = (size_t)(cf + 2) * 512 * sizeof(float);
  auto up256 = [](size_t x) { return (x + 255) & ~(size_t)255; };
  const size_t unit_off = up256(ch_bytes * channels), noise_off = up256(unit_off + (size_t)(cf + 1) * channels * C1_UNIT_BYTES),
               signal_off = up256(noise_off + (size_t)cf * channels * 16 * sizeof(double)),
               totals_off = up256(signal_off + (size_t)cf * channels * 16 * sizeof(double));
  if ((rc = ensure_io(ctx, totals_off + (size_t)cf * channels * 2 * sizeof(double)))) return rc;
  StreamDrain drain(ctx);
  double *d_noise = reinterpret_cast<double *>((char *)ctx->d_io + noise_off), *d_signal = reinterpret_cast<double *>((char *)ctx->d_io + signal_off),
         *d_totals = reinterpret_cast<double *>((char *)ctx->d_io + totals_off);
  for (int64_t f0 = 0, n = 0; f0 < frames; f0 += n) {
    n = std::min(chunk, frames - f0);
    const int hf = f0 > 0 ? 1 : halo_frames, hu = f0 > 0 ? 1 : halo_units;
    const size_t n_units = (size_t)n * channels, at = (size_t)f0 * channels;
    const float *dptr[C1_MAX_CHANNELS] = {nullptr, nullptr};
    for (int c = 0; c < channels; c++) {
      float *d = reinterpret_cast<float *>((char *)ctx->d_io + ch_bytes * c);
      HIP_TRY(hipMemcpyAsync(d, pcm[c] + (f0 - hf) * 512, (size_t)(n + hf) * 512 * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
      dptr[c] = d + (size_t)hf * 512;
    }
    const size_t halo_bytes = (size_t)hu * channels * C1_UNIT_BYTES;   // a multiple of 4
    uint8_t *d_units = (uint8_t *)ctx->d_io + unit_off;
    HIP_TRY(hipMemcpyAsync(d_units, units + at * C1_UNIT_BYTES - halo_bytes, n_units * C1_UNIT_BYTES + halo_bytes, hipMemcpyHostToDevice, ctx->stream));
    if ((rc = c1_measure_pcm_device(ctx, dptr, channels, n, hf, d_units + halo_bytes, hu, noise ? d_noise : nullptr, signal ? d_signal : nullptr,
                                    totals ? d_totals : nullptr))) return rc;
    if (noise) HIP_TRY(hipMemcpyAsync(noise + at * 16, d_noise, n_units * 16 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (signal) HIP_TRY(hipMemcpyAsync(signal + at * 16, d_signal, n_units * 16 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (totals) HIP_TRY(hipMemcpyAsync(totals + at * 2, d_totals, n_units * 2 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
  }
  return C1_OK;
}

// host only: the number of candidates, every byte's domain (as check_mode_bytes), no byte twice
static int check_mode_candidates(const char *what, const uint8_t *cand, int n) {
  static const char *const kField[3] = {"low", "mid", "high"};
  if (n < 1 || n > C1_MAX_MODE_CANDIDATES) return fail(C1_ERR_ARG, "%s: n_cand = %d is outside 1..%d", what, n, C1_MAX_MODE_CANDIDATES);
  if (!cand) return fail(C1_ERR_ARG, "%s: cand_modes is NULL", what);
  for (int i = 0; i < n; i++) {
    const int b = cand[i];
    for (int k = 0; k < 3; k++) {
      const int m = (b >> (2 * k)) & 3, other = k == 2 ? 3 : 2;
      if (m != 0 && m != other)
        return fail(C1_ERR_ARG, "%s: candidate %d: %s field of mode byte 0x%02x is %d, not 0 or %d", what, i, kField[k], b, m, other);
    }
    if (b & 0xc0) return fail(C1_ERR_ARG, "%s: candidate %d: bits 6-7 of mode byte 0x%02x are set", what, i, b);
    for (int j = 0; j < i; j++)
      if (cand[j] == b) return fail(C1_ERR_ARG, "%s: candidate %d: mode byte 0x%02x is candidate %d's", what, i, b, j);
  }
  return C1_OK;
}

int c1_encode_best_modes_device(c1_ctx *ctx, const float *const *pcm, int channels, int64_t frames, int halo_frames,
                                const c1_encode_options *opts, const uint8_t *cand_modes, int n_cand, uint8_t *units,
                                uint8_t *choice, uint8_t *modes_out, double *distortion, double *energy) {
  CTX_GUARD(ctx);
  int rc = ctx_bind(ctx);
  if (rc) return rc;
  if ((rc = check_channels(channels))) return rc;
  if (frames < 0 || halo_frames < 0 || halo_frames > 2) return fail(C1_ERR_ARG, "bad frames / halo_frames");
  if (frames > kMaxChunkFrames) return fail(C1_ERR_ARG, "at most %lld frames per call", (long long)kMaxChunkFrames);
  if ((rc = check_mode_candidates("c1_encode_best_modes_device", cand_modes, n_cand))) return rc;
  if (!units && !choice && !modes_out && !distortion && !energy)
    return fail(C1_ERR_ARG, "c1_encode_best_modes_device: units, choice, modes_out, distortion and energy are all NULL");
  if (!opts) return fail(C1_ERR_ARG, "options are NULL");
  c1_encode_options base = *opts;                              // of the options only the biased scale factors are read
  base.transient_threshold = 1.0;
  base.fixed_block_modes[0] = base.fixed_block_modes[1] = base.fixed_block_modes[2] = -1;
  BestModesCall mc = {n_cand, nullptr, choice, modes_out, distortion, energy};
  uint8_t cand[C1_MAX_MODE_CANDIDATES];                        // the caller's array may change once the call has returned
  memcpy(cand, cand_modes, (size_t)n_cand);
  mc.cand = cand;
  return encode_device_impl(ctx, pcm, channels, frames, halo_frames, &base, units, nullptr, nullptr, nullptr, nullptr, false,
                            nullptr, nullptr, nullptr, &mc);
}

int c1_encode_best_modes_batch(c1_ctx *ctx, const float *const *pcm, int channels, int64_t frames, int halo_frames,
                               const c1_encode_options *opts, const uint8_t *cand_modes, int n_cand, uint8_t *units,
                               uint8_t *choice, uint8_t *modes_out, double *distortion, double *energy) {
  // everything the arguments alone decide comes first and needs neither a context nor a device
  int rc = check_channels(channels);
  if (rc) return rc;
  if (frames < 0 || halo_frames < 0 || halo_frames > 2) return fail(C1_ERR_ARG, "bad frames / halo_frames");
  if (frames > kMaxModesBatchFrames) return fail(C1_ERR_ARG, "at most %lld frames per call", (long long)kMaxModesBatchFrames);
  if ((rc = check_mode_candidates("c1_encode_best_modes_batch", cand_modes, n_cand))) return rc;
  if (!units && !choice && !modes_out && !distortion && !energy)
    return fail(C1_ERR_ARG, "c1_encode_best_modes_batch: units, choice, modes_out, distortion and energy are all NULL");
  if (!opts) return fail(C1_ERR_ARG, "options are NULL");
  {
    c1_encode_options base = *opts;
    base.transient_threshold = 1.0;
    base.fixed_block_modes[0] = base.fixed_block_modes[1] = base.fixed_block_modes[2] = -1;
    std::unique_ptr<C1DevEncOpts> d(new C1DevEncOpts);
    if ((rc = build_encode_opts(base, d.get()))) return rc;
  }
  if (frames > 0) {
    if (!pcm) return fail(C1_ERR_ARG, "pcm is NULL");
    for (int c = 0; c < channels; c++) if (!pcm[c]) return fail(C1_ERR_ARG, "pcm[%d] is NULL", c);
  }
  if (!ctx) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count == 0) { (void)hipGetLastError(); return fail(C1_ERR_NO_DEVICE, "c1_encode_best_modes_batch: no HIP device available; this library has no CPU path"); }
    return fail(C1_ERR_ARG, "context is NULL");
  }
  CTX_GUARD(ctx);
  if ((rc = ctx_bind(ctx))) return rc;
  if (frames == 0) return C1_OK;
  // one copy in, the device call, one copy out per output
  const size_t n_units = (size_t)frames * channels;
  const size_t ch_bytes = (size_t)(frames + halo_frames) * 512 * sizeof(float);
  auto up256 = [](size_t x) { return (x + 255) & ~(size_t)255; };
  const size_t unit_off = up256(ch_bytes * channels), choice_off = up256(unit_off + n_units * C1_UNIT_BYTES), modes_off = up256(choice_off + n_units),
               dist_off = up256(modes_off + n_units), energy_off = up256(dist_off + n_units * n_cand * sizeof(double));
  if ((rc = ensure_io(ctx, energy_off + n_units * n_cand * sizeof(double)))) return rc;
  const float *dptr[C1_MAX_CHANNELS] = {nullptr, nullptr};
  for (int c = 0; c < channels; c++) {
    float *d = reinterpret_cast<float *>((char *)ctx->d_io + ch_bytes * c);
    HIP_TRY(hipMemcpyAsync(d, pcm[c] - (size_t)halo_frames * 512, ch_bytes, hipMemcpyHostToDevice, ctx->stream));
    dptr[c] = d + (size_t)halo_frames * 512;
  }
  uint8_t *d_units = (uint8_t *)ctx->d_io + unit_off, *d_choice = (uint8_t *)ctx->d_io + choice_off, *d_modes = (uint8_t *)ctx->d_io + modes_off;
  double *d_dist = reinterpret_cast<double *>((char *)ctx->d_io + dist_off), *d_energy = reinterpret_cast<double *>((char *)ctx->d_io + energy_off);
  if ((rc = c1_encode_best_modes_device(ctx, dptr, channels, frames, halo_frames, opts, cand_modes, n_cand, units ? d_units : nullptr,
                                        choice ? d_choice : nullptr, modes_out ? d_modes : nullptr, distortion ? d_dist : nullptr,
                                        energy ? d_energy : nullptr))) return rc;
  if (units) HIP_TRY(hipMemcpyAsync(units, d_units, n_units * C1_UNIT_BYTES, hipMemcpyDeviceToHost, ctx->stream));
  if (choice) HIP_TRY(hipMemcpyAsync(choice, d_choice, n_units, hipMemcpyDeviceToHost, ctx->stream));
  if (modes_out) HIP_TRY(hipMemcpyAsync(modes_out, d_modes, n_units, hipMemcpyDeviceToHost, ctx->stream));
  if (distortion) HIP_TRY(hipMemcpyAsync(distortion, d_dist, n_units * n_cand * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  if (energy) HIP_TRY(hipMemcpyAsync(energy, d_energy, n_units * n_cand * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return C1_OK;
}

int c1_encode_measured_modes_device(c1_ctx *ctx, const float *const *pcm, int channels, int64_t frames, int halo_frames,
                                    const c1_encode_options *opts, const uint8_t *cand_modes, int n_cand, const int8_t *sf_offsets,
                                    int n_offsets, uint8_t *units, uint8_t *choice, uint8_t *modes_out, uint8_t *taken, int8_t *shifts,
                                    double *distortion, double *energy) {
  CTX_GUARD(ctx);
  int rc = ctx_bind(ctx);
  if (rc) return rc;
  if ((rc = check_channels(channels))) return rc;
  if (frames < 0 || halo_frames < 0 || halo_frames > 2) return fail(C1_ERR_ARG, "bad frames / halo_frames");
  if (frames > kMaxChunkFrames) return fail(C1_ERR_ARG, "at most %lld frames per call", (long long)kMaxChunkFrames);
  if ((rc = check_measured_opts("c1_encode_measured_modes_device", opts, false))) return rc;
  if ((rc = check_mode_candidates("c1_encode_measured_modes_device", cand_modes, n_cand))) return rc;
  if ((rc = check_sf_offsets("c1_encode_measured_modes_device", sf_offsets, n_offsets))) return rc;
  if (!units && !choice && !modes_out && !taken && !shifts && !distortion && !energy)
    return fail(C1_ERR_ARG, "c1_encode_measured_modes_device: units, choice, modes_out, taken, shifts, distortion and energy are all NULL");
  c1_encode_options base = *opts;                              // the modes are the candidates': neither threshold nor fixed modes are read
  base.transient_threshold = 1.0;
  base.fixed_block_modes[0] = base.fixed_block_modes[1] = base.fixed_block_modes[2] = -1;
  BestModesCall mc = {n_cand, nullptr, choice, modes_out, distortion, energy};
  uint8_t cand[C1_MAX_MODE_CANDIDATES];                        // the caller's arrays may change once the call has returned
  int8_t offs[C1_MAX_SF_OFFSETS];
  memcpy(cand, cand_modes, (size_t)n_cand);
  memcpy(offs, sf_offsets, (size_t)n_offsets);
  mc.cand = cand;
  mc.sf_offsets = offs;
  mc.n_offsets = n_offsets;
  mc.taken = taken;
  mc.shifts = shifts;
  return encode_device_impl(ctx, pcm, channels, frames, halo_frames, &base, units, nullptr, nullptr, nullptr, nullptr, false,
                            nullptr, nullptr, nullptr, &mc);
}

int c1_encode_measured_modes_batch(c1_ctx *ctx, const float *const *pcm, int channels, int64_t frames, int halo_frames,
                                   const c1_encode_options *opts, const uint8_t *cand_modes, int n_cand, const int8_t *sf_offsets,
                                   int n_offsets, uint8_t *units, uint8_t *choice, uint8_t *modes_out, uint8_t *taken, int8_t *shifts,
                                   double *distortion, double *energy) {
  // everything the arguments alone decide comes first and needs neither a context nor a device
  int rc = check_channels(channels);
  if (rc) return rc;
  if (frames < 0 || halo_frames < 0 || halo_frames > 2) return fail(C1_ERR_ARG, "bad frames / halo_frames");
  if (frames > kMaxModesBatchFrames) return fail(C1_ERR_ARG, "at most %lld frames per call", (long long)kMaxModesBatchFrames);
  if ((rc = check_measured_opts("c1_encode_measured_modes_batch", opts, false))) return rc;
  if ((rc = check_mode_candidates("c1_encode_measured_modes_batch", cand_modes, n_cand))) return rc;
  if ((rc = check_sf_offsets("c1_encode_measured_modes_batch", sf_offsets, n_offsets))) return rc;
  if (!units && !choice && !modes_out && !taken && !shifts && !distortion && !energy)
    return fail(C1_ERR_ARG, "c1_encode_measured_modes_batch: units, choice, modes_out, taken, shifts, distortion and energy are all NULL");
  if (frames > 0) {
    if (!pcm) return fail(C1_ERR_ARG, "pcm is NULL");
    for (int c = 0; c < channels; c++) if (!pcm[c]) return fail(C1_ERR_ARG, "pcm[%d] is NULL", c);
  }
  if (!ctx) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count == 0) { (void)hipGetLastError(); return fail(C1_ERR_NO_DEVICE, "c1_encode_measured_modes_batch: no HIP device available; this library has no CPU path"); }
    return fail(C1_ERR_ARG, "context is NULL");
  }
  CTX_GUARD(ctx);
  if ((rc = ctx_bind(ctx))) return rc;
  if (frames == 0) return C1_OK;
  // one copy in, the device call, one copy out per output
  const size_t n_units = (size_t)frames * channels;
  const size_t ch_bytes = (size_t)(frames + halo_frames) * 512 * sizeof(float);
  auto up256 = [](size_t x) { return (x + 255) & ~(size_t)255; };
  const size_t unit_off = up256(ch_bytes * channels), choice_off = up256(unit_off + n_units * C1_UNIT_BYTES), modes_off = up256(choice_off + n_units),
               taken_off = up256(modes_off + n_units), shift_off = up256(taken_off + n_units), dist_off = up256(shift_off + n_units * 52),
               energy_off = up256(dist_off + n_units * n_cand * 2 * sizeof(double));
  if ((rc = ensure_io(ctx, energy_off + n_units * n_cand * sizeof(double)))) return rc;
  const float *dptr[C1_MAX_CHANNELS] = {nullptr, nullptr};
  for (int c = 0; c < channels; c++) {
    float *d = reinterpret_cast<float *>((char *)ctx->d_io + ch_bytes * c);
    HIP_TRY(hipMemcpyAsync(d, pcm[c] - (size_t)halo_frames * 512, ch_bytes, hipMemcpyHostToDevice, ctx->stream));
    dptr[c] = d + (size_t)halo_frames * 512;
  }
  uint8_t *d_units = (uint8_t *)ctx->d_io + unit_off, *d_choice = (uint8_t *)ctx->d_io + choice_off, *d_modes = (uint8_t *)ctx->d_io + modes_off,
          *d_taken = (uint8_t *)ctx->d_io + taken_off;
  int8_t *d_shifts = reinterpret_cast<int8_t *>((char *)ctx->d_io + shift_off);
  double *d_dist = reinterpret_cast<double *>((char *)ctx->d_io + dist_off), *d_energy = reinterpret_cast<double *>((char *)ctx->d_io + energy_off);
  if ((rc = c1_encode_measured_modes_device(ctx, dptr, channels, frames, halo_frames, opts, cand_modes, n_cand, sf_offsets, n_offsets,
                                            units ? d_units : nullptr, choice ? d_choice : nullptr, modes_out ? d_modes : nullptr,
                                            taken ? d_taken : nullptr, shifts ? d_shifts : nullptr, distortion ? d_dist : nullptr,
                                            energy ? d_energy : nullptr))) return rc;
  if (units) HIP_TRY(hipMemcpyAsync(units, d_units, n_units * C1_UNIT_BYTES, hipMemcpyDeviceToHost, ctx->stream));
  if (choice) HIP_TRY(hipMemcpyAsync(choice, d_choice, n_units, hipMemcpyDeviceToHost, ctx->stream));
  if (modes_out) HIP_TRY(hipMemcpyAsync(modes_out, d_modes, n_units, hipMemcpyDeviceToHost, ctx->stream));
  if (taken) HIP_TRY(hipMemcpyAsync(taken, d_taken, n_units, hipMemcpyDeviceToHost, ctx->stream));
  if (shifts) HIP_TRY(hipMemcpyAsync(shifts, d_shifts, n_units * 52, hipMemcpyDeviceToHost, ctx->stream));
  if (distortion) HIP_TRY(hipMemcpyAsync(distortion, d_dist, n_units * n_cand * 2 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  if (energy) HIP_TRY(hipMemcpyAsync(energy, d_energy, n_units * n_cand * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return C1_OK;
}

// ---- the mode search under one masking threshold per unit (c1_encode_measured_modes_masked_*) ---------------------------------
// c1_encode_measured_modes_device's chain with the tables of c1_encode_measured_masked_device: validated and uploaded as there, and
// the search's kernel weighs every candidate's errors with P_b from the unit's all-long spectrum
int c1_encode_measured_modes_masked_device(c1_ctx *ctx, const float *const *pcm, int channels, int64_t frames, int halo_frames,
                                           const c1_encode_options *opts, const uint8_t *cand_modes, int n_cand, const int8_t *sf_offsets,
                                           int n_offsets, const double *mask_floor, const double *mask_spread, uint8_t *units,
                                           uint8_t *choice, uint8_t *modes_out, uint8_t *taken, int8_t *shifts, double *distortion,
                                           double *energy, double *weights) {
  const char *const what = "c1_encode_measured_modes_masked_device";
  CTX_GUARD(ctx);
  int rc = ctx_bind(ctx);
  if (rc) return rc;
  if ((rc = check_channels(channels))) return rc;
  if (frames < 0 || halo_frames < 0 || halo_frames > 2) return fail(C1_ERR_ARG, "bad frames / halo_frames");
  if (frames > kMaxChunkFrames) return fail(C1_ERR_ARG, "at most %lld frames per call", (long long)kMaxChunkFrames);
  if ((rc = check_measured_opts(what, opts, false))) return rc;
  if ((rc = check_mode_candidates(what, cand_modes, n_cand))) return rc;
  if ((rc = check_sf_offsets(what, sf_offsets, n_offsets))) return rc;
  if ((rc = check_masking(what, mask_floor, mask_spread))) return rc;
  if (!units && !choice && !modes_out && !taken && !shifts && !distortion && !energy && !weights)
    return fail(C1_ERR_ARG, "%s: units, choice, modes_out, taken, shifts, distortion, energy and weights are all NULL", what);
  c1_encode_options base = *opts;                              // the modes are the candidates': neither threshold nor fixed modes are read
  base.transient_threshold = 1.0;
  base.fixed_block_modes[0] = base.fixed_block_modes[1] = base.fixed_block_modes[2] = -1;
  if (frames > 0) {
    // the tail of an earlier speculative encode may still run beside the context's stream: it reads none of this
    if ((rc = upload_masking(ctx, mask_floor, mask_spread))) return rc;
  }
  BestModesCall mc = {n_cand, nullptr, choice, modes_out, distortion, energy};
  uint8_t cand[C1_MAX_MODE_CANDIDATES];                        // the caller's arrays may change once the call has returned
  int8_t offs[C1_MAX_SF_OFFSETS];
  memcpy(cand, cand_modes, (size_t)n_cand);
  memcpy(offs, sf_offsets, (size_t)n_offsets);
  mc.cand = cand;
  mc.sf_offsets = offs;
  mc.n_offsets = n_offsets;
  mc.taken = taken;
  mc.shifts = shifts;
  mc.mask = ctx->d_mask;
  mc.has_spread = mask_spread != nullptr;
  mc.weights = weights;
  return encode_device_impl(ctx, pcm, channels, frames, halo_frames, &base, units, nullptr, nullptr, nullptr, nullptr, false,
                            nullptr, nullptr, nullptr, &mc);
}

int c1_encode_measured_modes_masked_batch(c1_ctx *ctx, const float *const *pcm, int channels, int64_t frames, int halo_frames,
                                          const c1_encode_options *opts, const uint8_t *cand_modes, int n_cand, const int8_t *sf_offsets,
                                          int n_offsets, const double *mask_floor, const double *mask_spread, uint8_t *units,
                                          uint8_t *choice, uint8_t *modes_out, uint8_t *taken, int8_t *shifts, double *distortion,
                                          double *energy, double *weights) {
  // everything the arguments alone decide comes first and needs neither a context nor a device
  const char *const what = "c1_encode_measured_modes_masked_batch";
  int rc = check_channels(channels);
  if (rc) return rc;
  if (frames < 0 || halo_frames < 0 || halo_frames > 2) return fail(C1_ERR_ARG, "bad frames / halo_frames");
  if (frames > kMaxModesBatchFrames) return fail(C1_ERR_ARG, "at most %lld frames per call", (long long)kMaxModesBatchFrames);
  if ((rc = check_measured_opts(what, opts, false))) return rc;
  if ((rc = check_mode_candidates(what, cand_modes, n_cand))) return rc;
  if ((rc = check_sf_offsets(what, sf_offsets, n_offsets))) return rc;
  if ((rc = check_masking(what, mask_floor, mask_spread))) return rc;
  if (!units && !choice && !modes_out && !taken && !shifts && !distortion && !energy && !weights)
    return fail(C1_ERR_ARG, "%s: units, choice, modes_out, taken, shifts, distortion, energy and weights are all NULL", what);
  if (frames > 0) {
    if (!pcm) return fail(C1_ERR_ARG, "pcm is NULL");
    for (int c = 0; c < channels; c++) if (!pcm[c]) return fail(C1_ERR_ARG, "pcm[%d] is NULL", c);
  }
  if (!ctx) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count == 0) { (void)hipGetLastError(); return fail(C1_ERR_NO_DEVICE, "%s: no HIP device available; this library has no CPU path", what); }
    return fail(C1_ERR_ARG, "context is NULL");
  }
  CTX_GUARD(ctx);
  if ((rc = ctx_bind(ctx))) return rc;
  if (frames == 0) return C1_OK;
  // one copy in, the device call, one copy out per output
  const size_t n_units = (size_t)frames * channels;
  const size_t ch_bytes = (size_t)(frames + halo_frames) * 512 * sizeof(float);
  auto up256 = [](size_t x) { return (x + 255) & ~(size_t)255; };
  const size_t unit_off = up256(ch_bytes * channels), choice_off = up256(unit_off + n_units * C1_UNIT_BYTES), modes_off = up256(choice_off + n_units),
               taken_off = up256(modes_off + n_units), shift_off = up256(taken_off + n_units), dist_off = up256(shift_off + n_units * 52),
               energy_off = up256(dist_off + n_units * n_cand * 2 * sizeof(double)),
               weight_off = up256(energy_off + n_units * n_cand * sizeof(double));
  if ((rc = ensure_io(ctx, weight_off + n_units * 52 * sizeof(double)))) return rc;
  const float *dptr[C1_MAX_CHANNELS] = {nullptr, nullptr};
  for (int c = 0; c < channels; c++) {
    float *d = reinterpret_cast<float *>((char *)ctx->d_io + ch_bytes * c);
    HIP_TRY(hipMemcpyAsync(d, pcm[c] - (size_t)halo_frames * 512, ch_bytes, hipMemcpyHostToDevice, ctx->stream));
    dptr[c] = d + (size_t)halo_frames * 512;
  }
  uint8_t *d_units = (uint8_t *)ctx->d_io + unit_off, *d_choice = (uint8_t *)ctx->d_io + choice_off, *d_modes = (uint8_t *)ctx->d_io + modes_off,
          *d_taken = (uint8_t *)ctx->d_io + taken_off;
  int8_t *d_shifts = reinterpret_cast<int8_t *>((char *)ctx->d_io + shift_off);
  double *d_dist = reinterpret_cast<double *>((char *)ctx->d_io + dist_off), *d_energy = reinterpret_cast<double *>((char *)ctx->d_io + energy_off),
         *d_weights = reinterpret_cast<double *>((char *)ctx->d_io + weight_off);
  if ((rc = c1_encode_measured_modes_masked_device(ctx, dptr, channels, frames, halo_frames, opts, cand_modes, n_cand, sf_offsets, n_offsets,
                                                   mask_floor, mask_spread, units ? d_units : nullptr, choice ? d_choice : nullptr,
                                                   modes_out ? d_modes : nullptr, taken ? d_taken : nullptr, shifts ? d_shifts : nullptr,
                                                   distortion ? d_dist : nullptr, energy ? d_energy : nullptr,
                                                   weights ? d_weights : nullptr))) return rc;
  if (units) HIP_TRY(hipMemcpyAsync(units, d_units, n_units * C1_UNIT_BYTES, hipMemcpyDeviceToHost, ctx->stream));
  if (choice) HIP_TRY(hipMemcpyAsync(choice, d_choice, n_units, hipMemcpyDeviceToHost, ctx->stream));
  if (modes_out) HIP_TRY(hipMemcpyAsync(modes_out, d_modes, n_units, hipMemcpyDeviceToHost, ctx->stream));
  if (taken) HIP_TRY(hipMemcpyAsync(taken, d_taken, n_units, hipMemcpyDeviceToHost, ctx->stream));
  if (shifts) HIP_TRY(hipMemcpyAsync(shifts, d_shifts, n_units * 52, hipMemcpyDeviceToHost, ctx->stream));
  if (distortion) HIP_TRY(hipMemcpyAsync(distortion, d_dist, n_units * n_cand * 2 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  if (energy) HIP_TRY(hipMemcpyAsync(energy, d_energy, n_units * n_cand * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  if (weights) HIP_TRY(hipMemcpyAsync(weights, d_weights, n_units * 52 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return C1_OK;
}

int c1_decode_device(c1_ctx *ctx, const uint8_t *units, int channels, int64_t frames, int halo_units,
                     float *const *pcm) {
  CTX_GUARD(ctx);
  int rc = ctx_bind(ctx);
  if (rc) return rc;
  if ((rc = check_channels(channels))) return rc;
  if (frames < 0) return fail(C1_ERR_ARG, "frames must be >= 0");
  if (halo_units < 0 || halo_units > 1) return fail(C1_ERR_ARG, "halo_units must be 0 or 1");
  if (ctx->profiling && ctx->timing_depth == 0) reset_timings(ctx);
  if (frames == 0) return C1_OK;
  if (!units || !pcm) return fail(C1_ERR_ARG, "units or pcm is NULL");
  if ((uintptr_t)units & 3) return fail(C1_ERR_ARG, "units must be 4-byte aligned on the device");
  C1DecodeLaunch L;
  memset(&L, 0, sizeof L);
  L.units = units;
  L.channels = channels;
  L.frames = frames;
  L.halo_units = halo_units;
  L.tables = ctx->d_tables;
  for (int c = 0; c < channels; c++) {
    if (!pcm[c]) return fail(C1_ERR_ARG, "pcm[%d] is NULL", c);
    if ((uintptr_t)pcm[c] & 15) return fail(C1_ERR_ARG, "pcm[%d] must be 16-byte aligned on the device", c);
    L.pcm[c] = pcm[c];
  }
  { ScopedTiming t(ctx, K_DECODE); c1k_launch_decode(L, ctx->decode_binary32, ctx->stream); }
  HIP_TRY(hipGetLastError());
  return C1_OK;
}

int c1_decode_batch(c1_ctx *ctx, const uint8_t *units, int channels, int64_t frames, int halo_units,
                    float *const *pcm) {
  CTX_GUARD(ctx);
  int rc = ctx_bind(ctx);
  if (rc) return rc;
  if ((rc = check_channels(channels))) return rc;
  if (frames < 0 || halo_units < 0 || halo_units > 1) return fail(C1_ERR_ARG, "bad frames / halo_units");
  if (frames == 0) return C1_OK;
  if (!units || !pcm) return fail(C1_ERR_ARG, "units or pcm is NULL");
  if (frames > 2 * kStreamChunkFrames) {
    for (int c = 0; c < channels; c++) if (!pcm[c]) return fail(C1_ERR_ARG, "pcm[%d] is NULL", c);
    return decode_batch_streamed(ctx, units, channels, frames, halo_units, pcm);
  }
  const size_t halo_bytes = (size_t)halo_units * channels * C1_UNIT_BYTES;   // multiple of 4
  const size_t unit_bytes = (size_t)frames * channels * C1_UNIT_BYTES + halo_bytes;
  const size_t pcm_off = (unit_bytes + 255) & ~(size_t)255;
  const size_t ch_bytes = (size_t)frames * 512 * sizeof(float);
  if ((rc = ensure_io(ctx, pcm_off + ch_bytes * channels))) return rc;
  HIP_TRY(hipMemcpyAsync(ctx->d_io, units - halo_bytes, unit_bytes, hipMemcpyHostToDevice, ctx->stream));
  float *dptr[C1_MAX_CHANNELS] = {nullptr, nullptr};
  for (int c = 0; c < channels; c++) dptr[c] = reinterpret_cast<float *>((char *)ctx->d_io + pcm_off + ch_bytes * c);
  if ((rc = c1_decode_device(ctx, (const uint8_t *)ctx->d_io + halo_bytes, channels, frames, halo_units, dptr))) return rc;
  for (int c = 0; c < channels; c++) {
    if (!pcm[c]) return fail(C1_ERR_ARG, "pcm[%d] is NULL", c);
    HIP_TRY(hipMemcpyAsync(pcm[c], dptr[c], ch_bytes, hipMemcpyDeviceToHost, ctx->stream));
  }
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return C1_OK;
}

// ---- decode from frame fields (k_decode_fields) -------------------------------------------------------------------------
namespace {
int launch_decode_fields(c1_ctx *ctx, const C1FieldPtrs &cur, const C1FieldPtrs &prev, int channels, int64_t frames, int halo_frames,
                         float *const *pcm) {
  C1DecodeFieldsLaunch L;
  memset(&L, 0, sizeof L);
  L.cur = cur;
  L.prev = halo_frames ? prev : cur;
  L.channels = channels;
  L.frames = frames;
  L.halo_frames = halo_frames;
  L.tables = ctx->d_tables;
  L.binary32 = ctx->decode_model == C1_DECODE_BINARY32;
  for (int c = 0; c < channels; c++) L.pcm[c] = pcm[c];
  { ScopedTiming t(ctx, K_DECODE_FIELDS); c1k_launch_decode_fields(L, ctx->stream); }
  HIP_TRY(hipGetLastError());
  return C1_OK;
}
}  // namespace

int c1_decode_fields_device(c1_ctx *ctx, int channels, int64_t frames, int halo_frames, const int32_t *nbfu,
                            const int32_t *block_modes, const int32_t *sfi, const int32_t *wl, const int32_t *quantized,
                            float *const *pcm) {
  CTX_GUARD(ctx);
  int rc = ctx_bind(ctx);
  if (rc) return rc;
  if ((rc = check_channels(channels))) return rc;
  if (frames < 0 || frames > kMaxChunkFrames) return fail(C1_ERR_ARG, "decode fields: frames must be 0 .. 2^27, got %lld", (long long)frames);
  if (halo_frames < 0 || halo_frames > 1) return fail(C1_ERR_ARG, "decode fields: halo_frames must be 0 or 1, got %d", halo_frames);
  if (ctx->profiling && ctx->timing_depth == 0) reset_timings(ctx);
  if (frames == 0) return C1_OK;
  if (!nbfu || !block_modes || !sfi || !wl || !quantized || !pcm) return fail(C1_ERR_ARG, "decode fields: NULL argument");
  if ((uintptr_t)quantized & 15) return fail(C1_ERR_ARG, "decode fields: quantized must be 16-byte aligned on the device");
  if (((uintptr_t)nbfu | (uintptr_t)block_modes | (uintptr_t)sfi | (uintptr_t)wl) & 3)
    return fail(C1_ERR_ARG, "decode fields: field arrays must be 4-byte aligned on the device");
  for (int c = 0; c < channels; c++) {
    if (!pcm[c]) return fail(C1_ERR_ARG, "pcm[%d] is NULL", c);
    if ((uintptr_t)pcm[c] & 15) return fail(C1_ERR_ARG, "pcm[%d] must be 16-byte aligned on the device", c);
  }
  const C1FieldPtrs cur{nbfu, block_modes, sfi, wl, quantized};
  const C1FieldPtrs prev = halo_frames ? field_unit(cur, -(int64_t)channels) : cur;
  return launch_decode_fields(ctx, cur, prev, channels, frames, halo_frames, pcm);
}

int c1_decode_fields_batch(c1_ctx *ctx, int channels, int64_t frames, int halo_frames, const int32_t *nbfu,
                           const int32_t *block_modes, const int32_t *sfi, const int32_t *wl, const int32_t *quantized,
                           float *const *pcm) {
  CTX_GUARD(ctx);
  int rc = ctx_bind(ctx);
  if (rc) return rc;
  if ((rc = check_channels(channels))) return rc;
  if (halo_frames < 0 || halo_frames > 1) return fail(C1_ERR_ARG, "decode fields: halo_frames must be 0 or 1, got %d", halo_frames);
  if (frames < 0 || frames > kMaxStageFrames) return fail(C1_ERR_ARG, "decode fields: frames must be 0 .. 2^20, got %lld", (long long)frames);
  if (frames == 0) return C1_OK;
  if (!nbfu || !block_modes || !sfi || !wl || !quantized || !pcm) return fail(C1_ERR_ARG, "decode fields: NULL argument");
  for (int c = 0; c < channels; c++) if (!pcm[c]) return fail(C1_ERR_ARG, "pcm[%d] is NULL", c);
  const int64_t h = (int64_t)halo_frames * channels, units = frames * channels + h;
  nbfu -= h; block_modes -= 3 * h; sfi -= 52 * h; wl -= 52 * h; quantized -= 512 * h;      // the halo's fields first
  if ((rc = check_field_domain("decode fields", units, channels, -halo_frames, nbfu, sfi, wl))) return rc;
  DeviceScratch ds;
  int32_t *d; float *dp;
  const size_t per = (size_t)frames * 512;
  if ((rc = ds.alloc(&d, (size_t)(kFieldInts * units))) || (rc = ds.alloc(&dp, per * channels))) return rc;
  const C1FieldPtrs all = field_layout(d, units);
  HIP_TRY(hipMemcpyAsync((void *)all.nbfu, nbfu, (size_t)units * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(hipMemcpyAsync((void *)all.modes, block_modes, 3 * (size_t)units * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(hipMemcpyAsync((void *)all.sfi, sfi, 52 * (size_t)units * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(hipMemcpyAsync((void *)all.wl, wl, 52 * (size_t)units * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(hipMemcpyAsync((void *)all.q, quantized, 512 * (size_t)units * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
  float *dptr[C1_MAX_CHANNELS] = {nullptr, nullptr};
  for (int c = 0; c < channels; c++) dptr[c] = dp + per * c;
  if (ctx->profiling && ctx->timing_depth == 0) reset_timings(ctx);
  if ((rc = launch_decode_fields(ctx, field_unit(all, h), all, channels, frames, halo_frames, dptr))) return rc;
  for (int c = 0; c < channels; c++) HIP_TRY(hipMemcpyAsync(pcm[c], dptr[c], per * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return C1_OK;
}

// ---- one batch over several devices ------------------------------------------------------------------------------------
namespace {
// Contexts for the *_multi entry points: one per shard for the duration of a call, checked out of a process-wide pool and
// given back at its end.  A context is never shared between two calls in flight nor destroyed while one uses it (a second
// call that needs the same device meanwhile gets another context); a context made before the last c1_set_tables() is
// retired when it comes back, so the *_multi entry points follow the installed tables like a context created afresh.
struct ShardPool {
  struct Entry { int device; uint64_t tables_gen; c1_ctx *ctx; bool busy; };
  std::mutex mu;
  std::vector<Entry> entries;
  c1_ctx *checkout(int device, int *rc) {
    const uint64_t gen = g_tables_gen.load();
    std::vector<c1_ctx *> stale;
    c1_ctx *found = nullptr;
    {
      std::lock_guard<std::mutex> lock(mu);
      for (size_t i = 0; i < entries.size();) {
        Entry &e = entries[i];
        if (!e.busy && e.tables_gen != gen) { stale.push_back(e.ctx); entries.erase(entries.begin() + (long)i); continue; }
        if (!found && !e.busy && e.device == device) { e.busy = true; found = e.ctx; }
        ++i;
      }
    }
    for (c1_ctx *c : stale) c1_ctx_destroy(c);
    *rc = C1_OK;
    if (found) return found;
    c1_ctx *c = nullptr;
    *rc = c1_ctx_create(device, nullptr, &c);
    if (*rc) return nullptr;
    std::lock_guard<std::mutex> lock(mu);
    entries.push_back({device, gen, c, true});
    return c;
  }
  void give_back(c1_ctx *c) {
    std::lock_guard<std::mutex> lock(mu);
    for (Entry &e : entries) if (e.ctx == c) e.busy = false;
  }
};
ShardPool g_shards;
struct ShardLease {           // the contexts of one *_multi call
  std::vector<c1_ctx *> ctxs;
  ~ShardLease() { for (c1_ctx *c : ctxs) if (c) g_shards.give_back(c); }
  int take(const int *devices, int shards) {
    for (int s = 0; s < shards; s++) {
      int rc = C1_OK;
      c1_ctx *c = g_shards.checkout(devices[s], &rc);
      if (rc) return rc;                               // c1_last_error() of this thread holds the reason
      ctxs.push_back(c);
    }
    return C1_OK;
  }
};

// contiguous ranges whose sizes differ by at most one frame
void shard_plan(int64_t frames, int shards, std::vector<std::pair<int64_t, int64_t>> *plan) {
  const int64_t base = frames / shards, extra = frames % shards;
  int64_t at = 0;
  for (int r = 0; r < shards; r++) {
    const int64_t n = base + (r < extra ? 1 : 0);
    plan->push_back({at, at + n});
    at += n;
  }
}
}  // namespace

int c1_encode_batch_multi(const int *devices, int n_devices, const float *const *pcm, int channels, int64_t frames,
                          int halo_frames, const c1_encode_options *opts, uint8_t *units) {
  int rc = check_channels(channels);
  if (rc) return rc;
  if (!devices || n_devices < 1 || n_devices > 64) return fail(C1_ERR_ARG, "devices: 1..64 entries");
  if (frames < 0 || halo_frames < 0 || halo_frames > 2) return fail(C1_ERR_ARG, "bad frames / halo_frames");
  if (frames == 0) return C1_OK;
  if (!pcm || !units || !opts) return fail(C1_ERR_ARG, "NULL argument");
  for (int c = 0; c < channels; c++) if (!pcm[c]) return fail(C1_ERR_ARG, "pcm[%d] is NULL", c);
  const int shards = (int)std::min<int64_t>(n_devices, frames);
  std::vector<std::pair<int64_t, int64_t>> plan;
  shard_plan(frames, shards, &plan);
  ShardLease lease;
  if ((rc = lease.take(devices, shards))) return rc;
  const std::vector<c1_ctx *> &ctxs = lease.ctxs;
  std::vector<int> rcs(shards, C1_OK);
  std::vector<std::string> errs(shards);
  std::vector<std::thread> threads;
  for (int s = 0; s < shards; s++)
    threads.emplace_back([&, s] {
      const int64_t a = plan[s].first, b = plan[s].second;
      const int h = (int)std::min<int64_t>(2, a + halo_frames);        // frames of real PCM directly in front of the range
      const float *ptrs[C1_MAX_CHANNELS] = {nullptr, nullptr};
      for (int c = 0; c < channels; c++) ptrs[c] = pcm[c] + a * 512;
      rcs[s] = c1_encode_batch(ctxs[s], ptrs, channels, b - a, h, opts, units + (size_t)a * channels * C1_UNIT_BYTES);
      if (rcs[s]) errs[s] = c1_last_error();
    });
  for (auto &t : threads) t.join();
  for (int s = 0; s < shards; s++)
    if (rcs[s]) return fail(rcs[s], "shard %d on device %d: %s", s, devices[s], errs[s].c_str());
  return C1_OK;
}

int c1_decode_batch_multi(const int *devices, int n_devices, const uint8_t *units, int channels, int64_t frames,
                          int halo_units, float *const *pcm) {
  int rc = check_channels(channels);
  if (rc) return rc;
  if (!devices || n_devices < 1 || n_devices > 64) return fail(C1_ERR_ARG, "devices: 1..64 entries");
  if (frames < 0 || halo_units < 0 || halo_units > 1) return fail(C1_ERR_ARG, "bad frames / halo_units");
  if (frames == 0) return C1_OK;
  if (!pcm || !units) return fail(C1_ERR_ARG, "NULL argument");
  for (int c = 0; c < channels; c++) if (!pcm[c]) return fail(C1_ERR_ARG, "pcm[%d] is NULL", c);
  const int shards = (int)std::min<int64_t>(n_devices, frames);
  std::vector<std::pair<int64_t, int64_t>> plan;
  shard_plan(frames, shards, &plan);
  ShardLease lease;
  if ((rc = lease.take(devices, shards))) return rc;
  const std::vector<c1_ctx *> &ctxs = lease.ctxs;
  std::vector<int> rcs(shards, C1_OK);
  std::vector<std::string> errs(shards);
  std::vector<std::thread> threads;
  for (int s = 0; s < shards; s++)
    threads.emplace_back([&, s] {
      const int64_t a = plan[s].first, b = plan[s].second;
      const int h = a > 0 ? 1 : halo_units;
      float *ptrs[C1_MAX_CHANNELS] = {nullptr, nullptr};
      for (int c = 0; c < channels; c++) ptrs[c] = pcm[c] + a * 512;
      rcs[s] = c1_decode_batch(ctxs[s], units + (size_t)a * channels * C1_UNIT_BYTES, channels, b - a, h, ptrs);
      if (rcs[s]) errs[s] = c1_last_error();
    });
  for (auto &t : threads) t.join();
  for (int s = 0; s < shards; s++)
    if (rcs[s]) return fail(rcs[s], "shard %d on device %d: %s", s, devices[s], errs[s].c_str());
  return C1_OK;
}

// ---- WAV body <-> units in one host call (streamed) -----------------------------------------------------------------
int c1_encode_wav_batch(c1_ctx *ctx, const void *interleaved, int bits, int channels, int64_t samples_per_channel,
                        const c1_encode_options *opts, uint8_t *units) {
  CTX_GUARD(ctx);
  int rc = ctx_bind(ctx);
  if (rc) return rc;
  if ((rc = check_channels(channels))) return rc;
  if (bits != 16 && bits != 24 && bits != 32) return fail(C1_ERR_ARG, "bits must be 16, 24 or 32, got %d", bits);
  if (samples_per_channel < 0) return fail(C1_ERR_ARG, "samples_per_channel must be >= 0");
  if (samples_per_channel == 0) return C1_OK;
  if (!interleaved || !units) return fail(C1_ERR_ARG, "interleaved or units is NULL");
  const int64_t frames = (samples_per_channel + 511) / 512, chunk = kStreamChunkFrames;
  const size_t bps = (size_t)bits / 8, frame_raw = 512 * (size_t)channels * bps;
  const size_t raw_bytes = ((size_t)(chunk + 2) * frame_raw + 255) & ~(size_t)255;
  const size_t pcm_bytes = (size_t)(chunk + 2) * 512 * sizeof(float);          // per channel
  const size_t out_bytes = ((size_t)chunk * channels * C1_UNIT_BYTES + 255) & ~(size_t)255;
  const size_t set_bytes = raw_bytes + pcm_bytes * channels + out_bytes;
  if ((rc = ensure_ring(ctx, 2 * set_bytes))) return rc;
  StreamDrain drain(ctx);
  const uint8_t *src = static_cast<const uint8_t *>(interleaved);
  auto download = [&](int64_t index) -> int {
    const int p = (int)(index & 1);
    const int64_t f0 = index * chunk, n = std::min(chunk, frames - f0);
    const uint8_t *d_units = reinterpret_cast<const uint8_t *>((char *)ctx->d_ring + (size_t)p * set_bytes + raw_bytes + pcm_bytes * channels);
    HIP_TRY(hipStreamWaitEvent(ctx->s_down, ctx->ev_run[p], 0));
    HIP_TRY(hipMemcpyAsync(units + (size_t)f0 * channels * C1_UNIT_BYTES, d_units, (size_t)n * channels * C1_UNIT_BYTES,
                           hipMemcpyDeviceToHost, ctx->s_down));
    HIP_TRY(hipEventRecord(ctx->ev_down[p], ctx->s_down));
    return C1_OK;
  };
  int64_t index = 0;
  for (int64_t f0 = 0; f0 < frames; f0 += chunk, ++index) {
    const int p = (int)(index & 1);
    const int64_t n = std::min(chunk, frames - f0);
    const int h = (int)std::min<int64_t>(2, f0);                 // frames of PCM history in front of the chunk
    char *set = (char *)ctx->d_ring + (size_t)p * set_bytes;
    if (index >= 2) {
      HIP_TRY(hipStreamWaitEvent(ctx->s_up, ctx->ev_run[p], 0));
      HIP_TRY(hipStreamWaitEvent(ctx->s_up, ctx->ev_down[p], 0));
      HIP_TRY(hipStreamWaitEvent(ctx->stream, ctx->ev_down[p], 0));
    }
    const int64_t s0 = (f0 - h) * 512;                                         // first sample (per channel) of the upload
    const int64_t have = std::min<int64_t>((n + h) * 512, samples_per_channel - s0);
    HIP_TRY(hipMemcpyAsync(set, src + (size_t)s0 * channels * bps, (size_t)have * channels * bps, hipMemcpyHostToDevice, ctx->s_up));
    HIP_TRY(hipEventRecord(ctx->ev_up[p], ctx->s_up));
    HIP_TRY(hipStreamWaitEvent(ctx->stream, ctx->ev_up[p], 0));
    float *dch[C1_MAX_CHANNELS] = {nullptr, nullptr};
    const float *dptr[C1_MAX_CHANNELS] = {nullptr, nullptr};
    for (int c = 0; c < channels; c++) {
      dch[c] = reinterpret_cast<float *>(set + raw_bytes + pcm_bytes * c);
      dptr[c] = dch[c] + (size_t)h * 512;
      if (have < (n + h) * 512)                                                // zero padding of the last, partial frame
        HIP_TRY(hipMemsetAsync(dch[c] + have, 0, (size_t)((n + h) * 512 - have) * sizeof(float), ctx->stream));
    }
    c1k_launch_pcm_from_int(set, bits, channels, have, dch, ctx->stream);
    if ((rc = encode_device_joined(ctx, dptr, channels, n, h, opts, reinterpret_cast<uint8_t *>(set + raw_bytes + pcm_bytes * channels)))) return rc;
    HIP_TRY(hipEventRecord(ctx->ev_run[p], ctx->stream));
    if (index >= 1 && (rc = download(index - 1))) return rc;
  }
  if ((rc = download(index - 1))) return rc;
  HIP_TRY(hipStreamSynchronize(ctx->s_down));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return C1_OK;
}

int c1_decode_wav16_batch(c1_ctx *ctx, const uint8_t *units, int channels, int64_t frames, int16_t *interleaved) {
  CTX_GUARD(ctx);
  int rc = ctx_bind(ctx);
  if (rc) return rc;
  if ((rc = check_channels(channels))) return rc;
  if (frames < 0) return fail(C1_ERR_ARG, "frames must be >= 0");
  if (frames == 0) return C1_OK;
  if (!units || !interleaved) return fail(C1_ERR_ARG, "units or interleaved is NULL");
  const int64_t chunk = kStreamChunkFrames;
  const size_t in_bytes = ((size_t)(chunk + 1) * channels * C1_UNIT_BYTES + 255) & ~(size_t)255;
  const size_t pcm_bytes = (size_t)chunk * 512 * sizeof(float);                // per channel
  const size_t out_bytes = (size_t)chunk * 512 * channels * sizeof(int16_t);
  const size_t set_bytes = in_bytes + pcm_bytes * channels + out_bytes;
  if ((rc = ensure_ring(ctx, 2 * set_bytes))) return rc;
  StreamDrain drain(ctx);
  auto download = [&](int64_t index) -> int {
    const int p = (int)(index & 1);
    const int64_t f0 = index * chunk, n = std::min(chunk, frames - f0);
    char *set = (char *)ctx->d_ring + (size_t)p * set_bytes;
    HIP_TRY(hipStreamWaitEvent(ctx->s_down, ctx->ev_run[p], 0));
    HIP_TRY(hipMemcpyAsync(interleaved + (size_t)f0 * 512 * channels, set + in_bytes + pcm_bytes * channels,
                           (size_t)n * 512 * channels * sizeof(int16_t), hipMemcpyDeviceToHost, ctx->s_down));
    HIP_TRY(hipEventRecord(ctx->ev_down[p], ctx->s_down));
    return C1_OK;
  };
  int64_t index = 0;
  for (int64_t f0 = 0; f0 < frames; f0 += chunk, ++index) {
    const int p = (int)(index & 1);
    const int64_t n = std::min(chunk, frames - f0);
    const int h = (int)std::min<int64_t>(1, f0);
    char *set = (char *)ctx->d_ring + (size_t)p * set_bytes;
    if (index >= 2) {
      HIP_TRY(hipStreamWaitEvent(ctx->s_up, ctx->ev_run[p], 0));
      HIP_TRY(hipStreamWaitEvent(ctx->s_up, ctx->ev_down[p], 0));
      HIP_TRY(hipStreamWaitEvent(ctx->stream, ctx->ev_down[p], 0));
    }
    const size_t hb = (size_t)h * channels * C1_UNIT_BYTES;
    HIP_TRY(hipMemcpyAsync(set, units + (size_t)f0 * channels * C1_UNIT_BYTES - hb, (size_t)n * channels * C1_UNIT_BYTES + hb,
                           hipMemcpyHostToDevice, ctx->s_up));
    HIP_TRY(hipEventRecord(ctx->ev_up[p], ctx->s_up));
    HIP_TRY(hipStreamWaitEvent(ctx->stream, ctx->ev_up[p], 0));
    float *dptr[C1_MAX_CHANNELS] = {nullptr, nullptr};
    for (int c = 0; c < channels; c++) dptr[c] = reinterpret_cast<float *>(set + in_bytes + pcm_bytes * c);
    if ((rc = c1_decode_device(ctx, (const uint8_t *)set + hb, channels, n, h, dptr))) return rc;
    c1k_launch_pcm_to_int16(dptr, channels, n * 512, reinterpret_cast<int16_t *>(set + in_bytes + pcm_bytes * channels), ctx->stream);
    HIP_TRY(hipEventRecord(ctx->ev_run[p], ctx->stream));
    if (index >= 1 && (rc = download(index - 1))) return rc;
  }
  if ((rc = download(index - 1))) return rc;
  HIP_TRY(hipStreamSynchronize(ctx->s_down));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  HIP_TRY(hipGetLastError());
  return C1_OK;
}

// ---- stateful streams -------------------------------------------------------------------------------
// What an encode() closure keeps besides the PCM is its detection history (bufferPool.transientDetection, encoder.js:142):
// the magnitudes of the last frame detection ran on, a function of that frame's bands.  A push with halo = 2 rebuilds them
// from the previous frame, which is right whenever that frame was detected.  After fixed modes it was not: the history is
// then a fresh pool's zeros (detection never ran) or the bands of the last detected frame, kept here since the switch to
// fixed modes, and the first frame of the next push under detection is encoded by the stage kernels against them.
// After a restore (c1_enc_stream_set_state) the whole pool is explicit: d_state holds it, and the next two pushed frames are
// encoded from it by the from-state kernel (c1_k_state.hip), which keeps d_state current.  Two frames on the PCM history is
// real again and every later frame takes the usual path (all state after a frame is a function of that frame
// and the 138 samples before it).  If the last of those frames ran under fixed modes, the detection history is neither a
// previous frame's nor stored bands but the magnitudes d_state still holds (HIST_MAGS: restored verbatim, or written by a
// from-state frame under detection); the first frame under detection after that is encoded from the state again.
enum EncHistory { HIST_PREV = 0, HIST_ZEROS = 1, HIST_STORED = 2, HIST_MAGS = 3 };

// scratch of the switch frame, one allocation carved per stream on first use; channels-interleaved where several
struct EncSwitchScratch {
  float *bands;      // 2 frames x channels x 512: the bands of t-1 and t (t-1's alone at a detection -> fixed switch)
  float *coefs;      // 2 frames x channels x 512, and side / alloc: the encode taps behind `bands`
  uint8_t *side, *alloc;
  float *rows;       // 2 x 512: [halo, t] for the block selection, then [t-1, t] for the MDCT
  float *mags;       // 2 x 256
  int32_t *modes;    // channels x 3
  uint8_t *mode_byte;
  uint32_t *lists;   // 4 + 2
  float *coef1;      // one frame: coefficients, side, allocation, candidates, work lists, fields
  uint8_t *side1, *alloc1, *cand1;
  uint32_t *work1;
  int32_t *nbfu, *sfi, *wl, *q;
};

struct c1_enc_stream {
  c1_ctx *ctx;
  int channels;
  c1_encode_options opts;
  float *d_hist;       // channels * 2 frames: the last 1024 PCM samples of each channel
  float *d_buf = nullptr;
  uint8_t *d_units = nullptr;
  uint8_t *d_given = nullptr;      // mode bytes of a push with given modes (c1_enc_stream_push_modes), cap_frames * channels
  uint8_t *d_bias = nullptr;       // bias index bytes of a push with a palette (c1_enc_stream_push_biases), cap_frames * channels
  void *d_meas = nullptr;          // the per-unit outputs of a measured push (c1_enc_stream_push_measured), meas_units units
  int64_t meas_units = 0;
  int64_t cap_frames = 0;
  int64_t pushed = 0;              // frames per channel encoded so far
  EncHistory hist = HIST_PREV;     // where the detection history of the next frame lives (same for every channel)
  float *d_stored = nullptr;       // channels x 512: the bands of the last detected frame (HIST_STORED), from d_sw's block
  void *d_sw_block = nullptr;
  EncSwitchScratch sw;
  float *d_state = nullptr;        // channels x c1_enc_state, then the same again as scratch, then one zero state per channel
  int state_frames = 0;            // frames still to be encoded from d_state (2 after a restore)
  bool state_live = false;         // d_state is the stream's whole current state (nothing was pushed on the usual path since)
};

namespace {
bool opts_detect(const c1_encode_options &o) { return o.fixed_block_modes[0] < 0; }

int enc_stream_scratch(c1_enc_stream *s) {
  if (s->d_sw_block) return C1_OK;
  const size_t C = (size_t)s->channels;
  size_t at = 0;
  auto take = [&](size_t bytes) { const size_t here = at; at += (bytes + 255) & ~(size_t)255; return here; };
  const size_t o_stored = take(C * 512 * 4), o_bands = take(2 * C * 512 * 4), o_coefs = take(2 * C * 512 * 4),
               o_side = take(2 * C * kSideBytes), o_alloc = take(2 * C * kAllocBytes), o_rows = take(2 * 512 * 4),
               o_mags = take(2 * 256 * 4), o_modes = take(C * 3 * 4), o_mb = take(1), o_lists = take(6 * 4), o_c1 = take(512 * 4),
               o_s1 = take(kSideBytes), o_a1 = take(kAllocBytes), o_k1 = take(kCandidateBytes), o_w1 = take((4 + 8) * 4),
               o_n = take(4), o_sfi = take(52 * 4), o_wl = take(52 * 4), o_q = take(512 * 4);
  void *block = nullptr;
  HIP_TRY(hipMalloc(&block, at));
  char *b = static_cast<char *>(block);
  s->d_sw_block = block;
  s->d_stored = reinterpret_cast<float *>(b + o_stored);
  EncSwitchScratch &w = s->sw;
  w.bands = reinterpret_cast<float *>(b + o_bands);
  w.coefs = reinterpret_cast<float *>(b + o_coefs);
  w.side = reinterpret_cast<uint8_t *>(b + o_side);
  w.alloc = reinterpret_cast<uint8_t *>(b + o_alloc);
  w.rows = reinterpret_cast<float *>(b + o_rows);
  w.mags = reinterpret_cast<float *>(b + o_mags);
  w.modes = reinterpret_cast<int32_t *>(b + o_modes);
  w.mode_byte = reinterpret_cast<uint8_t *>(b + o_mb);
  w.lists = reinterpret_cast<uint32_t *>(b + o_lists);
  w.coef1 = reinterpret_cast<float *>(b + o_c1);
  w.side1 = reinterpret_cast<uint8_t *>(b + o_s1);
  w.alloc1 = reinterpret_cast<uint8_t *>(b + o_a1);
  w.cand1 = reinterpret_cast<uint8_t *>(b + o_k1);
  w.work1 = reinterpret_cast<uint32_t *>(b + o_w1);
  w.nbfu = reinterpret_cast<int32_t *>(b + o_n);
  w.sfi = reinterpret_cast<int32_t *>(b + o_sfi);
  w.wl = reinterpret_cast<int32_t *>(b + o_wl);
  w.q = reinterpret_cast<int32_t *>(b + o_q);
  return C1_OK;
}

// QMF analysis of `frames` frames of every channel (pcm[c] at the first, `halo` frames of PCM before it) into s->sw.bands,
// channels interleaved: the encoder's own bands tap (c1_qmf_analysis_batch's path), run with the stream's detection options
// so that the options on the device stay as they are.  Device pointers, ordered on the context's stream.
int enc_stream_bands(c1_enc_stream *s, const float *const *pcm, int64_t frames, int halo) {
  return encode_device_impl(s->ctx, pcm, s->channels, frames, halo, &s->opts, nullptr, s->sw.bands, s->sw.coefs, s->sw.side,
                            s->sw.alloc);
}

// The first frame t of a push under detection while the history is not the previous frame's: pcm[c] points at frame t with two
// frames of history before it.  The reference's stages on the device, channel by channel: bands of t-1 and t (halo 1),
// blockSelectorStage against the stored bands or a fresh pool's zeros, mdctStage with t-1's bands as the overlap,
// quantizationStage, serializeFrame -> units[c * 212].
// per_channel: when not null, channel c's allocation runs under per_channel[c] (the stream's options with another bias table)
// mc: when not null, the measured allocation of channel c (output row c) runs between its allocation and its fields
int enc_stream_switch_frame(c1_enc_stream *s, const float *const *pcm, uint8_t *units, const c1_encode_options *per_channel = nullptr,
                            const MeasuredCall *mc = nullptr) {
  c1_ctx *ctx = s->ctx;
  EncSwitchScratch &w = s->sw;
  const int C = s->channels;
  const float *prev[C1_MAX_CHANNELS] = {nullptr, nullptr};
  for (int c = 0; c < C; c++) prev[c] = pcm[c] - 512;
  int rc = enc_stream_bands(s, prev, 2, 1);            // also puts s->opts on the device, which the allocation reads
  if (rc) return rc;
  for (int c = 0; c < C; c++) {
    const float *bands_prev = w.bands + (size_t)c * 512, *bands_t = w.bands + (size_t)(C + c) * 512;
    int32_t *modes = w.modes + 3 * c;
    const int halo = s->hist == HIST_STORED ? 1 : 0;
    if (halo) HIP_TRY(hipMemcpyAsync(w.rows, s->d_stored + (size_t)c * 512, 512 * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(w.rows + 512 * halo, bands_t, 512 * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
    c1k_launch_block_modes_from_bands(ctx->d_tables, w.rows, 1, halo, s->opts.transient_threshold, w.mags, modes, ctx->stream);
    HIP_TRY(hipMemcpyAsync(w.rows, bands_prev, 512 * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(w.rows + 512, bands_t, 512 * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
    c1k_launch_stage_mode_lists(modes, 1, w.mode_byte, w.lists, ctx->stream);
    C1EncodeLaunch L;
    memset(&L, 0, sizeof L);
    L.channels = 1;
    L.frames = 1;
    L.halo_frames = 1;
    L.tables = ctx->d_tables;
    L.opts = ctx->d_opts;
    L.coefs = w.coef1;
    L.side = w.side1;
    c1k_launch_mdct_bands(L, w.rows, w.mode_byte, w.lists, ctx->stream);
    c1k_launch_stage_scale_factors(ctx->d_tables, w.coef1, modes, 1, w.side1, ctx->stream);
    L.alloc = w.alloc1;
    L.cand = w.cand1;
    L.work_count = w.work1;
    L.work_list = w.work1 + 4;
    L.sel_list = w.work1 + 4 + 7;
    if (per_channel && (rc = upload_opts(ctx, &per_channel[c]))) return rc;
    c1k_launch_allocate(L, ctx->stream);
    if (mc) {
      // the measured kernel takes the unit's modes from the side record, where k_stage_scale_factors left zeros; a taken unit's
      // allocation record and scale-factor bytes are rewritten in place, and k_stage_fields reads both
      HIP_TRY(hipMemcpyAsync(w.side1 + 52, w.mode_byte, 1, hipMemcpyDeviceToDevice, ctx->stream));
      L.units = units + (size_t)c * C1_UNIT_BYTES;             // the launch packs: the records are finalized
      launch_measured(ctx, L, false, mc, c, ctx->stream);
    }
    c1k_launch_stage_fields(ctx->d_tables, w.coef1, modes, w.side1, w.alloc1, 1, w.nbfu, w.sfi, w.wl, w.q, ctx->stream);
    c1k_launch_pack_units(w.nbfu, modes, w.sfi, w.wl, w.q, 1, units + (size_t)c * C1_UNIT_BYTES, ctx->stream);
    HIP_TRY(hipGetLastError());
  }
  return C1_OK;
}

// ---- the frame closures over explicit pools (c1_k_state.hip) ---------------------------------------------------------
constexpr int kEncStateFloats = (int)(sizeof(c1_enc_state) / sizeof(float)), kDecStateFloats = (int)(sizeof(c1_dec_state) / sizeof(float));
constexpr int64_t kMaxStatePools = (int64_t)1 << 27;
constexpr int64_t kStateDecodeChunk = 65536;      // pools whose unpacked fields (2.4 KB each) one decode launch keeps in scratch

// n pools on the context's stream: the from-state kernel into the workspace, then the encoder's own allocation and packing
// kernels on it (one unit per pool).  Device pointers; pool i reads pcm + i * pcm_stride.  out may be in, or null.
// mc: when not null, the measured allocation of pool i (output row mc_at + i) runs between its allocation and packing
int encode_from_states_impl(c1_ctx *ctx, int64_t n, const float *pcm, int64_t pcm_stride, const float *in,
                            const c1_encode_options *opts, uint8_t *units, float *out, const MeasuredCall *mc = nullptr,
                            int64_t mc_at = 0) {
  int rc;
  if ((rc = upload_opts(ctx, opts))) return rc;
  if (ctx->profiling && ctx->timing_depth == 0) reset_timings(ctx);
  if (n == 0) return C1_OK;
  if ((rc = join_tail(ctx))) return rc;
  const int64_t chunk = chunk_for_call(ctx, n, 1, false);
  if ((rc = ensure_workspace(ctx, std::min(n, chunk)))) return rc;
  for (int64_t n0 = 0; n0 < n; n0 += chunk) {
    const int64_t m = std::min(chunk, n - n0);
    C1EncStateLaunch K;
    memset(&K, 0, sizeof K);
    K.pcm = pcm + n0 * pcm_stride;
    K.pcm_stride = pcm_stride;
    K.in = in + n0 * kEncStateFloats;
    K.out = out ? out + n0 * kEncStateFloats : nullptr;
    K.n = m;
    K.tables = ctx->d_tables;
    K.opts = ctx->d_opts;
    K.coefs = ctx->d_coefs[0];
    K.side = ctx->d_side[0];
    K.detect = -1;
    { ScopedTiming t(ctx, K_FROM_STATE); c1k_launch_encode_from_states(K, ctx->stream); }
    C1EncodeLaunch L;
    memset(&L, 0, sizeof L);
    L.channels = 1;
    L.frames = m;
    L.tables = ctx->d_tables;
    L.opts = ctx->d_opts;
    L.coefs = ctx->d_coefs[0];
    L.side = ctx->d_side[0];
    L.alloc = ctx->d_alloc[0];
    L.cand = ctx->d_cand[0];
    L.work_count = ctx->d_work[0];
    L.work_list = ctx->d_work[0] + 4;
    L.sel_list = ctx->d_work[0] + 4 + (size_t)ctx->ws_units * 7;
    L.units = units + n0 * C1_UNIT_BYTES;
    { ScopedTiming t(ctx, K_ALLOCATE); c1k_launch_allocate(L, ctx->stream); }
    if (mc) launch_measured(ctx, L, false, mc, mc_at + n0, ctx->stream);   // the side records carry the pools' mode bytes
    { ScopedTiming t(ctx, K_PACK); c1k_launch_pack(L, false, ctx->stream); }
  }
  HIP_TRY(hipGetLastError());
  return C1_OK;
}

// a mode-search call's outputs from unit `at` on
void bm_outputs_at(const BestModesCall &bm, int64_t at, BestModesCall *part) {
  *part = bm;
  if (part->choice) part->choice += at;
  if (part->modes_out) part->modes_out += at;
  if (part->taken) part->taken += at;
  if (part->shifts) part->shifts += at * 52;
  if (part->distortion) part->distortion += at * bm.n * 2;
  if (part->energy) part->energy += at * bm.n;
  if (part->weights) part->weights += at * 52;
}

// the options of a call whose modes are the candidates': neither threshold nor fixed modes are read
void modes_call_opts(const c1_encode_options &opts, c1_encode_options *base) {
  *base = opts;
  base->transient_threshold = 1.0;
  base->fixed_block_modes[0] = base->fixed_block_modes[1] = base->fixed_block_modes[2] = -1;
}

// encode_from_states_impl with the mode search of c1_encode_measured_modes_device (bm, offsets set, outputs at its pointers): the
// front end of that call on the from-state workspace.  The from-state kernel runs under all-long options into the workspace's
// planes and under all-short options into the mode search's own (a plane no candidate needs is not made); the pools advance once,
// with the last of the two (delay lines and overlap do not depend on the modes, and under fixed modes the magnitudes stay).  Then
// per candidate the composed side record and the allocation into its trial records, launch_measured_modes, packing.  n is a
// stream's channel count: one chunk
int encode_from_states_modes(c1_ctx *ctx, int64_t n, const float *pcm, int64_t pcm_stride, float *state, const c1_encode_options *base,
                             uint8_t *units, const BestModesCall *bm) {
  int rc;
  bool bm_long = false, bm_short = false;                      // some candidate codes a band long / short
  for (int k = 0; k < bm->n; k++) {
    if ((bm->cand[k] & 0x3f) != 0x3a) bm_long = true;
    if ((bm->cand[k] & 0x3f) != 0) bm_short = true;
  }
  if (bm->mask) bm_long = true;                                // the weights come from the all-long analysis, whatever the candidates
  if ((rc = join_tail(ctx))) return rc;
  if ((rc = ensure_workspace(ctx, n))) return rc;
  if ((rc = ensure_trial_allocs(ctx, n, bm->n))) return rc;
  if ((rc = ensure_best_modes_planes(ctx, n))) return rc;
  bool first = true;
  for (int pass = 0; pass < 2; pass++) {                       // 0: all long, 1: all short
    if (!(pass ? bm_short : bm_long)) continue;
    c1_encode_options one = *base;
    one.fixed_block_modes[0] = one.fixed_block_modes[1] = pass ? 2 : 0;
    one.fixed_block_modes[2] = pass ? 3 : 0;
    if ((rc = upload_opts(ctx, &one))) return rc;
    if (first && ctx->profiling && ctx->timing_depth == 0) reset_timings(ctx);
    first = false;
    C1EncStateLaunch K;
    memset(&K, 0, sizeof K);
    K.pcm = pcm;
    K.pcm_stride = pcm_stride;
    K.in = state;
    K.out = (pass == 1 || !bm_short) ? state : nullptr;        // the last pass leaves the pools
    K.n = n;
    K.tables = ctx->d_tables;
    K.opts = ctx->d_opts;
    K.coefs = pass ? ctx->d_bm_coefs : ctx->d_coefs[0];
    K.side = pass ? ctx->d_bm_side : ctx->d_side[0];
    K.detect = -1;
    ScopedTiming t(ctx, K_FROM_STATE);
    c1k_launch_encode_from_states(K, ctx->stream);
  }
  C1EncodeLaunch L;
  memset(&L, 0, sizeof L);
  L.channels = 1;
  L.frames = n;
  L.tables = ctx->d_tables;
  L.opts = ctx->d_opts;
  L.coefs = ctx->d_coefs[0];
  L.side = ctx->d_side[0];
  L.alloc = ctx->d_alloc[0];
  L.cand = ctx->d_cand[0];
  L.work_count = ctx->d_work[0];
  L.work_list = ctx->d_work[0] + 4;
  L.sel_list = ctx->d_work[0] + 4 + (size_t)ctx->ws_units * 7;
  L.units = units;
  const int64_t trial_stride = ctx->trial_units * kAllocBytes;
  for (int k = 0; k < bm->n; k++) {                            // one chain after the other: they share the side plane and the scratch
    { ScopedTiming t(ctx, K_ANALYSIS); c1k_launch_compose_side(L.side, ctx->d_bm_side, n, bm->cand[k], ctx->d_bm_cand_side, ctx->stream); }
    ScopedTiming t(ctx, K_ALLOCATE);
    C1EncodeLaunch A = L;
    A.side = ctx->d_bm_cand_side;
    A.alloc = ctx->d_trial + (size_t)k * trial_stride;
    c1k_launch_allocate(A, ctx->stream);
  }
  launch_measured_modes(ctx, L, ctx->d_trial, trial_stride, bm, 0, ctx->stream);
  { ScopedTiming t(ctx, K_PACK); c1k_launch_pack(L, false, ctx->stream); }
  HIP_TRY(hipGetLastError());
  return C1_OK;
}

// the first non-finite entry of `count` states of `floats` floats each: C1_ERR_ARG naming pool (or channel) and field
struct StateField { const char *name; int first, count; };
const StateField kEncStateFields[] = {{"qmf_low", 0, 46}, {"qmf_mid", 46, 46}, {"qmf_high", 92, 39}, {"mdct_overlap", 131, 96}, {"transient_mags", 227, 256}};
const StateField kDecStateFields[] = {{"qmf_low", 0, 46}, {"qmf_mid", 46, 46}, {"qmf_high", 92, 39}, {"imdct_tail", 131, 48}};
int check_states_finite(const char *what, const char *unit, const void *states, int64_t count, int floats, const StateField *fields, int n_fields) {
  const uint32_t *w = static_cast<const uint32_t *>(states);
  for (int64_t i = 0; i < count; i++)
    for (int k = 0; k < floats; k++)
      if ((w[i * floats + k] & 0x7f800000u) == 0x7f800000u) {
        for (int f = 0; f < n_fields; f++)
          if (k >= fields[f].first && k < fields[f].first + fields[f].count)
            return fail(C1_ERR_ARG, "%s: %s %lld: %s[%d] is not finite", what, unit, (long long)i, fields[f].name, k - fields[f].first);
      }
  return C1_OK;
}

int enc_stream_state_buffer(c1_enc_stream *s) {
  if (s->d_state) return C1_OK;
  const size_t bytes = 3 * (size_t)s->channels * sizeof(c1_enc_state);
  HIP_TRY(hipMalloc(&s->d_state, bytes));
  HIP_TRY(hipMemsetAsync(s->d_state, 0, bytes, s->ctx->stream));
  return C1_OK;
}

// d_state <- the pool the reference would hold now, for a stream on the usual path: delay lines and overlap from the two
// history frames (the from-state kernel, state output only, from a zero state: what a frame leaves is a function of that
// frame and the 138 samples before it), the magnitudes from wherever the stream's EncHistory says they live
int enc_stream_current_state(c1_enc_stream *s) {
  if (s->state_live) return C1_OK;
  c1_ctx *ctx = s->ctx;
  int rc = enc_stream_state_buffer(s);
  if (rc) return rc;
  const int C = s->channels;
  float *cur = s->d_state, *tmp = cur + (size_t)C * kEncStateFloats, *zero = tmp + (size_t)C * kEncStateFloats;
  C1EncStateLaunch K;
  memset(&K, 0, sizeof K);
  K.pcm = s->d_hist;
  K.pcm_stride = 1024;
  K.in = zero;
  K.out = tmp;
  K.n = C;
  K.tables = ctx->d_tables;
  K.opts = ctx->d_opts;
  K.state_only = 1;
  c1k_launch_encode_from_states(K, ctx->stream);
  K.pcm = s->d_hist + 512;
  K.in = tmp;
  K.detect = s->hist == HIST_PREV ? 1 : 0;     // the last pushed frame's own spectrum; else the zero state's zeros pass through
  c1k_launch_encode_from_states(K, ctx->stream);
  if (s->hist == HIST_STORED) c1k_launch_state_mags(ctx->d_tables, s->d_stored, C, tmp, ctx->stream);
  else if (s->hist == HIST_MAGS)
    HIP_TRY(hipMemcpy2DAsync(tmp + offsetof(c1_enc_state, transient_mags) / sizeof(float), sizeof(c1_enc_state),
                             cur + offsetof(c1_enc_state, transient_mags) / sizeof(float), sizeof(c1_enc_state),
                             sizeof(((c1_enc_state *)0)->transient_mags), (size_t)C, hipMemcpyDeviceToDevice, ctx->stream));
  HIP_TRY(hipMemcpyAsync(cur, tmp, (size_t)C * sizeof(c1_enc_state), hipMemcpyDeviceToDevice, ctx->stream));
  HIP_TRY(hipGetLastError());
  s->state_live = true;
  return C1_OK;
}

// detection -> fixed modes on the usual path (nothing left to encode from d_state): the detection history freezes at the last
// frame detection ran on.  HIST_PREV: that is the last pushed frame; its bands are kept (or there is none: a fresh pool's zeros)
int enc_stream_freeze_history(c1_enc_stream *s) {
  if (s->hist != HIST_PREV) return C1_OK;
  if (s->pushed == 0) { s->hist = HIST_ZEROS; return C1_OK; }
  int rc = enc_stream_scratch(s);
  if (rc) return rc;
  const float *last[C1_MAX_CHANNELS] = {nullptr, nullptr};
  for (int c = 0; c < s->channels; c++) last[c] = s->d_hist + 1024 * c + 512;
  if ((rc = enc_stream_bands(s, last, 1, 1))) return rc;
  HIP_TRY(hipMemcpyAsync(s->d_stored, s->sw.bands, (size_t)s->channels * 512 * sizeof(float), hipMemcpyDeviceToDevice, s->ctx->stream));
  HIP_TRY(hipStreamSynchronize(s->ctx->stream));
  s->hist = HIST_STORED;
  return C1_OK;
}

int enc_stream_push_impl(c1_enc_stream *s, const float *const *pcm, int64_t frames, const uint8_t *modes, uint8_t *units,
                         const c1_encode_options *palette = nullptr, int n_palette = 0, const uint8_t *bias_index = nullptr,
                         const MeasuredCall *mc = nullptr, const MeasuredCall *mc_host = nullptr, const BestModesCall *bm = nullptr,
                         const BestModesCall *bm_host = nullptr);
}  // namespace

int c1_enc_stream_create(c1_ctx *ctx, int channels, const c1_encode_options *opts, c1_enc_stream **out) {
  CTX_GUARD(ctx);
  int rc = ctx_bind(ctx);
  if (rc) return rc;
  if (!out || !opts) return fail(C1_ERR_ARG, "out or opts is NULL");
  if ((rc = check_channels(channels))) return rc;
  C1DevEncOpts probe;
  if ((rc = build_encode_opts(*opts, &probe))) return rc;
  c1_enc_stream *s = new c1_enc_stream();
  s->ctx = ctx; s->channels = channels; s->opts = *opts; s->d_hist = nullptr;
  s->hist = opts_detect(*opts) ? HIST_PREV : HIST_ZEROS;
  const size_t hb = (size_t)channels * 1024 * sizeof(float);
  hipError_t e = hipMalloc(&s->d_hist, hb);
  if (e == hipSuccess) e = hipMemsetAsync(s->d_hist, 0, hb, ctx->stream);   // zero history == stream start
  if (e != hipSuccess) { delete s; return fail(C1_ERR_HIP, "enc stream alloc: %s", hipGetErrorString(e)); }
  *out = s;
  return C1_OK;
}

int c1_enc_stream_set_options(c1_enc_stream *s, const c1_encode_options *opts) {
  if (!s) return fail(C1_ERR_ARG, "stream is NULL");
  c1_ctx *ctx = s->ctx;
  CTX_GUARD(ctx);
  int rc = ctx_bind(ctx);
  if (rc) return rc;
  if (!opts) return fail(C1_ERR_ARG, "opts is NULL");
  C1DevEncOpts probe;
  if ((rc = build_encode_opts(*opts, &probe))) return rc;
  if (s->state_frames > 0) {
    // the pool is explicit (d_state): the from-state kernel reads the options frame by frame, as the reference does
    s->opts = *opts;
    return C1_OK;
  }
  if (opts_detect(s->opts) && !opts_detect(*opts) && (rc = enc_stream_freeze_history(s))) return rc;
  s->opts = *opts;
  return C1_OK;
}

int c1_enc_stream_push(c1_enc_stream *s, const float *const *pcm, int64_t frames, uint8_t *units) {
  return enc_stream_push_impl(s, pcm, frames, nullptr, units);
}

int c1_enc_stream_push_modes(c1_enc_stream *s, const float *const *pcm, int64_t frames, const uint8_t *modes, uint8_t *units) {
  if (!modes && frames > 0) return fail(C1_ERR_ARG, "modes is NULL");
  return enc_stream_push_impl(s, pcm, frames, modes, units);
}

int c1_enc_stream_push_biases(c1_enc_stream *s, const float *const *pcm, int64_t frames, const c1_encode_options *palette,
                              int n_palette, const uint8_t *bias_index, const uint8_t *modes, uint8_t *units) {
  int rc = check_palette("c1_enc_stream_push_biases", palette, n_palette, false);
  if (rc) return rc;
  if (!bias_index && frames > 0) return fail(C1_ERR_ARG, "bias_index is NULL");
  return enc_stream_push_impl(s, pcm, frames, modes, units, palette, n_palette, bias_index);
}

// the staging of a measured push's per-unit outputs: one block of kMeasBlockBytes per unit, grown to the largest push so far
constexpr size_t kMeasBlockBytes = 52 * sizeof(double) + 3 * sizeof(double) + 52 + 8;
static int enc_stream_meas_block(c1_enc_stream *s, int64_t n_units) {
  if (n_units <= s->meas_units) return C1_OK;
  HIP_TRY(hipStreamSynchronize(s->ctx->stream));
  if (s->d_meas) (void)hipFree(s->d_meas);
  s->d_meas = nullptr; s->meas_units = 0;
  HIP_TRY(hipMalloc(&s->d_meas, (size_t)n_units * kMeasBlockBytes));
  s->meas_units = n_units;
  return C1_OK;
}

int c1_enc_stream_push_measured(c1_enc_stream *s, const float *const *pcm, int64_t frames, const uint8_t *modes,
                                const int8_t *sf_offsets, int n_offsets, const double *mask_floor, const double *mask_spread,
                                uint8_t *units, uint8_t *taken, int8_t *shifts, double *distortion, double *energy, double *weights) {
  // everything the arguments alone decide comes first and needs neither a stream nor a device
  const char *const what = "c1_enc_stream_push_measured";
  int rc;
  if (mask_spread && !mask_floor) return fail(C1_ERR_ARG, "%s: mask_spread is given without mask_floor", what);
  if (weights && !mask_floor) return fail(C1_ERR_ARG, "%s: weights is given without mask_floor", what);
  if (!sf_offsets && n_offsets != 0) return fail(C1_ERR_ARG, "%s: n_offsets = %d, but sf_offsets is NULL", what, n_offsets);
  if (sf_offsets && (rc = check_sf_offsets(what, sf_offsets, n_offsets))) return rc;
  if (mask_floor && (rc = check_masking(what, mask_floor, mask_spread))) return rc;
  if (!s) return fail(C1_ERR_ARG, "stream is NULL");
  c1_ctx *ctx = s->ctx;
  CTX_GUARD(ctx);
  if ((rc = ctx_bind(ctx))) return rc;
  if (frames < 0) return fail(C1_ERR_ARG, "frames must be >= 0");
  if (frames > kMaxModesBatchFrames) return fail(C1_ERR_ARG, "at most %lld frames per call", (long long)kMaxModesBatchFrames);
  if ((rc = check_measured_opts(what, &s->opts, modes == nullptr))) return rc;
  if (frames == 0) return C1_OK;
  if (!pcm || !units) return fail(C1_ERR_ARG, "pcm or units is NULL");
  for (int c = 0; c < s->channels; c++)
    if (!pcm[c]) return fail(C1_ERR_ARG, "pcm[%d] is NULL", c);
  if (modes && (rc = check_mode_bytes(what, modes, frames, s->channels))) return rc;
  // from here on only the device can fail.  The outputs' staging: one block, grown to the largest push so far
  const int64_t n_units = frames * s->channels;
  if ((rc = enc_stream_meas_block(s, n_units))) return rc;
  char *block = static_cast<char *>(s->d_meas);
  const size_t cap = (size_t)s->meas_units;
  double *d_weights = reinterpret_cast<double *>(block), *d_dist = d_weights + cap * 52, *d_energy = d_dist + cap * 2;
  int8_t *d_shifts = reinterpret_cast<int8_t *>(d_energy + cap);
  uint8_t *d_taken = reinterpret_cast<uint8_t *>(d_shifts + cap * 52);
  static const int8_t kOwnIndex[1] = {0};                      // tables without offsets: the masked call with the single offset 0
  MeasuredCall mc = {taken ? d_taken : nullptr, distortion ? d_dist : nullptr, energy ? d_energy : nullptr};
  if (sf_offsets || mask_floor) {
    mc.sf_offsets = sf_offsets ? sf_offsets : kOwnIndex;
    mc.n_offsets = sf_offsets ? n_offsets : 1;
    mc.shifts = shifts ? d_shifts : nullptr;
  }
  if (mask_floor) {
    if ((rc = upload_masking(ctx, mask_floor, mask_spread))) return rc;
    mc.mask = ctx->d_mask;
    mc.has_spread = mask_spread != nullptr;
    mc.weights = weights ? d_weights : nullptr;
  }
  MeasuredCall host = {taken, distortion, energy};
  host.shifts = shifts;
  host.weights = weights;
  if ((rc = enc_stream_push_impl(s, pcm, frames, modes, units, nullptr, 0, nullptr, &mc, &host))) return rc;
  if (shifts && !mc.shifts) memset(shifts, 0, (size_t)n_units * 52);   // c1_encode_measured_*: no index moves
  return C1_OK;
}

int c1_enc_stream_push_measured_modes(c1_enc_stream *s, const float *const *pcm, int64_t frames, const uint8_t *cand_modes, int n_cand,
                                      const int8_t *sf_offsets, int n_offsets, uint8_t *units, uint8_t *choice, uint8_t *modes_out,
                                      uint8_t *taken, int8_t *shifts, double *distortion, double *energy) {
  // everything the arguments alone decide comes first and needs neither a stream nor a device
  const char *const what = "c1_enc_stream_push_measured_modes";
  int rc;
  if (frames < 0) return fail(C1_ERR_ARG, "%s: frames must be >= 0", what);
  if (frames > kMaxModesBatchFrames) return fail(C1_ERR_ARG, "%s: at most %lld frames per call", what, (long long)kMaxModesBatchFrames);
  if ((rc = check_mode_candidates(what, cand_modes, n_cand))) return rc;
  if (!sf_offsets && n_offsets != 0) return fail(C1_ERR_ARG, "%s: n_offsets = %d, but sf_offsets is NULL", what, n_offsets);
  if (sf_offsets && (rc = check_sf_offsets(what, sf_offsets, n_offsets))) return rc;
  if (frames > 0 && (!pcm || !units)) return fail(C1_ERR_ARG, "%s: pcm or units is NULL", what);
  if (!s) return fail(C1_ERR_ARG, "%s: stream is NULL", what);
  c1_ctx *ctx = s->ctx;
  CTX_GUARD(ctx);
  if ((rc = ctx_bind(ctx))) return rc;
  if ((rc = check_measured_opts(what, &s->opts, false))) return rc;
  if (frames == 0) return C1_OK;
  for (int c = 0; c < s->channels; c++)
    if (!pcm[c]) return fail(C1_ERR_ARG, "%s: pcm[%d] is NULL", what, c);
  // from here on only the device can fail.  The outputs' staging: c1_enc_stream_push_measured's block, which holds these as well
  static_assert(kMeasBlockBytes >= C1_MAX_MODE_CANDIDATES * 3 * sizeof(double) + 52 + 3, "the staging block holds a mode search's outputs");
  const int64_t n_units = frames * s->channels;
  if ((rc = enc_stream_meas_block(s, n_units))) return rc;
  const size_t cap = (size_t)s->meas_units;
  double *d_dist = static_cast<double *>(s->d_meas), *d_energy = d_dist + cap * C1_MAX_MODE_CANDIDATES * 2;
  int8_t *d_shifts = reinterpret_cast<int8_t *>(d_energy + cap * C1_MAX_MODE_CANDIDATES);
  uint8_t *d_choice = reinterpret_cast<uint8_t *>(d_shifts + cap * 52), *d_modes = d_choice + cap, *d_taken = d_modes + cap;
  static const int8_t kOwnIndex[1] = {0};                      // no offsets: the search over the plain measured allocation
  uint8_t cand[C1_MAX_MODE_CANDIDATES];                        // the caller's arrays may change while the call runs
  int8_t offs[C1_MAX_SF_OFFSETS];
  memcpy(cand, cand_modes, (size_t)n_cand);
  if (sf_offsets) memcpy(offs, sf_offsets, (size_t)n_offsets);
  BestModesCall bm = {n_cand, cand, choice ? d_choice : nullptr, modes_out ? d_modes : nullptr, distortion ? d_dist : nullptr,
                      energy ? d_energy : nullptr};
  bm.sf_offsets = sf_offsets ? offs : kOwnIndex;
  bm.n_offsets = sf_offsets ? n_offsets : 1;
  bm.taken = taken ? d_taken : nullptr;
  bm.shifts = shifts ? d_shifts : nullptr;                     // a single offset 0 moves no index: zeros
  BestModesCall host = {n_cand, cand, choice, modes_out, distortion, energy};
  host.taken = taken;
  host.shifts = shifts;
  return enc_stream_push_impl(s, pcm, frames, nullptr, units, nullptr, 0, nullptr, nullptr, nullptr, &bm, &host);
}

int c1_enc_stream_push_measured_modes_masked(c1_enc_stream *s, const float *const *pcm, int64_t frames, const uint8_t *cand_modes, int n_cand,
                                             const int8_t *sf_offsets, int n_offsets, const double *mask_floor, const double *mask_spread,
                                             uint8_t *units, uint8_t *choice, uint8_t *modes_out, uint8_t *taken, int8_t *shifts,
                                             double *distortion, double *energy, double *weights) {
  // everything the arguments alone decide comes first and needs neither a stream nor a device
  const char *const what = "c1_enc_stream_push_measured_modes_masked";
  int rc;
  if (frames < 0) return fail(C1_ERR_ARG, "%s: frames must be >= 0", what);
  if (frames > kMaxModesBatchFrames) return fail(C1_ERR_ARG, "%s: at most %lld frames per call", what, (long long)kMaxModesBatchFrames);
  if ((rc = check_mode_candidates(what, cand_modes, n_cand))) return rc;
  if (!sf_offsets && n_offsets != 0) return fail(C1_ERR_ARG, "%s: n_offsets = %d, but sf_offsets is NULL", what, n_offsets);
  if (sf_offsets && (rc = check_sf_offsets(what, sf_offsets, n_offsets))) return rc;
  if ((rc = check_masking(what, mask_floor, mask_spread))) return rc;
  if (frames > 0 && (!pcm || !units)) return fail(C1_ERR_ARG, "%s: pcm or units is NULL", what);
  if (!s) return fail(C1_ERR_ARG, "%s: stream is NULL", what);
  c1_ctx *ctx = s->ctx;
  CTX_GUARD(ctx);
  if ((rc = ctx_bind(ctx))) return rc;
  if ((rc = check_measured_opts(what, &s->opts, false))) return rc;
  if (frames == 0) return C1_OK;
  for (int c = 0; c < s->channels; c++)
    if (!pcm[c]) return fail(C1_ERR_ARG, "%s: pcm[%d] is NULL", what, c);
  // from here on only the device can fail.  The outputs' staging: c1_enc_stream_push_measured's block, asked for twice the units:
  // that holds a search's outputs and the weights, laid out over this push's units
  constexpr size_t kBytes = 52 * sizeof(double) + C1_MAX_MODE_CANDIDATES * 3 * sizeof(double) + 52 + 3;
  static_assert(2 * kMeasBlockBytes >= kBytes, "two staging blocks hold a weighted mode search's outputs");
  const int64_t n_units = frames * s->channels;
  if ((rc = enc_stream_meas_block(s, 2 * n_units))) return rc;
  const size_t cap = (size_t)n_units;
  double *d_weights = static_cast<double *>(s->d_meas), *d_dist = d_weights + cap * 52, *d_energy = d_dist + cap * C1_MAX_MODE_CANDIDATES * 2;
  int8_t *d_shifts = reinterpret_cast<int8_t *>(d_energy + cap * C1_MAX_MODE_CANDIDATES);
  uint8_t *d_choice = reinterpret_cast<uint8_t *>(d_shifts + cap * 52), *d_modes = d_choice + cap, *d_taken = d_modes + cap;
  static const int8_t kOwnIndex[1] = {0};                      // no offsets: the search over the plain measured allocation
  uint8_t cand[C1_MAX_MODE_CANDIDATES];                        // the caller's arrays may change while the call runs
  int8_t offs[C1_MAX_SF_OFFSETS];
  memcpy(cand, cand_modes, (size_t)n_cand);
  if (sf_offsets) memcpy(offs, sf_offsets, (size_t)n_offsets);
  if ((rc = upload_masking(ctx, mask_floor, mask_spread))) return rc;
  BestModesCall bm = {n_cand, cand, choice ? d_choice : nullptr, modes_out ? d_modes : nullptr, distortion ? d_dist : nullptr,
                      energy ? d_energy : nullptr};
  bm.sf_offsets = sf_offsets ? offs : kOwnIndex;
  bm.n_offsets = sf_offsets ? n_offsets : 1;
  bm.taken = taken ? d_taken : nullptr;
  bm.shifts = shifts ? d_shifts : nullptr;                     // a single offset 0 moves no index: zeros
  bm.mask = ctx->d_mask;
  bm.has_spread = mask_spread != nullptr;
  bm.weights = weights ? d_weights : nullptr;
  BestModesCall host = {n_cand, cand, choice, modes_out, distortion, energy};
  host.taken = taken;
  host.shifts = shifts;
  host.weights = weights;
  return enc_stream_push_impl(s, pcm, frames, nullptr, units, nullptr, 0, nullptr, nullptr, nullptr, &bm, &host);
}

namespace {
// modes null: the stream's options decide.  Else the frames behave as if the options had been switched to fixed block modes
// for them, frame by frame and channel by channel, and back afterwards: the detector does not run, and on a stream under
// detection its history stays where c1_enc_stream_set_options would have frozen it.
// palette non-null (c1_enc_stream_push_biases): unit u allocates under the table of palette[bias_index[u]] instead of the
// stream's; nothing else of the entries is read, and the stream's options and state are as after the same push without it
// bm non-null (c1_enc_stream_push_measured_modes, everything validated): the frames behave as under given modes, which the mode
// search of c1_encode_measured_modes_device chooses: that call's chain with halo 2 on the usual path, encode_from_states_modes
// for the frames encoded from the explicit state; there is no detection frame and no switch frame.  bm's outputs are device
// memory over the push's units and are copied to bm_host's with the units
// mc non-null (c1_enc_stream_push_measured, everything validated and the tables uploaded): the measured allocation runs between
// allocation and packing on whichever of the three paths a frame takes; mc's outputs are device memory over the push's units and
// are copied to mc_host's with the units.  It keeps no state: the stream is as after the same push without it
int enc_stream_push_impl(c1_enc_stream *s, const float *const *pcm, int64_t frames, const uint8_t *modes, uint8_t *units,
                         const c1_encode_options *palette, int n_palette, const uint8_t *bias_index, const MeasuredCall *mc,
                         const MeasuredCall *mc_host, const BestModesCall *bm, const BestModesCall *bm_host) {
  if (!s) return fail(C1_ERR_ARG, "stream is NULL");
  c1_ctx *ctx = s->ctx;
  CTX_GUARD(ctx);
  int rc = ctx_bind(ctx);
  if (rc) return rc;
  if (frames < 0) return fail(C1_ERR_ARG, "frames must be >= 0");
  if (frames == 0) return C1_OK;
  if (!pcm || !units) return fail(C1_ERR_ARG, "pcm or units is NULL");
  for (int c = 0; c < s->channels; c++)
    if (!pcm[c]) return fail(C1_ERR_ARG, "pcm[%d] is NULL", c);
  if (palette && (rc = check_index_bytes("c1_enc_stream_push_biases", bias_index, frames, s->channels, n_palette))) return rc;
  if (modes && (rc = check_mode_bytes(palette ? "c1_enc_stream_push_biases" : "c1_enc_stream_push_modes", modes, frames, s->channels))) return rc;   // the stream is as it was
  if (palette && (rc = upload_palette(ctx, "c1_enc_stream_push_biases", palette, n_palette))) return rc;
  if ((modes || bm) && opts_detect(s->opts) && s->state_frames == 0 && (rc = enc_stream_freeze_history(s))) return rc;
  const bool detect = !modes && !bm && opts_detect(s->opts);
  // frames of this push that are encoded from the explicit state: the first two after a restore, or the first under
  // detection when the detection history is a set of magnitudes only the state holds
  int64_t from_state = std::min<int64_t>(frames, s->state_frames);
  if (from_state == 0 && detect && s->hist == HIST_MAGS) {
    if ((rc = enc_stream_current_state(s))) return rc;
    from_state = 1;
  }
  const bool switch_frame = from_state == 0 && detect && s->hist != HIST_PREV && s->pushed > 0;
  if (switch_frame && (rc = enc_stream_scratch(s))) return rc;
  if (frames > s->cap_frames) {
    if (s->d_buf) { hipFree(s->d_buf); hipFree(s->d_units); hipFree(s->d_given); hipFree(s->d_bias); }
    s->d_buf = nullptr; s->d_units = nullptr; s->d_given = nullptr; s->d_bias = nullptr; s->cap_frames = 0;
    HIP_TRY(hipMalloc(&s->d_buf, (size_t)s->channels * (frames + 2) * 512 * sizeof(float)));
    HIP_TRY(hipMalloc(&s->d_units, (size_t)s->channels * frames * C1_UNIT_BYTES));
    HIP_TRY(hipMalloc(&s->d_given, (size_t)s->channels * frames));
    HIP_TRY(hipMalloc(&s->d_bias, (size_t)s->channels * frames));
    s->cap_frames = frames;
  }
  const size_t stride = (size_t)(s->cap_frames + 2) * 512;
  const float *dptr[C1_MAX_CHANNELS] = {nullptr, nullptr};
  for (int c = 0; c < s->channels; c++) {
    float *d = s->d_buf + stride * c;
    HIP_TRY(hipMemcpyAsync(d, s->d_hist + 1024 * c, 1024 * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(d + 1024, pcm[c], (size_t)frames * 512 * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    dptr[c] = d + 1024;
  }
  if (modes) HIP_TRY(hipMemcpyAsync(s->d_given, modes, (size_t)frames * s->channels, hipMemcpyHostToDevice, ctx->stream));
  if (palette) HIP_TRY(hipMemcpyAsync(s->d_bias, bias_index, (size_t)frames * s->channels, hipMemcpyHostToDevice, ctx->stream));
  // the options frame f of channel c is encoded under where a kernel takes one set per launch: the stream's, with the given
  // modes and the unit's palette table in their places
  auto unit_opts = [&](int64_t f, int c) {
    c1_encode_options one = s->opts;
    if (modes) {
      const int b = modes[f * s->channels + c];
      one.fixed_block_modes[0] = b & 3; one.fixed_block_modes[1] = (b >> 2) & 3; one.fixed_block_modes[2] = (b >> 4) & 3;
    }
    if (palette) memcpy(one.biased_scale_factors, palette[bias_index[f * s->channels + c]].biased_scale_factors, sizeof one.biased_scale_factors);
    return one;
  };
  // the frames that are not encoded from the explicit state: the stream's options, or the given modes in their place
  auto encode_rest = [&](const float *const *p, int64_t first, int64_t n) {
    uint8_t *out = s->d_units + (size_t)first * s->channels * C1_UNIT_BYTES;
    if (bm) {                                                  // c1_encode_measured_modes_device with halo 2, the outputs from unit first * channels on
      BestModesCall part;
      c1_encode_options base;
      bm_outputs_at(*bm, first * s->channels, &part);
      modes_call_opts(s->opts, &base);
      return encode_device_impl(ctx, p, s->channels, n, 2, &base, out, nullptr, nullptr, nullptr, nullptr, false, nullptr, nullptr, nullptr,
                                &part);
    }
    if (!modes && !palette && !mc) return encode_device_joined(ctx, p, s->channels, n, 2, &s->opts, out);
    MeasuredCall part;
    if (mc) {                                                  // the call's outputs from unit first * channels on
      const int64_t at = first * s->channels;
      part = *mc;
      if (part.taken) part.taken += at;
      if (part.shifts) part.shifts += at * 52;
      if (part.distortion) part.distortion += at * 2;
      if (part.energy) part.energy += at;
      if (part.weights) part.weights += at * 52;
    }
    const PaletteCall pc = {n_palette, palette ? s->d_bias + (size_t)first * s->channels : nullptr};
    return encode_device_impl(ctx, p, s->channels, n, 2, &s->opts, out, nullptr, nullptr, nullptr, nullptr, false,
                              modes ? s->d_given + (size_t)first * s->channels : nullptr, palette ? &pc : nullptr, nullptr, nullptr,
                              mc ? &part : nullptr);
  };
  if (from_state > 0) {
    for (int64_t f = 0; f < from_state; f++) {   // frame after frame: each continues the pool the one before left
      if (bm) {
        BestModesCall part;
        c1_encode_options base;
        bm_outputs_at(*bm, f * s->channels, &part);
        modes_call_opts(s->opts, &base);
        if ((rc = encode_from_states_modes(ctx, s->channels, dptr[0] + f * 512, (int64_t)stride, s->d_state, &base,
                                           s->d_units + (size_t)f * s->channels * C1_UNIT_BYTES, &part))) return rc;
        continue;
      }
      if (!modes && !palette) {
        if ((rc = encode_from_states_impl(ctx, s->channels, dptr[0] + f * 512, (int64_t)stride, s->d_state, &s->opts,
                                          s->d_units + (size_t)f * s->channels * C1_UNIT_BYTES, s->d_state, mc, f * s->channels))) return rc;
        continue;
      }
      for (int c = 0; c < s->channels; c++) {    // the from-state kernel takes one triple per launch: a pool at a time
        const c1_encode_options one = unit_opts(f, c);
        if ((rc = encode_from_states_impl(ctx, 1, dptr[c] + f * 512, (int64_t)stride, s->d_state + (size_t)c * kEncStateFloats, &one,
                                          s->d_units + (size_t)(f * s->channels + c) * C1_UNIT_BYTES,
                                          s->d_state + (size_t)c * kEncStateFloats, mc, f * s->channels + c))) return rc;
      }
    }
    if (frames > from_state) {
      const float *rest[C1_MAX_CHANNELS] = {nullptr, nullptr};
      for (int c = 0; c < s->channels; c++) rest[c] = dptr[c] + from_state * 512;
      if ((rc = encode_rest(rest, from_state, frames - from_state))) return rc;
    }
  } else if (switch_frame) {
    const c1_encode_options per_channel[C1_MAX_CHANNELS] = {unit_opts(0, 0), unit_opts(0, s->channels - 1)};
    if ((rc = enc_stream_switch_frame(s, dptr, s->d_units, palette ? per_channel : nullptr, mc))) return rc;
    if (frames > 1) {
      const float *rest[C1_MAX_CHANNELS] = {nullptr, nullptr};
      for (int c = 0; c < s->channels; c++) rest[c] = dptr[c] + 512;
      if ((rc = encode_rest(rest, 1, frames - 1))) return rc;
    }
  } else if ((rc = encode_rest(dptr, 0, frames))) {
    return rc;
  }
  for (int c = 0; c < s->channels; c++)   // new history = the last two frames of [history | pushed]
    HIP_TRY(hipMemcpyAsync(s->d_hist + 1024 * c, s->d_buf + stride * c + (size_t)frames * 512, 1024 * sizeof(float),
                           hipMemcpyDeviceToDevice, ctx->stream));
  HIP_TRY(hipMemcpyAsync(units, s->d_units, (size_t)s->channels * frames * C1_UNIT_BYTES, hipMemcpyDeviceToHost, ctx->stream));
  if (mc && mc_host) {
    const size_t n_units = (size_t)s->channels * frames;
    if (mc_host->taken) HIP_TRY(hipMemcpyAsync(mc_host->taken, mc->taken, n_units, hipMemcpyDeviceToHost, ctx->stream));
    if (mc_host->shifts && mc->shifts) HIP_TRY(hipMemcpyAsync(mc_host->shifts, mc->shifts, n_units * 52, hipMemcpyDeviceToHost, ctx->stream));
    if (mc_host->distortion) HIP_TRY(hipMemcpyAsync(mc_host->distortion, mc->distortion, n_units * 2 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (mc_host->energy) HIP_TRY(hipMemcpyAsync(mc_host->energy, mc->energy, n_units * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (mc_host->weights) HIP_TRY(hipMemcpyAsync(mc_host->weights, mc->weights, n_units * 52 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  }
  if (bm && bm_host) {
    const size_t n_units = (size_t)s->channels * frames;
    if (bm_host->choice) HIP_TRY(hipMemcpyAsync(bm_host->choice, bm->choice, n_units, hipMemcpyDeviceToHost, ctx->stream));
    if (bm_host->modes_out) HIP_TRY(hipMemcpyAsync(bm_host->modes_out, bm->modes_out, n_units, hipMemcpyDeviceToHost, ctx->stream));
    if (bm_host->taken) HIP_TRY(hipMemcpyAsync(bm_host->taken, bm->taken, n_units, hipMemcpyDeviceToHost, ctx->stream));
    if (bm_host->shifts) HIP_TRY(hipMemcpyAsync(bm_host->shifts, bm->shifts, n_units * 52, hipMemcpyDeviceToHost, ctx->stream));
    if (bm_host->distortion) HIP_TRY(hipMemcpyAsync(bm_host->distortion, bm->distortion, n_units * bm->n * 2 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (bm_host->energy) HIP_TRY(hipMemcpyAsync(bm_host->energy, bm->energy, n_units * bm->n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (bm_host->weights) HIP_TRY(hipMemcpyAsync(bm_host->weights, bm->weights, n_units * 52 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  }
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  s->pushed += frames;
  if (from_state > 0) {
    if (s->state_frames > 0) s->state_frames -= (int)from_state;
    s->state_live = frames == from_state;
    if (!detect) s->hist = HIST_MAGS;              // the magnitudes d_state holds are the pool's transientDetection
  } else {
    s->state_live = false;
  }
  if (detect) s->hist = HIST_PREV;
  return C1_OK;
}
}  // namespace

int c1_enc_stream_destroy(c1_enc_stream *s) {
  if (!s) return C1_OK;
  hipSetDevice(s->ctx->device);
  hipStreamSynchronize(s->ctx->stream);
  if (s->d_hist) hipFree(s->d_hist);
  if (s->d_buf) hipFree(s->d_buf);
  if (s->d_units) hipFree(s->d_units);
  if (s->d_given) hipFree(s->d_given);
  if (s->d_bias) hipFree(s->d_bias);
  if (s->d_meas) hipFree(s->d_meas);
  if (s->d_sw_block) hipFree(s->d_sw_block);
  if (s->d_state) hipFree(s->d_state);
  delete s;
  return C1_OK;
}

// The decoded state after a frame is a function of that frame alone, so the stream keeps its previous frame: as a unit after a
// unit push (d_prev, k_decode's halo), as fields after a field push.  Fields live in two buffers used in turn (d_fields), so
// that a push reads its halo from the previous push's buffer while it writes its own; after a unit push the fields of d_prev
// are made by k_unpack_units when a field push needs them (d_prev_fields).
struct c1_dec_stream {
  c1_ctx *ctx;
  int channels;
  bool have_prev = false;
  bool prev_is_unit = false;   // the previous push was units: d_prev holds the previous frame
  uint8_t *d_prev = nullptr;   // channels units of the previous frame
  uint8_t *d_units = nullptr;
  float *d_pcm = nullptr;
  int64_t cap_frames = 0;
  C1FieldPtrs prev_fields = {nullptr, nullptr, nullptr, nullptr, nullptr};   // channels units; nbfu NULL: not made yet
  int32_t *d_fields[2] = {nullptr, nullptr};   // kFieldInts per unit, field_layout over the push's units
  int64_t fields_cap[2] = {0, 0};              // units
  int fields_next = 0;
  int32_t *d_prev_fields = nullptr;            // channels units, field_layout
  int32_t *h_stage = nullptr;                  // page-locked staging of a field push (one host-to-device copy)
  int64_t stage_cap = 0;                       // units
  // after c1_dec_stream_set_state: the pool is explicit (d_state) and the next pushed frame is decoded from it by the
  // from-state kernel; its fields are the history of everything behind it, as after any field push
  bool restored = false;
  float *d_state = nullptr;                    // channels x c1_dec_state, then one zero state per channel, then scratch
  int prev_model = C1_DECODE_EXACT;            // the context's decode model when the previous frame was decoded
};

namespace {
int dec_stream_reserve(c1_dec_stream *s, int64_t frames) {
  const size_t ub = (size_t)s->channels * C1_UNIT_BYTES;
  if (frames > s->cap_frames) {
    if (s->d_units) { hipFree(s->d_units); hipFree(s->d_pcm); }
    s->d_units = nullptr; s->d_pcm = nullptr; s->cap_frames = 0;
    HIP_TRY(hipMalloc(&s->d_units, ub * (frames + 1)));
    HIP_TRY(hipMalloc(&s->d_pcm, (size_t)s->channels * frames * 512 * sizeof(float)));
    s->cap_frames = frames;
  }
  return C1_OK;
}
// the fields buffer of this push (units = frames * channels), never the one the previous push left its last frame in
int dec_stream_fields(c1_dec_stream *s, int64_t units, int32_t **out) {
  const int p = s->fields_next;
  if (units > s->fields_cap[p]) {
    if (s->d_fields[p]) hipFree(s->d_fields[p]);
    s->d_fields[p] = nullptr; s->fields_cap[p] = 0;
    HIP_TRY(hipMalloc(&s->d_fields[p], (size_t)(kFieldInts * units) * sizeof(int32_t)));
    s->fields_cap[p] = units;
  }
  *out = s->d_fields[p];
  return C1_OK;
}
// the previous frame as fields: unpack the unit the last push ended with
int dec_stream_prev_fields(c1_dec_stream *s) {
  if (!s->have_prev || s->prev_fields.nbfu) return C1_OK;
  if (!s->d_prev_fields) HIP_TRY(hipMalloc(&s->d_prev_fields, (size_t)(kFieldInts * s->channels) * sizeof(int32_t)));
  const C1FieldPtrs pf = field_layout(s->d_prev_fields, s->channels);
  c1k_launch_unpack_units(s->d_prev, s->channels, (int32_t *)pf.nbfu, (int32_t *)pf.modes, (int32_t *)pf.sfi, (int32_t *)pf.wl,
                          (int32_t *)pf.q, s->ctx->stream);
  s->prev_fields = pf;
  return C1_OK;
}
int dec_stream_state_buffer(c1_dec_stream *s) {
  if (s->d_state) return C1_OK;
  const size_t bytes = 3 * (size_t)s->channels * sizeof(c1_dec_state);
  HIP_TRY(hipMalloc(&s->d_state, bytes));
  HIP_TRY(hipMemsetAsync(s->d_state, 0, bytes, s->ctx->stream));
  return C1_OK;
}
// The stream rebuilds the pool before a push from its previous frame, in the arithmetic of the push.  When the context's model
// went to or from C1_DECODE_BINARY32 since that frame was decoded, the pool is the one the frame left under the model that
// decoded it: it is made explicit here (as c1_dec_stream_get_state would have returned it), and the push continues from it as
// after c1_dec_stream_set_state.  A change between the other two models takes no part in this: they share every kernel but
// k_decode, which rebuilds its halo itself.
int dec_stream_follow_model(c1_dec_stream *s) {
  c1_ctx *ctx = s->ctx;
  const bool was32 = s->prev_model == C1_DECODE_BINARY32, is32 = ctx->decode_model == C1_DECODE_BINARY32;
  if (s->restored || !s->have_prev || was32 == is32) return C1_OK;
  int rc;
  if ((rc = dec_stream_state_buffer(s))) return rc;
  if ((rc = dec_stream_prev_fields(s))) return rc;
  C1DecStateLaunch K;
  memset(&K, 0, sizeof K);
  K.fields = s->prev_fields;
  K.in = s->d_state + (size_t)s->channels * kDecStateFloats;
  K.out = s->d_state;
  K.n = s->channels;
  K.tables = ctx->d_tables;
  K.binary32 = was32;
  c1k_launch_decode_from_states(K, ctx->stream);
  HIP_TRY(hipGetLastError());
  s->restored = true;
  return C1_OK;
}
// decode `frames` frames whose fields are at `cur` (layout over frames * channels units) from the stream's history, then make
// the last of them the history; downloads the PCM and synchronises
int dec_stream_decode_fields(c1_dec_stream *s, const C1FieldPtrs &cur, int64_t frames, float *const *pcm) {
  c1_ctx *ctx = s->ctx;
  int rc;
  if (!s->restored && (rc = dec_stream_prev_fields(s))) return rc;
  float *dptr[C1_MAX_CHANNELS] = {nullptr, nullptr};
  for (int c = 0; c < s->channels; c++) dptr[c] = s->d_pcm + (size_t)c * s->cap_frames * 512;
  if (ctx->profiling && ctx->timing_depth == 0) reset_timings(ctx);
  if (s->restored) {
    // the first frame from the restored pool, the others from that frame's fields as their halo
    C1DecStateLaunch K;
    memset(&K, 0, sizeof K);
    K.fields = cur;
    K.in = s->d_state;
    K.pcm = s->d_pcm;
    K.pcm_stride = s->cap_frames * 512;
    K.n = s->channels;
    K.tables = ctx->d_tables;
    K.binary32 = ctx->decode_model == C1_DECODE_BINARY32;
    { ScopedTiming t(ctx, K_FROM_STATE); c1k_launch_decode_from_states(K, ctx->stream); }
    HIP_TRY(hipGetLastError());
    if (frames > 1) {
      float *rest[C1_MAX_CHANNELS] = {nullptr, nullptr};
      for (int c = 0; c < s->channels; c++) rest[c] = dptr[c] + 512;
      if ((rc = launch_decode_fields(ctx, field_unit(cur, s->channels), cur, s->channels, frames - 1, 1, rest))) return rc;
    }
    s->restored = false;
  } else if ((rc = launch_decode_fields(ctx, cur, s->prev_fields, s->channels, frames, s->have_prev ? 1 : 0, dptr))) return rc;
  s->prev_fields = field_unit(cur, (frames - 1) * s->channels);
  s->fields_next ^= 1;
  s->have_prev = true;
  s->prev_is_unit = false;
  s->prev_model = ctx->decode_model;
  for (int c = 0; c < s->channels; c++)
    HIP_TRY(hipMemcpyAsync(pcm[c], dptr[c], (size_t)frames * 512 * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return C1_OK;
}
}  // namespace

int c1_dec_stream_create(c1_ctx *ctx, int channels, c1_dec_stream **out) {
  CTX_GUARD(ctx);
  int rc = ctx_bind(ctx);
  if (rc) return rc;
  if (!out) return fail(C1_ERR_ARG, "out is NULL");
  if ((rc = check_channels(channels))) return rc;
  c1_dec_stream *s = new c1_dec_stream();
  s->ctx = ctx; s->channels = channels;
  const hipError_t e = hipMalloc(&s->d_prev, (size_t)channels * C1_UNIT_BYTES);
  if (e != hipSuccess) { delete s; return fail(C1_ERR_HIP, "dec stream alloc: %s", hipGetErrorString(e)); }
  *out = s;
  return C1_OK;
}

int c1_dec_stream_push(c1_dec_stream *s, const uint8_t *units, int64_t frames, float *const *pcm) {
  if (!s) return fail(C1_ERR_ARG, "stream is NULL");
  c1_ctx *ctx = s->ctx;
  CTX_GUARD(ctx);
  int rc = ctx_bind(ctx);
  if (rc) return rc;
  if (frames < 0) return fail(C1_ERR_ARG, "frames must be >= 0");
  if (frames == 0) return C1_OK;
  if (!units || !pcm) return fail(C1_ERR_ARG, "units or pcm is NULL");
  for (int c = 0; c < s->channels; c++) if (!pcm[c]) return fail(C1_ERR_ARG, "pcm[%d] is NULL", c);
  const size_t ub = (size_t)s->channels * C1_UNIT_BYTES;
  if ((rc = dec_stream_reserve(s, frames))) return rc;
  if ((rc = dec_stream_follow_model(s))) return rc;
  if (s->restored || (s->have_prev && !s->prev_is_unit)) {
    // the previous frame is held as fields (or the pool is a restored one), which a unit cannot stand in for: unpack this push's units and decode them
    // from fields too (k_unpack_units + k_decode_fields decode any unit exactly as k_decode does)
    const int64_t units_n = frames * s->channels;
    int32_t *d;
    if ((rc = dec_stream_fields(s, units_n, &d))) return rc;
    const C1FieldPtrs cur = field_layout(d, units_n);
    HIP_TRY(hipMemcpyAsync(s->d_units + ub, units, ub * frames, hipMemcpyHostToDevice, ctx->stream));
    c1k_launch_unpack_units(s->d_units + ub, units_n, (int32_t *)cur.nbfu, (int32_t *)cur.modes, (int32_t *)cur.sfi, (int32_t *)cur.wl,
                            (int32_t *)cur.q, ctx->stream);
    HIP_TRY(hipMemcpyAsync(s->d_prev, s->d_units + ub * frames, ub, hipMemcpyDeviceToDevice, ctx->stream));
    if ((rc = dec_stream_decode_fields(s, cur, frames, pcm))) return rc;
    s->prev_is_unit = true;                        // d_prev and prev_fields both hold the last frame now: either kind may follow
    return C1_OK;
  }
  if (s->have_prev) HIP_TRY(hipMemcpyAsync(s->d_units, s->d_prev, ub, hipMemcpyDeviceToDevice, ctx->stream));
  HIP_TRY(hipMemcpyAsync(s->d_units + ub, units, ub * frames, hipMemcpyHostToDevice, ctx->stream));
  float *dptr[C1_MAX_CHANNELS] = {nullptr, nullptr};
  for (int c = 0; c < s->channels; c++) dptr[c] = s->d_pcm + (size_t)c * s->cap_frames * 512;
  if ((rc = c1_decode_device(ctx, s->d_units + ub, s->channels, frames, s->have_prev ? 1 : 0, dptr))) return rc;
  HIP_TRY(hipMemcpyAsync(s->d_prev, s->d_units + ub * frames, ub, hipMemcpyDeviceToDevice, ctx->stream));
  s->have_prev = true;
  s->prev_is_unit = true;
  s->prev_model = ctx->decode_model;
  s->prev_fields.nbfu = nullptr;
  for (int c = 0; c < s->channels; c++)
    HIP_TRY(hipMemcpyAsync(pcm[c], dptr[c], (size_t)frames * 512 * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return C1_OK;
}

int c1_dec_stream_push_fields(c1_dec_stream *s, int64_t frames, const int32_t *nbfu, const int32_t *block_modes,
                              const int32_t *sfi, const int32_t *wl, const int32_t *quantized, float *const *pcm) {
  if (!s) return fail(C1_ERR_ARG, "stream is NULL");
  c1_ctx *ctx = s->ctx;
  CTX_GUARD(ctx);
  int rc = ctx_bind(ctx);
  if (rc) return rc;
  if (frames < 0 || frames > kMaxStageFrames) return fail(C1_ERR_ARG, "decode fields: frames must be 0 .. 2^20, got %lld", (long long)frames);
  if (frames == 0) return C1_OK;
  if (!nbfu || !block_modes || !sfi || !wl || !quantized || !pcm) return fail(C1_ERR_ARG, "decode fields: NULL argument");
  for (int c = 0; c < s->channels; c++) if (!pcm[c]) return fail(C1_ERR_ARG, "pcm[%d] is NULL", c);
  const int64_t units_n = frames * s->channels;
  if ((rc = check_field_domain("decode fields", units_n, s->channels, 0, nbfu, sfi, wl))) return rc;
  if ((rc = dec_stream_reserve(s, frames))) return rc;
  if ((rc = dec_stream_follow_model(s))) return rc;
  if (units_n > s->stage_cap) {
    if (s->h_stage) hipHostFree(s->h_stage);
    s->h_stage = nullptr; s->stage_cap = 0;
    HIP_TRY(hipHostMalloc((void **)&s->h_stage, (size_t)(kFieldInts * units_n) * sizeof(int32_t), hipHostMallocDefault));
    s->stage_cap = units_n;
  }
  int32_t *d;
  if ((rc = dec_stream_fields(s, units_n, &d))) return rc;
  // one copy: the five arrays staged in the device buffer's layout (the last push's copy has completed: pushes synchronise)
  const C1FieldPtrs st = field_layout(s->h_stage, units_n);
  memcpy((void *)st.nbfu, nbfu, (size_t)units_n * sizeof(int32_t));
  memcpy((void *)st.modes, block_modes, 3 * (size_t)units_n * sizeof(int32_t));
  memcpy((void *)st.sfi, sfi, 52 * (size_t)units_n * sizeof(int32_t));
  memcpy((void *)st.wl, wl, 52 * (size_t)units_n * sizeof(int32_t));
  memcpy((void *)st.q, quantized, 512 * (size_t)units_n * sizeof(int32_t));
  HIP_TRY(hipMemcpyAsync(d, s->h_stage, (size_t)(kFieldInts * units_n) * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
  return dec_stream_decode_fields(s, field_layout(d, units_n), frames, pcm);
}

int c1_dec_stream_destroy(c1_dec_stream *s) {
  if (!s) return C1_OK;
  hipSetDevice(s->ctx->device);
  hipStreamSynchronize(s->ctx->stream);
  if (s->d_prev) hipFree(s->d_prev);
  if (s->d_units) hipFree(s->d_units);
  if (s->d_pcm) hipFree(s->d_pcm);
  for (int p = 0; p < 2; p++) if (s->d_fields[p]) hipFree(s->d_fields[p]);
  if (s->d_prev_fields) hipFree(s->d_prev_fields);
  if (s->h_stage) hipHostFree(s->h_stage);
  if (s->d_state) hipFree(s->d_state);
  delete s;
  return C1_OK;
}

// ---- stream state in the reference's BufferPool layout: the frame closures over explicit pools, snapshot and restore -------
int c1_encode_frames_from_states_device(c1_ctx *ctx, int64_t n, const float *pcm, const c1_enc_state *in, const c1_encode_options *opts,
                                        uint8_t *units, c1_enc_state *out) {
  CTX_GUARD(ctx);
  int rc = ctx_bind(ctx);
  if (rc) return rc;
  if (n < 0 || n > kMaxStatePools) return fail(C1_ERR_ARG, "encode from states: n must be 0 .. 2^27, got %lld", (long long)n);
  if (!pcm || !in || !opts || !units) return fail(C1_ERR_ARG, "encode from states: NULL argument");
  if ((uintptr_t)pcm & 15) return fail(C1_ERR_ARG, "encode from states: pcm must be 16-byte aligned on the device");
  if (((uintptr_t)in | (uintptr_t)out) & 3) return fail(C1_ERR_ARG, "encode from states: states must be 4-byte aligned on the device");
  return encode_from_states_impl(ctx, n, pcm, 512, reinterpret_cast<const float *>(in), opts, units, reinterpret_cast<float *>(out));
}

int c1_encode_frames_from_states(c1_ctx *ctx, int64_t n, const float *pcm, const c1_enc_state *in, const c1_encode_options *opts,
                                 uint8_t *units, c1_enc_state *out) {
  CTX_GUARD(ctx);
  int rc = ctx_bind(ctx);
  if (rc) return rc;
  if (n < 0 || n > kMaxStageFrames) return fail(C1_ERR_ARG, "encode from states: n must be 0 .. 2^20, got %lld", (long long)n);
  if (!pcm || !in || !opts || !units) return fail(C1_ERR_ARG, "encode from states: NULL argument");
  C1DevEncOpts probe;
  if ((rc = build_encode_opts(*opts, &probe))) return rc;
  if (n == 0) return C1_OK;
  if ((rc = check_states_finite("encode from states", "pool", in, n, kEncStateFloats, kEncStateFields, 5))) return rc;
  DeviceScratch ds;
  float *dp, *dst; uint8_t *du;
  const size_t N = (size_t)n;
  if ((rc = ds.alloc(&dp, N * 512)) || (rc = ds.alloc(&dst, N * kEncStateFloats)) || (rc = ds.alloc(&du, N * C1_UNIT_BYTES))) return rc;
  HIP_TRY(hipMemcpyAsync(dp, pcm, N * 512 * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(hipMemcpyAsync(dst, in, N * sizeof(c1_enc_state), hipMemcpyHostToDevice, ctx->stream));
  if ((rc = encode_from_states_impl(ctx, n, dp, 512, dst, opts, du, out ? dst : nullptr))) return rc;
  HIP_TRY(hipMemcpyAsync(units, du, N * C1_UNIT_BYTES, hipMemcpyDeviceToHost, ctx->stream));
  if (out) HIP_TRY(hipMemcpyAsync(out, dst, N * sizeof(c1_enc_state), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return C1_OK;
}

namespace {
// device pointers; the unpacked fields of a chunk of pools live in the context's call scratch
int decode_from_states_impl(c1_ctx *ctx, int64_t n, const uint8_t *units, const float *in, float *pcm, float *out) {
  int rc;
  if (ctx->profiling && ctx->timing_depth == 0) reset_timings(ctx);
  if (n == 0) return C1_OK;
  const int64_t chunk = std::min(n, kStateDecodeChunk);
  if ((rc = ensure_io(ctx, (size_t)(kFieldInts * chunk) * sizeof(int32_t)))) return rc;
  for (int64_t n0 = 0; n0 < n; n0 += chunk) {
    const int64_t m = std::min(chunk, n - n0);
    const C1FieldPtrs f = field_layout(static_cast<int32_t *>(ctx->d_io), m);
    c1k_launch_unpack_units(units + n0 * C1_UNIT_BYTES, m, (int32_t *)f.nbfu, (int32_t *)f.modes, (int32_t *)f.sfi, (int32_t *)f.wl,
                            (int32_t *)f.q, ctx->stream);
    C1DecStateLaunch K;
    memset(&K, 0, sizeof K);
    K.fields = f;
    K.in = in + n0 * kDecStateFloats;
    K.out = out ? out + n0 * kDecStateFloats : nullptr;
    K.pcm = pcm + n0 * 512;
    K.pcm_stride = 512;
    K.n = m;
    K.tables = ctx->d_tables;
    K.binary32 = ctx->decode_model == C1_DECODE_BINARY32;
    { ScopedTiming t(ctx, K_FROM_STATE); c1k_launch_decode_from_states(K, ctx->stream); }
  }
  HIP_TRY(hipGetLastError());
  return C1_OK;
}
}  // namespace

int c1_decode_frames_from_states_device(c1_ctx *ctx, int64_t n, const uint8_t *units, const c1_dec_state *in, float *pcm,
                                        c1_dec_state *out) {
  CTX_GUARD(ctx);
  int rc = ctx_bind(ctx);
  if (rc) return rc;
  if (n < 0 || n > kMaxStatePools) return fail(C1_ERR_ARG, "decode from states: n must be 0 .. 2^27, got %lld", (long long)n);
  if (!units || !in || !pcm) return fail(C1_ERR_ARG, "decode from states: NULL argument");
  if ((uintptr_t)pcm & 15) return fail(C1_ERR_ARG, "decode from states: pcm must be 16-byte aligned on the device");
  if (((uintptr_t)in | (uintptr_t)out | (uintptr_t)units) & 3) return fail(C1_ERR_ARG, "decode from states: units and states must be 4-byte aligned on the device");
  return decode_from_states_impl(ctx, n, units, reinterpret_cast<const float *>(in), pcm, reinterpret_cast<float *>(out));
}

int c1_decode_frames_from_states(c1_ctx *ctx, int64_t n, const uint8_t *units, const c1_dec_state *in, float *pcm, c1_dec_state *out) {
  CTX_GUARD(ctx);
  int rc = ctx_bind(ctx);
  if (rc) return rc;
  if (n < 0 || n > kMaxStageFrames) return fail(C1_ERR_ARG, "decode from states: n must be 0 .. 2^20, got %lld", (long long)n);
  if (!units || !in || !pcm) return fail(C1_ERR_ARG, "decode from states: NULL argument");
  if (n == 0) return C1_OK;
  if ((rc = check_states_finite("decode from states", "pool", in, n, kDecStateFloats, kDecStateFields, 4))) return rc;
  DeviceScratch ds;
  float *dp, *dst; uint8_t *du;
  const size_t N = (size_t)n;
  if ((rc = ds.alloc(&dp, N * 512)) || (rc = ds.alloc(&dst, N * kDecStateFloats)) || (rc = ds.alloc(&du, N * C1_UNIT_BYTES))) return rc;
  HIP_TRY(hipMemcpyAsync(du, units, N * C1_UNIT_BYTES, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(hipMemcpyAsync(dst, in, N * sizeof(c1_dec_state), hipMemcpyHostToDevice, ctx->stream));
  if ((rc = decode_from_states_impl(ctx, n, du, dst, dp, out ? dst : nullptr))) return rc;
  HIP_TRY(hipMemcpyAsync(pcm, dp, N * 512 * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  if (out) HIP_TRY(hipMemcpyAsync(out, dst, N * sizeof(c1_dec_state), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return C1_OK;
}

// ---- n signals of any lengths from their own pools in one call ---------------------------------------------
namespace {
constexpr int64_t kMaxSignals = (int64_t)1 << 20;
constexpr int64_t kMaxSignalFrames = (int64_t)1 << 27, kMaxSignalFramesHost = (int64_t)1 << 22;
constexpr int kUnitDwords = C1_UNIT_BYTES / 4;
static_assert(C1_UNIT_BYTES % 4 == 0, "sound units move as dwords");

int check_frame_offsets(const char *what, int64_t n, const int64_t *off, int64_t max_total, int64_t *total) {
  if (n < 0 || n > kMaxSignals) return fail(C1_ERR_ARG, "%s: n must be 0 .. 2^20, got %lld", what, (long long)n);
  if (!off) return fail(C1_ERR_ARG, "%s: frame_offsets is NULL", what);
  if (off[0] != 0) return fail(C1_ERR_ARG, "%s: frame_offsets must start at 0, got %lld", what, (long long)off[0]);
  for (int64_t i = 0; i < n; i++)
    if (off[i + 1] < off[i]) return fail(C1_ERR_ARG, "%s: frame_offsets decreases at signal %lld (%lld after %lld)", what, (long long)i, (long long)off[i + 1], (long long)off[i]);
  if (off[n] > max_total) return fail(C1_ERR_ARG, "%s: %lld frames in all, at most %lld per call", what, (long long)off[n], (long long)max_total);
  *total = off[n];
  return C1_OK;
}

struct TimingScope {         // one profiled call around several *_device calls: they keep the timings (c1_ctx::timing_depth)
  c1_ctx *ctx;
  explicit TimingScope(c1_ctx *c) : ctx(c) {
    if (ctx->profiling && ctx->timing_depth == 0) reset_timings(ctx);
    ctx->timing_depth++;
  }
  ~TimingScope() { ctx->timing_depth--; }
};

size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

// device scratch of a signals call, carved from one allocation that lives with the context
struct SigCarve {
  size_t bytes = 0;
  size_t take(size_t b) { const size_t at = bytes; bytes += align256(b); return at; }
};
int ensure_sig(c1_ctx *ctx, size_t bytes) {
  if (bytes <= ctx->d_sig_bytes) return C1_OK;
  if (ctx->d_sig) (void)hipFree(ctx->d_sig);               // waits for the device: nothing queued still reads it
  ctx->d_sig = nullptr; ctx->d_sig_bytes = 0;
  HIP_TRY(hipMalloc(&ctx->d_sig, bytes));
  ctx->d_sig_bytes = bytes;
  return C1_OK;
}
// the page-locked image of the index lists, free to be rewritten: the previous call's upload has left it
int rows_image(c1_ctx *ctx, size_t words, uint32_t **out) {
  if (ctx->rows_pending) { HIP_TRY(hipEventSynchronize(ctx->ev_rows)); ctx->rows_pending = false; }
  if (!ctx->ev_rows) HIP_TRY(hipEventCreateWithFlags(&ctx->ev_rows, hipEventDisableTiming));
  const size_t bytes = std::max<size_t>(words, 1) * sizeof(uint32_t);
  if (bytes > ctx->h_rows_bytes) {
    if (ctx->h_rows) (void)hipHostFree(ctx->h_rows);
    ctx->h_rows = nullptr; ctx->h_rows_bytes = 0;
    HIP_TRY(hipHostMalloc((void **)&ctx->h_rows, bytes, hipHostMallocDefault));
    ctx->h_rows_bytes = bytes;
  }
  *out = ctx->h_rows;
  return C1_OK;
}
int upload_rows(c1_ctx *ctx, uint32_t *dst, size_t words) {
  if (!words) return C1_OK;
  HIP_TRY(hipMemcpyAsync(dst, ctx->h_rows, words * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(hipEventRecord(ctx->ev_rows, ctx->stream));
  ctx->rows_pending = true;
  return C1_OK;
}

// One fix-up pass of the encoder: `rows` frames, row r the PCM frame src[r] from state in[in_rows[r]] (in_rows null: in[r];
// bcast: in[0]) to state out[out_rows[r]] (null: out[r]; out null: no state), through the from-state kernel into the
// workspace, the encoder's own allocation and packing on it, and the units scattered to units[src[r]].  W rows at a time.
// mc (c1_encode_signals_measured*): the measured allocation of the rows runs between their allocation and packing, its outputs
// go to the rows' staging `st` and one scatter launch moves unit and outputs to their places; units (and row_units) may then be
// null: nothing is packed
struct RowStage {            // per-row staging of a measured signals call, carved from c1_ctx::d_sig
  uint8_t *taken;
  int8_t *shifts;
  double *distortion, *energy, *weights;
};
// allocation, the measured step (mc non-null), packing and the move of m workspace rows to units dst_rows[0 .. m) of the call
void rows_chain(c1_ctx *ctx, int64_t m, const uint32_t *dst_rows, uint8_t *units, uint8_t *row_units, const MeasuredCall *mc,
                const RowStage *st) {
  C1EncodeLaunch L;
  memset(&L, 0, sizeof L);
  L.channels = 1;
  L.frames = m;
  L.tables = ctx->d_tables;
  L.opts = ctx->d_opts;
  L.coefs = ctx->d_coefs[0];
  L.side = ctx->d_side[0];
  L.alloc = ctx->d_alloc[0];
  L.cand = ctx->d_cand[0];
  L.work_count = ctx->d_work[0];
  L.work_list = ctx->d_work[0] + 4;
  L.sel_list = ctx->d_work[0] + 4 + (size_t)ctx->ws_units * 7;
  L.units = row_units;
  { ScopedTiming t(ctx, K_ALLOCATE); c1k_launch_allocate(L, ctx->stream); }
  if (mc) {
    MeasuredCall sm = *mc;                                     // the same definition, the outputs at the rows' staging
    sm.taken = mc->taken ? st->taken : nullptr;
    sm.shifts = mc->shifts ? st->shifts : nullptr;
    sm.distortion = mc->distortion ? st->distortion : nullptr;
    sm.energy = mc->energy ? st->energy : nullptr;
    sm.weights = mc->weights ? st->weights : nullptr;
    launch_measured(ctx, L, false, &sm, 0, ctx->stream);       // the side records carry the rows' mode bytes
  }
  if (row_units) { ScopedTiming t(ctx, K_PACK); c1k_launch_pack(L, false, ctx->stream); }
  ScopedTiming t(ctx, K_SIGNAL_STARTS);
  if (!mc) {
    c1k_launch_copy_rows(reinterpret_cast<uint32_t *>(units), dst_rows, reinterpret_cast<const uint32_t *>(row_units), nullptr, 0, m, kUnitDwords, ctx->stream);
    return;
  }
  C1ScatterRowsLaunch X;
  memset(&X, 0, sizeof X);
  X.dst_rows = dst_rows;
  X.n = m;
  if (row_units) { X.units_src = reinterpret_cast<const uint32_t *>(row_units); X.units_dst = reinterpret_cast<uint32_t *>(units); }
  if (mc->taken) { X.taken_src = st->taken; X.taken_dst = mc->taken; }
  if (mc->shifts) { X.shifts_src = reinterpret_cast<const uint32_t *>(st->shifts); X.shifts_dst = reinterpret_cast<uint32_t *>(mc->shifts); }
  if (mc->distortion) { X.distortion_src = reinterpret_cast<const uint32_t *>(st->distortion); X.distortion_dst = reinterpret_cast<uint32_t *>(mc->distortion); }
  if (mc->energy) { X.energy_src = reinterpret_cast<const uint32_t *>(st->energy); X.energy_dst = reinterpret_cast<uint32_t *>(mc->energy); }
  if (mc->weights) { X.weights_src = reinterpret_cast<const uint32_t *>(st->weights); X.weights_dst = reinterpret_cast<uint32_t *>(mc->weights); }
  c1k_launch_scatter_signal_rows(X, ctx->stream);
}

int encode_rows_pass(c1_ctx *ctx, const float *pcm, const uint32_t *src, const float *in, const uint32_t *in_rows, bool bcast,
                     float *out, const uint32_t *out_rows, int64_t rows, int64_t W, uint8_t *units, uint8_t *row_units,
                     const MeasuredCall *mc = nullptr, const RowStage *st = nullptr) {
  for (int64_t r0 = 0; r0 < rows; r0 += W) {
    const int64_t m = std::min(W, rows - r0);
    C1EncStateLaunch K;
    memset(&K, 0, sizeof K);
    K.pcm = pcm;
    K.src_rows = src + r0;
    K.in = (in_rows || bcast) ? in : in + r0 * kEncStateFloats;
    K.in_rows = in_rows ? in_rows + r0 : nullptr;
    K.in_broadcast = bcast ? 1 : 0;
    K.out = (!out || out_rows) ? out : out + r0 * kEncStateFloats;
    K.out_rows = out_rows ? out_rows + r0 : nullptr;
    K.n = m;
    K.tables = ctx->d_tables;
    K.opts = ctx->d_opts;
    K.coefs = ctx->d_coefs[0];
    K.side = ctx->d_side[0];
    K.detect = -1;
    { ScopedTiming t(ctx, K_SIGNAL_STARTS); c1k_launch_encode_rows(K, ctx->stream); }
    rows_chain(ctx, m, src + r0, units, row_units, mc, st);
  }
  return C1_OK;
}

// device pointers but frame_offsets; arguments checked by the callers
int encode_signals_impl(c1_ctx *ctx, int64_t n, const int64_t *off, const float *pcm, const float *in, const c1_encode_options *opts,
                        uint8_t *units, float *out) {
  int rc;
  TimingScope scope(ctx);
  const int64_t total = off[n];
  // 1. the whole concatenation as one mono stream: every unit but those of the first two frames of a signal is final.  The
  //    call returns with the context's stream waiting for all of its work (tails and internal streams): what follows is ordered
  const float *chan[1] = {pcm};
  if ((rc = encode_device_impl(ctx, chan, 1, total, 0, opts, units, nullptr, nullptr, nullptr, nullptr, false))) return rc;
  int64_t nA = 0, nB = 0, nC = 0, nZ = 0;
  for (int64_t i = 0; i < n; i++) {
    const int64_t len = off[i + 1] - off[i];
    nA += len >= 1; nB += len >= 2; nC += len >= 3; nZ += len == 0;
  }
  const bool copy_empty = out && out != in && nZ > 0;
  if (nA == 0 && !copy_empty) return C1_OK;
  if (!out) nC = 0;
  // index lists: A = signals of >= 1 frame (frame 0), B = of >= 2 (frame 1), C = of >= 3 (the last two frames), Z = empty ones
  const size_t words = (size_t)(2 * nA + 3 * nB + 3 * nC + nZ);
  uint32_t *h;
  if ((rc = rows_image(ctx, words, &h))) return rc;
  uint32_t *a_src = h, *a_sig = a_src + nA, *b_src = a_sig + nA, *b_sig = b_src + nB, *b_row = b_sig + nB, *c_src0 = b_row + nB,
           *c_src1 = c_src0 + nC, *c_sig = c_src1 + nC, *z_sig = c_sig + nC;
  {
    int64_t a = 0, b = 0, c = 0, z = 0;
    for (int64_t i = 0; i < n; i++) {
      const int64_t f0 = off[i], len = off[i + 1] - f0;
      if (len == 0) { z_sig[z++] = (uint32_t)i; continue; }
      if (len >= 2) { b_src[b] = (uint32_t)(f0 + 1); b_sig[b] = (uint32_t)i; b_row[b] = (uint32_t)a; b++; }
      if (len >= 3 && out) { c_src0[c] = (uint32_t)(f0 + len - 2); c_src1[c] = (uint32_t)(f0 + len - 1); c_sig[c] = (uint32_t)i; c++; }
      a_src[a] = (uint32_t)f0; a_sig[a] = (uint32_t)i; a++;
    }
  }
  int64_t W = 0;
  if (nA > 0) {
    if ((rc = join_tail(ctx))) return rc;
    W = std::min(nA, chunk_for_call(ctx, nA, 1, false));
    if ((rc = ensure_workspace(ctx, W))) return rc;
  }
  SigCarve cv;
  const size_t o_zero = cv.take(sizeof(c1_enc_state)), o_lists = cv.take(words * sizeof(uint32_t)),
               o_tmp = cv.take(out ? 0 : (size_t)nA * sizeof(c1_enc_state)), o_tmp2 = cv.take((size_t)nC * sizeof(c1_enc_state)),
               o_units = cv.take((size_t)W * C1_UNIT_BYTES);
  if ((rc = ensure_sig(ctx, cv.bytes))) return rc;
  uint8_t *base = static_cast<uint8_t *>(ctx->d_sig);
  float *zero = reinterpret_cast<float *>(base + o_zero), *tmp = reinterpret_cast<float *>(base + o_tmp), *tmp2 = reinterpret_cast<float *>(base + o_tmp2);
  uint32_t *d = reinterpret_cast<uint32_t *>(base + o_lists);
  const uint32_t *da_src = d, *da_sig = da_src + nA, *db_src = da_sig + nA, *db_sig = db_src + nB, *db_row = db_sig + nB, *dc_src0 = db_row + nB,
                 *dc_src1 = dc_src0 + nC, *dc_sig = dc_src1 + nC, *dz_sig = dc_sig + nC;
  HIP_TRY(hipMemsetAsync(zero, 0, sizeof(c1_enc_state), ctx->stream));
  if ((rc = upload_rows(ctx, d, words))) return rc;
  // the pools in flight live in `out` at their signal's index, or in scratch at their row of list A when out is NULL
  float *S = out ? out : tmp;
  // 2. frame 0 of every signal from in[i] (a fresh pool when in is NULL)
  if ((rc = encode_rows_pass(ctx, pcm, da_src, in ? in : zero, in ? da_sig : nullptr, !in, (out || nB) ? S : nullptr, out ? da_sig : nullptr,
                             nA, W, units, base + o_units))) return rc;
  // 3. frame 1 from the pool step 2 left, in place
  if ((rc = encode_rows_pass(ctx, pcm, db_src, S, out ? db_sig : db_row, false, S, out ? db_sig : db_row, nB, W, units, base + o_units))) return rc;
  if (out) {
    // 4. signals of three frames and more: the pool after the last frame is a function of the last two frames (state only, from
    //    zeros: c1_enc_stream_get_state does the same); under fixed modes transient_mags keeps what steps 2 and 3 passed through
    const bool detect = opts->fixed_block_modes[0] < 0;
    C1EncStateLaunch K;
    memset(&K, 0, sizeof K);
    K.pcm = pcm;
    K.src_rows = dc_src0;
    K.in = zero;
    K.in_broadcast = 1;
    K.out = tmp2;
    K.n = nC;
    K.tables = ctx->d_tables;
    K.opts = ctx->d_opts;
    K.state_only = 1;
    K.detect = 0;                                          // the zero pool's magnitudes pass through: every float of tmp2 is written
    ScopedTiming t(ctx, K_SIGNAL_STARTS);
    c1k_launch_encode_rows(K, ctx->stream);
    K.src_rows = dc_src1;
    K.in = tmp2;
    K.in_broadcast = 0;
    K.out = out;
    K.out_rows = dc_sig;
    K.detect = detect ? 1 : 0;
    K.keep_mags = detect ? 0 : 1;
    c1k_launch_encode_rows(K, ctx->stream);
    // empty signals: the pool passes through
    if (copy_empty)
      c1k_launch_copy_rows(reinterpret_cast<uint32_t *>(out), dz_sig, reinterpret_cast<const uint32_t *>(in ? in : zero), in ? dz_sig : nullptr,
                           in ? 0 : 1, nZ, kEncStateFloats, ctx->stream);
  }
  HIP_TRY(hipGetLastError());
  return C1_OK;
}

// a mode byte in blockSelectorStage's domain, as the kernels bring it there, and its number 0 .. 7 among the domain's eight
int mode_byte_in_domain(int b) { return (b & 0x02) | (b & 0x08) | ((b & 0x30) == 0x30 ? 0x30 : 0); }
int mode_byte_number(int b) { return ((b >> 1) & 1) | (((b >> 3) & 1) << 1) | ((b & 0x30) == 0x30 ? 4 : 0); }

// encode_signals_impl with the measured allocation: device pointers but frame_offsets; arguments checked by the
// callers.  d_modes: one byte per frame of the concatenation (device memory) or null; h_modes: the same bytes in host memory
// when the caller has them (the two-pass route sorts its rows by them).  mc: the call's definition and outputs, over the units
// of the concatenation.  units may be null
int encode_signals_measured_impl(c1_ctx *ctx, int64_t n, const int64_t *off, const float *pcm, const float *in, const c1_encode_options *opts,
                                 const uint8_t *d_modes, const uint8_t *h_modes, const MeasuredCall *mc, uint8_t *units, float *out) {
  int rc;
  TimingScope scope(ctx);
  const int64_t total = off[n];
  const bool fused = ctx->signal_starts_fused;
  // with given modes neither threshold nor fixed modes are read
  c1_encode_options base = *opts;
  if (d_modes) {
    base.transient_threshold = 1.0;
    base.fixed_block_modes[0] = base.fixed_block_modes[1] = base.fixed_block_modes[2] = -1;
  }
  const bool detect = !d_modes && opts->fixed_block_modes[0] < 0;
  std::vector<uint8_t> fetched;
  if (d_modes && !fused && !h_modes && total > 0) {            // the row kernel takes one triple per launch: the bytes decide the launches
    fetched.resize((size_t)total);
    HIP_TRY(hipMemcpyAsync(fetched.data(), d_modes, (size_t)total, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    h_modes = fetched.data();
  }
  // 1. the whole concatenation as one mono stream, as c1_encode_measured_*_device runs it: every row but those of the first two
  //    frames of a signal is final
  const float *chan[1] = {pcm};
  if ((rc = encode_device_impl(ctx, chan, 1, total, 0, &base, units, nullptr, nullptr, nullptr, nullptr, false, total > 0 ? d_modes : nullptr,
                               nullptr, nullptr, nullptr, total > 0 ? mc : nullptr))) return rc;
  int64_t nA = 0, nB = 0, nC = 0, nZ = 0;
  for (int64_t i = 0; i < n; i++) {
    const int64_t len = off[i + 1] - off[i];
    nA += len >= 1; nB += len >= 2; nC += len >= 3; nZ += len == 0;
  }
  const bool copy_empty = out && out != in && nZ > 0;
  if (nA == 0 && !copy_empty) return C1_OK;
  if (!out) nC = 0;
  const int64_t nR = nA + nB;
  // index lists.  Two passes: encode_signals_impl's (A, B, C, Z), with A and B sorted by the mode byte of their frame when modes
  // are given.  Fused: per signal of >= 1 frame its first frame, index, frame count and first row; per row its unit; C and Z
  const size_t words = fused ? (size_t)(4 * nA + nR + 2 * nC + nZ) : (size_t)(2 * nA + 3 * nB + 3 * nC + nZ);
  uint32_t *h;
  if ((rc = rows_image(ctx, words, &h))) return rc;
  uint32_t *a_src = h, *a_sig = a_src + nA;
  uint32_t *a_cnt = nullptr, *a_first = nullptr, *row_dst = nullptr, *b_src = nullptr, *b_sig = nullptr, *b_row = nullptr, *c_src0, *c_src1 = nullptr, *c_sig, *z_sig;
  if (fused) { a_cnt = a_sig + nA; a_first = a_cnt + nA; row_dst = a_first + nA; c_src0 = row_dst + nR; c_sig = c_src0 + nC; z_sig = c_sig + nC; }
  else { b_src = a_sig + nA; b_sig = b_src + nB; b_row = b_sig + nB; c_src0 = b_row + nB; c_src1 = c_src0 + nC; c_sig = c_src1 + nC; z_sig = c_sig + nC; }
  int64_t a_group[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, b_group[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};   // rows of A / B before mode byte number g
  const bool by_mode = !fused && d_modes;
  if (by_mode) {
    for (int64_t i = 0; i < n; i++) {
      const int64_t f0 = off[i], len = off[i + 1] - f0;
      if (len >= 1) a_group[mode_byte_number(h_modes[f0]) + 1]++;
      if (len >= 2) b_group[mode_byte_number(h_modes[f0 + 1]) + 1]++;
    }
    for (int g = 0; g < 8; g++) { a_group[g + 1] += a_group[g]; b_group[g + 1] += b_group[g]; }
  }
  {
    int64_t a = 0, b = 0, c = 0, z = 0, row = 0;
    int64_t a_at[8], b_at[8];
    for (int g = 0; g < 8; g++) { a_at[g] = a_group[g]; b_at[g] = b_group[g]; }
    for (int64_t i = 0; i < n; i++) {
      const int64_t f0 = off[i], len = off[i + 1] - f0;
      if (len == 0) { z_sig[z++] = (uint32_t)i; continue; }
      if (len >= 3 && out) { c_src0[c] = (uint32_t)(f0 + len - 2); if (c_src1) c_src1[c] = (uint32_t)(f0 + len - 1); c_sig[c] = (uint32_t)i; c++; }
      if (fused) {
        a_src[a] = (uint32_t)f0; a_sig[a] = (uint32_t)i; a_cnt[a] = len >= 2 ? 2u : 1u; a_first[a] = (uint32_t)row;
        row_dst[row++] = (uint32_t)f0;
        if (len >= 2) row_dst[row++] = (uint32_t)(f0 + 1);
        a++;
        continue;
      }
      const int64_t ai = by_mode ? a_at[mode_byte_number(h_modes[f0])]++ : a++;
      a_src[ai] = (uint32_t)f0; a_sig[ai] = (uint32_t)i;
      if (len >= 2) {
        const int64_t bi = by_mode ? b_at[mode_byte_number(h_modes[f0 + 1])]++ : b++;
        b_src[bi] = (uint32_t)(f0 + 1); b_sig[bi] = (uint32_t)i; b_row[bi] = (uint32_t)ai;
      }
    }
  }
  int64_t W = 0;
  if (nA > 0) {
    if ((rc = join_tail(ctx))) return rc;
    const int64_t rows = fused ? nR : nA;
    W = std::max<int64_t>(2, std::min(rows, chunk_for_call(ctx, rows, 1, false)));
    if ((rc = ensure_workspace(ctx, W))) return rc;
  }
  SigCarve cv;
  const size_t o_zero = cv.take(sizeof(c1_enc_state)), o_lists = cv.take(words * sizeof(uint32_t)),
               o_tmp = cv.take((out || fused) ? 0 : (size_t)nA * sizeof(c1_enc_state)), o_tmp2 = cv.take(fused ? 0 : (size_t)nC * sizeof(c1_enc_state)),
               o_units = cv.take((size_t)W * C1_UNIT_BYTES), o_taken = cv.take((size_t)W), o_shifts = cv.take((size_t)W * 52),
               o_dist = cv.take((size_t)W * 2 * sizeof(double)), o_energy = cv.take((size_t)W * sizeof(double)),
               o_weights = cv.take(mc->weights ? (size_t)W * 52 * sizeof(double) : 0);
  if ((rc = ensure_sig(ctx, cv.bytes))) return rc;
  uint8_t *base_p = static_cast<uint8_t *>(ctx->d_sig);
  float *zero = reinterpret_cast<float *>(base_p + o_zero), *tmp = reinterpret_cast<float *>(base_p + o_tmp), *tmp2 = reinterpret_cast<float *>(base_p + o_tmp2);
  const uint32_t *d = reinterpret_cast<uint32_t *>(base_p + o_lists);
  const RowStage st = {base_p + o_taken, reinterpret_cast<int8_t *>(base_p + o_shifts), reinterpret_cast<double *>(base_p + o_dist),
                       reinterpret_cast<double *>(base_p + o_energy), reinterpret_cast<double *>(base_p + o_weights)};
  uint8_t *row_units = units ? base_p + o_units : nullptr;
  HIP_TRY(hipMemsetAsync(zero, 0, sizeof(c1_enc_state), ctx->stream));
  if ((rc = upload_rows(ctx, const_cast<uint32_t *>(d), words))) return rc;
  auto dev = [&](const uint32_t *host_list) { return host_list ? d + (host_list - h) : nullptr; };
  if (fused) {
    // 2. frames 0 and 1 of every signal in one pass: the pool between them stays in the kernel; a chunk of W rows never splits a pair
    for (int64_t a0 = 0; a0 < nA;) {
      const int64_t r0 = a_first[a0];
      int64_t a1 = a0, m = 0;
      while (a1 < nA && m + a_cnt[a1] <= W) m += a_cnt[a1++];
      C1SignalStartsLaunch K;
      memset(&K, 0, sizeof K);
      K.pcm = pcm;
      K.src_rows = dev(a_src) + a0;
      K.in = in ? in : zero;
      K.in_rows = in ? dev(a_sig) + a0 : nullptr;
      K.in_broadcast = in ? 0 : 1;
      K.out = out;
      K.out_rows = dev(a_sig) + a0;
      K.counts = dev(a_cnt) + a0;
      K.first_rows = dev(a_first) + a0;
      K.row_base = r0;
      K.n = a1 - a0;
      K.tables = ctx->d_tables;
      K.opts = ctx->d_opts;
      K.coefs = ctx->d_coefs[0];
      K.side = ctx->d_side[0];
      K.detect = -1;
      K.modes = d_modes;
      { ScopedTiming t(ctx, K_SIGNAL_STARTS); c1k_launch_signal_starts(K, ctx->stream); }
      rows_chain(ctx, m, dev(row_dst) + r0, units, row_units, mc, &st);
      a0 = a1;
    }
  } else {
    // the pools in flight live in `out` at their signal's index, or in scratch at their row of list A when out is NULL
    float *S = out ? out : tmp;
    for (int pass = 0; pass < 2; pass++) {
      // 2. frame 0 of every signal from in[i] (a fresh pool when in is NULL); 3. frame 1 from the pool step 2 left, in place.
      //    With given modes once per mode byte present, over that byte's rows, under that byte's fixed modes
      for (int g = 0; g < (by_mode ? 8 : 1); g++) {
        const int64_t g0 = by_mode ? (pass ? b_group[g] : a_group[g]) : 0;
        const int64_t rows = by_mode ? (pass ? b_group[g + 1] : a_group[g + 1]) - g0 : (pass ? nB : nA);
        if (rows == 0) continue;
        if (by_mode) {
          c1_encode_options one = *opts;
          one.fixed_block_modes[0] = (g & 1) ? 2 : 0; one.fixed_block_modes[1] = (g & 2) ? 2 : 0; one.fixed_block_modes[2] = (g & 4) ? 3 : 0;
          if ((rc = upload_opts(ctx, &one))) return rc;
        }
        if (pass == 0) {
          const bool keep = out || nB;
          float *o = !keep ? nullptr : (out ? out : tmp + g0 * kEncStateFloats);
          rc = encode_rows_pass(ctx, pcm, dev(a_src) + g0, in ? in : zero, in ? dev(a_sig) + g0 : nullptr, !in, o, out ? dev(a_sig) + g0 : nullptr, rows, W,
                                units, row_units, mc, &st);
        } else {
          const uint32_t *at = (out ? dev(b_sig) : dev(b_row)) + g0;
          rc = encode_rows_pass(ctx, pcm, dev(b_src) + g0, S, at, false, S, at, rows, W, units, row_units, mc, &st);
        }
        if (rc) return rc;
      }
    }
  }
  if (out) {
    // 4. signals of three frames and more: the pool after the last frame is a function of the last two frames (state only, from
    //    zeros: c1_enc_stream_get_state does the same); without detection transient_mags keeps what steps 2 and 3 passed through
    ScopedTiming t(ctx, K_SIGNAL_STARTS);
    if (fused) {
      C1SignalStartsLaunch K;
      memset(&K, 0, sizeof K);
      K.pcm = pcm;
      K.src_rows = dev(c_src0);
      K.count_all = 2;
      K.in = zero;
      K.in_broadcast = 1;
      K.out = out;
      K.out_rows = dev(c_sig);
      K.n = nC;
      K.tables = ctx->d_tables;
      K.opts = ctx->d_opts;
      K.state_only = 1;
      K.detect = detect ? 1 : 0;
      K.keep_mags = detect ? 0 : 1;
      c1k_launch_signal_starts(K, ctx->stream);
    } else {
      C1EncStateLaunch K;
      memset(&K, 0, sizeof K);
      K.pcm = pcm;
      K.src_rows = dev(c_src0);
      K.in = zero;
      K.in_broadcast = 1;
      K.out = tmp2;
      K.n = nC;
      K.tables = ctx->d_tables;
      K.opts = ctx->d_opts;
      K.state_only = 1;
      K.detect = 0;                                          // the zero pool's magnitudes pass through: every float of tmp2 is written
      c1k_launch_encode_rows(K, ctx->stream);
      K.src_rows = dev(c_src1);
      K.in = tmp2;
      K.in_broadcast = 0;
      K.out = out;
      K.out_rows = dev(c_sig);
      K.detect = detect ? 1 : 0;
      K.keep_mags = detect ? 0 : 1;
      c1k_launch_encode_rows(K, ctx->stream);
    }
    // empty signals: the pool passes through
    if (copy_empty)
      c1k_launch_copy_rows(reinterpret_cast<uint32_t *>(out), dev(z_sig), reinterpret_cast<const uint32_t *>(in ? in : zero), in ? dev(z_sig) : nullptr,
                           in ? 0 : 1, nZ, kEncStateFloats, ctx->stream);
  }
  HIP_TRY(hipGetLastError());
  return C1_OK;
}

// per-row staging of a mode search over signals, carved from c1_ctx::d_sig: a BestModesCall's outputs over W rows
struct RowStageModes {
  uint8_t *choice, *modes_out, *taken;
  int8_t *shifts;
  double *distortion, *energy;
};

// encode_rows_pass with the mode search of c1_encode_measured_modes_device (bm: candidates, offsets and the call's outputs over
// the units of the concatenation): encode_from_states_modes over row lists.  Per chunk of W rows the from-state row kernel under
// all-long options into the workspace's planes and under all-short options into the search's own (a plane no candidate needs is
// not made), the pools advanced once, by the last of the two; per candidate the composed side record and the allocation chain
// into trial record k; launch_measured_modes into the rows' staging, packing, and one launch that moves unit and outputs to
// units[src[r]].  base: the call's options with neither threshold nor fixed modes.  units (and row_units) may be null
int encode_rows_pass_modes(c1_ctx *ctx, const float *pcm, const uint32_t *src, const float *in, const uint32_t *in_rows, bool bcast,
                           float *out, const uint32_t *out_rows, int64_t rows, int64_t W, const c1_encode_options *base,
                           const BestModesCall *bm, const RowStageModes *st, uint8_t *units, uint8_t *row_units) {
  int rc;
  bool bm_long = false, bm_short = false;                      // some candidate codes a band long / short
  for (int k = 0; k < bm->n; k++) {
    if ((bm->cand[k] & 0x3f) != 0x3a) bm_long = true;
    if ((bm->cand[k] & 0x3f) != 0) bm_short = true;
  }
  BestModesCall sm = *bm;                                      // the same definition, the outputs at the rows' staging
  sm.choice = bm->choice ? st->choice : nullptr;
  sm.modes_out = bm->modes_out ? st->modes_out : nullptr;
  sm.taken = bm->taken ? st->taken : nullptr;
  sm.shifts = bm->shifts ? st->shifts : nullptr;
  sm.distortion = bm->distortion ? st->distortion : nullptr;
  sm.energy = bm->energy ? st->energy : nullptr;
  const int64_t trial_stride = ctx->trial_units * kAllocBytes;
  for (int64_t r0 = 0; r0 < rows; r0 += W) {
    const int64_t m = std::min(W, rows - r0);
    for (int pass = 0; pass < 2; pass++) {                     // 0: all long, 1: all short
      if (!(pass ? bm_short : bm_long)) continue;
      c1_encode_options one = *base;
      one.fixed_block_modes[0] = one.fixed_block_modes[1] = pass ? 2 : 0;
      one.fixed_block_modes[2] = pass ? 3 : 0;
      if ((rc = upload_opts(ctx, &one))) return rc;
      const bool last = pass == 1 || !bm_short;                // the last pass leaves the pools
      C1EncStateLaunch K;
      memset(&K, 0, sizeof K);
      K.pcm = pcm;
      K.src_rows = src + r0;
      K.in = (in_rows || bcast) ? in : in + r0 * kEncStateFloats;
      K.in_rows = in_rows ? in_rows + r0 : nullptr;
      K.in_broadcast = bcast ? 1 : 0;
      K.out = !last ? nullptr : ((!out || out_rows) ? out : out + r0 * kEncStateFloats);
      K.out_rows = (last && out_rows) ? out_rows + r0 : nullptr;
      K.n = m;
      K.tables = ctx->d_tables;
      K.opts = ctx->d_opts;
      K.coefs = pass ? ctx->d_bm_coefs : ctx->d_coefs[0];
      K.side = pass ? ctx->d_bm_side : ctx->d_side[0];
      K.detect = -1;
      ScopedTiming t(ctx, K_SIGNAL_STARTS);
      c1k_launch_encode_rows(K, ctx->stream);
    }
    C1EncodeLaunch L;
    memset(&L, 0, sizeof L);
    L.channels = 1;
    L.frames = m;
    L.tables = ctx->d_tables;
    L.opts = ctx->d_opts;
    L.coefs = ctx->d_coefs[0];
    L.side = ctx->d_side[0];
    L.alloc = ctx->d_alloc[0];
    L.cand = ctx->d_cand[0];
    L.work_count = ctx->d_work[0];
    L.work_list = ctx->d_work[0] + 4;
    L.sel_list = ctx->d_work[0] + 4 + (size_t)ctx->ws_units * 7;
    L.units = row_units;
    for (int k = 0; k < bm->n; k++) {                          // one chain after the other: they share the side plane and the scratch
      { ScopedTiming t(ctx, K_ANALYSIS); c1k_launch_compose_side(L.side, ctx->d_bm_side, m, bm->cand[k], ctx->d_bm_cand_side, ctx->stream); }
      ScopedTiming t(ctx, K_ALLOCATE);
      C1EncodeLaunch A = L;
      A.side = ctx->d_bm_cand_side;
      A.alloc = ctx->d_trial + (size_t)k * trial_stride;
      c1k_launch_allocate(A, ctx->stream);
    }
    launch_measured_modes(ctx, L, ctx->d_trial, trial_stride, &sm, 0, ctx->stream);
    if (row_units) { ScopedTiming t(ctx, K_PACK); c1k_launch_pack(L, false, ctx->stream); }
    ScopedTiming t(ctx, K_SIGNAL_STARTS);
    C1ScatterRowsModesLaunch X;
    memset(&X, 0, sizeof X);
    X.dst_rows = src + r0;
    X.n = m;
    X.n_cand = bm->n;
    if (row_units) { X.units_src = reinterpret_cast<const uint32_t *>(row_units); X.units_dst = reinterpret_cast<uint32_t *>(units); }
    if (bm->choice) { X.choice_src = st->choice; X.choice_dst = bm->choice; }
    if (bm->modes_out) { X.modes_src = st->modes_out; X.modes_dst = bm->modes_out; }
    if (bm->taken) { X.taken_src = st->taken; X.taken_dst = bm->taken; }
    if (bm->shifts) { X.shifts_src = reinterpret_cast<const uint32_t *>(st->shifts); X.shifts_dst = reinterpret_cast<uint32_t *>(bm->shifts); }
    if (bm->distortion) { X.distortion_src = reinterpret_cast<const uint32_t *>(st->distortion); X.distortion_dst = reinterpret_cast<uint32_t *>(bm->distortion); }
    if (bm->energy) { X.energy_src = reinterpret_cast<const uint32_t *>(st->energy); X.energy_dst = reinterpret_cast<uint32_t *>(bm->energy); }
    c1k_launch_scatter_signal_rows_modes(X, ctx->stream);
  }
  return C1_OK;
}

// encode_signals_impl with the measured block-mode search: device pointers but frame_offsets; arguments checked by
// the callers.  bm: the call's candidates, offsets (set) and outputs, over the units of the concatenation.  units may be null.
// Both settings of C1_SIGNAL_STARTS take the two-pass route
int encode_signals_measured_modes_impl(c1_ctx *ctx, int64_t n, const int64_t *off, const float *pcm, const float *in,
                                       const c1_encode_options *opts, const BestModesCall *bm, uint8_t *units, float *out) {
  int rc;
  TimingScope scope(ctx);
  const int64_t total = off[n];
  c1_encode_options base;
  modes_call_opts(*opts, &base);
  // 1. the whole concatenation as one mono stream, as c1_encode_measured_modes_device runs it: every row but those of the first
  //    two frames of a signal is final
  const float *chan[1] = {pcm};
  if ((rc = encode_device_impl(ctx, chan, 1, total, 0, &base, units, nullptr, nullptr, nullptr, nullptr, false, nullptr, nullptr, nullptr, bm))) return rc;
  int64_t nA = 0, nB = 0, nC = 0, nZ = 0;
  for (int64_t i = 0; i < n; i++) {
    const int64_t len = off[i + 1] - off[i];
    nA += len >= 1; nB += len >= 2; nC += len >= 3; nZ += len == 0;
  }
  const bool copy_empty = out && out != in && nZ > 0;
  if (nA == 0 && !copy_empty) return C1_OK;
  if (!out) nC = 0;
  // index lists, as encode_signals_impl's: A = signals of >= 1 frame (frame 0), B = of >= 2 (frame 1), C = of >= 3 (the last
  // two frames), Z = empty ones
  const size_t words = (size_t)(2 * nA + 3 * nB + 3 * nC + nZ);
  uint32_t *h;
  if ((rc = rows_image(ctx, words, &h))) return rc;
  uint32_t *a_src = h, *a_sig = a_src + nA, *b_src = a_sig + nA, *b_sig = b_src + nB, *b_row = b_sig + nB, *c_src0 = b_row + nB,
           *c_src1 = c_src0 + nC, *c_sig = c_src1 + nC, *z_sig = c_sig + nC;
  {
    int64_t a = 0, b = 0, c = 0, z = 0;
    for (int64_t i = 0; i < n; i++) {
      const int64_t f0 = off[i], len = off[i + 1] - f0;
      if (len == 0) { z_sig[z++] = (uint32_t)i; continue; }
      if (len >= 2) { b_src[b] = (uint32_t)(f0 + 1); b_sig[b] = (uint32_t)i; b_row[b] = (uint32_t)a; b++; }
      if (len >= 3 && out) { c_src0[c] = (uint32_t)(f0 + len - 2); c_src1[c] = (uint32_t)(f0 + len - 1); c_sig[c] = (uint32_t)i; c++; }
      a_src[a] = (uint32_t)f0; a_sig[a] = (uint32_t)i; a++;
    }
  }
  // a chunk of W rows: the workspace, the second planes, the candidate side plane and a trial record per unit and candidate
  int64_t W = 0;
  if (nA > 0) {
    if ((rc = join_tail(ctx))) return rc;
    W = std::min(nA, chunk_for_call(ctx, nA, 1, false, bm->n, true));
    if ((rc = ensure_workspace(ctx, W))) return rc;
    if ((rc = ensure_trial_allocs(ctx, W, bm->n))) return rc;
    if ((rc = ensure_best_modes_planes(ctx, W))) return rc;
  }
  SigCarve cv;
  const size_t o_zero = cv.take(sizeof(c1_enc_state)), o_lists = cv.take(words * sizeof(uint32_t)),
               o_tmp = cv.take(out ? 0 : (size_t)nA * sizeof(c1_enc_state)), o_tmp2 = cv.take((size_t)nC * sizeof(c1_enc_state)),
               o_units = cv.take((size_t)W * C1_UNIT_BYTES), o_choice = cv.take((size_t)W), o_modes = cv.take((size_t)W),
               o_taken = cv.take((size_t)W), o_shifts = cv.take((size_t)W * 52),
               o_dist = cv.take((size_t)W * bm->n * 2 * sizeof(double)), o_energy = cv.take((size_t)W * bm->n * sizeof(double));
  if ((rc = ensure_sig(ctx, cv.bytes))) return rc;
  uint8_t *base_p = static_cast<uint8_t *>(ctx->d_sig);
  float *zero = reinterpret_cast<float *>(base_p + o_zero), *tmp = reinterpret_cast<float *>(base_p + o_tmp), *tmp2 = reinterpret_cast<float *>(base_p + o_tmp2);
  uint32_t *d = reinterpret_cast<uint32_t *>(base_p + o_lists);
  const uint32_t *da_src = d, *da_sig = da_src + nA, *db_src = da_sig + nA, *db_sig = db_src + nB, *db_row = db_sig + nB, *dc_src0 = db_row + nB,
                 *dc_src1 = dc_src0 + nC, *dc_sig = dc_src1 + nC, *dz_sig = dc_sig + nC;
  const RowStageModes st = {base_p + o_choice, base_p + o_modes, base_p + o_taken, reinterpret_cast<int8_t *>(base_p + o_shifts),
                            reinterpret_cast<double *>(base_p + o_dist), reinterpret_cast<double *>(base_p + o_energy)};
  uint8_t *row_units = units ? base_p + o_units : nullptr;
  HIP_TRY(hipMemsetAsync(zero, 0, sizeof(c1_enc_state), ctx->stream));
  if ((rc = upload_rows(ctx, d, words))) return rc;
  // the pools in flight live in `out` at their signal's index, or in scratch at their row of list A when out is NULL
  float *S = out ? out : tmp;
  // 2. frame 0 of every signal from in[i] (a fresh pool when in is NULL)
  if ((rc = encode_rows_pass_modes(ctx, pcm, da_src, in ? in : zero, in ? da_sig : nullptr, !in, (out || nB) ? S : nullptr, out ? da_sig : nullptr,
                                   nA, W, &base, bm, &st, units, row_units))) return rc;
  // 3. frame 1 from the pool step 2 left, in place
  if ((rc = encode_rows_pass_modes(ctx, pcm, db_src, S, out ? db_sig : db_row, false, S, out ? db_sig : db_row, nB, W, &base, bm, &st, units,
                                   row_units))) return rc;
  if (out) {
    // 4. signals of three frames and more: the pool after the last frame is a function of the last two frames (state only, from
    //    zeros: c1_enc_stream_get_state does the same); the modes are given, so transient_mags keeps what steps 2 and 3 passed through
    C1EncStateLaunch K;
    memset(&K, 0, sizeof K);
    K.pcm = pcm;
    K.src_rows = dc_src0;
    K.in = zero;
    K.in_broadcast = 1;
    K.out = tmp2;
    K.n = nC;
    K.tables = ctx->d_tables;
    K.opts = ctx->d_opts;
    K.state_only = 1;
    K.detect = 0;                                          // the zero pool's magnitudes pass through: every float of tmp2 is written
    ScopedTiming t(ctx, K_SIGNAL_STARTS);
    c1k_launch_encode_rows(K, ctx->stream);
    K.src_rows = dc_src1;
    K.in = tmp2;
    K.in_broadcast = 0;
    K.out = out;
    K.out_rows = dc_sig;
    K.keep_mags = 1;
    c1k_launch_encode_rows(K, ctx->stream);
    // empty signals: the pool passes through
    if (copy_empty)
      c1k_launch_copy_rows(reinterpret_cast<uint32_t *>(out), dz_sig, reinterpret_cast<const uint32_t *>(in ? in : zero), in ? dz_sig : nullptr,
                           in ? 0 : 1, nZ, kEncStateFloats, ctx->stream);
  }
  HIP_TRY(hipGetLastError());
  return C1_OK;
}

int decode_signals_impl(c1_ctx *ctx, int64_t n, const int64_t *off, const uint8_t *units, const float *in, float *pcm, float *out) {
  int rc;
  TimingScope scope(ctx);
  const int64_t total = off[n];
  // 1. the concatenation as one mono stream: every frame but the first of a signal is final
  float *chan[1] = {pcm};
  if ((rc = c1_decode_device(ctx, units, 1, total, 0, chan))) return rc;
  int64_t nA = 0, nZ = 0;
  for (int64_t i = 0; i < n; i++) { nA += off[i + 1] > off[i]; nZ += off[i + 1] == off[i]; }
  const bool copy_empty = out && out != in && nZ > 0;
  if (nA == 0 && !copy_empty) return C1_OK;
  const size_t words = (size_t)(3 * nA + nZ);
  uint32_t *h;
  if ((rc = rows_image(ctx, words, &h))) return rc;
  uint32_t *a_first = h, *a_last = a_first + nA, *a_sig = a_last + nA, *z_sig = a_sig + nA;
  {
    int64_t a = 0, z = 0;
    for (int64_t i = 0; i < n; i++) {
      if (off[i + 1] == off[i]) { z_sig[z++] = (uint32_t)i; continue; }
      a_first[a] = (uint32_t)off[i]; a_last[a] = (uint32_t)(off[i + 1] - 1); a_sig[a] = (uint32_t)i; a++;
    }
  }
  const int64_t W = std::min(nA, kStateDecodeChunk / 2), per = out ? 2 : 1;       // rows per pass: first units, then last units
  SigCarve cv;
  const size_t o_zero = cv.take(sizeof(c1_dec_state)), o_lists = cv.take(words * sizeof(uint32_t)),
               o_units = cv.take((size_t)(per * W) * C1_UNIT_BYTES), o_fields = cv.take((size_t)(per * W * kFieldInts) * sizeof(int32_t));
  if ((rc = ensure_sig(ctx, cv.bytes))) return rc;
  uint8_t *base = static_cast<uint8_t *>(ctx->d_sig);
  float *zero = reinterpret_cast<float *>(base + o_zero);
  uint32_t *d = reinterpret_cast<uint32_t *>(base + o_lists);
  const uint32_t *da_first = d, *da_last = da_first + nA, *da_sig = da_last + nA, *dz_sig = da_sig + nA;
  uint32_t *g = reinterpret_cast<uint32_t *>(base + o_units);
  HIP_TRY(hipMemsetAsync(zero, 0, sizeof(c1_dec_state), ctx->stream));
  if ((rc = upload_rows(ctx, d, words))) return rc;
  const uint32_t *u32 = reinterpret_cast<const uint32_t *>(units);
  for (int64_t r0 = 0; r0 < nA; r0 += W) {
    const int64_t m = std::min(W, nA - r0);
    const C1FieldPtrs f = field_layout(reinterpret_cast<int32_t *>(base + o_fields), per * m);
    ScopedTiming t(ctx, K_SIGNAL_STARTS);
    c1k_launch_copy_rows(g, nullptr, u32, da_first + r0, 0, m, kUnitDwords, ctx->stream);
    if (out) c1k_launch_copy_rows(g + m * kUnitDwords, nullptr, u32, da_last + r0, 0, m, kUnitDwords, ctx->stream);
    c1k_launch_unpack_units(reinterpret_cast<const uint8_t *>(g), per * m, (int32_t *)f.nbfu, (int32_t *)f.modes, (int32_t *)f.sfi, (int32_t *)f.wl,
                            (int32_t *)f.q, ctx->stream);
    // 2. the first frame of every signal from in[i], straight to its place
    C1DecStateLaunch K;
    memset(&K, 0, sizeof K);
    K.fields = f;
    K.in = in ? in : zero;
    K.in_rows = in ? da_sig + r0 : nullptr;
    K.in_broadcast = in ? 0 : 1;
    K.pcm = pcm;
    K.dst_rows = da_first + r0;
    K.n = m;
    K.tables = ctx->d_tables;
    K.binary32 = ctx->decode_model == C1_DECODE_BINARY32;
    c1k_launch_decode_rows(K, ctx->stream);
    if (out) {
      // 3. the pool after a signal is a function of its last unit alone: state only, from zeros (c1_dec_stream_get_state)
      K.fields = field_unit(f, m);
      K.in = zero;
      K.in_rows = nullptr;
      K.in_broadcast = 1;
      K.pcm = nullptr;
      K.dst_rows = nullptr;
      K.out = out;
      K.out_rows = da_sig + r0;
      c1k_launch_decode_rows(K, ctx->stream);
    }
  }
  if (copy_empty) {
    ScopedTiming t(ctx, K_SIGNAL_STARTS);
    c1k_launch_copy_rows(reinterpret_cast<uint32_t *>(out), dz_sig, reinterpret_cast<const uint32_t *>(in ? in : zero), in ? dz_sig : nullptr,
                         in ? 0 : 1, nZ, kDecStateFloats, ctx->stream);
  }
  HIP_TRY(hipGetLastError());
  return C1_OK;
}
}  // namespace

int c1_encode_signals_device(c1_ctx *ctx, int64_t n, const int64_t *frame_offsets, const float *pcm, const c1_enc_state *in,
                             const c1_encode_options *opts, uint8_t *units, c1_enc_state *out) {
  CTX_GUARD(ctx);
  int rc = ctx_bind(ctx);
  if (rc) return rc;
  int64_t total = 0;
  if ((rc = check_frame_offsets("encode signals", n, frame_offsets, kMaxSignalFrames, &total))) return rc;
  if (!opts) return fail(C1_ERR_ARG, "encode signals: options are NULL");
  if (total > 0 && (!pcm || !units)) return fail(C1_ERR_ARG, "encode signals: %s is NULL", !pcm ? "pcm" : "units");
  if ((uintptr_t)pcm & 15) return fail(C1_ERR_ARG, "encode signals: pcm must be 16-byte aligned on the device");
  if (((uintptr_t)in | (uintptr_t)out | (uintptr_t)units) & 3) return fail(C1_ERR_ARG, "encode signals: units and states must be 4-byte aligned on the device");
  return encode_signals_impl(ctx, n, frame_offsets, pcm, reinterpret_cast<const float *>(in), opts, units, reinterpret_cast<float *>(out));
}

int c1_decode_signals_device(c1_ctx *ctx, int64_t n, const int64_t *frame_offsets, const uint8_t *units, const c1_dec_state *in, float *pcm,
                             c1_dec_state *out) {
  CTX_GUARD(ctx);
  int rc = ctx_bind(ctx);
  if (rc) return rc;
  int64_t total = 0;
  if ((rc = check_frame_offsets("decode signals", n, frame_offsets, kMaxSignalFrames, &total))) return rc;
  if (total > 0 && (!pcm || !units)) return fail(C1_ERR_ARG, "decode signals: %s is NULL", !pcm ? "pcm" : "units");
  if ((uintptr_t)pcm & 15) return fail(C1_ERR_ARG, "decode signals: pcm must be 16-byte aligned on the device");
  if (((uintptr_t)in | (uintptr_t)out | (uintptr_t)units) & 3) return fail(C1_ERR_ARG, "decode signals: units and states must be 4-byte aligned on the device");
  return decode_signals_impl(ctx, n, frame_offsets, units, reinterpret_cast<const float *>(in), pcm, reinterpret_cast<float *>(out));
}

int c1_encode_signals(c1_ctx *ctx, int64_t n, const int64_t *frame_offsets, const float *pcm, const c1_enc_state *in,
                      const c1_encode_options *opts, uint8_t *units, c1_enc_state *out) {
  CTX_GUARD(ctx);
  int rc = ctx_bind(ctx);
  if (rc) return rc;
  int64_t total = 0;
  if ((rc = check_frame_offsets("encode signals", n, frame_offsets, kMaxSignalFramesHost, &total))) return rc;
  if (!opts) return fail(C1_ERR_ARG, "encode signals: options are NULL");
  if (total > 0 && (!pcm || !units)) return fail(C1_ERR_ARG, "encode signals: %s is NULL", !pcm ? "pcm" : "units");
  C1DevEncOpts probe;
  if ((rc = build_encode_opts(*opts, &probe))) return rc;
  if (in && (rc = check_states_finite("encode signals", "signal", in, n, kEncStateFloats, kEncStateFields, 5))) return rc;
  if (n == 0) return C1_OK;
  DeviceScratch ds;
  float *dp, *dst = nullptr; uint8_t *du;
  const size_t T = (size_t)total, N = (size_t)n;
  if ((rc = ds.alloc(&dp, T * 512)) || (rc = ds.alloc(&du, T * C1_UNIT_BYTES))) return rc;
  if ((in || out) && (rc = ds.alloc(&dst, N * kEncStateFloats))) return rc;
  if (T) HIP_TRY(hipMemcpyAsync(dp, pcm, T * 512 * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  if (in) HIP_TRY(hipMemcpyAsync(dst, in, N * sizeof(c1_enc_state), hipMemcpyHostToDevice, ctx->stream));
  if ((rc = encode_signals_impl(ctx, n, frame_offsets, dp, in ? dst : nullptr, opts, du, out ? dst : nullptr))) return rc;
  if (T) HIP_TRY(hipMemcpyAsync(units, du, T * C1_UNIT_BYTES, hipMemcpyDeviceToHost, ctx->stream));
  if (out) HIP_TRY(hipMemcpyAsync(out, dst, N * sizeof(c1_enc_state), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return C1_OK;
}

namespace {
// what the measured arguments of c1_encode_signals_measured* decide alone, as c1_enc_stream_push_measured judges them
int check_signals_measured_args(const char *what, const c1_encode_options *opts, bool have_modes, const int8_t *sf_offsets, int n_offsets,
                                const double *mask_floor, const double *mask_spread, const double *weights) {
  int rc;
  if (mask_spread && !mask_floor) return fail(C1_ERR_ARG, "%s: mask_spread is given without mask_floor", what);
  if (weights && !mask_floor) return fail(C1_ERR_ARG, "%s: weights is given without mask_floor", what);
  if (!sf_offsets && n_offsets != 0) return fail(C1_ERR_ARG, "%s: n_offsets = %d, but sf_offsets is NULL", what, n_offsets);
  if (sf_offsets && (rc = check_sf_offsets(what, sf_offsets, n_offsets))) return rc;
  if (mask_floor && (rc = check_masking(what, mask_floor, mask_spread))) return rc;
  return check_measured_opts(what, opts, !have_modes);
}
}  // namespace

int c1_encode_signals_measured_device(c1_ctx *ctx, int64_t n, const int64_t *frame_offsets, const float *pcm, const c1_enc_state *in,
                                      const c1_encode_options *opts, const uint8_t *modes, const int8_t *sf_offsets, int n_offsets,
                                      const double *mask_floor, const double *mask_spread, uint8_t *units, c1_enc_state *out,
                                      uint8_t *taken, int8_t *shifts, double *distortion, double *energy, double *weights) {
  const char *const what = "c1_encode_signals_measured_device";
  CTX_GUARD(ctx);
  int rc = ctx_bind(ctx);
  if (rc) return rc;
  if ((rc = check_signals_measured_args(what, opts, modes != nullptr, sf_offsets, n_offsets, mask_floor, mask_spread, weights))) return rc;
  int64_t total = 0;
  if ((rc = check_frame_offsets(what, n, frame_offsets, kMaxSignalFrames, &total))) return rc;
  if (!units && !taken && !shifts && !distortion && !energy && !weights) return fail(C1_ERR_ARG, "%s: units, taken, shifts, distortion, energy and weights are all NULL", what);
  if (total > 0 && !pcm) return fail(C1_ERR_ARG, "%s: pcm is NULL", what);
  if ((uintptr_t)pcm & 15) return fail(C1_ERR_ARG, "%s: pcm must be 16-byte aligned on the device", what);
  if (((uintptr_t)in | (uintptr_t)out | (uintptr_t)units | (uintptr_t)shifts) & 3) return fail(C1_ERR_ARG, "%s: units, states and shifts must be 4-byte aligned on the device", what);
  if (((uintptr_t)distortion | (uintptr_t)energy | (uintptr_t)weights) & 7) return fail(C1_ERR_ARG, "%s: distortion, energy and weights must be 8-byte aligned on the device", what);
  int8_t offs[C1_MAX_SF_OFFSETS];                              // the caller's array may change while the call runs
  if (sf_offsets) memcpy(offs, sf_offsets, (size_t)n_offsets);
  static const int8_t kOwnIndex[1] = {0};                      // tables without offsets: the masked call with the single offset 0
  MeasuredCall mc = {taken, distortion, energy};
  if (sf_offsets || mask_floor) {
    mc.sf_offsets = sf_offsets ? offs : kOwnIndex;
    mc.n_offsets = sf_offsets ? n_offsets : 1;
    mc.shifts = shifts;
  } else if (shifts && total > 0) {
    HIP_TRY(hipMemsetAsync(shifts, 0, (size_t)total * 52, ctx->stream));   // c1_encode_measured_*: no index moves
  }
  if (mask_floor) {
    if (total > 0 && (rc = upload_masking(ctx, mask_floor, mask_spread))) return rc;
    mc.mask = ctx->d_mask;
    mc.has_spread = mask_spread != nullptr;
    mc.weights = weights;
  }
  return encode_signals_measured_impl(ctx, n, frame_offsets, pcm, reinterpret_cast<const float *>(in), opts, total > 0 ? modes : nullptr, nullptr, &mc,
                                      units, reinterpret_cast<float *>(out));
}

int c1_encode_signals_measured(c1_ctx *ctx, int64_t n, const int64_t *frame_offsets, const float *pcm, const c1_enc_state *in,
                               const c1_encode_options *opts, const uint8_t *modes, const int8_t *sf_offsets, int n_offsets,
                               const double *mask_floor, const double *mask_spread, uint8_t *units, c1_enc_state *out,
                               uint8_t *taken, int8_t *shifts, double *distortion, double *energy, double *weights) {
  // everything the arguments alone decide comes first and needs neither a context nor a device
  const char *const what = "c1_encode_signals_measured";
  int rc;
  if ((rc = check_signals_measured_args(what, opts, modes != nullptr, sf_offsets, n_offsets, mask_floor, mask_spread, weights))) return rc;
  int64_t total = 0;
  if ((rc = check_frame_offsets(what, n, frame_offsets, kMaxSignalFramesHost, &total))) return rc;
  if (!units && !taken && !shifts && !distortion && !energy && !weights) return fail(C1_ERR_ARG, "%s: units, taken, shifts, distortion, energy and weights are all NULL", what);
  if (total > 0 && !pcm) return fail(C1_ERR_ARG, "%s: pcm is NULL", what);
  if (modes && total > 0 && (rc = check_mode_bytes(what, modes, total, 1))) return rc;
  if (in && (rc = check_states_finite(what, "signal", in, n, kEncStateFloats, kEncStateFields, 5))) return rc;
  if (!ctx) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count == 0) { (void)hipGetLastError(); return fail(C1_ERR_NO_DEVICE, "%s: no HIP device available; this library has no CPU path", what); }
    return fail(C1_ERR_ARG, "context is NULL");
  }
  CTX_GUARD(ctx);
  if ((rc = ctx_bind(ctx))) return rc;
  if (n == 0) return C1_OK;
  // from here on only the device can fail
  DeviceScratch ds;
  float *dp, *dst = nullptr; uint8_t *du = nullptr, *dm = nullptr, *d_taken = nullptr; int8_t *d_shifts = nullptr;
  double *d_dist = nullptr, *d_energy = nullptr, *d_weights = nullptr;
  const size_t T = (size_t)total, N = (size_t)n;
  if ((rc = ds.alloc(&dp, T * 512))) return rc;
  if (units && (rc = ds.alloc(&du, T * C1_UNIT_BYTES))) return rc;
  if (modes && T && (rc = ds.alloc(&dm, T))) return rc;
  if ((in || out) && (rc = ds.alloc(&dst, N * kEncStateFloats))) return rc;
  if (taken && (rc = ds.alloc(&d_taken, T))) return rc;
  if (shifts && (sf_offsets || mask_floor) && (rc = ds.alloc(&d_shifts, T * 52))) return rc;
  if (distortion && (rc = ds.alloc(&d_dist, T * 2))) return rc;
  if (energy && (rc = ds.alloc(&d_energy, T))) return rc;
  if (weights && (rc = ds.alloc(&d_weights, T * 52))) return rc;
  if (T) HIP_TRY(hipMemcpyAsync(dp, pcm, T * 512 * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  if (dm) HIP_TRY(hipMemcpyAsync(dm, modes, T, hipMemcpyHostToDevice, ctx->stream));
  if (in) HIP_TRY(hipMemcpyAsync(dst, in, N * sizeof(c1_enc_state), hipMemcpyHostToDevice, ctx->stream));
  static const int8_t kOwnIndex[1] = {0};                      // tables without offsets: the masked call with the single offset 0
  MeasuredCall mc = {d_taken, d_dist, d_energy};
  if (sf_offsets || mask_floor) {
    mc.sf_offsets = sf_offsets ? sf_offsets : kOwnIndex;
    mc.n_offsets = sf_offsets ? n_offsets : 1;
    mc.shifts = d_shifts;
  }
  if (mask_floor) {
    if (T && (rc = upload_masking(ctx, mask_floor, mask_spread))) return rc;
    mc.mask = ctx->d_mask;
    mc.has_spread = mask_spread != nullptr;
    mc.weights = d_weights;
  }
  if ((rc = encode_signals_measured_impl(ctx, n, frame_offsets, dp, in ? dst : nullptr, opts, dm, dm ? modes : nullptr, &mc, du, out ? dst : nullptr))) return rc;
  if (units && T) HIP_TRY(hipMemcpyAsync(units, du, T * C1_UNIT_BYTES, hipMemcpyDeviceToHost, ctx->stream));
  if (d_taken && T) HIP_TRY(hipMemcpyAsync(taken, d_taken, T, hipMemcpyDeviceToHost, ctx->stream));
  if (d_shifts && T) HIP_TRY(hipMemcpyAsync(shifts, d_shifts, T * 52, hipMemcpyDeviceToHost, ctx->stream));
  if (d_dist && T) HIP_TRY(hipMemcpyAsync(distortion, d_dist, T * 2 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  if (d_energy && T) HIP_TRY(hipMemcpyAsync(energy, d_energy, T * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  if (d_weights && T) HIP_TRY(hipMemcpyAsync(weights, d_weights, T * 52 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  if (out) HIP_TRY(hipMemcpyAsync(out, dst, N * sizeof(c1_enc_state), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  if (shifts && !d_shifts && T) memset(shifts, 0, T * 52);     // c1_encode_measured_*: no index moves
  return C1_OK;
}

namespace {
// what the arguments of c1_encode_signals_measured_modes* decide alone, as c1_enc_stream_push_measured_modes judges them
int check_signals_measured_modes_args(const char *what, const c1_encode_options *opts, const uint8_t *cand_modes, int n_cand,
                                      const int8_t *sf_offsets, int n_offsets) {
  int rc;
  if ((rc = check_mode_candidates(what, cand_modes, n_cand))) return rc;
  if (!sf_offsets && n_offsets != 0) return fail(C1_ERR_ARG, "%s: n_offsets = %d, but sf_offsets is NULL", what, n_offsets);
  if (sf_offsets && (rc = check_sf_offsets(what, sf_offsets, n_offsets))) return rc;
  return check_measured_opts(what, opts, false);
}
}  // namespace

int c1_encode_signals_measured_modes_device(c1_ctx *ctx, int64_t n, const int64_t *frame_offsets, const float *pcm, const c1_enc_state *in,
                                            const c1_encode_options *opts, const uint8_t *cand_modes, int n_cand, const int8_t *sf_offsets,
                                            int n_offsets, uint8_t *units, c1_enc_state *out, uint8_t *choice, uint8_t *modes_out,
                                            uint8_t *taken, int8_t *shifts, double *distortion, double *energy) {
  const char *const what = "c1_encode_signals_measured_modes_device";
  CTX_GUARD(ctx);
  int rc = ctx_bind(ctx);
  if (rc) return rc;
  if ((rc = check_signals_measured_modes_args(what, opts, cand_modes, n_cand, sf_offsets, n_offsets))) return rc;
  int64_t total = 0;
  if ((rc = check_frame_offsets(what, n, frame_offsets, kMaxSignalFrames, &total))) return rc;
  if (!units && !choice && !modes_out && !taken && !shifts && !distortion && !energy)
    return fail(C1_ERR_ARG, "%s: units, choice, modes_out, taken, shifts, distortion and energy are all NULL", what);
  if (total > 0 && !pcm) return fail(C1_ERR_ARG, "%s: pcm is NULL", what);
  if ((uintptr_t)pcm & 15) return fail(C1_ERR_ARG, "%s: pcm must be 16-byte aligned on the device", what);
  if (((uintptr_t)in | (uintptr_t)out | (uintptr_t)units | (uintptr_t)shifts) & 3) return fail(C1_ERR_ARG, "%s: units, states and shifts must be 4-byte aligned on the device", what);
  if (((uintptr_t)distortion | (uintptr_t)energy) & 7) return fail(C1_ERR_ARG, "%s: distortion and energy must be 8-byte aligned on the device", what);
  static const int8_t kOwnIndex[1] = {0};                      // no offsets: the search over the plain measured allocation
  uint8_t cand[C1_MAX_MODE_CANDIDATES];                        // the caller's arrays may change while the call runs
  int8_t offs[C1_MAX_SF_OFFSETS];
  memcpy(cand, cand_modes, (size_t)n_cand);
  if (sf_offsets) memcpy(offs, sf_offsets, (size_t)n_offsets);
  BestModesCall bm = {n_cand, cand, choice, modes_out, distortion, energy};
  bm.sf_offsets = sf_offsets ? offs : kOwnIndex;
  bm.n_offsets = sf_offsets ? n_offsets : 1;
  bm.taken = taken;
  bm.shifts = shifts;                                          // a single offset 0 moves no index: zeros
  return encode_signals_measured_modes_impl(ctx, n, frame_offsets, pcm, reinterpret_cast<const float *>(in), opts, &bm, units,
                                            reinterpret_cast<float *>(out));
}

int c1_encode_signals_measured_modes(c1_ctx *ctx, int64_t n, const int64_t *frame_offsets, const float *pcm, const c1_enc_state *in,
                                     const c1_encode_options *opts, const uint8_t *cand_modes, int n_cand, const int8_t *sf_offsets,
                                     int n_offsets, uint8_t *units, c1_enc_state *out, uint8_t *choice, uint8_t *modes_out, uint8_t *taken,
                                     int8_t *shifts, double *distortion, double *energy) {
  // everything the arguments alone decide comes first and needs neither a context nor a device
  const char *const what = "c1_encode_signals_measured_modes";
  int rc;
  if ((rc = check_signals_measured_modes_args(what, opts, cand_modes, n_cand, sf_offsets, n_offsets))) return rc;
  int64_t total = 0;
  if ((rc = check_frame_offsets(what, n, frame_offsets, kMaxSignalFramesHost, &total))) return rc;
  if (!units && !choice && !modes_out && !taken && !shifts && !distortion && !energy)
    return fail(C1_ERR_ARG, "%s: units, choice, modes_out, taken, shifts, distortion and energy are all NULL", what);
  if (total > 0 && !pcm) return fail(C1_ERR_ARG, "%s: pcm is NULL", what);
  if (in && (rc = check_states_finite(what, "signal", in, n, kEncStateFloats, kEncStateFields, 5))) return rc;
  if (!ctx) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count == 0) { (void)hipGetLastError(); return fail(C1_ERR_NO_DEVICE, "%s: no HIP device available; this library has no CPU path", what); }
    return fail(C1_ERR_ARG, "context is NULL");
  }
  CTX_GUARD(ctx);
  if ((rc = ctx_bind(ctx))) return rc;
  if (n == 0) return C1_OK;
  // from here on only the device can fail
  DeviceScratch ds;
  float *dp, *dst = nullptr; uint8_t *du = nullptr, *d_choice = nullptr, *d_modes = nullptr, *d_taken = nullptr; int8_t *d_shifts = nullptr;
  double *d_dist = nullptr, *d_energy = nullptr;
  const size_t T = (size_t)total, N = (size_t)n, C = (size_t)n_cand;
  if ((rc = ds.alloc(&dp, T * 512))) return rc;
  if (units && (rc = ds.alloc(&du, T * C1_UNIT_BYTES))) return rc;
  if ((in || out) && (rc = ds.alloc(&dst, N * kEncStateFloats))) return rc;
  if (choice && (rc = ds.alloc(&d_choice, T))) return rc;
  if (modes_out && (rc = ds.alloc(&d_modes, T))) return rc;
  if (taken && (rc = ds.alloc(&d_taken, T))) return rc;
  if (shifts && (rc = ds.alloc(&d_shifts, T * 52))) return rc;
  if (distortion && (rc = ds.alloc(&d_dist, T * C * 2))) return rc;
  if (energy && (rc = ds.alloc(&d_energy, T * C))) return rc;
  if (T) HIP_TRY(hipMemcpyAsync(dp, pcm, T * 512 * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  if (in) HIP_TRY(hipMemcpyAsync(dst, in, N * sizeof(c1_enc_state), hipMemcpyHostToDevice, ctx->stream));
  static const int8_t kOwnIndex[1] = {0};                      // no offsets: the search over the plain measured allocation
  BestModesCall bm = {n_cand, cand_modes, d_choice, d_modes, d_dist, d_energy};
  bm.sf_offsets = sf_offsets ? sf_offsets : kOwnIndex;
  bm.n_offsets = sf_offsets ? n_offsets : 1;
  bm.taken = d_taken;
  bm.shifts = d_shifts;
  if ((rc = encode_signals_measured_modes_impl(ctx, n, frame_offsets, dp, in ? dst : nullptr, opts, &bm, du, out ? dst : nullptr))) return rc;
  if (units && T) HIP_TRY(hipMemcpyAsync(units, du, T * C1_UNIT_BYTES, hipMemcpyDeviceToHost, ctx->stream));
  if (choice && T) HIP_TRY(hipMemcpyAsync(choice, d_choice, T, hipMemcpyDeviceToHost, ctx->stream));
  if (modes_out && T) HIP_TRY(hipMemcpyAsync(modes_out, d_modes, T, hipMemcpyDeviceToHost, ctx->stream));
  if (taken && T) HIP_TRY(hipMemcpyAsync(taken, d_taken, T, hipMemcpyDeviceToHost, ctx->stream));
  if (shifts && T) HIP_TRY(hipMemcpyAsync(shifts, d_shifts, T * 52, hipMemcpyDeviceToHost, ctx->stream));
  if (distortion && T) HIP_TRY(hipMemcpyAsync(distortion, d_dist, T * C * 2 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  if (energy && T) HIP_TRY(hipMemcpyAsync(energy, d_energy, T * C * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  if (out) HIP_TRY(hipMemcpyAsync(out, dst, N * sizeof(c1_enc_state), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return C1_OK;
}

int c1_decode_signals(c1_ctx *ctx, int64_t n, const int64_t *frame_offsets, const uint8_t *units, const c1_dec_state *in, float *pcm,
                      c1_dec_state *out) {
  CTX_GUARD(ctx);
  int rc = ctx_bind(ctx);
  if (rc) return rc;
  int64_t total = 0;
  if ((rc = check_frame_offsets("decode signals", n, frame_offsets, kMaxSignalFramesHost, &total))) return rc;
  if (total > 0 && (!pcm || !units)) return fail(C1_ERR_ARG, "decode signals: %s is NULL", !pcm ? "pcm" : "units");
  if (in && (rc = check_states_finite("decode signals", "signal", in, n, kDecStateFloats, kDecStateFields, 4))) return rc;
  if (n == 0) return C1_OK;
  DeviceScratch ds;
  float *dp, *dst = nullptr; uint8_t *du;
  const size_t T = (size_t)total, N = (size_t)n;
  if ((rc = ds.alloc(&dp, T * 512)) || (rc = ds.alloc(&du, T * C1_UNIT_BYTES))) return rc;
  if ((in || out) && (rc = ds.alloc(&dst, N * kDecStateFloats))) return rc;
  if (T) HIP_TRY(hipMemcpyAsync(du, units, T * C1_UNIT_BYTES, hipMemcpyHostToDevice, ctx->stream));
  if (in) HIP_TRY(hipMemcpyAsync(dst, in, N * sizeof(c1_dec_state), hipMemcpyHostToDevice, ctx->stream));
  if ((rc = decode_signals_impl(ctx, n, frame_offsets, du, in ? dst : nullptr, dp, out ? dst : nullptr))) return rc;
  if (T) HIP_TRY(hipMemcpyAsync(pcm, dp, T * 512 * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  if (out) HIP_TRY(hipMemcpyAsync(out, dst, N * sizeof(c1_dec_state), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return C1_OK;
}

int c1_enc_stream_get_state(c1_enc_stream *s, c1_enc_state *out) {
  if (!s) return fail(C1_ERR_ARG, "stream is NULL");
  c1_ctx *ctx = s->ctx;
  CTX_GUARD(ctx);
  int rc = ctx_bind(ctx);
  if (rc) return rc;
  if (!out) return fail(C1_ERR_ARG, "out is NULL");
  if ((rc = enc_stream_current_state(s))) return rc;
  HIP_TRY(hipMemcpyAsync(out, s->d_state, (size_t)s->channels * sizeof(c1_enc_state), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return C1_OK;
}

int c1_enc_stream_set_state(c1_enc_stream *s, const c1_enc_state *in) {
  if (!s) return fail(C1_ERR_ARG, "stream is NULL");
  c1_ctx *ctx = s->ctx;
  CTX_GUARD(ctx);
  int rc = ctx_bind(ctx);
  if (rc) return rc;
  if (!in) return fail(C1_ERR_ARG, "in is NULL");
  if ((rc = check_states_finite("encoder state", "channel", in, s->channels, kEncStateFloats, kEncStateFields, 5))) return rc;
  if ((rc = enc_stream_state_buffer(s))) return rc;
  HIP_TRY(hipMemcpyAsync(s->d_state, in, (size_t)s->channels * sizeof(c1_enc_state), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  s->state_frames = 2;
  s->state_live = true;
  return C1_OK;
}

int c1_dec_stream_get_state(c1_dec_stream *s, c1_dec_state *out) {
  if (!s) return fail(C1_ERR_ARG, "stream is NULL");
  c1_ctx *ctx = s->ctx;
  CTX_GUARD(ctx);
  int rc = ctx_bind(ctx);
  if (rc) return rc;
  if (!out) return fail(C1_ERR_ARG, "out is NULL");
  const size_t bytes = (size_t)s->channels * sizeof(c1_dec_state);
  if (!s->restored && !s->have_prev) { memset(out, 0, bytes); return C1_OK; }   // a fresh pool
  if ((rc = dec_stream_state_buffer(s))) return rc;
  const float *src = s->d_state;
  if (!s->restored) {
    // what a frame leaves is a function of that frame alone: decode the previous frame once more, state output only, in the
    // arithmetic of the model that decoded it
    if ((rc = dec_stream_prev_fields(s))) return rc;
    float *zero = s->d_state + (size_t)s->channels * kDecStateFloats, *tmp = zero + (size_t)s->channels * kDecStateFloats;
    C1DecStateLaunch K;
    memset(&K, 0, sizeof K);
    K.fields = s->prev_fields;
    K.in = zero;
    K.out = tmp;
    K.n = s->channels;
    K.tables = ctx->d_tables;
    K.binary32 = s->prev_model == C1_DECODE_BINARY32;
    c1k_launch_decode_from_states(K, ctx->stream);
    HIP_TRY(hipGetLastError());
    src = tmp;
  }
  HIP_TRY(hipMemcpyAsync(out, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return C1_OK;
}

int c1_dec_stream_set_state(c1_dec_stream *s, const c1_dec_state *in) {
  if (!s) return fail(C1_ERR_ARG, "stream is NULL");
  c1_ctx *ctx = s->ctx;
  CTX_GUARD(ctx);
  int rc = ctx_bind(ctx);
  if (rc) return rc;
  if (!in) return fail(C1_ERR_ARG, "in is NULL");
  if ((rc = check_states_finite("decoder state", "channel", in, s->channels, kDecStateFloats, kDecStateFields, 4))) return rc;
  if ((rc = dec_stream_state_buffer(s))) return rc;
  HIP_TRY(hipMemcpyAsync(s->d_state, in, (size_t)s->channels * sizeof(c1_dec_state), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  s->restored = true;
  return C1_OK;
}

// ---- formats either side of the path ---------------------------------------------------------------------
int c1_pcm_from_int_device(c1_ctx *ctx, const void *interleaved, int bits, int channels, int64_t samples_per_channel,
                           float *const *pcm) {
  CTX_GUARD(ctx);
  int rc = ctx_bind(ctx);
  if (rc) return rc;
  if ((rc = check_channels(channels))) return rc;
  if (bits != 16 && bits != 24 && bits != 32) return fail(C1_ERR_ARG, "bits must be 16, 24 or 32, got %d", bits);
  if (samples_per_channel < 0) return fail(C1_ERR_ARG, "samples_per_channel must be >= 0");
  if (samples_per_channel == 0) return C1_OK;
  if (!interleaved || !pcm || !pcm[0] || (channels == 2 && !pcm[1])) return fail(C1_ERR_ARG, "NULL buffer");
  c1k_launch_pcm_from_int(interleaved, bits, channels, samples_per_channel, pcm, ctx->stream);
  HIP_TRY(hipGetLastError());
  return C1_OK;
}

int c1_pcm_to_int16_device(c1_ctx *ctx, const float *const *pcm, int channels, int64_t samples_per_channel,
                           int16_t *interleaved) {
  CTX_GUARD(ctx);
  int rc = ctx_bind(ctx);
  if (rc) return rc;
  if ((rc = check_channels(channels))) return rc;
  if (samples_per_channel < 0) return fail(C1_ERR_ARG, "samples_per_channel must be >= 0");
  if (samples_per_channel == 0) return C1_OK;
  if (!interleaved || !pcm || !pcm[0] || (channels == 2 && !pcm[1])) return fail(C1_ERR_ARG, "NULL buffer");
  if (channels == 2 && ((uintptr_t)interleaved & 3)) return fail(C1_ERR_ARG, "stereo int16 output must be 4-byte aligned");
  c1k_launch_pcm_to_int16(pcm, channels, samples_per_channel, interleaved, ctx->stream);
  HIP_TRY(hipGetLastError());
  return C1_OK;
}

int c1_aea_header(const char *title, uint32_t unit_count, int channels, uint8_t out[2048]) {
  if (!out) return fail(C1_ERR_ARG, "out is NULL");
  memset(out, 0, 2048);
  out[0] = 0x00; out[1] = 0x08; out[2] = 0x00; out[3] = 0x00;          // AEA_MAGIC
  if (title) {
    size_t n = strlen(title);
    if (n > 255) n = 255;                                               // AEA_TITLE_SIZE - 1
    memcpy(out + 4, title, n);
  }
  out[260] = (uint8_t)unit_count; out[261] = (uint8_t)(unit_count >> 8);
  out[262] = (uint8_t)(unit_count >> 16); out[263] = (uint8_t)(unit_count >> 24);
  out[264] = (uint8_t)channels;
  return C1_OK;
}

// ---- synthetic input ----------------------------------------------------------------------------------
int c1_generate_device(c1_ctx *ctx, int signal, uint32_t seed, int64_t frames, float *pcm) {
  CTX_GUARD(ctx);
  int rc = ctx_bind(ctx);
  if (rc) return rc;
  if (frames < 0) return fail(C1_ERR_ARG, "frames must be >= 0");
  if (frames == 0) return C1_OK;
  if (!pcm || ((uintptr_t)pcm & 15)) return fail(C1_ERR_ARG, "pcm must be a 16-byte aligned device pointer");
  if (seed == 0) return fail(C1_ERR_ARG, "xorshift32 seed must be non-zero");
  if (signal != C1_SIGNAL_WHITE && signal != C1_SIGNAL_PINK_BURSTS && signal != C1_SIGNAL_MIXED && signal != C1_SIGNAL_PARTIALS) return fail(C1_ERR_ARG, "unknown signal %d", signal);
  std::vector<uint32_t> white_states, pink_states;
  if (signal == C1_SIGNAL_WHITE || signal == C1_SIGNAL_MIXED) {
    // one draw per sample: state before frame f = T^(512 f) seed
    const XsMatrix jump = xs_power(512);
    white_states.resize((size_t)frames);
    uint32_t s = seed;
    for (int64_t f = 0; f < frames; f++) { white_states[(size_t)f] = s; s = jump.apply(s); }
  }
  if (signal == C1_SIGNAL_PINK_BURSTS || signal == C1_SIGNAL_MIXED) {
    // 512-frame segments; per 8 frames the generator draws 8*512 + 256 values, so the PRNG state at the
    // start of every segment is the exact continuation; the integrator restarts from 0 there
    const int64_t segs = (frames + 511) / 512;
    const XsMatrix jump = xs_power(64ull * (8 * 512 + 256));
    pink_states.resize((size_t)segs);
    uint32_t s = seed;
    for (int64_t k = 0; k < segs; k++) { pink_states[(size_t)k] = s; s = jump.apply(s); }
  }
  uint32_t *d_states = nullptr;
  const size_t nw = white_states.size(), np = pink_states.size();
  HIP_TRY(hipMalloc(&d_states, (nw + np + 1) * sizeof(uint32_t)));
  hipError_t e = hipSuccess;
  if (nw) e = hipMemcpy(d_states, white_states.data(), nw * sizeof(uint32_t), hipMemcpyHostToDevice);
  if (e == hipSuccess && np) e = hipMemcpy(d_states + nw, pink_states.data(), np * sizeof(uint32_t), hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    if (signal == C1_SIGNAL_WHITE) c1k_launch_generate_white(d_states, frames, pcm, 15, 0.5, ctx->stream);
    else if (signal == C1_SIGNAL_PINK_BURSTS) c1k_launch_generate_pink(d_states + nw, frames, pcm, 15, ctx->stream);
    else if (signal == C1_SIGNAL_PARTIALS) c1k_launch_generate_sines(frames, pcm, 15, seed, ctx->stream);
    else {
      // mixed corpus (BASELINE configs[3]): 512-frame segments cycling white noise / pink noise with bursts /
      // stationary partials / quiet white noise
      c1k_launch_generate_white(d_states, frames, pcm, 1, 0.5, ctx->stream);
      c1k_launch_generate_pink(d_states + nw, frames, pcm, 2, ctx->stream);
      c1k_launch_generate_sines(frames, pcm, 4, seed, ctx->stream);
      c1k_launch_generate_white(d_states, frames, pcm, 8, 0.02, ctx->stream);
    }
    e = hipStreamSynchronize(ctx->stream);
  }
  hipFree(d_states);
  if (e != hipSuccess) return fail(C1_ERR_HIP, "generate: %s", hipGetErrorString(e));
  return C1_OK;
}

}  // extern "C"
