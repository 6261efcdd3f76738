// c1_detect_core.h -- the exact transient detector's device code (blockSelectorStage, encoder.js:111-152; analysis/transient.js),
// shared by the detection kernels of c1_k_detect.hip and the block-selection stage of c1_k_encode_stages.hip: Math.log / exp /
// log1p / log10 as the reference's engine evaluates them, the radix-8 transient FFT in the reference's rounding, the per-bin
// feature terms and their 18 sequential sums, and the per-band decision from the sums of a frame and of its predecessor.
#pragma once
#include "c1_device.h"

namespace {

__device__ __forceinline__ int tslot(int pos) { return pos + (pos >> 3); }

// =====================================================================================================
// Math.log / exp / log1p / log10 as the reference's engine evaluates them (transient.js:129, :137, :185, :211).
// V8 (src/base/ieee754.cc) ports the published fdlibm algorithms; they are not correctly rounded, so another libm
// returns a neighbouring double for 1-7 % of the arguments.  These restate the same algorithms operation for
// operation (contraction is off in this file); tests/test_gpu_parity.py checks them bit for bit against V8's results
// (tests/golden/libm_v8_*.bin) through c1_libm_device.
// =====================================================================================================
__device__ __forceinline__ double js_with_hi(double x, int hi) { return __hiloint2double(hi, __double2loint(x)); }
constexpr double kLn2Hi = 6.93147180369123816490e-01, kLn2Lo = 1.90821492927058770002e-10, kTwo54 = 1.80143985094819840000e+16;

// e_log.c.  The four return expressions of the main path are one: with dk = 0 the k != 0 forms reduce to the k == 0 ones
// exactly (0 - (a - f) == f - a, P + 0 == P), and the two mantissa ranges differ in two operands.
__device__ __forceinline__ double js_log(double x) {
  constexpr double Lg1 = 6.666666666666735130e-01, Lg2 = 3.999999999940941908e-01, Lg3 = 2.857142874366239149e-01,
                   Lg4 = 2.222219843214978396e-01, Lg5 = 1.818357216161805012e-01, Lg6 = 1.531383769920937332e-01,
                   Lg7 = 1.479819860511658591e-01;
  int hx = __double2hiint(x), k = 0;
  if (hx < 0x00100000) {
    if (((hx & 0x7fffffff) | __double2loint(x)) == 0) return -__builtin_huge_val();
    if (hx < 0) return __builtin_nan("");
    k = -54; x *= kTwo54; hx = __double2hiint(x);
  }
  if (hx >= 0x7ff00000) return x + x;
  k += (hx >> 20) - 1023;
  hx &= 0x000fffff;
  const int i = (hx + 0x95f64) & 0x100000;
  x = js_with_hi(x, hx | (i ^ 0x3ff00000));
  k += (i >> 20);
  const double f = x - 1.0, dk = (double)k;
  const double hi = dk * kLn2Hi, lo = dk * kLn2Lo;
  if ((0x000fffff & (2 + hx)) < 3) {
    if (f == 0.0) return hi + lo;
    const double R = f * f * (0.5 - 0.33333333333333333 * f);
    return hi - ((R - lo) - f);
  }
  const double s = f / (2.0 + f), z = s * s, w = z * z;
  const double t1 = w * (Lg2 + w * (Lg4 + w * Lg6));
  const double t2 = z * (Lg1 + w * (Lg3 + w * (Lg5 + w * Lg7)));
  const double R = t2 + t1;
  const bool mid = ((hx - 0x6147a) | (0x6b851 - hx)) > 0;
  const double hfsq = 0.5 * f * f;
  const double P = s * ((mid ? hfsq : f) + (mid ? R : -R));
  const double Q = mid ? hfsq - (P + lo) : P - lo;
  return hi - (Q - f);
}

// e_exp.c
__device__ double js_exp(double x) {
  constexpr double o_threshold = 7.09782712893383973096e+02, u_threshold = -7.45133219101941108420e+02, invln2 = 1.44269504088896338700e+00,
                   P1 = 1.66666666666666019037e-01, P2 = -2.77777777770155933842e-03, P3 = 6.61375632143793436117e-05,
                   P4 = -1.65339022054652515390e-06, P5 = 4.13813679705723846039e-08, E = 2.718281828459045,
                   huge = 1.0e+300, twom1000 = 9.33263618503218878990e-302, two1023 = 8.988465674311579539e307;
  double hi = 0.0, lo = 0.0;
  int k = 0;
  uint32_t hx = (uint32_t)__double2hiint(x);
  const int xsb = (int)(hx >> 31);
  hx &= 0x7fffffffu;
  if (hx >= 0x40862E42u) {
    if (hx >= 0x7ff00000u) {
      if (((hx & 0xfffffu) | (uint32_t)__double2loint(x)) != 0) return x + x;
      return xsb == 0 ? x : 0.0;
    }
    if (x > o_threshold) return huge * huge;
    if (x < u_threshold) return twom1000 * twom1000;
  }
  if (hx > 0x3fd62e42u) {
    if (hx < 0x3FF0A2B2u) {
      if (x == 1.0) return E;
      hi = x - (xsb ? -kLn2Hi : kLn2Hi); lo = xsb ? -kLn2Lo : kLn2Lo; k = 1 - xsb - xsb;
    } else {
      k = (int)(invln2 * x + (xsb ? -0.5 : 0.5));
      const double t = (double)k;
      hi = x - t * kLn2Hi;
      lo = t * kLn2Lo;
    }
    x = hi - lo;
  } else if (hx < 0x3e300000u) {
    if (huge + x > 1.0) return 1.0 + x;
  }
  const double t = x * x;
  const double twopk = __hiloint2double(0x3ff00000 + ((k >= -1021 ? k : k + 1000) << 20), 0);
  const double c = x - t * (P1 + t * (P2 + t * (P3 + t * (P4 + t * P5))));
  if (k == 0) return 1.0 - ((x * c) / (c - 2.0) - x);
  const double y = 1.0 - ((lo - (x * c) / (2.0 - c)) - hi);
  if (k >= -1021) {
    if (k == 1024) return y * 2.0 * two1023;
    return y * twopk;
  }
  return y * twopk * twom1000;
}

// s_log1p.c
__device__ double js_log1p(double x) {
  constexpr double Lp1 = 6.666666666666735130e-01, Lp2 = 3.999999999940941908e-01, Lp3 = 2.857142874366239149e-01,
                   Lp4 = 2.222219843214978396e-01, Lp5 = 1.818357216161805012e-01, Lp6 = 1.531383769920937332e-01,
                   Lp7 = 1.479819860511658591e-01;
  double f = 0.0, c = 0.0, u;
  int hu = 0, k = 1;
  const int hx = __double2hiint(x), ax = hx & 0x7fffffff;
  if (hx < 0x3FDA827A) {
    if (ax >= 0x3ff00000) {
      if (x == -1.0) return -__builtin_huge_val();
      return __builtin_nan("");
    }
    if (ax < 0x3e200000) {
      if (kTwo54 + x > 0.0 && ax < 0x3c900000) return x;
      return x - x * x * 0.5;
    }
    if (hx > 0 || hx <= (int)0xbfd2bec4) { k = 0; f = x; hu = 1; }
  }
  if (hx >= 0x7ff00000) return x + x;
  if (k != 0) {
    if (hx < 0x43400000) {
      u = 1.0 + x;
      hu = __double2hiint(u);
      k = (hu >> 20) - 1023;
      c = (k > 0) ? 1.0 - (u - x) : x - (u - 1.0);
      c /= u;
    } else {
      u = x;
      hu = __double2hiint(u);
      k = (hu >> 20) - 1023;
      c = 0.0;
    }
    hu &= 0x000fffff;
    if (hu < 0x6a09e) {
      u = js_with_hi(u, hu | 0x3ff00000);
    } else {
      k += 1;
      u = js_with_hi(u, hu | 0x3fe00000);
      hu = (0x00100000 - hu) >> 2;
    }
    f = u - 1.0;
  }
  const double hfsq = 0.5 * f * f, dk = (double)k;
  if (hu == 0) {
    if (f == 0.0) {
      if (k == 0) return 0.0;
      c += dk * kLn2Lo;
      return dk * kLn2Hi + c;
    }
    const double R = hfsq * (1.0 - 0.66666666666666666 * f);
    if (k == 0) return f - R;
    return dk * kLn2Hi - ((R - (dk * kLn2Lo + c)) - f);
  }
  const double s = f / (2.0 + f), z = s * s;
  const double R = z * (Lp1 + z * (Lp2 + z * (Lp3 + z * (Lp4 + z * (Lp5 + z * (Lp6 + z * Lp7))))));
  if (k == 0) return f - (hfsq - s * (hfsq + R));
  return dk * kLn2Hi - ((hfsq - (s * (hfsq + R) + (dk * kLn2Lo + c))) - f);
}

// e_log10.c as V8 carries it (log of the normalised argument, then the exponent in two pieces)
__device__ double js_log10(double x) {
  constexpr double ivln10 = 4.34294481903251816668e-01, log10_2hi = 3.01029995663611771306e-01, log10_2lo = 3.69423907715893078616e-13;
  int hx = __double2hiint(x), k = 0;
  uint32_t lx = (uint32_t)__double2loint(x);
  if (hx < 0x00100000) {
    if (((hx & 0x7fffffff) | lx) == 0) return -__builtin_huge_val();
    if (hx < 0) return __builtin_nan("");
    k = -54; x *= kTwo54; hx = __double2hiint(x); lx = (uint32_t)__double2loint(x);
  }
  if (hx >= 0x7ff00000) return x + x;
  if (hx == 0x3ff00000 && lx == 0) return 0.0;
  k += (hx >> 20) - 1023;
  const int i = (int)(((uint32_t)k & 0x80000000u) >> 31);
  hx = (hx & 0x000fffff) | ((0x3ff - i) << 20);
  const double y = (double)(k + i);
  x = __hiloint2double(hx, (int)lx);
  const double z = y * log10_2lo + ivln10 * js_log(x);
  return z + y * log10_2hi;
}

// ---- lane-only geometry of the transient FFT: lanes 0..15 band 0 (128 points), 16..31 band 1, 32..63 band 2 (256);
// eight points per lane and round
struct TGeom {
  int band, g, S;          // S = N/8: sample stride of round A, point stride of round C
  int src;                 // band sample of the lane's first round-A input (bit-reversed group)
  int za, zb, zc, zc_stride;
  int twb, twc, twc_stride, twd;             // byte offsets into fft_tw (binary64 pairs)
  int twb32, twc32, twc32_stride, twd32;     // the same entries of tw32 (binary32 pairs)
  int mag;                 // magnitude index of the lane's first bin; the next bins are S further each
};
__device__ __forceinline__ TGeom tfft_geometry(int lane0) {
  TGeom G;
  G.band = lane0 < 16 ? 0 : (lane0 < 32 ? 1 : 2);
  G.g = lane0 - (G.band == 0 ? 0 : (G.band == 1 ? 16 : 32));
  G.S = G.band == 2 ? 32 : 16;
  G.src = (G.band == 0 ? 0 : (G.band == 1 ? 128 : 256)) + bitrev(G.g, G.band == 2 ? 5 : 4);
  const int pbase = G.band == 0 ? 0 : (G.band == 1 ? 128 : 256);
  G.za = tslot(pbase + 8 * G.g);
  G.zb = tslot(pbase + 64 * (G.g >> 3) + (G.g & 7));
  G.zc = tslot(pbase + G.g);
  G.zc_stride = G.S + G.S / 8;
  const int eb = 7 + (G.g & 7), ec = (G.band == 2 ? 127 : 63) + G.g, ed = 63 + (G.g & 31);
  G.twb = (int)offsetof(C1DevTables, fft_tw) + 16 * eb;
  G.twc = (int)offsetof(C1DevTables, fft_tw) + 16 * ec;
  G.twc_stride = 16 * G.S;
  G.twd = (int)offsetof(C1DevTables, fft_tw) + 16 * ed;
  G.twb32 = (int)offsetof(C1DevTables, tw32) + 8 * eb;
  G.twc32 = (int)offsetof(C1DevTables, tw32) + 8 * ec;
  G.twc32_stride = 8 * G.S;
  G.twd32 = (int)offsetof(C1DevTables, tw32) + 8 * ed;
  G.mag = (G.band == 0 ? 0 : (G.band == 1 ? 64 : 128)) + G.g;
  return G;
}

// Round A of the transient FFT (performFFT, transient.js:17-35): real input, stages h = 1, 2, 4 on the points at
// bit-reversed positions 8g..8g+7.  Seven of the twelve butterflies have the twiddle (1, 0); when every sample is
// finite, not -0 and small enough not to overflow they are exact as Float32 adds (see r2_unit_ok), and the
// imaginary parts they touch are +0 throughout.
__device__ __forceinline__ void tfft_round_a(float2 (&x)[8], TablesPtr T) {
  const double2 w0 = make_double2(T->fft_tw[0][0], T->fft_tw[0][1]), w1 = make_double2(T->fft_tw[1][0], T->fft_tw[1][1]);
  const double2 w2 = make_double2(T->fft_tw[2][0], T->fft_tw[2][1]), w3 = make_double2(T->fft_tw[3][0], T->fft_tw[3][1]);
  const double2 w4 = make_double2(T->fft_tw[4][0], T->fft_tw[4][1]), w5 = make_double2(T->fft_tw[5][0], T->fft_tw[5][1]);
  const double2 w6 = make_double2(T->fft_tw[6][0], T->fft_tw[6][1]);
  uint32_t big = 0;
  bool neg_zero = false;
#pragma unroll
  for (int j = 0; j < 8; j++) {
    const uint32_t u = __float_as_uint(x[j].x);
    big = max(big, u & 0x7fffffffu);
    neg_zero |= (u == 0x80000000u);
  }
  const bool exact = big < 0x7b800000u && !neg_zero;      // |x| < 2^120 (also excludes inf and NaN)
  if (__all(exact)) {
    // stage 1: all unit; stage 2: (0,2) (4,6) unit; stage 3: (0,4) unit.  Real parts only where the imaginary is +0.
    float a0 = x[0].x + x[1].x, a1 = x[0].x - x[1].x, a2 = x[2].x + x[3].x, a3 = x[2].x - x[3].x;
    float a4 = x[4].x + x[5].x, a5 = x[4].x - x[5].x, a6 = x[6].x + x[7].x, a7 = x[6].x - x[7].x;
    x[0] = make_float2(a0 + a2, 0.0f); x[2] = make_float2(a0 - a2, 0.0f);
    x[4] = make_float2(a4 + a6, 0.0f); x[6] = make_float2(a4 - a6, 0.0f);
    x[1] = make_float2(a1, 0.0f); x[3] = make_float2(a3, 0.0f); x[5] = make_float2(a5, 0.0f); x[7] = make_float2(a7, 0.0f);
    r2_butterfly(x[1], x[3], w2); r2_butterfly(x[5], x[7], w2);
    const float b0 = x[0].x + x[4].x, b4 = x[0].x - x[4].x;
    x[0].x = b0; x[4].x = b4;
  } else {
    r2_butterfly(x[0], x[1], w0); r2_butterfly(x[2], x[3], w0); r2_butterfly(x[4], x[5], w0); r2_butterfly(x[6], x[7], w0);
    r2_butterfly(x[0], x[2], w1); r2_butterfly(x[1], x[3], w2); r2_butterfly(x[4], x[6], w1); r2_butterfly(x[5], x[7], w2);
    r2_butterfly(x[0], x[4], w3);
  }
  r2_butterfly(x[1], x[5], w4); r2_butterfly(x[2], x[6], w5); r2_butterfly(x[3], x[7], w6);
}
// e-output only of a butterfly: the last stage feeds the positive-frequency half (transient.js:29-32)
__device__ __forceinline__ float2 r2_butterfly_e(const float2 e, const float2 o, const double2 w) {
  const double er = e.x, ei = e.y, orr = o.x, oi = o.y;
  const double xr = orr * w.x - oi * w.y;
  const double xi = orr * w.y + oi * w.x;
  return make_float2(f32(er + xr), f32(ei + xi));
}

// performFFT (transient.js:17-35) of the three bands in `band`, exactly as the reference rounds it, in radix-8 rounds
// through `z`; mg = the Float32 magnitudes of the lane's four bins.  Ends with a fence: z may be reused.
__device__ __forceinline__ void tfft_exact(const float *band, float2 *z, const TGeom &G, TablesPtr T, TablesRsrc RT, float (&mg)[4]) {
  float2 x[8];
  {
    const float *src = band + G.src;
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const int jr = ((j & 1) << 2) | (j & 2) | (j >> 2);          // bitrev3
      x[j] = make_float2(src[jr * G.S], 0.0f);
    }
  }
  // twiddles of round B are requested before round A computes, those of round C before round B
  const double2 w8 = table_pair(RT, G.twb), w16a = table_pair(RT, G.twb + 128), w16b = table_pair(RT, G.twb + 256);
  const double2 w32a = table_pair(RT, G.twb + 384), w32b = table_pair(RT, G.twb + 512);
  const double2 w32c = table_pair(RT, G.twb + 640), w32d = table_pair(RT, G.twb + 768);
  __builtin_amdgcn_s_setprio(0);
  tfft_round_a(x, T);
  {
    float4 *dst = reinterpret_cast<float4 *>(z + G.za);
#pragma unroll
    for (int j = 0; j < 4; j++) dst[j] = make_float4(x[2 * j].x, x[2 * j].y, x[2 * j + 1].x, x[2 * j + 1].y);
  }
  wave_fence();
  {
    float2 *p = z + G.zb;                                    // stages 8, 16, 32 on the points p + 8j
#pragma unroll
    for (int j = 0; j < 8; j++) x[j] = p[9 * j];
    r2_butterfly(x[0], x[1], w8); r2_butterfly(x[2], x[3], w8); r2_butterfly(x[4], x[5], w8); r2_butterfly(x[6], x[7], w8);
    r2_butterfly(x[0], x[2], w16a); r2_butterfly(x[1], x[3], w16b); r2_butterfly(x[4], x[6], w16a); r2_butterfly(x[5], x[7], w16b);
    r2_butterfly(x[0], x[4], w32a); r2_butterfly(x[1], x[5], w32b); r2_butterfly(x[2], x[6], w32c); r2_butterfly(x[3], x[7], w32d);
#pragma unroll
    for (int j = 0; j < 8; j++) p[9 * j] = x[j];
  }
  const double2 wDa = table_pair(RT, G.twd), wDb = table_pair(RT, G.twd + 512);
  const double2 wC0 = table_pair(RT, G.twc), wC1 = table_pair(RT, G.twc + G.twc_stride);
  const double2 wC2 = table_pair(RT, G.twc + 2 * G.twc_stride), wC3 = table_pair(RT, G.twc + 3 * G.twc_stride);
  wave_fence();
  {
    // points g + S*t, t = 0..7.  Band 2 first runs stage 64 on them; then stage N/2 (64 for the 128-point
    // transforms, 128 for the 256-point one) pairs (t, t+4) and only its e-outputs, the bins g + S*t, are needed
    const float2 *p = z + G.zc;
#pragma unroll
    for (int t = 0; t < 8; t++) x[t] = p[t * G.zc_stride];
    if (G.band == 2) {
      r2_butterfly(x[0], x[2], wDa); r2_butterfly(x[1], x[3], wDb); r2_butterfly(x[4], x[6], wDa); r2_butterfly(x[5], x[7], wDb);
    }
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const float2 e = r2_butterfly_e(x[i], x[i + 4], i == 0 ? wC0 : (i == 1 ? wC1 : (i == 2 ? wC2 : wC3)));
      const double r = e.x, im = e.y;
      mg[i] = f32(sqrt(r * r + im * im));
    }
  }
  wave_fence();                                           // the per-bin terms reuse the memory of the points
}

// feature terms per bin, then the reference's 18 sequential sums (transient.js:92-189) -> feat[0..18), nv[3] as int32 behind
__device__ __forceinline__ void exact_sums(double (*term)[256], const TGeom &G, int lane, const float (&mg)[4], const float (&pmag)[4],
                                           double *feat) {
  bool valid[4];
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const int g = G.mag + i * G.S;
    const double cm = (double)mg[i], pm = (double)pmag[i];
    const double diff = cm - pm;
    valid[i] = cm > 1e-10;
    term[0][g] = diff > 0 ? diff : 0.0;            // spectral flux terms (transient.js:96-106)
    term[1][g] = cm * cm;                          // energy terms (exact product)
    term[2][g] = valid[i] ? js_log(cm) : 0.0;      // flatness terms (transient.js:126-133)
    term[3][g] = valid[i] ? cm : 0.0;
  }
  int nv_all = 0;
  {
    uint64_t m = 0;
    int n0 = 0, n1 = 0, n2 = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
      m = __ballot(valid[i]);
      n0 += __popc((uint32_t)m & 0xffffu); n1 += __popc((uint32_t)m >> 16); n2 += __popcll(m >> 32);
    }
    nv_all = lane == 0 ? n0 : (lane == 1 ? n1 : n2);
  }
  wave_fence();
  if (lane < 18) {
    // 18 lanes each own one running sum (3 bands x {flux, energy, log, linear, low, high}), index ascending
    const int b = lane / 6, kind = lane - 6 * b;
    const int n = b == 2 ? 128 : 64, g0 = b == 0 ? 0 : (b == 1 ? 64 : 128);
    const int which = kind == 0 ? 0 : (kind == 2 ? 2 : (kind == 3 ? 3 : 1));
    const int start = g0 + (kind == 5 ? n / 2 : 0);
    const int len = kind >= 4 ? n / 2 : n;
    const double2 *arr = reinterpret_cast<const double2 *>(term[which] + start);
    double acc = 0.0;
#pragma unroll
    for (int blk = 0; blk < 4; blk++) {
      if (32 * blk < len) {
#pragma unroll
        for (int i = 0; i < 16; i++) { const double2 v = arr[16 * blk + i]; acc += v.x; acc += v.y; }
      }
    }
    feat[lane] = acc;
  }
  if (lane < 3) reinterpret_cast<int *>(feat + 18)[lane] = nv_all;
}

// features of one band of one frame from its sums (transient.js:88-189); `flux` needs the previous magnitudes and
// is only meaningful for the current frame
struct BandFeatures { double flux, flat, hf, energy; };
__device__ __forceinline__ BandFeatures band_features(const double *s, int nv) {
  BandFeatures r;
  const double s_flux = s[0], s_e = s[1], s_log = s[2], s_lin = s[3], s_lo = s[4], s_hi = s[5];
  double norm = sqrt(s_e);
  if (!(norm != 0.0)) norm = 1e-6;                       // `Math.sqrt(e) || 1e-6`
  r.flux = s_flux / norm;
  r.flat = 0.0;                                          // calculateSpectralFlatness :120-141
  if (nv > 0) {
    const double gm = js_exp(s_log / (double)nv), am = s_lin / (double)nv;
    r.flat = am > 1e-10 ? gm / am : 0.0;
  }
  const double tot = s_lo + s_hi;                        // calculateHighFrequencyRatio :149-164
  r.hf = tot > 0 ? s_hi / tot : 0.0;
  r.energy = s_e;
  return r;
}

// block mode of band b of one sound unit from the feature sums of its frame (`cur`: 18 sums, nv[3] behind) and of the
// previous one (`prev`, or null for the zero state of a fresh BufferPool) (encoder.js:137-143).  JS_NAN: the energy terms
// clamp as Math.max / Math.min do (transient.js:181-188, :215), a NaN energy making the score NaN and the band long; the
// encoder's own detector (JS_NAN = false) takes 1e-10, 0 and 1 there instead, which it only meets on bands with non-finite
// magnitudes (PCM near the float32 maximum or not finite)
template <bool JS_NAN = false>
__device__ __forceinline__ int detect_band_mode(const double *cur, const double *prev, int b, double log1p10, double threshold,
                                                double *score_out) {
  const BandFeatures c = band_features(cur + 6 * b, reinterpret_cast<const int *>(cur + 18)[b]);
  double prev_flat = 0.0, prev_hf = 0.0, prev_e = 0.0;
  if (prev) {
    const BandFeatures p = band_features(prev + 6 * b, reinterpret_cast<const int *>(prev + 18)[b]);
    prev_flat = p.flat; prev_hf = p.hf; prev_e = p.energy;
  }
  const double ce = c.energy > 1e-10 ? c.energy : (JS_NAN && c.energy != c.energy ? c.energy : 1e-10);   // calculateEnergyChange :172-189
  const double pe = prev_e > 1e-10 ? prev_e : (JS_NAN && prev_e != prev_e ? prev_e : 1e-10);
  const double db = 10.0 * js_log10(ce / pe);
  const double e_change = db > 0 ? db : (JS_NAN && db != db ? db : 0.0);
  const double flat_c = sqrt(fabs(c.flat - prev_flat));       // calculateTransientScore :197-226
  const double hf_c = js_log1p(fabs(c.hf - prev_hf) * 10.0) / log1p10;
  const double e_c = e_change / 30.0 < 1.0 ? e_change / 30.0 : (JS_NAN && e_change != e_change ? e_change : 1.0);
  const double score = (c.flux + flat_c + hf_c + e_c) / 4.0;
  if (score_out) *score_out = score;
  return (score > threshold) ? (b + 1 > 2 ? b + 1 : 2) : 0;   // encoder.js:143
}

}  // namespace
