// c1_k_state.hip -- the encode() and decode() frame closures over EXPLICIT BufferPool state (encoder.js:438-450,
// decoder.js:408-411; the pool: codec/core/buffers.js:30-72): one wave per pool, n independent pools per launch.
// The frame-walking kernels (c1_k_analysis.hip, c1_k_detect.hip, c1_k_decode.hip) hold exactly this state in LDS between the
// frames of a run and reach it by warming up on a halo; these kernels LOAD it from a c1_enc_state / c1_dec_state, run one
// frame and write the state the pool holds afterwards.  State that no PCM or unit history could have produced is honoured
// bit for bit: every value enters the arithmetic as the reference reads it from its typed arrays.
// Number model: the reference's always (binary64 operations, binary32 at every typed-array store).  The QMF cores, the exact
// transient FFT, the feature sums and the decision, the mixed long/short MDCT core, the scale-factor scan, the IMDCT, the
// overlap-add and the synthesis are the device code of those kernels (c1_device.h, c1_detect_core.h, c1_decode_core.h).
// The encoder kernel ends where the analysis kernels end (coefficients + side record in the workspace); bit allocation and
// packing are the encoder's own kernels on that workspace (c1_api.hip).
// A pool's state is 483 / 179 floats: a multiple of 4 bytes, not of 16, so arrays of states are read and written with
// dword accesses (a lane's element each: consecutive lanes, consecutive dwords); PCM and coefficients move as 16 bytes.
#include "c1_detect_core.h"
#include "c1_decode_core.h"

namespace {

// float offsets of the fields of c1_enc_state / c1_dec_state (include/carta1_hip.h)
constexpr int kEsLow = 0, kEsMid = 46, kEsHigh = 92, kEsOverlap = 131, kEsMags = 227, kEsFloats = 483;
constexpr int kDsLow = 0, kDsMid = 46, kDsHigh = 92, kDsTail = 131, kDsFloats = 179;
static_assert(sizeof(c1_enc_state) == kEsFloats * sizeof(float) && offsetof(c1_enc_state, transient_mags) == kEsMags * sizeof(float), "c1_enc_state layout");
static_assert(sizeof(c1_dec_state) == kDsFloats * sizeof(float) && offsetof(c1_dec_state, imdct_tail) == kDsTail * sizeof(float), "c1_dec_state layout");

struct alignas(16) EncStateLds {
  alignas(16) float band[512];   // low128 | mid128 | high256 (behind its 39-sample delay), raw
  alignas(16) float ovl[96];     // mdctOverlap: the pool's on entry, the frame's once the staging has read it
  alignas(4) uint8_t sfi[64];
  float high[40];                // the new qmfDelays.highBand: the last 39 high-band samples of the frame
  int mode[4];
  alignas(16) double feat_c[kFeatureWsDoubles];
  alignas(16) double feat_p[kFeatureWsDoubles];
  // scratch with disjoint lifetimes inside the frame, as in DetectLds / MixedLds
  union alignas(16) {
    struct { alignas(16) double w1[698]; } q1;
    struct { alignas(16) double w2[454]; } q2;
    struct { alignas(16) float2 z[576]; } t;
    struct { alignas(16) double term[4][256]; } tt;
    struct {
      union alignas(16) {
        struct { alignas(16) float in[kStageFloats]; } g;
        struct { alignas(16) float coef[512]; } c;
      } a;
      union alignas(16) { float2 z[320]; } zz;
    } m;
  } u;
};
// no larger than the detector's image (d1, d2, hbuf, band and the same union: 12 160 bytes), whose kernels this one is modelled on
static_assert(sizeof(EncStateLds) <= 12160, "encode-from-state: LDS per wave no larger than k_detect_features'");

// mix_stage (c1_device.h) for block modes that are only known at run time (the detector's decision of this very frame): the
// same staging, with the choice between a long band's raw and windowed samples made value by value.  As a choice between the
// two 16-byte groups the compiler keeps both in private memory and loads the chosen one back: scratch traffic on the counter
// the frame's loads and stores share.
__device__ __forceinline__ void mix_stage_rt(const float *band_, const float *ovl_, float *stage, const FrameModes &M, int lane, TablesRsrc RT) {
  const int wofs = (int)offsetof(C1DevTables, window) + 8 * 4 * (lane & 7);
  const double2 wl01 = table_pair(RT, wofs), wl23 = table_pair(RT, wofs + 16);
  const int hofs = (int)offsetof(C1DevTables, window) + 8 * (28 - 4 * (lane & 7));
  const double2 wh32 = table_pair(RT, hofs), wh10 = table_pair(RT, hofs + 16);    // W[28-4m .. 31-4m]
  const float4 zero4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll
  for (int pass = 0; pass < 2; pass++) {
    const int b = pass == 0 ? (lane >> 5) : 2;
    const int s = pass == 0 ? 4 * (lane & 31) : 4 * lane;
    const int Sb = b == 2 ? 256 : 128, R = stage_region(b), ws = b == 2 ? 112 : 48;
    const bool lng = M.mode_of_band(b) == 0;
    const float4 v = *reinterpret_cast<const float4 *>(band_ + (b == 0 ? 0 : (b == 1 ? 128 : 256)) + s);
    float4 lo, hi;
    lo.x = f32(wl01.x * (double)v.x); lo.y = f32(wl01.y * (double)v.y); lo.z = f32(wl23.x * (double)v.z); lo.w = f32(wl23.y * (double)v.w);
    hi.x = f32((double)v.x * wh10.y); hi.y = f32((double)v.y * wh10.x); hi.z = f32((double)v.z * wh32.y); hi.w = f32((double)v.w * wh32.x);
    const bool tail = s >= Sb - 32;
    const float4 body = make_float4(tail ? hi.x : v.x, tail ? hi.y : v.y, tail ? hi.z : v.z, tail ? hi.w : v.w);
    if (lng) {
      *reinterpret_cast<float4 *>(stage + R + ws + 32 + s) = body;
    } else {
      *reinterpret_cast<float4 *>(stage + R + 32 + s) = lo;
      *reinterpret_cast<float4 *>(stage + R + 32 + Sb + s) = hi;
    }
    // overlap of the previous frame, and the zero regions of a long band
    const int l8 = pass == 0 ? (lane & 31) : lane;
    if (l8 < 8) *reinterpret_cast<float4 *>(stage + R + (lng ? ws : 0) + 4 * l8) = *reinterpret_cast<const float4 *>(ovl_ + 32 * b + 4 * l8);
    if (lng) {
      const int nz = ws / 4;                                 // float4 per zero region: [0, ws) and [ws + 32 + Sb, 2 ws + 32 + Sb)
      const int l = l8 - 8;
      if (l >= 0 && l < 2 * nz) *reinterpret_cast<float4 *>(stage + R + (l < nz ? 4 * l : ws + 32 + Sb + 4 * (l - nz))) = zero4;
    }
  }
}

// kRows: the row-indexed form (C1EncStateLaunch's index lists: the signals entry points).  The lists are wave-uniform: scalar
// loads, no vector register of the frame body is spent on them
template <bool kRows>
__global__ __launch_bounds__(C1_WAVE, 3) void k_encode_from_state(C1EncStateLaunch L) {
  __shared__ EncStateLds S;
  const int lane0 = threadIdx.x;
  const C1DevEncOpts *O = L.opts;
  const TablesRsrc RT = tables_rsrc(L.tables);
  // blockSelectorStage's branch (encoder.js:130-132): detection, or the fixed modes with transientDetection left alone
  const bool detect = L.detect < 0 ? O->modes[0] < 0 : L.detect != 0;
  for (int64_t pool = blockIdx.x; pool < L.n; pool += gridDim.x) {
    TablesPtr T = tables_for_this_frame(L.tables);
    const int lane = lane_for_this_frame(lane0);
    // `in` and `out` may be the same array: everything of the pool's state is read here, before anything is written
    int64_t in_row = pool, src_off = pool * L.pcm_stride, out_row = pool;
    if constexpr (kRows) {
      in_row = L.in_broadcast ? 0 : (L.in_rows ? (int64_t)L.in_rows[pool] : pool);
      src_off = (L.src_rows ? (int64_t)L.src_rows[pool] : pool) << 9;
      out_row = L.out_rows ? (int64_t)L.out_rows[pool] : pool;
    }
    const float *in = L.in + in_row * kEsFloats;
    typedef float v4f __attribute__((ext_vector_type(4)));
    const v4f *p4 = reinterpret_cast<const v4f *>(L.pcm + src_off);
    const v4f a = p4[lane], b = p4[64 + lane];
    const float s_low = in[kEsLow + (lane < 46 ? lane : 45)], s_mid = in[kEsMid + (lane < 46 ? lane : 45)];
    const float s_high = in[kEsHigh + (lane < 39 ? lane : 38)];
    const float s_ov0 = in[kEsOverlap + lane], s_ov1 = in[kEsOverlap + (lane < 32 ? 64 + lane : lane)];
    // the lane's four bins of the magnitude spectra (TGeom::mag, TGeom::S): the geometry itself is rebuilt where the
    // transient FFT runs, not carried through the QMF stages
    const int mag0 = lane < 16 ? lane : (lane < 32 ? 48 + lane : 96 + lane), magS = lane < 32 ? 16 : 32;
    float pmag[4];
#pragma unroll
    for (int k = 0; k < 4; k++) pmag[k] = in[kEsMags + mag0 + k * magS];

    // ---------------- qmfAnalysisStage (encoder.js:57-96) from the pool's delay lines ----------------
    double *w1 = S.u.q1.w1;
    if (lane < 46) w1[pidx<3>(lane)] = (double)s_low;
    {
      const int e0 = 46 + 4 * lane;
      *reinterpret_cast<double2 *>(&w1[pidx<3>(e0)]) = make_double2((double)a.x, (double)a.y);
      *reinterpret_cast<double2 *>(&w1[pidx<3>(e0 + 2)]) = make_double2((double)a.z, (double)a.w);
      *reinterpret_cast<double2 *>(&w1[pidx<3>(e0 + 256)]) = make_double2((double)b.x, (double)b.y);
      *reinterpret_cast<double2 *>(&w1[pidx<3>(e0 + 258)]) = make_double2((double)b.z, (double)b.w);
    }
    if (lane < 39) S.band[256 + lane] = s_high;              // the delayed high band starts with the pool's 39 samples (:84-90)
    S.ovl[lane] = s_ov0;
    if (lane < 32) S.ovl[64 + lane] = s_ov1;
    wave_fence();
    float nd1 = 0.0f, nd2 = 0.0f;                            // the new delay lines: the last 46 inputs of either stage
    {
      double ev[4], od[4];
      if (own_block()) qmf_analysis_core<4, 3>(w1, lane, T, ev, od); else { for (int d = 0; d < 4; d++) { ev[d] = w1[lane + d]; od[d] = 1.0; } }
      if (lane < 46) nd1 = (float)w1[pidx<3>(512 + lane)];
      wave_fence();                                          // w2 is the memory of w1
      double *w2 = S.u.q2.w2;
      if (lane < 46) w2[pidx<2>(lane)] = (double)s_mid;
      float lo[4];
#pragma unroll
      for (int d = 0; d < 4; d++) {
        lo[d] = f32(ev[d] + od[d]);                          // qmf.js:44-45
        const float hi = f32(ev[d] - od[d]);
        const int j = 39 + 4 * lane + d;                     // high band enters behind its 39-sample delay
        if (j < 256) S.band[256 + j] = hi; else S.high[j - 256] = hi;
      }
      *reinterpret_cast<double2 *>(&w2[pidx<2>(46 + 4 * lane)]) = make_double2((double)lo[0], (double)lo[1]);
      *reinterpret_cast<double2 *>(&w2[pidx<2>(48 + 4 * lane)]) = make_double2((double)lo[2], (double)lo[3]);
    }
    wave_fence();
    {
      double ev[2], od[2];
      double *w2 = S.u.q2.w2;
      if (own_block()) qmf_analysis_core<2, 2>(w2, lane, T, ev, od); else { for (int d = 0; d < 2; d++) { ev[d] = w2[lane + d]; od[d] = 1.0; } }
      *reinterpret_cast<float2 *>(&S.band[2 * lane]) = make_float2(f32(ev[0] + od[0]), f32(ev[1] + od[1]));
      *reinterpret_cast<float2 *>(&S.band[128 + 2 * lane]) = make_float2(f32(ev[0] - od[0]), f32(ev[1] - od[1]));
      if (lane < 46) nd2 = (float)w2[pidx<2>(256 + lane)];
    }
    wave_fence();

    // ---------------- blockSelectorStage (encoder.js:111-152) against the pool's transientDetection ----------------
    float mg[4] = {pmag[0], pmag[1], pmag[2], pmag[3]};      // fixed modes: the pool's magnitudes pass through (:130-132)
    int m0 = 0, m1 = 0, m2 = 0;
    if (detect) {
      const TGeom G = tfft_geometry(lane_for_this_frame(lane));
      tfft_exact(S.band, S.u.t.z, G, T, RT, mg);             // performFFT (transient.js:17-35): the frame's magnitudes (:142)
      if (!L.state_only) {
        const float zero[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        exact_sums(S.u.tt.term, G, lane, pmag, zero, S.feat_p);   // the pool's spectrum, whatever wrote it; its flux sum is not used
        wave_fence();
        exact_sums(S.u.tt.term, G, lane, mg, pmag, S.feat_c);
        wave_fence();
        if (lane < 3) S.mode[lane] = detect_band_mode<true>(S.feat_c, S.feat_p, lane, T->log1p10, O->threshold, nullptr);
        wave_fence();
        m0 = __builtin_amdgcn_readfirstlane(S.mode[0]);
        m1 = __builtin_amdgcn_readfirstlane(S.mode[1]);
        m2 = __builtin_amdgcn_readfirstlane(S.mode[2]);
      }
      __builtin_amdgcn_s_setprio(1);
    } else {
      m0 = O->modes[0]; m1 = O->modes[1]; m2 = O->modes[2];
    }

    // ---------------- mdctStage (encoder.js:170-349) with the pool's mdctOverlap ----------------
    const FrameModes M{m0, m1, m2};
    float *coef = S.u.m.a.c.coef;
    if (!L.state_only) {
      const MixGeometry GM = mix_geometry(lane, M);
      mix_stage_rt(S.band, S.ovl, S.u.m.a.g.in, M, lane, RT);
      wave_fence();
      mdct_mixed_r4(S.u.m.a.g.in, S.u.m.zz.z, coef, GM, M.m0 == 0 || M.m1 == 0 || M.m2 == 0, M.m2 == 0, T, RT);
    }
    // applyTailWindowing's overlap half (encoder.js:309-316): W[i] * last 32 raw samples of the band
    for (int i = lane; i < 96; i += 64) {
      const int bb = i >> 5, k = i & 31;
      const int Sb = bb == 2 ? 256 : 128, off = bb == 0 ? 0 : (bb == 1 ? 128 : 256);
      S.ovl[i] = f32(T->window[k] * (double)S.band[off + Sb - 32 + k]);
    }
    wave_fence();

    // ---------------- coefficients out + scale-factor indices (bitallocation.js:80-90) ----------------
    if (!L.state_only) {
      {
        float4 *dst = reinterpret_cast<float4 *>(L.coefs + (pool << 9));
        const float4 *src = reinterpret_cast<const float4 *>(coef);
        dst[lane] = src[lane];
        dst[64 + lane] = src[64 + lane];
      }
      const SfLong SFM = sf_geometry(lane, m0, m1, m2);
      sf_long(coef, S.sfi, SFM, T);
      if (lane >= 60 && lane < 63) reinterpret_cast<uint32_t *>(S.sfi)[13 + (lane - 60)] = lane == 60 ? (uint32_t)((M.m0 & 3) | ((M.m1 & 3) << 2) | ((M.m2 & 3) << 4)) : 0u;
      wave_fence();
      if (lane < 16) reinterpret_cast<uint32_t *>(L.side + pool * kSideBytes)[lane] = reinterpret_cast<const uint32_t *>(S.sfi)[lane];
    }

    // ---------------- the pool after the frame ----------------
    if (L.out) {
      float *out = L.out + out_row * kEsFloats;
      if (lane < 46) { out[kEsLow + lane] = nd1; out[kEsMid + lane] = nd2; }
      if (lane < 39) out[kEsHigh + lane] = S.high[lane];
      out[kEsOverlap + lane] = S.ovl[lane];
      if (lane < 32) out[kEsOverlap + 64 + lane] = S.ovl[64 + lane];
      if (!kRows || !L.keep_mags) {
#pragma unroll
        for (int k = 0; k < 4; k++) out[kEsMags + mag0 + k * magS] = mg[k];
      }
    }
    wave_fence();
  }
}

// performFFT's magnitudes (transient.js:17-35) of stored band rows into the transient_mags of a state array: what the pool's
// transientDetection holds when its last detected frame is kept as bands (a stream that went from detection to fixed modes)
struct alignas(16) StateMagsLds {
  alignas(16) float band[512];
  alignas(16) float2 z[576];
};
__global__ __launch_bounds__(C1_WAVE) void k_state_mags(const C1DevTables *tables, const float *__restrict__ bands, int64_t rows,
                                                       float *__restrict__ states) {
  __shared__ StateMagsLds S;
  const int lane = threadIdx.x;
  const int64_t r = blockIdx.x;
  if (r >= rows) return;
  const TGeom G = tfft_geometry(lane);
  const TablesRsrc RT = tables_rsrc(tables);
  TablesPtr T = C1_TABLES(tables);
  const float4 *src = reinterpret_cast<const float4 *>(bands + r * 512);
  reinterpret_cast<float4 *>(S.band)[lane] = src[lane];
  reinterpret_cast<float4 *>(S.band)[64 + lane] = src[64 + lane];
  wave_fence();
  float mg[4];
  tfft_exact(S.band, S.z, G, T, RT, mg);
#pragma unroll
  for (int i = 0; i < 4; i++) states[r * kEsFloats + kEsMags + G.mag + i * G.S] = mg[i];
}

// ---- decode ---------------------------------------------------------------------------------------------------------
// One frame's fields in the layout c1_unpack_units writes (as k_decode_fields loads them): the lane's eight mantissas, the
// word-length and scale-factor index of BFU `lane`, the wave-uniform nBfu and band modes.
struct PoolFields {
  int4 qa, qb;
  int wl, sfi;
  int n, m0, m1, m2;
};
__device__ __forceinline__ PoolFields load_pool_fields(const C1FieldPtrs &P, int64_t u, int lane) {
  PoolFields F;
  const int4 *q = reinterpret_cast<const int4 *>(P.q + u * 512 + 8 * lane);
  F.qa = q[0];
  F.qb = q[1];
  const int b = lane < 52 ? lane : 51;
  F.wl = P.wl[u * 52 + b];
  F.sfi = P.sfi[u * 52 + b];
  F.n = P.nbfu[u];
  F.m0 = P.modes[3 * u];
  F.m1 = P.modes[3 * u + 1];
  F.m2 = P.modes[3 * u + 2];
  return F;
}

// the LDS image is k_decode_fields' own (DecodeLds<R>): the same stages run on it.  R = float (C1_DECODE_BINARY32) is
// k_decode<float>'s arithmetic, operation for operation, as in k_decode_fields<float>; the state's floats enter and leave the
// binary32 delay lines as they are
template <typename R, bool kRows>
__global__ __launch_bounds__(C1_WAVE, (std::is_same<R, float>::value ? 4 : 3)) void k_decode_from_state(C1DecStateLaunch L) {
  constexpr bool F32 = std::is_same<R, float>::value;
  __shared__ DecodeLds<R> S;
  const int lane0 = threadIdx.x;
  if constexpr (F32) {
    S.sf_tab[lane0] = (R)C1_TABLES(L.tables)->scale_factors[lane0];
    if (lane0 < 16) S.inv_tab[lane0] = (R)C1_TABLES(L.tables)->inv_range[lane0];
    if (lane0 < 32) S.wtab[lane0] = (R)C1_TABLES(L.tables)->win32[lane0];
  } else {
    S.sf_tab[lane0] = C1_TABLES(L.tables)->scale_factors[lane0];
    if (lane0 < 32) S.wtab[lane0] = C1_TABLES(L.tables)->window[lane0];
  }
  const TablesRsrc RT = tables_rsrc(L.tables);
  wave_fence();
  for (int64_t pool = blockIdx.x; pool < L.n; pool += gridDim.x) {
    TablesPtr T = tables_for_this_frame(L.tables);
    const int lane = lane_for_this_frame(lane0);
    // `in` and `out` may be the same array: the pool's state is read here, before anything is written
    int64_t in_row = pool, dst_off = pool * L.pcm_stride, out_row = pool;
    if constexpr (kRows) {
      in_row = L.in_broadcast ? 0 : (L.in_rows ? (int64_t)L.in_rows[pool] : pool);
      dst_off = (L.dst_rows ? (int64_t)L.dst_rows[pool] : pool) << 9;
      out_row = L.out_rows ? (int64_t)L.out_rows[pool] : pool;
    }
    const float *in = L.in + in_row * kDsFloats;
    const PoolFields F = load_pool_fields(L.fields, pool, lane);
    const float s_low = in[kDsLow + (lane < 46 ? lane : 45)], s_mid = in[kDsMid + (lane < 46 ? lane : 45)];
    const float s_high = in[kDsHigh + (lane < 39 ? lane : 38)], s_tail = in[kDsTail + (lane < 48 ? lane : 47)];
    if (lane < 46) { S.d1[lane] = (R)s_low; S.d2[lane] = (R)s_mid; }
    if (lane < 39) S.dhi[lane] = s_high;
    if (lane < 48) S.tail[lane] = s_tail;

    // ---------------- dequantizationStage (decoder.js:52-98) from the fields, as k_decode_fields ----------------
    const int n = F.n < 0 ? 0 : (F.n > 52 ? 52 : F.n);
    if (lane < 52) S.desc[lane] = lane < n ? (uint32_t)wl_bits(F.wl & 15) | ((uint32_t)(F.sfi & 63) << 5) : 0u;
    wave_fence();
    {
      const int q[8] = {F.qa.x, F.qa.y, F.qa.z, F.qa.w, F.qb.x, F.qb.y, F.qb.z, F.qb.w};
#pragma unroll
      for (int m = 0; m < 8; m++) {
        const int slot = 8 * lane + m, b = bfu_of_slot(slot);
        const uint32_t d = S.desc[b];
        const int bits = (int)(d & 31u), sf = (int)(d >> 5);
        float v = 0.0f;
        if constexpr (F32) {                         // k_decode<float>'s step product, also for a silent BFU (k_decode_fields<float>)
          const R step = sf != 0 ? S.sf_tab[sf] * S.inv_tab[bits > 0 ? bits - 1 : 0] : (R)0;
          v = (float)((R)(bits != 0 ? q[m] : 0) * step);
        } else if (bits != 0 && sf != 0) {           // quantization.js:65-78: Float32((q * SF) / range), q any int32
          const int32_t range = (1 << (bits - 1)) - 1;
          v = f32(((double)q[m] * S.sf_tab[sf]) / (double)range);
        }
        const int mode = b >= 36 ? F.m2 : (b >= 20 ? F.m1 : F.m0);
        S.cb.coef[mode == 0 ? slot : slot - (int)kBfuFirst[b] + (int)kStartShort[b]] = v;
      }
    }
    wave_fence();

    // ---------------- imdctStage (decoder.js:116-330) with the pool's imdctOverlap tails ----------------
    const FrameModes M{F.m0, F.m1, F.m2};
    float *mid = S.u.m.zz.mid;
    const IMixGeometry IG = imix_geometry<R>(lane, M);
    imdct_r4<R>(S.cb.coef, S.u.m.zz.z, mid, IG, M.m0 == 0 || M.m1 == 0 || M.m2 == 0, M.m2 == 0, T, RT);
    wave_fence();
    overlap_add_mixed<R>(S, mid, lane, M);
    wave_fence();
    save_imdct_tails<R>(S, mid, lane);
    wave_fence();

    // ---------------- qmfSynthesisStage (decoder.js:349-389) with the pool's delay lines ----------------
    R s0[4], s1[4];
    qmf_synthesis_frame<R>(S, lane, T, s0, s1);
    wave_fence();
    if (L.pcm) {
      float4 *dst = reinterpret_cast<float4 *>(L.pcm + dst_off + 8 * lane);
      dst[0] = make_float4((float)s1[0], (float)s0[0], (float)s1[1], (float)s0[1]);
      dst[1] = make_float4((float)s1[2], (float)s0[2], (float)s1[3], (float)s0[3]);
    }
    if (L.out) {
      float *out = L.out + out_row * kDsFloats;
      if (lane < 46) { out[kDsLow + lane] = (float)S.d1[lane]; out[kDsMid + lane] = (float)S.d2[lane]; }
      if (lane < 39) out[kDsHigh + lane] = S.dhi[lane];
      if (lane < 48) out[kDsTail + lane] = S.tail[lane];
    }
    wave_fence();
  }
}

// dst[dst_rows[r]] = src[src_rows[r]], rows of `dwords` 32-bit words: a lane per dword, a wave per row and pass of the grid.
// Every row's source is read by the lanes that write it, within one pass: rows that are their own source (in place) are safe
__global__ __launch_bounds__(C1_WAVE) void k_copy_rows(uint32_t *__restrict__ dst, const uint32_t *__restrict__ dst_rows,
                                                      const uint32_t *__restrict__ src, const uint32_t *__restrict__ src_rows,
                                                      int src_broadcast, int64_t n, int dwords) {
  const int lane = threadIdx.x;
  for (int64_t r = blockIdx.x; r < n; r += gridDim.x) {
    const int64_t sr = src_broadcast ? 0 : (src_rows ? (int64_t)src_rows[r] : r), dr = dst_rows ? (int64_t)dst_rows[r] : r;
    const uint32_t *s = src + sr * dwords;
    uint32_t *d = dst + dr * dwords;
    for (int k = lane; k < dwords; k += C1_WAVE) d[k] = s[k];
  }
}

// one wave per workgroup; a bounded grid strides over the pools (k_analysis_fast's list mode does the same)
unsigned state_grid(int64_t n) { return (unsigned)std::min<int64_t>(n, 256 * 12); }

}  // namespace

void c1k_launch_encode_from_states(const C1EncStateLaunch &L, hipStream_t stream) {
  if (L.n <= 0) return;
  hipLaunchKernelGGL(k_encode_from_state<false>, dim3(state_grid(L.n)), dim3(C1_WAVE), 0, stream, L);
}
void c1k_launch_state_mags(const C1DevTables *tables, const float *bands, int64_t rows, float *states, hipStream_t stream) {
  if (rows <= 0) return;
  hipLaunchKernelGGL(k_state_mags, dim3((unsigned)rows), dim3(C1_WAVE), 0, stream, tables, bands, rows, states);
}
void c1k_launch_decode_from_states(const C1DecStateLaunch &L, hipStream_t stream) {
  if (L.n <= 0) return;
  if (L.binary32) hipLaunchKernelGGL((k_decode_from_state<float, false>), dim3(state_grid(L.n)), dim3(C1_WAVE), 0, stream, L);
  else hipLaunchKernelGGL((k_decode_from_state<double, false>), dim3(state_grid(L.n)), dim3(C1_WAVE), 0, stream, L);
}
void c1k_launch_encode_rows(const C1EncStateLaunch &L, hipStream_t stream) {
  if (L.n <= 0) return;
  hipLaunchKernelGGL(k_encode_from_state<true>, dim3(state_grid(L.n)), dim3(C1_WAVE), 0, stream, L);
}
void c1k_launch_decode_rows(const C1DecStateLaunch &L, hipStream_t stream) {
  if (L.n <= 0) return;
  if (L.binary32) hipLaunchKernelGGL((k_decode_from_state<float, true>), dim3(state_grid(L.n)), dim3(C1_WAVE), 0, stream, L);
  else hipLaunchKernelGGL((k_decode_from_state<double, true>), dim3(state_grid(L.n)), dim3(C1_WAVE), 0, stream, L);
}
void c1k_launch_copy_rows(uint32_t *dst, const uint32_t *dst_rows, const uint32_t *src, const uint32_t *src_rows, int src_broadcast,
                          int64_t n, int dwords, hipStream_t stream) {
  if (n <= 0 || dwords <= 0) return;
  hipLaunchKernelGGL(k_copy_rows, dim3(state_grid(n)), dim3(C1_WAVE), 0, stream, dst, dst_rows, src, src_rows, src_broadcast, n, dwords);
}
