// c1_k_signal_starts.hip -- the first two frames of many independent signals in ONE pass: the frame closure of
// c1_k_state.hip's k_encode_from_state, walked over one or two consecutive frames of a signal by one wave, with the pool between
// the two frames kept on the chip.  The row kernel there advances a pool by one frame per launch and hands it on through memory,
// so the first two frames of n signals cost two chains of latency-bound launches (rows, allocation, measured step, packing,
// copy); here they fill consecutive workspace rows of one chain.
// Number model: the reference's, as in c1_k_state.hip.  Every value the second frame takes over from the first is a binary32
// value at the point where the reference stores it to a typed array of its BufferPool (the two QMF delay lines and the four
// magnitude bins of a lane in registers; the high band's 39-sample delay and the MDCT overlap in LDS): the second frame sees bit
// for bit what it would read back from a c1_enc_state.
// The helpers of c1_k_state.hip (EncStateLds, mix_stage_rt) are repeated here so that its code stays as it is.
#include "c1_detect_core.h"

namespace {

// float offsets of the fields of c1_enc_state (include/carta1_hip.h)
constexpr int kEsLow = 0, kEsMid = 46, kEsHigh = 92, kEsOverlap = 131, kEsMags = 227, kEsFloats = 483;
static_assert(sizeof(c1_enc_state) == kEsFloats * sizeof(float) && offsetof(c1_enc_state, transient_mags) == kEsMags * sizeof(float), "c1_enc_state layout");

// the domain of a mode byte is what blockSelectorStage writes (encoder.js:143): 0 or 2 in the low and mid fields, 0 or 3 in
// the high one.  Every mode byte is brought into it before anything selects with its fields
__device__ __forceinline__ int mode_in_domain(int b) { return (b & 0x02) | (b & 0x08) | ((b & 0x30) == 0x30 ? 0x30 : 0); }

struct alignas(16) EncStateLds {
  alignas(16) float band[512];   // low128 | mid128 | high256 (behind its 39-sample delay), raw
  alignas(16) float ovl[96];     // mdctOverlap: the pool's on entry, the frame's once the staging has read it
  alignas(4) uint8_t sfi[64];
  float high[40];                // qmfDelays.highBand: the pool's on entry, the last 39 high-band samples of the frame after it
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
static_assert(sizeof(EncStateLds) <= 11184, "signal starts: LDS per wave no larger than k_encode_from_state's");

// mix_stage (c1_device.h) for block modes that are only known at run time, as in c1_k_state.hip
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

// One wave per signal.  The lists are wave-uniform: scalar loads, no vector register of the frame body is spent on them.  The
// frame body is k_encode_from_state's, as a loop body (it is one there too: the loop over the pools); what the frames of one
// signal hand each other is six values per lane (two delay-line samples, four magnitude bins) and the LDS arrays `high` and `ovl`
__global__ __launch_bounds__(C1_WAVE, 3) void k_encode_signal_starts(C1SignalStartsLaunch L) {
  __shared__ EncStateLds S;
  const int lane0 = threadIdx.x;
  const C1DevEncOpts *O = L.opts;
  const TablesRsrc RT = tables_rsrc(L.tables);
  // blockSelectorStage's branch (encoder.js:130-132): detection, or the fixed modes with transientDetection left alone; under
  // given mode bytes the detector does not run and the magnitudes pass through
  const bool detect = L.modes ? false : (L.detect < 0 ? O->modes[0] < 0 : L.detect != 0);
  for (int64_t sig = blockIdx.x; sig < L.n; sig += gridDim.x) {
    // `in` and `out` may be the same array: everything of the pool's state is read here, before anything is written
    const int64_t in_row = L.in_broadcast ? 0 : (L.in_rows ? (int64_t)L.in_rows[sig] : sig);
    const int64_t src0 = L.src_rows ? (int64_t)L.src_rows[sig] : sig;
    const int64_t out_row = L.out_rows ? (int64_t)L.out_rows[sig] : sig;
    const int count = L.counts ? (int)L.counts[sig] : L.count_all;
    const int64_t row0 = L.first_rows ? (int64_t)L.first_rows[sig] - L.row_base : 0;
    const float *in = L.in + in_row * kEsFloats;
    float s_low, s_mid;
    float pmag[4];
    const int mag0 = lane0 < 16 ? lane0 : (lane0 < 32 ? 48 + lane0 : 96 + lane0), magS = lane0 < 32 ? 16 : 32;
    {
      s_low = in[kEsLow + (lane0 < 46 ? lane0 : 45)];
      s_mid = in[kEsMid + (lane0 < 46 ? lane0 : 45)];
      const float s_high = in[kEsHigh + (lane0 < 39 ? lane0 : 38)];
      const float s_ov0 = in[kEsOverlap + lane0], s_ov1 = in[kEsOverlap + (lane0 < 32 ? 64 + lane0 : lane0)];
#pragma unroll
      for (int k = 0; k < 4; k++) pmag[k] = in[kEsMags + mag0 + k * magS];
      if (lane0 < 39) S.high[lane0] = s_high;
      S.ovl[lane0] = s_ov0;
      if (lane0 < 32) S.ovl[64 + lane0] = s_ov1;
    }
    wave_fence();

#pragma unroll 1
    for (int f = 0; f < count; f++) {
      TablesPtr T = tables_for_this_frame(L.tables);
      const int lane = lane_for_this_frame(lane0);
      typedef float v4f __attribute__((ext_vector_type(4)));
      const v4f *p4 = reinterpret_cast<const v4f *>(L.pcm + ((src0 + f) << 9));
      const v4f a = p4[lane], b = p4[64 + lane];
      // the state-only walk needs the magnitudes of its last frame alone
      const bool detect_f = detect && (!L.state_only || f == count - 1);

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
      if (lane < 39) S.band[256 + lane] = S.high[lane];        // the delayed high band starts with the pool's 39 samples (:84-90)
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
      float mg[4] = {pmag[0], pmag[1], pmag[2], pmag[3]};      // fixed or given modes: the pool's magnitudes pass through (:130-132)
      int m0 = 0, m1 = 0, m2 = 0;
      if (detect_f) {
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
      } else if (L.modes) {
        const int byte = mode_in_domain((int)L.modes[src0 + f]);
        m0 = byte & 3; m1 = (byte >> 2) & 3; m2 = (byte >> 4) & 3;
      } else if (!L.state_only) {
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
        const int64_t row = row0 + f;
        {
          float4 *dst = reinterpret_cast<float4 *>(L.coefs + (row << 9));
          const float4 *src = reinterpret_cast<const float4 *>(coef);
          dst[lane] = src[lane];
          dst[64 + lane] = src[64 + lane];
        }
        const SfLong SFM = sf_geometry(lane, m0, m1, m2);
        sf_long(coef, S.sfi, SFM, T);
        if (lane >= 60 && lane < 63) reinterpret_cast<uint32_t *>(S.sfi)[13 + (lane - 60)] = lane == 60 ? (uint32_t)((M.m0 & 3) | ((M.m1 & 3) << 2) | ((M.m2 & 3) << 4)) : 0u;
        wave_fence();
        if (lane < 16) reinterpret_cast<uint32_t *>(L.side + row * kSideBytes)[lane] = reinterpret_cast<const uint32_t *>(S.sfi)[lane];
      }

      // ---------------- the pool after the frame: what the next frame of this signal starts from ----------------
      s_low = nd1;
      s_mid = nd2;
#pragma unroll
      for (int k = 0; k < 4; k++) pmag[k] = mg[k];
      wave_fence();
    }

    // ---------------- the pool after the last frame ----------------
    if (L.out) {
      float *out = L.out + out_row * kEsFloats;
      if (lane0 < 46) { out[kEsLow + lane0] = s_low; out[kEsMid + lane0] = s_mid; }
      if (lane0 < 39) out[kEsHigh + lane0] = S.high[lane0];
      out[kEsOverlap + lane0] = S.ovl[lane0];
      if (lane0 < 32) out[kEsOverlap + 64 + lane0] = S.ovl[64 + lane0];
      if (!L.keep_mags) {
#pragma unroll
        for (int k = 0; k < 4; k++) out[kEsMags + mag0 + k * magS] = pmag[k];
      }
    }
    wave_fence();
  }
}

// One wave per workspace row: the unit of row r and each of its measured outputs that the call asked for, from the rows'
// staging (row-major, r the index) to unit dst_rows[r] of the call's arrays.  A row is read whole before any of it is written
__global__ __launch_bounds__(C1_WAVE) void k_scatter_signal_rows(C1ScatterRowsLaunch L) {
  const int lane = threadIdx.x;
  for (int64_t r = blockIdx.x; r < L.n; r += gridDim.x) {
    const int64_t d = (int64_t)L.dst_rows[r];
    uint32_t unit = 0, sh = 0, di = 0, en = 0, w0 = 0, w1 = 0;
    uint8_t tk = 0;
    if (L.units_dst && lane < 53) unit = L.units_src[r * 53 + lane];
    if (L.taken_dst && lane == 0) tk = L.taken_src[r];
    if (L.shifts_dst && lane < 13) sh = L.shifts_src[r * 13 + lane];
    if (L.distortion_dst && lane < 4) di = L.distortion_src[r * 4 + lane];
    if (L.energy_dst && lane < 2) en = L.energy_src[r * 2 + lane];
    if (L.weights_dst) { w0 = L.weights_src[r * 104 + lane]; if (lane < 40) w1 = L.weights_src[r * 104 + 64 + lane]; }
    if (L.units_dst && lane < 53) L.units_dst[d * 53 + lane] = unit;
    if (L.taken_dst && lane == 0) L.taken_dst[d] = tk;
    if (L.shifts_dst && lane < 13) L.shifts_dst[d * 13 + lane] = sh;
    if (L.distortion_dst && lane < 4) L.distortion_dst[d * 4 + lane] = di;
    if (L.energy_dst && lane < 2) L.energy_dst[d * 2 + lane] = en;
    if (L.weights_dst) { L.weights_dst[d * 104 + lane] = w0; if (lane < 40) L.weights_dst[d * 104 + 64 + lane] = w1; }
  }
}

// one wave per workgroup; a bounded grid strides over the rows (as c1_k_state.hip's launchers)
unsigned starts_grid(int64_t n) { return (unsigned)std::min<int64_t>(n, 256 * 12); }

}  // namespace

void c1k_launch_signal_starts(const C1SignalStartsLaunch &L, hipStream_t stream) {
  if (L.n <= 0) return;
  hipLaunchKernelGGL(k_encode_signal_starts, dim3(starts_grid(L.n)), dim3(C1_WAVE), 0, stream, L);
}
void c1k_launch_scatter_signal_rows(const C1ScatterRowsLaunch &L, hipStream_t stream) {
  if (L.n <= 0) return;
  hipLaunchKernelGGL(k_scatter_signal_rows, dim3(starts_grid(L.n)), dim3(C1_WAVE), 0, stream, L);
}
