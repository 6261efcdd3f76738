// c1_k_decode_fields.hip -- the decode() closure (decoder.js:408-411) from frame fields instead of sound units: one wave per
// run of frames of one channel, as k_decode<double> walks them.  Only the front end is new: each frame reads its fields in the
// layout c1_unpack_units writes and dequantizes them with the reference's general formula; the IMDCT, the overlap-add, the
// imdctOverlap tails and the QMF synthesis are k_decode<double>'s own device code (c1_decode_core.h).
// Number model: k_decode_fields<double> the reference's (binary64 operations, binary32 at every typed-array store);
// k_decode_fields<float> (C1_DECODE_BINARY32) k_decode<float>'s, operation for operation: the same LDS image (binary32 scale
// factors, RN(1 / range) and window), the step product SF * RN(1 / range) in place of the division, and the later stages in
// binary32.  Fields unpacked from sound units then decode to k_decode<float>'s bits.
#include "c1_decode_core.h"

namespace {

// One frame's fields, loaded one frame ahead: the lane's eight mantissas (slots 8 lane .. 8 lane + 7), the word-length and
// scale-factor index of BFU `lane` (lanes 0..51), and the wave-uniform nBfu and band modes.
struct FrameFields {
  int4 qa, qb;
  int wl, sfi;
  int n, m0, m1, m2;
};

__device__ __forceinline__ FrameFields load_fields(const C1FieldPtrs &P, int64_t u, int lane) {
  FrameFields F;
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

template <typename R>
__global__ __launch_bounds__(C1_WAVE, (std::is_same<R, float>::value ? 4 : 3)) void k_decode_fields(C1DecodeFieldsLaunch L) {
  constexpr bool F32 = std::is_same<R, float>::value;
  __shared__ DecodeLds<R> S;
  const int lane0 = threadIdx.x;
  const int ch = blockIdx.x % L.channels;
  const int64_t f0 = (int64_t)(blockIdx.x / L.channels) * L.run_frames;
  float *__restrict__ pcm = L.pcm[ch];

  for (int i = lane0; i < 46; i += 64) { S.d1[i] = 0; S.d2[i] = 0; }
  for (int i = lane0; i < 39; i += 64) S.dhi[i] = 0.0f;
  for (int i = lane0; i < 48; i += 64) S.tail[i] = 0.0f;
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

  const int64_t f_end = (f0 + L.run_frames < L.frames) ? f0 + L.run_frames : L.frames;
  int64_t f_first = f0 - 1;                                  // the frame before the run rebuilds the state
  if (f_first < -(int64_t)L.halo_frames) f_first = f0;
  // frame -1 is the halo (unit `ch` of L.prev); frame f >= 0 is unit f * channels + ch of L.cur
  auto fields_of = [&](int64_t fr) -> FrameFields {
    return fr < 0 ? load_fields(L.prev, ch, lane0) : load_fields(L.cur, fr * L.channels + ch, lane0);
  };
  FrameFields next = fields_of(f_first);
  for (int64_t f = f_first; f < f_end; ++f) {
    const bool emit = f >= f0;
    TablesPtr T = tables_for_this_frame(L.tables);
    const int lane = lane_for_this_frame(lane0);
    const FrameFields F = next;

    // ---------------- dequantizationStage (decoder.js:52-98) from the fields ----------------
    // Only BFUs below nBfu are read; indices are masked so that any int32 stays inside the tables (the host entries
    // reject them before they get here).  Per BFU: bits(5) | sfi(6) << 5, zero for a BFU the reference does not read.
    const int n = F.n < 0 ? 0 : (F.n > 52 ? 52 : F.n);
    if (lane < 52) S.desc[lane] = lane < n ? (uint32_t)wl_bits(F.wl & 15) | ((uint32_t)(F.sfi & 63) << 5) : 0u;
    wave_fence();
    next = fields_of(f + 1 < f_end ? f + 1 : f);
    {
      const int q[8] = {F.qa.x, F.qa.y, F.qa.z, F.qa.w, F.qb.x, F.qb.y, F.qb.z, F.qb.w};
#pragma unroll
      for (int m = 0; m < 8; m++) {
        const int slot = 8 * lane + m, b = bfu_of_slot(slot);
        const uint32_t d = S.desc[b];
        const int bits = (int)(d & 31u), sf = (int)(d >> 5);
        float v = 0.0f;
        if constexpr (F32) {
          // k_decode<float>: q * (SF * RN(1 / range)) with q = 0 where there are no bits; the product also for a silent BFU
          // (step 0: the zero takes q's sign)
          const R step = sf != 0 ? S.sf_tab[sf] * S.inv_tab[bits > 0 ? bits - 1 : 0] : (R)0;
          v = (float)((R)(bits != 0 ? q[m] : 0) * step);
        } else if (bits != 0 && sf != 0) {           // quantization.js:65-78: Float32((q * SF) / range), q any int32
          const int32_t range = (1 << (bits - 1)) - 1;
          v = f32(((double)q[m] * S.sf_tab[sf]) / (double)range);
        }
        // a band is long only when its mode is exactly 0 (decoder.js:82); a short band's BFUs interleave over its blocks
        const int mode = b >= 36 ? F.m2 : (b >= 20 ? F.m1 : F.m0);
        S.cb.coef[mode == 0 ? slot : slot - (int)kBfuFirst[b] + (int)kStartShort[b]] = v;
      }
    }
    wave_fence();

    // ---------------- imdctStage (decoder.js:116-330) ----------------
    const FrameModes M{F.m0, F.m1, F.m2};
    float *mid = S.u.m.zz.mid;
    const IMixGeometry IG = imix_geometry<R>(lane, M);
    imdct_r4<R>(S.cb.coef, S.u.m.zz.z, mid, IG, M.m0 == 0 || M.m1 == 0 || M.m2 == 0, M.m2 == 0, T, RT);
    wave_fence();
    overlap_add_mixed<R>(S, mid, lane, M);
    wave_fence();
    save_imdct_tails<R>(S, mid, lane);
    wave_fence();

    // ---------------- qmfSynthesisStage (decoder.js:349-389) ----------------
    R s0[4], s1[4];
    qmf_synthesis_frame<R>(S, lane, T, s0, s1);
    // the next frame's fields have arrived: nothing waits on a load behind the stores below (loads and stores share one
    // counter on this part, c1_k_decode.hip)
    asm volatile("" : "+v"(next.qa.x), "+v"(next.qb.x), "+v"(next.wl), "+v"(next.sfi));
    if (emit) {
      float4 *dst = reinterpret_cast<float4 *>(pcm + f * 512 + 8 * lane);
      dst[0] = make_float4((float)s1[0], (float)s0[0], (float)s1[1], (float)s0[1]);
      dst[1] = make_float4((float)s1[2], (float)s0[2], (float)s1[3], (float)s0[3]);
    }
    wave_fence();
  }
}

}  // namespace

void c1k_launch_decode_fields(const C1DecodeFieldsLaunch &L0, hipStream_t stream) {
  C1DecodeFieldsLaunch L = L0;
  L.run_frames = c1k_pick_run(L.frames, L.channels, 0);
  const int64_t runs = (L.frames + L.run_frames - 1) / L.run_frames;
  const dim3 grid((unsigned)(runs * L.channels)), block(C1_WAVE);
  if (L.binary32) hipLaunchKernelGGL((k_decode_fields<float>), grid, block, 0, stream, L);
  else hipLaunchKernelGGL((k_decode_fields<double>), grid, block, 0, stream, L);
}
