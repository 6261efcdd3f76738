// c1_k_decode.hip -- deserializeFrame + the decode() closure (decoder.js:408-411): one wave per run of units
// k_decode<double>: the reference's arithmetic (binary64 operations, binary32 at every typed-array store): decoded PCM
//                   bit-identical to the reference.
// k_decode<float>:  the same computation in binary32 (opt-in, c1_ctx_set_decode_precision): no conversions, half the
//                   LDS for the synthesis windows; the PCM differs from the reference's by rounding noise: measured on an
//                   MI355X, 3.0 .. 3.2 u (u = 2^-24) of the stream's RMS on encoded pink noise from full scale to -80 dB, on
//                   random bytes and on overrunning units, and at most 11.1 u of the peak of any single coefficient's
//                   response under any block modes (tests/test_gpu_decode32_pinned.py bounds both); RMS
//                   5.8e-8 absolute on the benchmark's full-scale white noise.
#include "c1_decode_core.h"

namespace {
template <typename R>
__global__ __launch_bounds__(C1_WAVE, (std::is_same<R, float>::value ? 4 : 3)) void k_decode(C1DecodeLaunch L) {
  typedef R real;
  typedef typename Pair2<R>::type pair;
  constexpr bool F32 = std::is_same<R, float>::value;
  __shared__ DecodeLds<R> S;
  const int lane0 = threadIdx.x;
  int lane = lane0;
  const int ch = blockIdx.x % L.channels;
  const int64_t f0 = (int64_t)(blockIdx.x / L.channels) * L.run_frames;
  float *__restrict__ pcm = L.pcm[ch];

  for (int i = lane; i < 46; i += 64) { S.d1[i] = 0; S.d2[i] = 0; }
  for (int i = lane; i < 39; i += 64) S.dhi[i] = 0.0f;
  for (int i = lane; i < 48; i += 64) S.tail[i] = 0.0f;
  if (lane < 3) S.words[53 + lane] = 0u;
  S.sf_tab[lane] = (real)C1_TABLES(L.tables)->scale_factors[lane];
  if (lane < 16) S.inv_tab[lane] = (real)C1_TABLES(L.tables)->inv_range[lane];
  if (lane < 32) S.wtab[lane] = F32 ? (real)C1_TABLES(L.tables)->win32[lane] : (real)C1_TABLES(L.tables)->window[lane];
  // lane-only geometry, computed once per wave
  // A lane dequantizes the eight CONSECUTIVE slots 8 lane .. 8 lane + 7 (BFU-major order = bit-stream order = coefficient
  // order of a long band): one running bit cursor, one 64-bit window read per mantissa, two 16-byte stores.  They lie in at
  // most three BFUs b0, b0 + 1, b0 + 2: dq_geo = b0 | index of slot 8 lane inside b0 << 6 | mask of the slots past the first
  // boundary << 11 | mask of the slots past the second << 19 (| SPECS_PER_BFU[lane] << 27, for the bit offsets).
  uint32_t dq_geo;
  {
    const int s0 = 8 * lane0, b0 = bfu_of_slot(s0);
    uint32_t m1 = 0, m2 = 0;
#pragma unroll
    for (int m = 0; m < 8; m++) {
      const int k = bfu_of_slot(s0 + m) - b0;
      m1 |= (k >= 1 ? 1u : 0u) << m;
      m2 |= (k >= 2 ? 1u : 0u) << m;
    }
    dq_geo = (uint32_t)b0 | ((uint32_t)(s0 - kBfuFirst[b0]) << 6) | (m1 << 11) | (m2 << 19) | ((uint32_t)(lane0 < 52 ? kSpecs[lane0] : 0) << 27);
  }
  if (lane0 < 52) S.dshort[lane0] = (int16_t)((int)kStartShort[lane0] - (int)kBfuFirst[lane0]);
  IMixGeometry IGL = imix_geometry<R>(lane0, FrameModes{0, 0, 0});   // all-long frames
#pragma unroll
  for (int j = 0; j < 4; j++) {
    S.late[j][lane0] = (uint32_t)IGL.ox[j] | ((uint32_t)IGL.oy[j] << 16);
    S.late[4 + j][lane0] = (uint32_t)IGL.post_tab[j];
    IGL.ox[j] = IGL.oy[j] = IGL.post_tab[j] = 0;              // not carried through the loop
  }
  const TablesRsrc RT = tables_rsrc(L.tables);
  wave_fence();

  const int64_t f_end = (f0 + L.run_frames < L.frames) ? f0 + L.run_frames : L.frames;
  int64_t f_first = f0 - 1;                                  // the unit before the run rebuilds the state
  if (f_first < -(int64_t)L.halo_units) f_first = f0;
  // the unit's 53 dwords are requested one unit ahead (a lane's dword) and taken delivery of before the PCM stores of the
  // unit in between are issued: loads and stores share one counter on this part, so a wait for a load behind a store is
  // a wait for the store to reach memory (c1_k_spec.hip)
  auto unit_word = [&](int64_t fr) -> uint32_t {
    return reinterpret_cast<const uint32_t *>(L.units + (fr * L.channels + ch) * C1_UNIT_BYTES)[lane0 < 53 ? lane0 : 0];
  };
  uint32_t next_word = unit_word(f_first);
  for (int64_t f = f_first; f < f_end; ++f) {
    const bool emit = f >= f0;
    TablesPtr T = tables_for_this_frame(L.tables);
    lane = lane_for_this_frame(lane0);

    // ---------------- deserializeFrame (serialization.js:111-176) ----------------
    if (lane < 53) S.words[lane] = __builtin_bswap32(next_word);
    next_word = unit_word(f + 1 < f_end ? f + 1 : f);
    wave_fence();
    const uint32_t header = S.words[0] >> 16;
    const int m0 = 2 - (int)((header >> 14) & 3), m1 = 2 - (int)((header >> 12) & 3), m2 = 3 - (int)((header >> 10) & 3);
    const int n = bfu_amount((header >> 5) & 7);
    int wl = 0, sfi = 0;
    if (lane < n) {
      wl = (int)get_bits_be(S.words, 16 + 4 * lane, 4);
      sfi = (int)get_bits_be(S.words, 16 + 4 * n + 6 * lane, 6);
    }
    const int mybits = wl_bits(wl) * (int)(dq_geo >> 27);            // SPECS_PER_BFU[lane] rides in the geometry word
    const int scan = wave_inclusive_scan(mybits);
    if (lane < 52) {
      S.desc[lane] = (uint32_t)wl_bits(wl) | ((uint32_t)sfi << 5) | ((uint32_t)(16 + 10 * n + scan - mybits) << 11);
      // SF * RN(1 / range) (see dq_step); a BFU with scale factor 0 dequantizes to zeros (quantization.js:66-68)
      S.step[lane] = sfi != 0 ? S.sf_tab[sfi] * S.inv_tab[wl_bits(wl) > 0 ? wl_bits(wl) - 1 : 0] : (real)0;
    }
    wave_fence();
    // ---------------- dequantizationStage (decoder.js:52-98) ----------------
    const bool all_long = (m0 | m1 | m2) == 0;
    {
      const int b0 = (int)(dq_geo & 63u), b1 = b0 + 1 < 52 ? b0 + 1 : 51, b2 = b0 + 2 < 52 ? b0 + 2 : 51;
      const uint32_t in1 = (dq_geo >> 11) & 255u, in2 = (dq_geo >> 19) & 255u;
      const uint32_t d0 = S.desc[b0], d1 = S.desc[b1], d2 = S.desc[b2];
      const real st0 = S.step[b0], st1 = S.step[b1], st2 = S.step[b2];
      const int nb0 = (int)(d0 & 31u), nb1 = (int)(d1 & 31u), nb2 = (int)(d2 & 31u);
      // the slow formulations are only needed where the tables fail the host's check (binary64) or the unit's mantissas run
      // past its 212 bytes (bytes no encoder wrote: unpackBits then returns what is left, bitstream.js:49-70)
      const int last_bits = (int)(S.desc[51] >> 11) + (int)(S.desc[51] & 31u) * 20;
      const bool plain = last_bits <= C1_UNIT_BYTES * 8 && (F32 || T->dq_step != 0);
      int pos = (int)(d0 >> 11) + (int)((dq_geo >> 6) & 31u) * nb0;      // bit position of the lane's first mantissa
      float v[8];
#pragma unroll
      for (int m = 0; m < 8; m++) {
        const bool p1 = (in1 >> m) & 1u, p2 = (in2 >> m) & 1u;
        const int bits = p2 ? nb2 : (p1 ? nb1 : nb0);
        const real st = p2 ? st2 : (p1 ? st1 : st0);
        if (plain) {
          const int w = pos >> 5, o = pos & 31;
          const uint64_t two = ((uint64_t)S.words[w] << 32) | (uint64_t)S.words[w + 1];
          // the mantissa as a signed bit field: bits o .. o + bits of the 64-bit window (bitstream.js:78-82)
          const int64_t field = (int64_t)(two << o) >> ((64 - bits) & 63);
          const int32_t q = bits != 0 ? (int32_t)field : 0;
          v[m] = (float)((real)q * st);                           // == Float32((q * SF) / range) for every input (checked on the host)
        } else {
          const uint32_t dsc = p2 ? d2 : (p1 ? d1 : d0);
          const int sf = (int)((dsc >> 5) & 63u);
          float r = 0.0f;
          if (bits != 0) {
            const uint32_t raw = get_bits_be(S.words, pos, bits);
            const int32_t q = raw >= (1u << (bits - 1)) ? (int32_t)raw - (1 << bits) : (int32_t)raw;
            const int32_t range = (1 << (bits - 1)) - 1;
            if (sf != 0) {                                          // quantization.js:65-78
              if constexpr (F32) r = (float)q * (float)st;
              else {
                const double a = (double)q * S.sf_tab[sf];
                if (T->dq_step) r = f32((double)q * (double)st);
                else if (T->dq_fast) {
                  const double y = S.inv_tab[bits - 1], q0 = a * y;
                  r = f32(__builtin_fma(__builtin_fma(-q0, (double)range, a), y, q0));              // == a / range (checked on the host)
                } else r = f32(a / (double)range);
              }
            }
          }
          v[m] = r;
        }
        pos += bits;
      }
      if (all_long) {
        float4 *dst = reinterpret_cast<float4 *>(S.cb.coef + 8 * lane);
        dst[0] = make_float4(v[0], v[1], v[2], v[3]);
        dst[1] = make_float4(v[4], v[5], v[6], v[7]);
      } else {
        // a short band's BFUs are interleaved over its blocks (BFU_START_SHORT, constants.js:46-52)
        const int e0 = (b0 >= 36 ? m2 : (b0 >= 20 ? m1 : m0)) != 0 ? (int)S.dshort[b0] : 0;
        const int e1 = (b1 >= 36 ? m2 : (b1 >= 20 ? m1 : m0)) != 0 ? (int)S.dshort[b1] : 0;
        const int e2 = (b2 >= 36 ? m2 : (b2 >= 20 ? m1 : m0)) != 0 ? (int)S.dshort[b2] : 0;
#pragma unroll
        for (int m = 0; m < 8; m++) {
          const bool p1 = (in1 >> m) & 1u, p2 = (in2 >> m) & 1u;
          S.cb.coef[8 * lane + m + (p2 ? e2 : (p1 ? e1 : e0))] = v[m];
        }
      }
    }
    wave_fence();

    // ---------------- imdctStage (decoder.js:116-330) ----------------
    float *mid = S.u.m.zz.mid;
    if (all_long) {
      imdct_r4<R>(S.cb.coef, S.u.m.zz.z, mid, IGL, true, true, T, RT, &S.late[0][0] + lane);
      wave_fence();
      // overlap-add of the first 32 samples of every band (mdct.js:230-245 via decoder.js:203-232) ...
      if (lane < 32) {
        const bool lo = lane < 16;
        const int i = lo ? lane : 31 - lane;
        const real wa = S.wtab[i], wb = S.wtab[31 - i];   // w1 = W[i], w2 = W[31-i]
#pragma unroll
        for (int b = 0; b < 3; b++) {
          const int off = b == 0 ? 0 : (b == 1 ? 128 : 256);
          const real pv = S.tail[16 * b + i], cv = mid[off + 15 - i];
          S.cb.band[off + lane] = lo ? (float)(pv * wb - cv * wa) : (float)(pv * wa + cv * wb);
        }
      }
      // ... the rest of the band is invBuf[16 .. S-16) (decoder.js:215-221)
      if (lane < 48) {
        const int off = lane < 24 ? 0 : 128, q4 = lane < 24 ? lane : lane - 24;
        *reinterpret_cast<float4 *>(&S.cb.band[off + 32 + 4 * q4]) = *reinterpret_cast<const float4 *>(&mid[off + 16 + 4 * q4]);
      }
      if (lane < 56) *reinterpret_cast<float4 *>(&S.cb.band[256 + 32 + 4 * lane]) = *reinterpret_cast<const float4 *>(&mid[256 + 16 + 4 * lane]);
    } else {
    FrameModes M{m0, m1, m2};
    const IMixGeometry IG = imix_geometry<R>(lane, M);
    imdct_r4<R>(S.cb.coef, S.u.m.zz.z, mid, IG, m0 == 0 || m1 == 0 || m2 == 0, m2 == 0, T, RT);
    wave_fence();
    overlap_add_mixed<R>(S, mid, lane, M);
    }
    wave_fence();
    save_imdct_tails<R>(S, mid, lane);
    wave_fence();

    // ---------------- qmfSynthesisStage (decoder.js:349-389) ----------------
    real *w2 = S.u.q2.w2, *w1 = S.u.q1.w1;
    // high band delay compensation (:360-366): delayed high sample j = j < 39 ? previous tail : band2[j-39]
    float hi4[4];
#pragma unroll
    for (int t = 0; t < 4; t++) {
      const int j = 4 * lane + t;
      hi4[t] = j < 39 ? S.dhi[j] : S.cb.band[256 + j - 39];
    }
    {
      float keep = 0.0f;
      if (lane < 39) keep = S.cb.band[256 + 217 + lane];
      // stage 2: low + mid -> 256 samples (qmf.js:78-84 interleave)
      if (lane < 46) w2[pidx<2>(lane)] = S.d2[lane];
#pragma unroll
      for (int d = 0; d < 2; d++) {
        const int i = 2 * lane + d;
        const real l = S.cb.band[i], h = S.cb.band[128 + i];
        pair v2; v2.x = (real)(float)((real)0.5 * (l + h)); v2.y = (real)(float)((real)0.5 * (l - h));
        *reinterpret_cast<pair *>(&w2[pidx<2>(46 + 2 * i)]) = v2;
      }
      wave_fence();
      if (lane < 39) S.dhi[lane] = keep;
    }
    {
      real s0[2], s1[2];
      qmf_synth_r<R, 2, 2>(w2, lane, T, s0, s1);
      if (lane < 46) S.d2[lane] = w2[pidx<2>(256 + lane)];
      wave_fence();                                    // w1 reuses the memory of w2 from here on
      if (lane < 46) w1[pidx<3>(lane)] = S.d1[lane];
      // stage 1 input: (stage-2 output, delayed high); stage-2 output pair of i: out[2i] = s1, out[2i+1] = s0
#pragma unroll
      for (int d = 0; d < 2; d++) {
#pragma unroll
        for (int t = 0; t < 2; t++) {
          const int sidx = 4 * lane + 2 * d + t;          // sample index in the 256-sample low band
          const real l = (real)(float)(t == 0 ? s1[d] : s0[d]);
          const real h = hi4[2 * d + t];
          pair v2; v2.x = (real)(float)((real)0.5 * (l + h)); v2.y = (real)(float)((real)0.5 * (l - h));
          *reinterpret_cast<pair *>(&w1[pidx<3>(46 + 2 * sidx)]) = v2;
        }
      }
    }
    wave_fence();
    {
      real s0[4], s1[4];
      qmf_synth_r<R, 4, 3>(w1, lane, T, s0, s1);
      if (lane < 46) S.d1[lane] = w1[pidx<3>(512 + lane)];
      asm volatile("" : "+v"(next_word));                 // the next unit has arrived: nothing waits on a load behind the stores below
      if (emit) {
        float4 *dst = reinterpret_cast<float4 *>(pcm + f * 512 + 8 * lane);
        dst[0] = make_float4((float)s1[0], (float)s0[0], (float)s1[1], (float)s0[1]);
        dst[1] = make_float4((float)s1[2], (float)s0[2], (float)s1[3], (float)s0[3]);
      }
    }
    wave_fence();
  }
}

}  // namespace

void c1k_launch_decode(const C1DecodeLaunch &L0, bool binary32, hipStream_t stream) {
  static const int slots = c1k_wave_slots(k_decode<double>);
  C1DecodeLaunch L = L0;
  L.run_frames = c1k_pick_run(L.frames, L.channels, slots);
  const int64_t runs = (L.frames + L.run_frames - 1) / L.run_frames;
  const dim3 grid((unsigned)(runs * L.channels)), block(C1_WAVE);
  if (binary32) hipLaunchKernelGGL((k_decode<float>), grid, block, 0, stream, L);
  else hipLaunchKernelGGL((k_decode<double>), grid, block, 0, stream, L);
}
