// c1_k_decode_stages.hip -- the decoder's pipeline stages on their own (codec/pipeline/decoder.js exports them next to
// decode()): deserializeFrame (serialization.js:111-176), dequantizationStage (decoder.js:52-98), imdctStage (:116-330) and
// qmfSynthesisStage (:349-389), batched over consecutive frames of one channel, in the reference's number model (binary64
// operations, binary32 at every typed-array store).  The IMDCT, the overlap-add and the synthesis are k_decode<double>'s own
// device code (c1_decode_core.h).  The hot path never calls these kernels: c1_decode_* decodes in one k_decode launch.
#include "c1_decode_core.h"

namespace {

// deserializeFrame, one wave per unit.  Fields the reference leaves unset (BFUs at or above nBfu, mantissas of word
// length 0) are written as zeros.
__global__ __launch_bounds__(C1_WAVE) void k_unpack_units(const uint8_t *__restrict__ units, int64_t frames, int32_t *__restrict__ nbfu,
                                                          int32_t *__restrict__ modes, int32_t *__restrict__ sfi_out,
                                                          int32_t *__restrict__ wl_out, int32_t *__restrict__ q_out) {
  __shared__ uint32_t words[56];
  __shared__ uint32_t desc[52];           // per BFU: bits(5) | mantissa bit offset << 5
  const int lane = threadIdx.x;
  const int64_t f = blockIdx.x;
  if (f >= frames) return;
  const uint32_t *u = reinterpret_cast<const uint32_t *>(units + f * C1_UNIT_BYTES);
  if (lane < 53) words[lane] = __builtin_bswap32(u[lane]);
  else if (lane < 56) words[lane] = 0u;
  wave_fence();
  const uint32_t header = words[0] >> 16;
  const int n = bfu_amount((header >> 5) & 7);
  int wl = 0, sfi = 0;
  if (lane < n) {
    wl = (int)get_bits_be(words, 16 + 4 * lane, 4);
    sfi = (int)get_bits_be(words, 16 + 4 * n + 6 * lane, 6);
  }
  const int mybits = lane < 52 ? wl_bits(wl) * (int)kSpecs[lane] : 0;
  const int scan = wave_inclusive_scan(mybits);
  if (lane < 52) {
    desc[lane] = (uint32_t)wl_bits(wl) | ((uint32_t)(16 + 10 * n + scan - mybits) << 5);
    sfi_out[f * 52 + lane] = sfi;
    wl_out[f * 52 + lane] = wl;
  }
  if (lane == 0) {
    nbfu[f] = n;
    modes[3 * f] = 2 - (int)((header >> 14) & 3);
    modes[3 * f + 1] = 2 - (int)((header >> 12) & 3);
    modes[3 * f + 2] = 3 - (int)((header >> 10) & 3);
  }
  wave_fence();
#pragma unroll
  for (int m = 0; m < 8; m++) {
    const int slot = 8 * lane + m, b = bfu_of_slot(slot);
    const uint32_t d = desc[b];
    const int bits = (int)(d & 31u);
    int32_t q = 0;
    if (b < n && bits != 0) {            // unpackSignedBits (bitstream.js:78-82), past the unit's end as unpackBits reads it
      const uint32_t raw = get_bits_be(words, (int)(d >> 5) + (slot - (int)kBfuFirst[b]) * bits, bits);
      q = raw >= (1u << (bits - 1)) ? (int32_t)raw - (1 << bits) : (int32_t)raw;
    }
    q_out[f * 512 + slot] = q;
  }
}

// dequantizationStage, one wave per frame, eight consecutive slots per lane.  The mantissas may be any int32, so the
// dequantization is the reference's own formula Float32((q * SF) / range) (quantization.js:65-78), not k_decode's
// reciprocal shortcuts, which the host verifies only for mantissas inside their word length's range.
__global__ __launch_bounds__(C1_WAVE) void k_dequantize_frames(const C1DevTables *tables, const int32_t *__restrict__ nbfu,
                                                               const int32_t *__restrict__ modes, const int32_t *__restrict__ sfi,
                                                               const int32_t *__restrict__ wl, const int32_t *__restrict__ q,
                                                               int64_t frames, float *__restrict__ coefs) {
  const int lane = threadIdx.x;
  const int64_t f = blockIdx.x;
  if (f >= frames) return;
  const int n = nbfu[f];
#pragma unroll
  for (int m = 0; m < 8; m++) {
    const int slot = 8 * lane + m, b = bfu_of_slot(slot);
    const int bits = wl_bits(wl[f * 52 + b]), sf = sfi[f * 52 + b];
    float v = 0.0f;
    if (b < n && bits != 0 && sf != 0) {
      const int32_t range = (1 << (bits - 1)) - 1;
      v = f32(((double)q[f * 512 + slot] * tables->scale_factors[sf]) / (double)range);
    }
    // a band is long only when its mode is exactly 0 (decoder.js:82); a short band's BFUs interleave over its blocks
    const bool lng = modes[3 * f + band_of_bfu(b)] == 0;
    coefs[f * 512 + (lng ? slot : slot - (int)kBfuFirst[b] + (int)kStartShort[b])] = v;
  }
}

// imdctStage, one wave per run of frames as k_decode walks them: the frame before the run (the halo, or the batch's
// previous frame) rebuilds imdctOverlap, which after a frame is that frame's last 16 IMDCT samples per band and
// nothing else; without one the state is a fresh pool's zeros.  coefs / modes point at frame -halo.
__global__ __launch_bounds__(C1_WAVE, 3) void k_imdct_frames(const C1DevTables *tables, const float *__restrict__ coefs,
                                                             const int32_t *__restrict__ modes, int64_t frames, int halo,
                                                             int run_frames, float *__restrict__ bands) {
  __shared__ DecodeLds<double> S;
  const int lane0 = threadIdx.x;
  const int64_t f0 = (int64_t)blockIdx.x * run_frames;
  for (int i = lane0; i < 48; i += 64) S.tail[i] = 0.0f;
  if (lane0 < 32) S.wtab[lane0] = C1_TABLES(tables)->window[lane0];
  const TablesRsrc RT = tables_rsrc(tables);
  wave_fence();
  const int64_t f_end = (f0 + run_frames < frames) ? f0 + run_frames : frames;
  int64_t f_first = f0 - 1;
  if (f_first < -(int64_t)halo) f_first = f0;
  for (int64_t f = f_first; f < f_end; ++f) {
    TablesPtr T = tables_for_this_frame(tables);
    const int lane = lane_for_this_frame(lane0);
    const int64_t at = f + halo;
    const float4 *src = reinterpret_cast<const float4 *>(coefs + at * 512 + 8 * lane);
    float4 *dst = reinterpret_cast<float4 *>(S.cb.coef + 8 * lane);
    dst[0] = src[0];
    dst[1] = src[1];
    const FrameModes M{modes[3 * at], modes[3 * at + 1], modes[3 * at + 2]};
    wave_fence();
    float *mid = S.u.m.zz.mid;
    const IMixGeometry IG = imix_geometry<double>(lane, M);
    imdct_r4<double>(S.cb.coef, S.u.m.zz.z, mid, IG, M.m0 == 0 || M.m1 == 0 || M.m2 == 0, M.m2 == 0, T, RT);
    wave_fence();
    overlap_add_mixed<double>(S, mid, lane, M);
    wave_fence();
    if (f >= f0) {
      const float4 *b = reinterpret_cast<const float4 *>(S.cb.band + 8 * lane);
      float4 *o = reinterpret_cast<float4 *>(bands + f * 512 + 8 * lane);
      o[0] = b[0];
      o[1] = b[1];
    }
    save_imdct_tails<double>(S, mid, lane);
    wave_fence();
  }
}

// qmfSynthesisStage, one wave per run of frames.  qmfDelays after a frame are functions of that frame's bands alone (the
// last 39 high-band samples; the last 23 low/mid pairs; stage 1's last 23 inputs, which stage 2 computes from samples 93..127
// of the low and mid bands), so the frame before the run rebuilds them; without one they are a fresh pool's zeros.
// bands points at frame -halo.
__global__ __launch_bounds__(C1_WAVE, 3) void k_qmf_synthesis_frames(const C1DevTables *tables, const float *__restrict__ bands,
                                                                     int64_t frames, int halo, int run_frames, float *__restrict__ pcm) {
  __shared__ DecodeLds<double> S;
  const int lane0 = threadIdx.x;
  const int64_t f0 = (int64_t)blockIdx.x * run_frames;
  for (int i = lane0; i < 46; i += 64) { S.d1[i] = 0; S.d2[i] = 0; }
  for (int i = lane0; i < 39; i += 64) S.dhi[i] = 0.0f;
  wave_fence();
  const int64_t f_end = (f0 + run_frames < frames) ? f0 + run_frames : frames;
  int64_t f_first = f0 - 1;
  if (f_first < -(int64_t)halo) f_first = f0;
  for (int64_t f = f_first; f < f_end; ++f) {
    TablesPtr T = tables_for_this_frame(tables);
    const int lane = lane_for_this_frame(lane0);
    const float4 *src = reinterpret_cast<const float4 *>(bands + (f + halo) * 512 + 8 * lane);
    float4 *dst = reinterpret_cast<float4 *>(S.cb.band + 8 * lane);
    dst[0] = src[0];
    dst[1] = src[1];
    wave_fence();
    double s0[4], s1[4];
    qmf_synthesis_frame<double>(S, lane, T, s0, s1);
    if (f >= f0) {
      float4 *o = reinterpret_cast<float4 *>(pcm + f * 512 + 8 * lane);
      o[0] = make_float4((float)s1[0], (float)s0[0], (float)s1[1], (float)s0[1]);
      o[1] = make_float4((float)s1[2], (float)s0[2], (float)s1[3], (float)s0[3]);
    }
    wave_fence();
  }
}

}  // namespace

void c1k_launch_unpack_units(const uint8_t *units, int64_t frames, int32_t *nbfu, int32_t *modes, int32_t *sfi, int32_t *wl,
                             int32_t *q, hipStream_t stream) {
  hipLaunchKernelGGL(k_unpack_units, dim3((unsigned)frames), dim3(C1_WAVE), 0, stream, units, frames, nbfu, modes, sfi, wl, q);
}
void c1k_launch_dequantize_frames(const C1DevTables *tables, const int32_t *nbfu, const int32_t *modes, const int32_t *sfi,
                                  const int32_t *wl, const int32_t *q, int64_t frames, float *coefs, hipStream_t stream) {
  hipLaunchKernelGGL(k_dequantize_frames, dim3((unsigned)frames), dim3(C1_WAVE), 0, stream, tables, nbfu, modes, sfi, wl, q, frames, coefs);
}
void c1k_launch_imdct_frames(const C1DevTables *tables, const float *coefs, const int32_t *modes, int64_t frames, int halo,
                             float *bands, hipStream_t stream) {
  const int run = c1k_pick_run(frames, 1, 0);
  const int64_t runs = (frames + run - 1) / run;
  hipLaunchKernelGGL(k_imdct_frames, dim3((unsigned)runs), dim3(C1_WAVE), 0, stream, tables, coefs, modes, frames, halo, run, bands);
}
void c1k_launch_qmf_synthesis_frames(const C1DevTables *tables, const float *bands, int64_t frames, int halo, float *pcm,
                                     hipStream_t stream) {
  const int run = c1k_pick_run(frames, 1, 0);
  const int64_t runs = (frames + run - 1) / run;
  hipLaunchKernelGGL(k_qmf_synthesis_frames, dim3((unsigned)runs), dim3(C1_WAVE), 0, stream, tables, bands, frames, halo, run, pcm);
}
