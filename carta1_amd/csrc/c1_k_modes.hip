// c1_k_modes.hip -- the encoder's front end when the caller supplies the block modes (c1_encode_modes_device): band samples
// without the transient detector, and the MDCT work lists from the caller's mode bytes
#include "c1_device.h"
#include "c1_qmf_core.h"

namespace {

// =====================================================================================================
// blockSelectorStage with options.fixedBlockModes set before every frame (encoder.js:129-133)
// =====================================================================================================
//   k_qmf_bands     one wave per run of frames of one channel: qmfAnalysisStage as in k_detect_features, and nothing else --
//                   no transient FFT, no sums, no feature record.  Writes the band samples (2 KB) of every frame to the
//                   workspace in the layout k_mdct_bands reads (slot (frame + 1) * channels + channel; slot row 0 is frame
//                   -1 of the batch, whose tails are frame 0's overlap).
//   k_modes_lists   one lane per sound unit: the caller's mode byte, masked to the fields blockSelectorStage produces,
//                   and the unit appended to the all-long or the mixed list.
// k_mdct_bands (c1_k_detect.hip) transforms the two lists exactly as it does behind the detector.
struct alignas(16) QmfLds {
  double d1[46];
  double d2[46];
  alignas(16) float hbuf[296];
  alignas(16) float band[512];
  union alignas(16) {
    struct { alignas(16) double w1[698]; } q1;
    struct { alignas(16) double w2[454]; } q2;
  } u;
};
static_assert(sizeof(QmfLds) <= 10240, "band front end: 16 waves per CU");

__global__ __launch_bounds__(C1_WAVE, 4) void k_qmf_bands(C1EncodeLaunch L, float *bands_ws) {
  __shared__ QmfLds S;
  const int lane0 = threadIdx.x;
  int lane = lane0;
  const int ch = blockIdx.x % L.channels;
  const int64_t f0 = (int64_t)(blockIdx.x / L.channels) * L.run_frames;
  const float *__restrict__ pcm = L.pcm[ch];
  for (int i = lane; i < 46; i += 64) { S.d1[i] = 0.0; S.d2[i] = 0.0; }
  for (int i = lane; i < 296; i += 64) S.hbuf[i] = 0.0f;
  wave_fence();

  const int64_t f_end = (f0 + L.run_frames < L.frames) ? f0 + L.run_frames : L.frames;
  // What a frame leaves in the delay lines is a function of that frame alone (46 + 2 * 46 + 2 * 39 samples reach back less
  // than one frame), so one warm-up frame makes the run's first frame exact.  The first run also emits frame -1 (slot row 0)
  // and warms up on frame -2 for it, as far as the halo reaches; before the halo everything is the zero state.
  int64_t f_first = f0 == 0 ? -2 : f0 - 1;
  if (f_first < -(int64_t)L.halo_frames) f_first = -(int64_t)L.halo_frames;
  typedef float v4f __attribute__((ext_vector_type(4)));   // whole 16-byte register groups, as in k_detect_features
  v4f pre_a, pre_b;
  {
    const v4f *p4 = reinterpret_cast<const v4f *>(pcm + f_first * 512);
    pre_a = p4[lane0]; pre_b = p4[64 + lane0];
    // delivered before the loop: a load still pending at the loop's entry makes the compiler wait inside the loop, every frame
    asm volatile("" : "+v"(pre_a), "+v"(pre_b));
  }
  for (int64_t f = f_first; f < f_end; ++f) {
    const bool emit = (f >= f0) || (f0 == 0 && f == -1);
    TablesPtr T = tables_for_this_frame(L.tables);
    lane = lane_for_this_frame(lane0);

    // ---------------- qmfAnalysisStage (encoder.js:57-96) and the request for the next frame's PCM ----------------
#include "c1_qmf_frame.inc"
    // the next frame's PCM is taken delivery of before this frame's stores are issued (loads and stores share one in-order
    // counter, vmcnt: behind the stores the wait for it would be a wait for them)
    asm volatile("" : "+v"(pre_a), "+v"(pre_b));
    if (emit) {
      const int64_t slot = (f + 1) * L.channels + ch;
      float4 *dst = reinterpret_cast<float4 *>(bands_ws + (slot << 9));
      const float4 *src = reinterpret_cast<const float4 *>(S.band);
      dst[lane] = src[lane];
      dst[64 + lane] = src[64 + lane];
    }
    wave_fence();
  }
}

// the domain of a mode byte is what blockSelectorStage writes (encoder.js:143): 0 or 2 in the low and mid fields, 0 or 3 in
// the high one.  Any byte is brought into it before a kernel indexes with its fields (the device entry point does not check)
__global__ __launch_bounds__(256) void k_modes_lists(const uint8_t *__restrict__ given, int64_t units, uint8_t *__restrict__ modes,
                                                      uint32_t *__restrict__ lists) {
  const int64_t unit = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = unit < units;
  const int b = live ? given[unit] : 0;
  const int mode_byte = (b & 0x02) | (b & 0x08) | ((b & 0x30) == 0x30 ? 0x30 : 0);
  if (live) modes[unit] = (uint8_t)mode_byte;
  append_by_mode(live, mode_byte == 0 ? 0 : 1, unit, units, lists);
}

}  // namespace

void c1k_launch_modes_front(const C1EncodeLaunch &L0, const uint8_t *given_modes, float *bands_ws, uint8_t *modes_ws, uint32_t *lists_ws,
                            hipStream_t stream) {
  static const int slots = c1k_wave_slots(k_qmf_bands);
  C1EncodeLaunch L = L0;
  L.run_frames = c1k_pick_run(L.frames, L.channels, slots);
  const int64_t runs = (L.frames + L.run_frames - 1) / L.run_frames, units = L.frames * L.channels;
  (void)hipMemsetAsync(lists_ws, 0, 4 * sizeof(uint32_t), stream);
  hipLaunchKernelGGL(k_qmf_bands, dim3((unsigned)(runs * L.channels)), dim3(C1_WAVE), 0, stream, L, bands_ws);
  hipLaunchKernelGGL(k_modes_lists, dim3((unsigned)((units + 255) / 256)), dim3(256), 0, stream, given_modes, units, modes_ws, lists_ws);
}
