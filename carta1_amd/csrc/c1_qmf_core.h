// c1_qmf_core.h -- what the two band front ends of the encoder share besides the QMF frame body (c1_qmf_frame.inc):
// k_detect_features / k_detect_decide (c1_k_detect.hip, transient detection) and k_qmf_bands / k_modes_lists (c1_k_modes.hip,
// block modes given by the caller) both leave band rows, mode bytes and unit lists for k_mdct_bands.
#pragma once
#include "c1_device.h"

namespace {

// two work lists for the MDCT stage: all-long units and units with a short band (lists[0], lists[1] = counts, then
// `units` entries each), and behind them the units the speculative detector could not decide (lists[2]).  One atomic per
// 256-thread block and list: the three counters take about 5 ns per atomic whoever issues it, and one per wave (94 k
// for 2 M units) was 0.56 of the speculative decision kernel's 0.80 ms.
__device__ __forceinline__ void append_by_mode(bool live, int kind, int64_t unit, int64_t units, uint32_t *__restrict__ lists) {
  __shared__ uint32_t wave_count[3][4], wave_base[3][4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t below = (1ull << lane) - 1ull;
  uint64_t m[3];
#pragma unroll
  for (int k = 0; k < 3; k++) {
    m[k] = __ballot(live && kind == k);
    if (lane == 0) wave_count[k][wave] = (uint32_t)__popcll(m[k]);
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    const int k = threadIdx.x;
    const uint32_t c0 = wave_count[k][0], c1 = wave_count[k][1], c2 = wave_count[k][2], c3 = wave_count[k][3];
    const uint32_t total = c0 + c1 + c2 + c3;
    const uint32_t base = total ? atomicAdd(&lists[k], total) : 0u;
    wave_base[k][0] = base; wave_base[k][1] = base + c0; wave_base[k][2] = base + c0 + c1; wave_base[k][3] = base + c0 + c1 + c2;
  }
  __syncthreads();
  const uint64_t mine = kind == 0 ? m[0] : (kind == 1 ? m[1] : m[2]);
  if (live) lists[4 + (int64_t)kind * units + wave_base[kind][wave] + __popcll(mine & below)] = (uint32_t)unit;
}

}  // namespace
