// c1_k_palette.hip -- the allocation bias per sound unit, from a palette of biased scale-factor tables (c1_encode_biases_device):
// the units of a chunk sorted by palette entry into disjoint lists, and one allocation chain per entry over its list
#include "c1_device.h"

namespace {

// =====================================================================================================
// quantizationStage with options.allocationBias set before every frame (encoder.js:393)
// =====================================================================================================
// The allocation kernels read their C1DevEncOpts wave-uniformly (scalar loads) while a lane is a unit, so one launch has one
// table.  They have a list mode, though, and every per-unit slot they touch is keyed by the unit: the chunk's units are
// sorted by entry here, and the chain runs once per entry over that entry's list.
//   k_palette_lists   one lane per sound unit: the caller's index byte, brought into 0 .. n - 1 (anything else selects entry
//                     0), then per entry one ballot and one atomic per wave append the wave's units to lists + entry * stride.
//                     stride >= units, so no list can outgrow its array whatever the bytes are.  The order inside a list
//                     depends on the order of the atomics; no output byte depends on it (a unit's allocation reads and
//                     writes that unit's slots alone).
__global__ __launch_bounds__(256) void k_palette_lists(const uint8_t *__restrict__ index, int64_t units, int n, uint32_t *__restrict__ counts,
                                                        uint32_t *__restrict__ lists, int64_t stride) {
  const int64_t unit = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = unit < units;
  const int lane = threadIdx.x & (C1_WAVE - 1);
  const int b = live ? index[unit] : 0;
  const int entry = b < n ? b : 0;
  for (int k = 0; k < n; k++) {                                // n is wave-uniform (a kernel argument), at most C1_MAX_BIAS_PALETTE
    const uint64_t mask = __builtin_amdgcn_ballot_w64(live && entry == k);
    if (mask == 0) continue;
    uint32_t base = 0;
    if (lane == __builtin_ctzll(mask)) base = atomicAdd(counts + k, (uint32_t)__popcll(mask));
    base = (uint32_t)__builtin_amdgcn_readlane((int)base, __builtin_ctzll(mask));
    if (live && entry == k) lists[(int64_t)k * stride + base + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull))] = (uint32_t)unit;
  }
}

}  // namespace

void c1k_launch_allocate_palette(const C1EncodeLaunch &L, const C1DevEncOpts *palette, int n, const uint8_t *index, uint32_t *counts,
                                 uint32_t *lists, int64_t stride, hipStream_t stream) {
  const int64_t units = L.frames * L.channels;
  if (units <= 0 || n <= 0) return;
  (void)hipMemsetAsync(counts, 0, (size_t)n * sizeof(uint32_t), stream);
  hipLaunchKernelGGL(k_palette_lists, dim3((unsigned)((units + 255) / 256)), dim3(256), 0, stream, index, units, n, counts, lists, stride);
  for (int k = 0; k < n; k++) {
    C1EncodeLaunch A = L;
    A.opts = palette + k;
    A.unit_list = lists + (int64_t)k * stride;
    A.unit_count = counts + k;
    c1k_launch_allocate(A, stream);
  }
}
