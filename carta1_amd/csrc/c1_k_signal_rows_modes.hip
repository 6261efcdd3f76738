// c1_k_signal_rows_modes.hip -- the rows of a measured mode search over n signals to their places:
// c1_k_signal_starts.hip's k_scatter_signal_rows for the outputs of c1_encode_signals_measured_modes*.  The start rows of the
// signals are encoded W at a time in the workspace and their unit and outputs land in row-major staging; this moves row r of
// every requested plane to unit dst_rows[r] of the call's arrays in one launch.
// No arithmetic: dwords and bytes pass through as bit patterns (the doubles as pairs of dwords), so nothing here has a number model.
#include "c1_device.h"

namespace {

// One wave per workspace row, a bounded grid striding over the rows.  A row is read whole before any of it is written.  Per row
// 53 dwords of the unit, one byte each of choice, modes_out and taken (a lane each), 13 dwords of shifts, 4 * n_cand dwords of
// distortion (2 * n_cand doubles: at most 32 dwords, a lane each) and 2 * n_cand of energy (at most 16)
__global__ __launch_bounds__(C1_WAVE) void k_scatter_signal_rows_modes(C1ScatterRowsModesLaunch L) {
  const int lane = threadIdx.x;
  const int n_cand = L.n_cand < 1 ? 1 : (L.n_cand > C1_MAX_MODE_CANDIDATES ? C1_MAX_MODE_CANDIDATES : L.n_cand);
  const int nd = 4 * n_cand, ne = 2 * n_cand;                  // dwords of a row's distortion / energy: <= 32 / <= 16
  for (int64_t r = blockIdx.x; r < L.n; r += gridDim.x) {
    const int64_t d = (int64_t)L.dst_rows[r];
    uint32_t unit = 0, sh = 0, di = 0, en = 0;
    uint8_t by = 0;
    // lanes 0, 1 and 2 carry the three bytes
    const uint8_t *bsrc = lane == 0 ? L.choice_src : (lane == 1 ? L.modes_src : L.taken_src);
    uint8_t *bdst = lane == 0 ? L.choice_dst : (lane == 1 ? L.modes_dst : L.taken_dst);
    const bool has_byte = lane < 3 && bdst != nullptr;
    if (L.units_dst && lane < 53) unit = L.units_src[r * 53 + lane];
    if (has_byte) by = bsrc[r];
    if (L.shifts_dst && lane < 13) sh = L.shifts_src[r * 13 + lane];
    if (L.distortion_dst && lane < nd) di = L.distortion_src[r * nd + lane];
    if (L.energy_dst && lane < ne) en = L.energy_src[r * ne + lane];
    if (L.units_dst && lane < 53) L.units_dst[d * 53 + lane] = unit;
    if (has_byte) bdst[d] = by;
    if (L.shifts_dst && lane < 13) L.shifts_dst[d * 13 + lane] = sh;
    if (L.distortion_dst && lane < nd) L.distortion_dst[d * nd + lane] = di;
    if (L.energy_dst && lane < ne) L.energy_dst[d * ne + lane] = en;
  }
}

// one wave per workgroup; a bounded grid strides over the rows (as c1_k_signal_starts.hip's launchers)
unsigned rows_grid(int64_t n) { return (unsigned)std::min<int64_t>(n, 256 * 12); }

}  // namespace

void c1k_launch_scatter_signal_rows_modes(const C1ScatterRowsModesLaunch &L, hipStream_t stream) {
  if (L.n <= 0) return;
  hipLaunchKernelGGL(k_scatter_signal_rows_modes, dim3(rows_grid(L.n)), dim3(C1_WAVE), 0, stream, L);
}
