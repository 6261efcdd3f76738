// c1_internal.h -- shared between the HIP kernels (c1_k_*.hip, c1_device.h) and the C-ABI host side
// (c1_api.hip).  Not part of the public boundary (that is include/carta1_hip.h).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "../../include/carta1_hip.h"

// ---- device-resident tables (one copy per context, in HBM; hot entries live in L1/K$) -------
struct C1DevTables {
  double tap_e[24];          // (double)QMF_EVEN[j]   constants.js:94-107
  double tap_o[24];          // (double)QMF_ODD[j]  == tap_e[23-j]
  double window[32];         // WINDOW_SHORT
  double mdct_fwd64[32];
  double mdct_fwd256[128];
  double mdct_fwd512[256];
  double mdct_inv64[32];
  double mdct_inv256[128];
  double mdct_inv512[256];
  double fft_tw[256][2];     // twiddle of butterfly k in a stage of half-stride h: [h-1+k]; fft.js:44-64
  double scale_factors[64];
  double norm[64 * 16];      // quantRange(wl)/SCALE_FACTORS[sfi]   quantization.js:42-44
  double log1p10;
  // findScaleFactor is ceil(3 (log2 m + 21)) (bitallocation.js:290-299): its boundaries are the powers 2^(i/3-21), not the
  // installed table.  sf_m1 / sf_m2 are the fraction bits (23) of floor_f32(2^(1/3)) and floor_f32(2^(2/3)) of those
  // boundaries (constants: the kernels always read the index off the bit pattern).  sf_fast = 1 when the installed
  // scale_factors share one such pattern in every octave, with exact powers of two at i % 3 == 0: a structural check the
  // speculative paths require (spec_ok), reported by c1_table_fast_paths
  uint32_t sf_m1, sf_m2;
  int32_t sf_fast;
  // dequantization (q * SF) / range as q0 = a*y, r = fma(-q0, range, a), fma(r, y, q0) with y = RN(1/range)
  // (Markstein): dq_fast = 1 when the host has checked it against the division for every (bits, sfi, q) of
  // the installed table (8.3 M cases), else the kernel divides
  int32_t dq_fast;
  // stronger: Float32((q * SF) / range) == Float32(q * RN(SF * y)) for every (bits, sfi, q) of the installed table (the
  // host checks all of them): one product per BFU, then a conversion, a multiply and a conversion per coefficient
  int32_t dq_step;
  double inv_range[16];      // RN(1 / (2^(wl) - 1)) by word-length index wl = 1..15
  // ---- binary32 tables of the speculative path (c1_k_spec.hip): roundings of the tables above ----
  float tap32[24];           // QMF_EVEN (binary32 in the reference already)
  float tap_pair[26][2];     // (E[23-j], E[j]) for j < 24: one packed FMA advances an (odd, even) chain pair; then (0, E[11]), (E[11], 0)
  float win32[32];           // fl32(WINDOW_SHORT)
  float pre32_64[16][2];     // fl32 of the MDCT (cos, sin) pairs
  float pre32_256[64][2];
  float pre32_512[128][2];
  float r4b[4][3][2];        // radix-4 round over stages 4, 8:  k -> wa = tw[3+k], wb = tw[7+k], fl32(wa*wb)
  float r4c[16][3][2];       // radix-4 round over stages 16, 32: k -> wa = tw[15+k], wb = tw[31+k], fl32(wa*wb)
  float r2d[64][2];          // stage 64: fl32(tw[63+k])
  float norm32[64 * 16];     // fl32(norm)
  float inv32_64[16][2], inv32_256[64][2], inv32_512[128][2];   // fl32 of the inverse MDCT tables (binary32 decode)
  float tw32[256][2];        // fl32(fft_tw)
  // error-bound coefficients per band (rounded up): eps_b = cz*Z_b + cw*W + cl*L + eabs
  float spec_cz[4], spec_cw[4], spec_cl[4];
  float spec_cz_short[4], spec_cw_short[4], spec_cl_short[4];   // the same for a band coded with short blocks (16-point transforms)
  float spec_eabs;
  // speculative transient detector (c1_detect_bound.h): Delta_b = det_ck[b] * ||band samples|| + det_eabs, rounded up
  float det_ck[4];
  float det_eabs;
  int32_t spec_ok;           // 0: the installed tables fail the structural checks the bound relies on -> exact path only
};

// ---- per-call encoder options in device form ---------------------------------------------------
struct C1DevEncOpts {
  double biased[64];         // pow(SCALE_FACTORS, bias) from the host
  double threshold;
  int32_t modes[3];          // fixed modes or -1
  int32_t pad_;
  uint16_t rank[64 * 16];    // rank (1..960) of the Float32 heap priority of (sfi, wl); 0 = unused
  // when the rank order is the order of an integer form A*sfi - B*wl (wl >= 1) / A*sfi + C (wl == 0),
  // as it is for the usual biases, the kernels compute it instead of reading the table
  int32_t rank_affine, rank_a, rank_b, rank_c, rank_off;
  // log2(biased[s]) ~ la_slope * s + la_off: only steers the multiplier search of the candidate bounds (k_alloc_bound);
  // the bounds themselves are formed from `biased`, so an inexact fit costs pruning power, never correctness
  float la_slope, la_off;
  int32_t alloc_no_tonal;     // experiments (C1_ALLOC_NO_TONAL=1): always run the 52-BFU candidate first
  // with rank_affine: what one successful heap step adds to the root's entry (word length + 1 and the rank of the next
  // priority), from word length 0 and from any other; checked on the host for every (sfi, wl), else rank_affine is 0
  uint32_t rank_step0, rank_step;
  // calculateTotalDistortion's terms per (BFU size, sfi), sizes in the order of kDistSizes: [..][0] = the zero-bit term
  // Float32(biased * 2 * size) as a double (0 for sfi 0), [..][1] = biased * size, whose exponent minus `bits` is the
  // coded term biased * 2^-bits * size.  dist_tables = 1 when the host found that identity to hold bit for bit for every
  // (size, sfi, word length) of this table; the kernels form the terms as the reference does otherwise.
  int32_t dist_tables;
  alignas(16) double dist[8][64][2];
};
constexpr int kDistSizes[8] = {4, 6, 7, 8, 9, 10, 12, 20};   // the BFU sizes there are (constants.js:29-36)

// ---- geometry ------------------------------------------------------------------------------------
constexpr int kRunFrames = 16;   // consecutive frames of one channel processed by one wave
constexpr int kRunFramesDecode = 64; // consecutive units of one channel decoded by one wave
constexpr int kRunFramesLong = 64;   // same, in the all-long-blocks fast path
constexpr int kSideBytes = 64;   // per unit: sfi[52], modes byte, pad
constexpr int kAllocBytes = 32;  // per unit: 52 wl nibbles, amount index, fallback flag
constexpr int kCandidateBytes = 8 * 8 + 8 * 32 + 8 * 8;  // per unit: 8 totals + 8 results + 8 lower bounds (bit allocation scratch)
constexpr int kCandLbOffset = 8 * 8 + 8 * 32;
constexpr int kEpsFloats = 4;    // per unit (speculative path): error bound of bands 0..2, flags
constexpr uint32_t kEpsFlagSfOpen = 1u;   // flag word: a scale-factor index is not certain within the bound
constexpr uint32_t kEpsFlagExact = 2u;    // flag word: the coefficients are the exact kernels' (bounds are zero)
constexpr int kSpecCheckFrames = 16;      // the speculative analysis re-assesses its material every so many frames of a run

struct C1EncodeLaunch {
  const float *pcm[C1_MAX_CHANNELS];
  int channels;
  int64_t frames;
  int halo_frames;
  const C1DevTables *tables;
  const C1DevEncOpts *opts;
  float *coefs;      // frames*channels*512   (workspace or caller tap)
  uint8_t *side;     // frames*channels*64
  uint8_t *alloc;    // frames*channels*32
  uint8_t *cand;     // frames*channels*kCandBytes: per-candidate totals and results
  uint32_t *work_list;   // frames*channels*7 entries (unit<<3 | candidate): first-round heaps at [0, units), second round behind them
  uint32_t *work_count;  // [0] first-round entries of work_list, [1] entries of sel_list, [2] second-round entries
  uint32_t *sel_list;    // units that kept more than the 52-BFU candidate alive: k_alloc_select picks among their results
  float *bands;      // optional tap (may be null)
  float *mags;       // optional tap of the transient detector's magnitude spectra, frames*channels*256 (64 | 64 | 128)
  float *mag_bounds; // optional tap (speculative detector only): frames*channels*3, Delta of the three bands
  uint8_t *units;    // frames*channels*212   (may be null for stage taps)
  // speculative binary32 path
  float *eps;            // frames*channels*kEpsFloats: per-band bound on |binary32 coefficient - reference coefficient|
  uint32_t *redo_list;   // units whose decisions are not certain within the bound (filled by the pack kernel)
  uint32_t *redo_count;
  uint32_t *realloc_list;   // the listed units whose scale-factor indices were not certain: their allocation is redone too
  uint32_t *realloc_count;
  uint32_t *reana_list;     // the listed units whose coefficients are binary32 ones: the exact analysis rebuilds them (units
  uint32_t *reana_count;    // of runs the exact kernels analysed in the first place are only packed again)
  // material-local speculation: the speculative analysis estimates, every kSpecCheckFrames frames of a
  // run, how many decisions of a unit the guards will leave open; past spec_defer it hands the rest of its run to the
  // exact kernels: defer_list[run * channels + channel] = first unit of the deferred part of that run, 0xffffffff = none
  uint32_t *defer_list;
  // per run and channel, bit k set when the scale-factor guard left frame k of the run open (open_masks[run * channels +
  // channel]; null: not collected).  Those units are re-analysed exactly BEFORE the allocation (c1_api.hip), so that the
  // allocation sees the reference's indices the first time and the redo pass has no allocation chain of its own.
  unsigned long long *open_masks;
  int list_zero_eps;        // list mode of the analysis kernels: also write bounds of zero (the unit's coefficients are exact now)
  float spec_defer;         // threshold on the predicted number of open decisions per unit; +inf: never defer
  // list mode: when unit_list is non-null the kernels process units unit_list[0 .. *unit_count) instead of all
  const uint32_t *unit_list;
  const uint32_t *unit_count;
  int list_runs;         // list mode of the analysis kernels: an entry is the first unit of a run that ends where the run of
                         // run_frames frames around it ends (the runs the speculative kernel handed over), not a single unit
  int run_frames;        // consecutive frames of one channel a wave walks (set by the launchers, c1k_pick_run)
  int spread_bits;       // speculative analysis: ceil(log2(workgroups)) for its block -> run permutation, 0 = stream order
};

struct C1DecodeLaunch {
  const uint8_t *units;
  int channels;
  int64_t frames;
  int halo_units;
  const C1DevTables *tables;
  float *pcm[C1_MAX_CHANNELS];
  int run_frames;        // consecutive units of one channel a wave decodes (set by the launcher)
};

// c1_measure_pcm_device: the decoder's inputs, the PCM the units were made from (halo_frames whole frames in front of the
// pointers) and the three outputs (each may be null)
struct C1MeasurePcmLaunch {
  const uint8_t *units;
  int channels;
  int64_t frames;
  int halo_units;
  int halo_frames;
  const C1DevTables *tables;
  const float *pcm[C1_MAX_CHANNELS];
  double *noise, *signal, *totals;   // frames*channels*16, frames*channels*16, frames*channels*2
  int run_frames;        // consecutive units of one channel a wave decodes (set by the launcher)
};

// frame fields in the layout c1_unpack_units writes: unit u at nbfu[u], modes[3u], sfi[52u], wl[52u], q[512u] (q 16-byte aligned)
struct C1FieldPtrs {
  const int32_t *nbfu, *modes, *sfi, *wl, *q;
};
struct C1DecodeFieldsLaunch {
  C1FieldPtrs cur;       // frame f >= 0 of channel c: unit f * channels + c
  C1FieldPtrs prev;      // halo_frames 1: the frame before frame 0, unit c (need not precede `cur` in memory)
  int channels;
  int64_t frames;
  int halo_frames;
  const C1DevTables *tables;
  float *pcm[C1_MAX_CHANNELS];
  int run_frames;        // consecutive frames of one channel a wave decodes (set by the launcher)
  int binary32;          // k_decode_fields<float>: k_decode<float>'s arithmetic (C1_DECODE_BINARY32); 0: the reference's
};

// The frame closures over explicit BufferPool state (c1_k_state.hip): pool i encodes the frame at pcm + i * pcm_stride from
// in[i] (c1_enc_state, 483 floats) and leaves its pool in out[i]; out may be in, or null.  Coefficients and side records go
// to coefs + i * 512 / side + i * kSideBytes, where the allocation and packing kernels take over (channels = 1, frames = n).
struct C1EncStateLaunch {
  const float *pcm;      // 16-byte aligned, as pcm_stride * 4 is
  int64_t pcm_stride;    // floats between the frames of consecutive pools
  const float *in;
  float *out;
  int64_t n;
  const C1DevTables *tables;
  const C1DevEncOpts *opts;
  float *coefs;
  uint8_t *side;
  int detect;            // -1: as opts say; 0: transient_mags pass through; 1: the frame's magnitudes are written
  int state_only;        // no coefficients, no side records, no block decision: only the state after the frame
  // row-indexed form (c1k_launch_encode_rows; the signals entry points): row r reads the PCM frame at pcm + src_rows[r] * 512
  // and the state in[in_rows[r]], and writes the state out[out_rows[r]]; coefficients and side records stay at row r.  A null
  // list is the identity; in_broadcast: every row reads in[0] (a fresh pool).  keep_mags: transient_mags of `out` is left as
  // it is (a state rebuilt from zeros under fixed block modes keeps what the pool held)
  const uint32_t *src_rows, *in_rows, *out_rows;
  int in_broadcast, keep_mags;
};
// decode twin: pool i decodes the frame fields of unit i (layout of c1_unpack_units) from in[i] (c1_dec_state, 179 floats)
// into pcm + i * pcm_stride (null: state only) and leaves its pool in out[i]; out may be in, or null
struct C1DecStateLaunch {
  C1FieldPtrs fields;
  const float *in;
  float *out;
  float *pcm;
  int64_t pcm_stride;
  int64_t n;
  const C1DevTables *tables;
  // row-indexed form (c1k_launch_decode_rows): row r decodes the fields of unit r from in[in_rows[r]] into the PCM frame at
  // pcm + dst_rows[r] * 512 and writes the state out[out_rows[r]]; null lists and in_broadcast as in C1EncStateLaunch
  const uint32_t *dst_rows, *in_rows, *out_rows;
  int in_broadcast;
  int binary32;          // k_decode_from_state<float, .>: k_decode<float>'s arithmetic (C1_DECODE_BINARY32); 0: the reference's
};

// The first frames of many signals in one pass (c1_k_signal_starts.hip): wave r walks counts[r] (1 or 2; null: count_all)
// consecutive PCM frames from pcm + src_rows[r] * 512 on, starting from the state in[in_rows[r]], and writes the coefficients
// and side record of frame f to workspace row first_rows[r] - row_base + f and the state after the last frame to
// out[out_rows[r]] (out null: no state).  Null lists, in_broadcast, detect, state_only and keep_mags as in C1EncStateLaunch;
// state_only reads no first_rows.  modes (one byte per frame of pcm, device memory, any value: brought into blockSelectorStage's
// domain): frame src_rows[r] + f takes its block modes from its byte, the detector does not run and transient_mags pass through
struct C1SignalStartsLaunch {
  const float *pcm;      // 16-byte aligned
  const float *in;
  float *out;
  int64_t n;
  const C1DevTables *tables;
  const C1DevEncOpts *opts;
  float *coefs;
  uint8_t *side;
  int detect, state_only;
  const uint32_t *src_rows, *in_rows, *out_rows, *counts, *first_rows;
  int64_t row_base;
  int in_broadcast, keep_mags, count_all;
  const uint8_t *modes;
};
// The rows of a signals call to their places (k_scatter_signal_rows): row r of every *_src plane (row-major staging; 53 dwords of a
// sound unit, one taken byte, 13 dwords of shifts, 4 of distortion, 2 of energy, 104 of weights) to unit dst_rows[r] of the plane
// *_dst.  A null *_dst plane is not moved; the dword planes are 4-byte aligned
struct C1ScatterRowsLaunch {
  const uint32_t *dst_rows;
  int64_t n;
  const uint32_t *units_src; uint32_t *units_dst;
  const uint8_t *taken_src; uint8_t *taken_dst;
  const uint32_t *shifts_src; uint32_t *shifts_dst;
  const uint32_t *distortion_src; uint32_t *distortion_dst;
  const uint32_t *energy_src; uint32_t *energy_dst;
  const uint32_t *weights_src; uint32_t *weights_dst;
};
// The same for the rows of a measured mode search (k_scatter_signal_rows_modes, c1_k_signal_rows_modes.hip): per row 53 dwords of
// a sound unit, one byte each of choice, modes_out and taken, 13 dwords of shifts, 4 * n_cand of distortion and 2 * n_cand of
// energy (n_cand 1 .. C1_MAX_MODE_CANDIDATES; the kernel clamps it)
struct C1ScatterRowsModesLaunch {
  const uint32_t *dst_rows;
  int64_t n;
  int n_cand;
  const uint32_t *units_src; uint32_t *units_dst;
  const uint8_t *choice_src; uint8_t *choice_dst;
  const uint8_t *modes_src; uint8_t *modes_dst;
  const uint8_t *taken_src; uint8_t *taken_dst;
  const uint32_t *shifts_src; uint32_t *shifts_dst;
  const uint32_t *distortion_src; uint32_t *distortion_dst;
  const uint32_t *energy_src; uint32_t *energy_dst;
};

// Run length of the frame-walking kernels: consecutive frames of one channel a wave walks, carrying the filter state
// (one extra warm-up frame per run).  Measured on MI355X (1 M stereo frames, A/B in one session): 64-frame runs beat
// runs sized to fill the wave slots exactly once (205 frames: every wave then finishes at the same moment, and the
// dispatcher has nothing left to balance) by 5 % (speculative analysis) to 8 % (decode); 32 and 128 are within noise
// of 64.  C1_RUN_FRAMES overrides it for experiments.
constexpr int kRunDefault = 64;
// Small batches (a streaming push, a frame closure) take shorter runs: 64 frames walked by one wave are 64 frames of
// latency (a 64-frame mono push: 0.41 ms, of which the walk is 0.3) while the rest of the machine idles; the batch is
// spread over up to 2 048 waves instead, and a run is never shorter than 4 frames (each pays one warm-up frame).
// A function of the batch alone: every kernel of a call, and the run lists they hand each other, use the same length.
// A forced run is clamped to at least 4 frames too: the speculative path's deferred-run slots and open-scale-factor
// masks share one allocation (c1_api.hip, ensure_workspace / bind_defer) sized for at most one slot per 4 units.
inline int c1k_pick_run(int64_t frames, int channels, int slots) {
  static const int forced = getenv("C1_RUN_FRAMES") ? atoi(getenv("C1_RUN_FRAMES")) : 0;
  (void)slots;
  if (forced > 0) return forced < 4 ? 4 : forced;
  const int64_t units = frames * channels;
  if (units >= (int64_t)kRunDefault * 2048) return kRunDefault;
  const int run = (int)((units + 2047) / 2048);
  return run < 4 ? 4 : run;
}
// wave slots of the current device for a 64-thread kernel (occupancy x compute units), cached by the caller
template <class Kernel>
inline int c1k_wave_slots(Kernel kernel) {
  int per_cu = 0, cus = 0, dev = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, 64, 0) != hipSuccess || per_cu <= 0) per_cu = 8;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
  return per_cu * cus;
}

// launchers (one per c1_k_*.hip file); all asynchronous on `stream`
void c1k_launch_analysis(const C1EncodeLaunch &L, bool detect, hipStream_t stream);
void c1k_launch_analysis_long(const C1EncodeLaunch &L, hipStream_t stream);   // fixed modes [0,0,0]
// binary32 + error bound: fixed modes [0,0,0] (all_short = false) or all three bands short (true)
void c1k_launch_analysis_spec(const C1EncodeLaunch &L, bool all_short, hipStream_t stream);
// transient detection: features (runs) -> decisions (per unit) -> MDCT from the stored bands (per unit).
// bands_ws: (units + channels) * 512 floats, feat_ws: (units + channels) * kFeatureWsDoubles doubles, modes_ws: units bytes
constexpr int kFeatureWsDoubles = 20;
// lists_ws: 4 + 3 * units uint32 (three counts, then the all-long list, the mixed list, and the units the speculative
// detector left to the exact recheck).  speculative: binary32 detector with a score interval.
// score_tap (tests): units * 3 * 2 doubles {lo, hi} (speculative) or {score, score}.  L.coefs null: decisions only.
void c1k_launch_detect(const C1EncodeLaunch &L, float *bands_ws, double *feat_ws, uint8_t *modes_ws, uint32_t *lists_ws,
                       bool speculative, double *score_tap, hipStream_t stream);
// block modes given by the caller (c1_k_modes.hip): QMF analysis alone into bands_ws (k_qmf_bands), then the caller's mode bytes
// (one per unit, device memory, any value: masked to blockSelectorStage's domain) into modes_ws and the all-long / mixed lists
// (k_modes_lists).  Workspaces as for c1k_launch_detect; c1k_launch_mdct_bands takes over from there
void c1k_launch_modes_front(const C1EncodeLaunch &L, const uint8_t *given_modes, float *bands_ws, uint8_t *modes_ws, uint32_t *lists_ws,
                            hipStream_t stream);
// mdctStage + scale factors from stored band samples (k_mdct_bands): bands_ws (units + channels) * 512 floats with slot row 0 =
// frame -1, modes_ws one byte per unit, lists_ws = {count all-long, count mixed, -, -} then the two unit lists, `units` entries apart
void c1k_launch_mdct_bands(const C1EncodeLaunch &L, const float *bands_ws, const uint8_t *modes_ws, const uint32_t *lists_ws, hipStream_t stream);
// the decoder's pipeline stages on their own (c1_k_decode_stages.hip), one channel; device pointers; coefs / modes / bands in
// point at frame -halo
void c1k_launch_unpack_units(const uint8_t *units, int64_t frames, int32_t *nbfu, int32_t *modes, int32_t *sfi, int32_t *wl,
                             int32_t *q, hipStream_t stream);
void c1k_launch_dequantize_frames(const C1DevTables *tables, const int32_t *nbfu, const int32_t *modes, const int32_t *sfi,
                                  const int32_t *wl, const int32_t *q, int64_t frames, float *coefs, hipStream_t stream);
void c1k_launch_imdct_frames(const C1DevTables *tables, const float *coefs, const int32_t *modes, int64_t frames, int halo,
                             float *bands, hipStream_t stream);
void c1k_launch_qmf_synthesis_frames(const C1DevTables *tables, const float *bands, int64_t frames, int halo, float *pcm,
                                     hipStream_t stream);
// the encoder's block selection and quantization stages on their own (c1_k_encode_stages.hip), one channel; device pointers.
// bands point at frame -halo; mags: (halo + frames) * 256 floats of scratch; modes: frames * 3 int32
void c1k_launch_block_modes_from_bands(const C1DevTables *tables, const float *bands, int64_t frames, int halo, double threshold,
                                       float *mags, int32_t *modes, hipStream_t stream);
// block modes (frames * 3 int32) -> k_mdct_bands' mode bytes (frames) and frame lists (4 + 2 * frames uint32); for a few frames
void c1k_launch_stage_mode_lists(const int32_t *modes, int64_t frames, uint8_t *mode_bytes, uint32_t *lists, hipStream_t stream);
// findScaleFactor per BFU -> side records (kSideBytes per frame) for c1k_launch_allocate
void c1k_launch_stage_scale_factors(const C1DevTables *tables, const float *coefs, const int32_t *modes, int64_t frames, uint8_t *side,
                                    hipStream_t stream);
// allocation + side records -> frame fields (nbfu[frames], sfi / wl [frames * 52], q [frames * 512])
void c1k_launch_stage_fields(const C1DevTables *tables, const float *coefs, const int32_t *modes, const uint8_t *side,
                             const uint8_t *alloc, int64_t frames, int32_t *nbfu, int32_t *sfi, int32_t *wl, int32_t *q,
                             hipStream_t stream);
// frame fields (as above) -> units = frames * 212 bytes, serializeFrame (serialization.js:41-98); nbfu must be 0..52
void c1k_launch_pack_units(const int32_t *nbfu, const int32_t *modes, const int32_t *sfi, const int32_t *wl, const int32_t *q,
                           int64_t frames, uint8_t *units, hipStream_t stream);
// the single-stage functions the reference exports next to encode()/decode() (c1_k_stages.hip); device pointers
void c1k_launch_quantize_one(const C1DevTables *tables, const float *x, int n, int sfi, int bits, int32_t *out, hipStream_t stream);
void c1k_launch_dequantize_one(const C1DevTables *tables, const int32_t *q, int n, int sfi, int bits, float *out, hipStream_t stream);
void c1k_launch_fft_reference(float *real, float *imag, int n, const double *w, double *twiddle_scratch /* n doubles */, hipStream_t stream);
void c1k_launch_window_bands(const float *bands, const uint8_t *modes, int64_t units, const C1DevTables *tables, float *out, hipStream_t stream);
// the decision functions of analysis/transient.js and coding/bitallocation.js over batches of independent problems
// (c1_k_decision.hip); device pointers.  Offsets index `values`; every range has been checked by the caller
void c1k_launch_js_log2(const double *in, double *out, int64_t n, hipStream_t stream);
void c1k_launch_find_scale_factors(const double *values, const int64_t *offsets, const int64_t *counts, int64_t problems, int32_t *out,
                                   hipStream_t stream);
// offsets[problems + 1]; w = log2(n) host twiddle pairs; tw 2n doubles, re / im problems * n floats, mag problems * n / 2; n >= 2
void c1k_launch_perform_fft(const double *samples, const int64_t *offsets, int64_t problems, int n, const double *w, double *tw,
                            float *re, float *im, float *mag, hipStream_t stream);
void c1k_launch_detect_transients(const double *cur, const int64_t *cur_off, const double *prev, const int64_t *prev_off,
                                  const uint8_t *has_prev, const double *thresholds, int64_t problems, const C1DevTables *tables,
                                  uint8_t *transient, double *scores, hipStream_t stream);
// max_bfus 0..52; bfu_off / bfu_len / bfu_sizes / wl / sfi: problems * 52; bsf = 64 biased scale factors
void c1k_launch_allocate_bits(const double *data, const int64_t *bfu_off, const int32_t *bfu_len, const int32_t *bfu_sizes,
                              const int32_t *max_bfus, int64_t problems, const double *bsf, int32_t *count, int32_t *wl, int32_t *sfi,
                              uint8_t *fallback, hipStream_t stream);
void c1k_launch_detect_spec_tap(const C1EncodeLaunch &L, float *bands_ws, double *feat_ws, hipStream_t stream);   // L.mags, L.mag_bounds
void c1k_launch_libm(int fn, const double *in, double *out, int64_t n, hipStream_t stream);
void c1k_launch_log2f_error(uint32_t first, uint64_t count, unsigned long long *out, hipStream_t stream);   // out: 2 x u64 on the device
void c1k_launch_allocate(const C1EncodeLaunch &L, hipStream_t stream);
void c1k_launch_alloc_tap(const C1EncodeLaunch &L, double *out, hipStream_t stream);   // test tap: totals and lower bounds of all candidates
// the allocation bias per unit (c1_k_palette.hip): index = one byte per unit of L (device memory, any value: a byte >= n selects
// entry 0), palette = n C1DevEncOpts on the device.  The units are sorted by entry into lists + k * stride (stride >= units,
// counts[k] entries), then c1k_launch_allocate runs once per entry over its list, one chain after the other on `stream`
void c1k_launch_allocate_palette(const C1EncodeLaunch &L, const C1DevEncOpts *palette, int n, const uint8_t *index, uint32_t *counts,
                                 uint32_t *lists, int64_t stride, hipStream_t stream);
// the allocation bias chosen per unit by least coding error (c1_k_choose.hip): trial = n_palette allocation records per unit of L,
// entry k's at trial + k * trial_stride + unit * kAllocBytes (trial_stride >= units * kAllocBytes), as c1k_launch_allocate left
// them with L.alloc pointed there.  Per unit: D(u, k) = sum (c - dequantize(quantize(c)))^2 and E(u) = sum c^2 in binary64 over
// the 512 coefficients, choice = the smallest k of least D (a NaN never wins; all NaN: 0), and that entry's record copied to
// L.alloc, where the packing kernels read it.  choice (units), distortion (units * n_palette, unit-major) and energy (units)
// may each be null.  all_long: every unit has modes [0,0,0] (the side records' mode byte is not read)
void c1k_launch_choose_bias(const C1EncodeLaunch &L, const uint8_t *trial, int64_t trial_stride, int n_palette, bool all_long,
                            uint8_t *choice, double *distortion, double *energy, hipStream_t stream);
// the block modes chosen per unit by least coding error (c1_k_choose_modes.hip).  Every unit under one mode byte: the byte into
// modes_ws and the unit into k_mdct_bands' all-long (byte 0) or mixed list, as k_modes_lists would leave them
void c1k_launch_const_mode_lists(int byte, int64_t units, uint8_t *modes_ws, uint32_t *lists_ws, hipStream_t stream);
// out = per unit the side record of mode byte `byte`: the scale-factor indices of a band from side_short where the byte codes it
// short, else from side_long (the records of the all-short and the all-long analysis), and the byte itself
void c1k_launch_compose_side(const uint8_t *side_long, const uint8_t *side_short, int64_t units, int byte, uint8_t *out, hipStream_t stream);
// L.coefs / L.side: the all-long analysis, coefs_short / side_short: the all-short one (a plane no candidate needs is not read);
// trial as for c1k_launch_choose_bias, entry k allocated from candidate k's composed side record; cand: n_cand (1 ..
// C1_MAX_MODE_CANDIDATES) HOST bytes of the domain.  Per unit D(u, k) and E(u, k) (weighted, include/carta1_hip.h), choice = the
// smallest k of least D, modes_out = its byte; finalize: the winner's allocation, side record and coefficients are left in
// L.alloc, L.side and L.coefs, where the packing kernels read them.  choice, modes_out (units), distortion and energy (units *
// n_cand, unit-major) may each be null
void c1k_launch_choose_modes(const C1EncodeLaunch &L, const float *coefs_short, const uint8_t *side_short, const uint8_t *trial,
                             int64_t trial_stride, const uint8_t *cand, int n_cand, bool finalize, uint8_t *choice, uint8_t *modes_out,
                             double *distortion, double *energy, hipStream_t stream);
// the block modes chosen per unit by the error of the measured allocation (c1_k_measured_modes.hip; the definition is
// include/carta1_hip.h's).  The planes, the trial records and cand as for c1k_launch_choose_modes; sf_offsets as for
// c1k_launch_measured_sf.  Per (unit, candidate) what c1k_launch_measured_sf reports under that constant byte: distortion (units *
// n_cand * 2, unit-major: T_ref, T(n*)) and energy (units * n_cand); choice = the smallest k of least T_final, modes_out = its
// byte, taken and shifts (units * 52) the winner's; finalize: the winner's coefficients, side record (with the chosen indices)
// and allocation are left in L.coefs, L.side and L.alloc, where the packing kernels read them.  Every output may be null
void c1k_launch_measured_modes(const C1EncodeLaunch &L, const float *coefs_short, const uint8_t *side_short, const uint8_t *trial,
                               int64_t trial_stride, const uint8_t *cand, int n_cand, const int8_t *sf_offsets, int n_offsets, bool finalize,
                               uint8_t *choice, uint8_t *modes_out, uint8_t *taken, int8_t *shifts, double *distortion, double *energy,
                               hipStream_t stream);
// c1k_launch_measured_modes for few units (c1_k_measured_modes_wide.hip): a workgroup of eight waves per unit, one all-long and
// one all-short table instead of one per candidate, the 8 x n_cand greedy chains dealt over the waves; the same arguments, the
// same workspace, every output bit for bit
void c1k_launch_measured_modes_wide(const C1EncodeLaunch &L, const float *coefs_short, const uint8_t *side_short, const uint8_t *trial,
                                    int64_t trial_stride, const uint8_t *cand, int n_cand, const int8_t *sf_offsets, int n_offsets,
                                    bool finalize, uint8_t *choice, uint8_t *modes_out, uint8_t *taken, int8_t *shifts, double *distortion,
                                    double *energy, hipStream_t stream);
// launches of at most this many units take c1k_launch_measured_modes_wide: the largest count of DESIGN.md 6q's sweep (1 .. 8 192
// units, two candidates at offset 0 and eight at five offsets), at every one of which it was the faster kernel (10 times at up to
// 256 units with eight candidates, 1.4 to 2.4 times at 8 192); C1_MEASURED_WIDE overrides
constexpr int64_t kMeasuredModesWideUnits = 8192;
// c1k_launch_measured_modes / _wide with every candidate's errors weighed by one threshold per unit and BFU
// (c1_k_measured_modes_masked.hip, c1_k_measured_modes_masked_wide.hip; the definition is include/carta1_hip.h's): mask as for
// c1k_launch_measured_masked (floor[52], then the transposed matrix, device memory), P_b from the unit's all-long plane in L.coefs,
// which therefore always holds the all-long analysis, whatever the candidates.  weights (units * 52) may be null as every output
void c1k_launch_measured_modes_masked(const C1EncodeLaunch &L, const float *coefs_short, const uint8_t *side_short, const uint8_t *trial,
                                      int64_t trial_stride, const uint8_t *cand, int n_cand, const int8_t *sf_offsets, int n_offsets,
                                      const double *mask, bool has_spread, bool finalize, uint8_t *choice, uint8_t *modes_out,
                                      uint8_t *taken, int8_t *shifts, double *distortion, double *energy, double *weights,
                                      hipStream_t stream);
void c1k_launch_measured_modes_masked_wide(const C1EncodeLaunch &L, const float *coefs_short, const uint8_t *side_short,
                                           const uint8_t *trial, int64_t trial_stride, const uint8_t *cand, int n_cand,
                                           const int8_t *sf_offsets, int n_offsets, const double *mask, bool has_spread, bool finalize,
                                           uint8_t *choice, uint8_t *modes_out, uint8_t *taken, int8_t *shifts, double *distortion,
                                           double *energy, double *weights, hipStream_t stream);
// the word lengths allocated by the measured coding error (c1_k_measured.hip; the definition is include/carta1_hip.h's).  L.coefs,
// L.side: the analysis' planes; L.alloc: the record c1k_launch_allocate left for every unit.  Per unit the table e(b, w), the
// greedy allocation for each of the eight amounts, T_ref over the record and T(n*) over the best greedy one; taken = T(n*) <
// T_ref.  finalize: a taken unit's greedy record replaces the one in L.alloc, where the packing kernels read it; otherwise
// L.alloc is left alone.  taken (units), distortion (units * 2: T_ref, T(n*)) and energy (units) may each be null.  all_long:
// every unit has modes [0,0,0] (the side records' mode byte is not read)
void c1k_launch_measured_alloc(const C1EncodeLaunch &L, bool all_long, bool finalize, uint8_t *taken, double *distortion, double *energy,
                               hipStream_t stream);
// the measured allocation with every BFU's scale-factor index chosen by the same error (c1_k_measured_sf.hip; the definition is
// include/carta1_hip.h's): c1k_launch_measured_alloc over the table of least errors of the n_offsets candidate indices
// findScaleFactor + sf_offsets[k] (host memory, sf_offsets[0] == 0, n_offsets 1 .. 8).  finalize: a taken unit's greedy record
// replaces the one in L.alloc and its chosen indices the scale-factor bytes of L.side; otherwise both are left alone.  shifts
// (units * 52: the offset written per BFU, 0 where none) may be null like the other outputs
void c1k_launch_measured_sf(const C1EncodeLaunch &L, bool all_long, bool finalize, const int8_t *sf_offsets, int n_offsets, uint8_t *taken,
                            int8_t *shifts, double *distortion, double *energy, hipStream_t stream);
// c1k_launch_measured_sf with every BFU's error divided by a masking threshold (c1_k_measured_masked.hip; the definition is
// include/carta1_hip.h's).  mask: 52 + 52 * 52 doubles on the device, floor[b] at [b] and spread[b][c] at [52 + 52 * c + b] (the
// matrix transposed); has_spread false: M_b = +0.0 and the matrix is not read.  weights (units * 52: P_b) may be null like the
// other outputs
void c1k_launch_measured_masked(const C1EncodeLaunch &L, bool all_long, bool finalize, const int8_t *sf_offsets, int n_offsets,
                                const double *mask, bool has_spread, uint8_t *taken, int8_t *shifts, double *distortion, double *energy,
                                double *weights, hipStream_t stream);
// the three launches above for few units (c1_k_measured_wide.hip): a workgroup of eight waves per unit, the sixteen table rows
// dealt over the waves and one greedy amount per wave; every output is bit for bit the kernels' above.  mask null: P_b = 1 and no
// weights (c1k_launch_measured_sf); one offset 0 besides: c1k_launch_measured_alloc
void c1k_launch_measured_wide(const C1EncodeLaunch &L, bool all_long, bool finalize, const int8_t *sf_offsets, int n_offsets,
                              const double *mask, bool has_spread, uint8_t *taken, int8_t *shifts, double *distortion, double *energy,
                              double *weights, hipStream_t stream);
// launches of at most this many units take c1k_launch_measured_wide: the largest count of DESIGN.md 6l's sweep (1 .. 8 192 units),
// at every one of which it was the faster kernel (5 times at up to 256 units, 1.3 times at 8 192); C1_MEASURED_WIDE overrides
constexpr int64_t kMeasuredWideUnits = 8192;
// the coding error of given sound units (c1_k_measure_units.hip; the definition is include/carta1_hip.h's).  The mode byte of
// each of n units (device memory, 212 bytes each, any alignment) as deserializeFrame reports its block modes, low | mid << 2 |
// high << 4, not yet brought into the domain: c1k_launch_modes_front's input
void c1k_launch_unit_mode_bytes(const uint8_t *units, int64_t n, uint8_t *modes, hipStream_t stream);
// coefs: n * 512 coefficients of the exact analysis under those modes; units 4-byte aligned; mask as for
// c1k_launch_measured_masked, or null: P_b = 1.0.  noise, signal, weights (n * 52) and totals (n * 2) may each be null
void c1k_launch_measure_units(const C1DevTables *tables, const float *coefs, const uint8_t *units, int64_t n, const double *mask,
                              bool has_spread, double *noise, double *signal, double *totals, double *weights, hipStream_t stream);
// the same under the all-long threshold (c1_k_measure_units_shared.hip): coefs_long holds the n * 512 coefficients of the exact
// analysis under mode byte 0, from which the weights come as c1k_launch_measured_modes_masked forms them; mask is not null
void c1k_launch_measure_units_shared(const C1DevTables *tables, const float *coefs, const float *coefs_long, const uint8_t *units,
                                     int64_t n, const double *mask, bool has_spread, double *noise, double *signal, double *totals,
                                     double *weights, hipStream_t stream);
// the error of the decoded PCM of given sound units against the delayed input (c1_k_measure_pcm.hip; the definition is
// include/carta1_hip.h's): k_decode<double>'s walk over the units, the comparison in place of the PCM stores
void c1k_launch_measure_pcm(const C1MeasurePcmLaunch &L, hipStream_t stream);
void c1k_launch_pack(const C1EncodeLaunch &L, bool all_long, hipStream_t stream);   // all_long: every unit has modes [0,0,0]
void c1k_launch_pack_spec(const C1EncodeLaunch &L, bool all_long, hipStream_t stream);   // binary32 quantization with the guard band; fills the redo list
// running totals (c1_ctx::d_spec_totals) and their page-locked mirror; kind 0 speculative call (counts = list head), 1 binary32
// quantization of exact coefficients (counts[0] = repacked), 2 speculative detector (counts[0] = rechecked)
void c1k_launch_spec_totals(unsigned long long *totals, uint64_t units, const uint32_t *counts, int kind, hipStream_t stream);
// the speculative kernel's slot array (L.defer_list) -> dense list of deferred runs; counts[0] = entries, counts[1] = units covered
void c1k_launch_defer_compact(const C1EncodeLaunch &L, uint32_t *list, uint32_t *counts, hipStream_t stream);
// open_masks -> a dense list of units (counts[0] = entries), for the exact pre-pass of the units with an open scale factor
void c1k_launch_open_compact(const C1EncodeLaunch &L, uint32_t *list, uint32_t *count, hipStream_t stream);
void c1k_launch_decode(const C1DecodeLaunch &L, bool binary32, hipStream_t stream);   // binary32: opt-in, PCM within rounding noise of the reference
// the decode() closure from frame fields (c1_k_decode_fields.hip), the reference's number model always.  Any int32 field value
// is memory-safe (nbfu clamped to 0..52, wl & 15, sfi & 63 on the read path); the output is the reference's for nbfu 0..52 and,
// below nbfu, wl 0..15 and sfi 0..63
void c1k_launch_decode_fields(const C1DecodeFieldsLaunch &L, hipStream_t stream);
// the frame closures over explicit pool state (c1_k_state.hip); n <= 0 launches nothing
void c1k_launch_encode_from_states(const C1EncStateLaunch &L, hipStream_t stream);
void c1k_launch_decode_from_states(const C1DecStateLaunch &L, hipStream_t stream);
// the same closures over index lists (C1EncStateLaunch / C1DecStateLaunch, row-indexed form)
void c1k_launch_encode_rows(const C1EncStateLaunch &L, hipStream_t stream);
void c1k_launch_decode_rows(const C1DecStateLaunch &L, hipStream_t stream);
// rows of `dwords` 32-bit words each: dst[dst_rows[r]] = src[src_rows[r]] for r < n, a lane per dword (sound units are 53
// dwords, states 483 / 179: multiples of 4 bytes, not of 16).  A null list is the identity; src_broadcast: every row copies
// src row 0.  Rows of one launch must not overlap each other
void c1k_launch_copy_rows(uint32_t *dst, const uint32_t *dst_rows, const uint32_t *src, const uint32_t *src_rows, int src_broadcast,
                          int64_t n, int dwords, hipStream_t stream);
// the first one or two frames of n signals in one pass, and the rows of a signals call to their places (c1_k_signal_starts.hip)
void c1k_launch_signal_starts(const C1SignalStartsLaunch &L, hipStream_t stream);
void c1k_launch_scatter_signal_rows(const C1ScatterRowsLaunch &L, hipStream_t stream);
// the rows of a measured mode search over n signals to their places (c1_k_signal_rows_modes.hip)
void c1k_launch_scatter_signal_rows_modes(const C1ScatterRowsModesLaunch &L, hipStream_t stream);
// performFFT's magnitudes of `rows` stored band rows (512 floats each) into the transient_mags of states[0 .. rows)
void c1k_launch_state_mags(const C1DevTables *tables, const float *bands, int64_t rows, float *states, hipStream_t stream);
// kind_mask: bit k = fill the 512-frame segments with (segment & 3) == k (15 = all)
void c1k_launch_generate_white(const uint32_t *frame_states, int64_t frames, float *pcm, int kind_mask, double amp, hipStream_t stream);
void c1k_launch_generate_pink(const uint32_t *segment_states, int64_t frames, float *pcm, int kind_mask, hipStream_t stream);
void c1k_launch_generate_sines(int64_t frames, float *pcm, int kind_mask, uint32_t seed, hipStream_t stream);
void c1k_launch_pcm_from_int(const void *src, int bits, int channels, int64_t n, float *const *pcm, hipStream_t stream);
void c1k_launch_pcm_to_int16(const float *const *pcm, int channels, int64_t n, int16_t *dst, hipStream_t stream);
