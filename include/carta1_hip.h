/*
 * carta1_hip.h -- C ABI of libcarta1_hip.so: the MI355X (gfx950) ATRAC1 hot path.
 *
 * This is the drop-in boundary for aynik/carta1's encode/decode hot path.  The
 * reference has no FFI of its own; the seam is the module boundary between
 * codec/pipeline/ and codec/io/processor.js (stay JavaScript) and
 * codec/transforms/{qmf,mdct,fft}.js, codec/analysis/transient.js,
 * codec/coding/{bitallocation,quantization}.js (replaced by HIP kernels).  Each
 * entry point below names the reference code it stands in for (file:line in
 * aynik/carta1 v1.1.10).  The N-API addon (carta1_amd/js/addon/) and the ctypes
 * binding (carta1_amd/capi.py) bind exactly these symbols; INTEGRATION.md shows
 * the reference-side patch.
 *
 * Conventions
 *  - every function returns 0 on success, non-zero on error; c1_last_error()
 *    (thread-local) then holds the message.  There is NO CPU fallback: without a
 *    usable HIP device every compute entry point fails with C1_ERR_NO_DEVICE.
 *  - PCM is planar float32, one pointer per channel, 512 samples per frame.
 *  - sound units are 212 bytes each, interleaved L,R,L,R,... for stereo
 *    (codec/io/processor.js:125-130), unit index = frame * channels + channel.
 *  - "history": a frame's unit depends on at most the 650 PCM samples before it
 *    (266 with fixed block modes).  Batch calls take `halo_frames`
 *    = how many whole frames (0..2) of real PCM sit in memory directly BEFORE the
 *    pcm pointers; samples before that are taken as zero, which is exactly a
 *    stream start (codec/core/buffers.js:30-42 zero-initialised BufferPool).
 *  - decoded PCM of frame n depends on units n and n-1 only; decode calls take
 *    `halo_units` (0 or 1) = whether the unit(s) of frame -1 precede the pointer.
 */
#ifndef CARTA1_HIP_H
#define CARTA1_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define C1_FRAME_SAMPLES 512
#define C1_UNIT_BYTES 212
#define C1_MAX_CHANNELS 2
#define C1_ABI_VERSION 3

enum {
  C1_OK = 0,
  C1_ERR_ARG = 1,        /* bad argument (message says which) */
  C1_ERR_NO_DEVICE = 2,  /* no HIP device / runtime: the product path never falls back to CPU */
  C1_ERR_HIP = 3,        /* a HIP call failed */
  C1_ERR_STATE = 4       /* handle used in the wrong state */
};

/* Numeric tables the reference builds at module load with V8's Math.sin/cos/pow/sqrt
 * (codec/core/constants.js:60-66,144-150; codec/transforms/mdct.js:27-36;
 * codec/transforms/fft.js:37-39).  libm differs from V8 in the last bit on some entries,
 * so the library never recomputes them: it carries the values the reference produced
 * (c1_get_default_tables) and a JavaScript host may install the ones its own V8 computes
 * (c1_set_tables) so results track the reference running in that same process. */
typedef struct c1_tables {
  double scale_factors[64];   /* SCALE_FACTORS            constants.js:144-150 */
  double window_short[32];    /* WINDOW_SHORT             constants.js:60-66   */
  double mdct_fwd64[32];      /* mdct64.sinCosTable       mdct.js:215          */
  double mdct_fwd256[128];    /* mdct256.sinCosTable      mdct.js:216          */
  double mdct_fwd512[256];    /* mdct512.sinCosTable      mdct.js:217          */
  double mdct_inv64[32];      /* imdct64.sinCosTable      mdct.js:219          */
  double mdct_inv256[128];    /* imdct256.sinCosTable     mdct.js:220          */
  double mdct_inv512[256];    /* imdct512.sinCosTable     mdct.js:221          */
  double fft_w[8][2];         /* (cos,sin)(-2*pi/stride), stride = 2..256; fft.js:37-39 */
  double log1p_10;            /* Math.log1p(10)           transient.js:211     */
} c1_tables;

/* EncoderOptions as the hot path consumes them (codec/core/options.js:17-23). */
typedef struct c1_encode_options {
  double biased_scale_factors[64]; /* pow(SCALE_FACTORS[i], allocationBias), bitallocation.js:46-61;
                                      computed by the HOST (its Math.pow), bias==1 -> SCALE_FACTORS */
  double transient_threshold;      /* options.transientThresholdLow: the pipeline uses the LOW
                                      threshold for all three bands (encoder.js:137-141) */
  int32_t fixed_block_modes[3];    /* options.fixedBlockModes, or {-1,-1,-1} for transient detection */
  int32_t reserved;
} c1_encode_options;

typedef struct c1_ctx c1_ctx; /* one per (device, stream): workspace + tables on that device */

/* ---- library ------------------------------------------------------------------------- */
int c1_abi_version(void);
const char *c1_last_error(void);
int c1_device_count(int *count);                 /* hipGetDeviceCount */
int c1_get_default_tables(c1_tables *out);       /* the V8-produced defaults compiled into the library */
int c1_set_tables(const c1_tables *tables);      /* NULL restores defaults; applies to contexts created afterwards */
/* fills biased_scale_factors for allocationBias == 1 (exact copy, bitallocation.js:51-52) and sets
 * threshold 1.0 / detection on: the EncoderOptions defaults (options.js:17-23) */
int c1_default_encode_options(c1_encode_options *out);
/* Diagnostics (host only, no device needed): two properties of the tables currently installed.
 *  scale_factor_bits  1 when SCALE_FACTORS has the structure of 2^(i/3-21) in binary32 (exact powers of two at i % 3 == 0,
 *                     one pair of fraction patterns shared by every octave); the speculative paths require it.  It does
 *                     not change findScaleFactor (bitallocation.js:290-299), which is ceil(3 (log2 m + 21)) whatever the
 *                     table: the kernels always read it off the binary32 bit pattern against those fixed boundaries.
 *  dequant_reciprocal dequantize's (q * SF) / range (quantization.js:65-78): 1 = as multiply + two FMAs with RN(1 / range);
 *                     2 = moreover, after the store to the Float32 array, equal to q * RN(SF * RN(1 / range)) for every
 *                     (word length, scale factor, q): one product per BFU and one per coefficient.  Both are verified on
 *                     the host against the division for the whole input domain when tables are installed; the kernels
 *                     fall back to it when a check fails */
int c1_table_fast_paths(int *scale_factor_bits, int *dequant_reciprocal);
/* Diagnostics (host only): how the bit allocation will order heap priorities for opts' biased table.  affine = 1: by
 * the integer form A*sfi + C (word length 0) / A*sfi - B*(wl + 1) (wl >= 1) plus an offset, coef = {A, B, C, offset};
 * affine = 0: by the table of ranks of the Float32 priorities (coef zero).  Fails as encoding would on a bad table. */
int c1_alloc_rank_form(const c1_encode_options *opts, int *affine, int *coef);
/* Diagnostics (host only): the tables the bit allocation kernels derive from opts' biased table (any pointer may be NULL).
 *  affine, steps   1 and the two words a successful heap step adds to the root's entry (from word length 0, from any
 *                  other); 0 and zeros when the kernels look ranks up instead
 *  rank            64 x 16: the rank field of the heap entry of (sfi, wl) as the kernels form it (sfi 0 and wl 15 unused)
 *  dist_ok, dist   8 x 64 x 2 doubles per (BFU size in the order 4 6 7 8 9 10 12 20, sfi): the zero-bit term
 *                  Float32(biased * 2 * size) and biased * size, whose exponent minus the bit count is the coded term;
 *                  dist_ok = 1 when that equals the reference's biased * 2^-bits * size for every case (else the kernels
 *                  form the terms as the reference does) */
int c1_alloc_tables(const c1_encode_options *opts, int *affine, uint32_t *steps, uint16_t *rank, int *dist_ok, double *dist);

/* ---- contexts ------------------------------------------------------------------------- */
/* A context works on one device and one stream: its own (hip_stream NULL; a non-blocking stream, ordered with nothing of
 * the caller's, see c1_ctx_synchronize) or the caller's.  On a caller's stream every *_device call behaves like one kernel
 * launch on that stream, whatever internal streams it uses:
 *   - it is ordered after everything queued on the stream before it: inputs written by earlier work are read as written;
 *   - when it returns, the stream has been made to wait for all of its work, so everything queued after it sees the finished
 *     outputs and may overwrite every buffer of the call, inputs included;
 *   - the host-resident entry points return with the stream drained, work queued before them included;
 *   - the stream is never destroyed by the library: c1_ctx_destroy waits for the context's work on it and leaves it usable;
 *   - several contexts may be created on one stream; their calls are ordered as they are issued.
 * A call that changes the options or grows the workspace synchronises the stream on the host. */
int c1_ctx_create(int device, void *hip_stream /* hipStream_t or NULL = own stream */, c1_ctx **out);
int c1_ctx_destroy(c1_ctx *ctx);
int c1_ctx_synchronize(c1_ctx *ctx);
/* milliseconds the device spent in the named kernel during the most recent *_device call on this
 * context ("analysis", "allocate", "pack", "decode", "redo", "choose", "measure", "meter", or "total"), in the most recent c1_pack_units call
 * ("pack_units"), or in the most recent decode from frame fields -- c1_decode_fields_*, c1_dec_stream_push_fields or a
 * unit push that follows one ("decode_fields") -- or in the from-state kernel of the most recent c1_*_frames_from_states*
 * call ("from_state") -- from HIP events on the context's stream; c1_ctx_set_profiling(ctx, 1)
 * must have been set before the call.  After a c1_*_signals* call, "signal_starts" is the time in the kernels that call adds
 * to the bulk pass (the row-indexed from-state kernels and the row copies), the other names cover the bulk pass plus the
 * allocation and packing of the re-encoded frames, and "total" the whole call */
int c1_ctx_set_profiling(c1_ctx *ctx, int enabled);
int c1_ctx_kernel_ms(c1_ctx *ctx, const char *name, double *ms, int *launches);

/* Speculative encoding of fixed-block-mode streams.  The encoder's outputs are integers; they are
 * decisions taken on the MDCT coefficients (bitallocation.js:290-299, quantization.js:43-53).  For fixedBlockModes
 * [0,0,0] the library first computes the coefficients in binary32 together with a proven bound on their distance
 * from the reference's binary64-then-rounded values, accepts every sound unit whose decisions are the same for all
 * values within the bound, and re-encodes the others with the exact kernels: the result is bit-identical to the
 * exact path by construction.  mode: 0 = exact kernels only; 1 = material-local (default): every 16 frames of a
 * 64-frame run the speculative kernel predicts, from the scale-factor indices and its bound, how many decisions of a
 * unit the guards will leave open, and past a threshold hands the rest of that run to the exact kernels -- the choice
 * is taken per run inside the call, never carried from one call or stream to the next; 2 = always speculate.
 * In mode 1 a call of fewer than 64 sound units (a frame closure, a short streaming push) uses the exact kernels only:
 * it is bound by the number of launches behind it, and every shortcut adds some.
 * The environment variable C1_SPEC (0/1/2) sets the default of new contexts. */
int c1_ctx_set_speculation(c1_ctx *ctx, int mode);
/* units that stayed with the speculative analysis and units among them that were redone exactly, since the context
 * was created (or since the last call with reset != 0); synchronises the context's stream */
int c1_ctx_speculation_stats(c1_ctx *ctx, uint64_t *units, uint64_t *redone, int reset);
/* units of speculative calls whose runs the speculative analysis handed to the exact kernels (mode 1; cleared by
 * c1_ctx_speculation_stats(reset)); synchronises the context's stream */
int c1_ctx_speculation_deferred(c1_ctx *ctx, uint64_t *units);
/* The exact paths (transient detection, mixed fixed modes, runs the speculative analysis handed over)
 * quantize the reference's coefficients in binary32 with the same guard band and pack the few units it cannot certify
 * again in binary64 (0.07 % of noise-like units to 4 % of stationary partials): units packed that way so far and units
 * packed twice (cleared by c1_ctx_speculation_stats(reset)).  Like the detector below it is used whenever speculation is
 * not 0; no decision of the encode path depends on what a context encoded before. */
int c1_ctx_quantization_stats(c1_ctx *ctx, uint64_t *units, uint64_t *repacked);
/* Transient detection (blockSelectorStage, encoder.js:111-152) runs speculatively too unless speculation is 0: the
 * transient FFT (transient.js:17-35) in binary32, an interval that provably contains the reference's transient score
 * (transient.js:197-226), the decision `score > threshold` where the whole interval lies on one side, and the
 * reference's own arithmetic for the units left open.  Units decided that way so far and units among them that needed
 * the exact recheck (cleared by c1_ctx_speculation_stats(reset)). */
int c1_ctx_detection_stats(c1_ctx *ctx, uint64_t *units, uint64_t *rechecked);

/* Decoder arithmetic: one of three models per context.
 *   C1_DECODE_EXACT (0, default): the reference's -- binary64 operations, binary32 at every typed-array store -- decoded PCM
 *     and decoder state bit-identical to the reference, on every entry.
 *   C1_DECODE_BINARY32_BULK (1): the unit-walking kernel alone (c1_decode_device / _batch, c1_decode_wav16_batch, the bulk of
 *     c1_decode_signals*, a c1_dec_stream while it is pushed units) computes in binary32; the PCM then differs from the
 *     reference's by rounding noise (at most 11 u of a coefficient's peak response and 3 u of a stream's RMS, u = 2^-24,
 *     DESIGN.md 6s).  Everything that decodes from frame fields or from a c1_dec_state stays exact: c1_decode_fields_*,
 *     c1_decode_frames_from_states*, the first frame of every signal of c1_decode_signals* and the states it writes,
 *     c1_dec_stream_push_fields, a stream's pushes from a c1_dec_stream_set_state or push_fields onwards, and
 *     c1_dec_stream_get_state.
 *   C1_DECODE_BINARY32 (2): every decode entry of the context that produces PCM or decoder state computes in binary32, in the
 *     unit-walking kernel's arithmetic operation for operation: c1_decode_device / _batch, c1_decode_wav16_batch,
 *     c1_decode_fields_device / _batch, c1_decode_frames_from_states*, c1_decode_signals* (the bulk, the first frames and the
 *     states written out), c1_dec_stream_push in all its branches, c1_dec_stream_push_fields and c1_dec_stream_get_state /
 *     _set_state.  Sound units decode to the same bits through any of them and through any split into calls.
 * A stream reads its context's model at every call.  A c1_dec_state is 179 floats under any model (the binary32 delay lines
 * are stored as they are, the exact ones hold binary32 values already), so a change of model between two pushes is well
 * defined: each frame is decoded from the state before it under the model in force.
 * Under every model these stay in the reference's arithmetic: c1_measure_pcm_*, the single-stage exports (c1_dequantize,
 * c1_dequantize_frames, c1_imdct_batch, c1_qmf_synthesis_batch, c1_unpack_units) and c1_decode_batch_multi, which takes no
 * context.
 * c1_ctx_set_decode_model: C1_ERR_ARG for a NULL context or any other value, which leaves the model unchanged.
 * c1_ctx_set_decode_precision(ctx, x) is c1_ctx_set_decode_model(ctx, x ? C1_DECODE_BINARY32_BULK : C1_DECODE_EXACT). */
#define C1_DECODE_EXACT 0
#define C1_DECODE_BINARY32_BULK 1
#define C1_DECODE_BINARY32 2
int c1_ctx_set_decode_model(c1_ctx *ctx, int model);
int c1_ctx_get_decode_model(c1_ctx *ctx, int *model);
int c1_ctx_set_decode_precision(c1_ctx *ctx, int binary32);

/* ---- encode: replaces the encode() frame closure body, encoder.js:438-450
 *      (qmfAnalysisStage :57-96, blockSelectorStage :111-152, mdctStage :170-349,
 *      quantizationStage :365-418) plus serializeFrame (serialization.js:41-98), batched ----- */

/* device-resident: pcm[c] and units are DEVICE pointers; asynchronous on the context's stream: the call only enqueues
 * work and never waits for the device (it blocks only to grow the workspace on a first, larger call, or when the
 * options change while earlier calls are still queued).
 * Device memory: the context keeps a workspace of 2.6 KB per sound unit (4.8 KB with transient detection) for the largest
 * batch it has seen, until it is destroyed.  A batch is kept in one piece when that fits (up to 2^24 frames per channel, or
 * C1_CHUNK_FRAMES from the environment) and is otherwise cut into chunks of what 90 % of the free device memory holds; the
 * output is the same bytes either way. */
int c1_encode_device(c1_ctx *ctx, const float *const *pcm, int channels, int64_t frames,
                     int halo_frames, const c1_encode_options *opts, uint8_t *units);
/* host-resident: copies in, runs c1_encode_device, copies out, synchronises.
 * This is what encodeAeaPcm's hot loop (processor.js:119-136) calls once per batch. */
int c1_encode_batch(c1_ctx *ctx, const float *const *pcm, int channels, int64_t frames,
                    int halo_frames, const c1_encode_options *opts, uint8_t *units);

/* ---- encode with the block modes supplied by the caller: encode() with options.fixedBlockModes set before every frame
 *      (blockSelectorStage reads it on every call, encoder.js:129-133) -------------------------------------------------------
 * Frames 0 .. frames-1 of every channel are encoded exactly as the reference's closure encodes them when fixedBlockModes =
 * the frame's modes is set before each call: the detector does not run (transientDetection is not touched, :130-132), the QMF
 * delays and the MDCT overlap carry across frames whatever the modes are (functions of the PCM history alone, as under
 * c1_enc_stream_set_options), and every channel has its own mode per frame.
 * modes: one byte per sound unit, m0 | m1 << 2 | m2 << 4 (low, mid, high band), unit index = frame * channels + channel --
 * the bytes c1_detect_stages_device and c1_detect_scores_device write into `modes`, so a tap's output can be edited and fed
 * straight back.  Domain: what blockSelectorStage produces (:143): low and mid fields 0 or 2, high field 0 or 3, bits 6-7
 * clear.  Modes cover the call's frames only; halo frames need none.
 * opts->biased_scale_factors = allocationBias's table (threshold and fixed modes are not read); opts is validated as every
 * encode call validates it.
 * The bytes do not depend on the speculation mode (given modes always take the exact analysis; unless speculation is 0 the
 * quantization runs in binary32 behind its guard, as on the other exact paths), on how the call is cut into chunks
 * (C1_CHUNK_FRAMES, C1_PIPELINE, C1_OVERLAP) or on the run length.  c1_ctx_kernel_ms counts the front end and the MDCT under
 * "analysis".
 *
 * device-resident: pcm[c] (16-byte aligned), modes (any alignment) and units are DEVICE pointers; asynchronous on the context's
 * stream like c1_encode_device, chunked like it (a transient-detection call's workspace, 4.8 KB per unit); frames 0 .. 2^27 per
 * channel.  The mode bytes are NOT checked: every byte is brought into the domain before a kernel indexes with its fields
 * (fields & 2 for low and mid; high 3 when it is 3, else 0), so no access leaves the buffers, and for a byte outside the
 * domain the unit's content is unspecified. */
int c1_encode_modes_device(c1_ctx *ctx, const float *const *pcm, int channels, int64_t frames, int halo_frames,
                           const c1_encode_options *opts, const uint8_t *modes /* device, frames*channels */, uint8_t *units);
/* host-resident, synchronous: every mode byte is validated before any device work -- a byte outside the domain returns
 * C1_ERR_ARG naming the frame, the channel (of two) and the field, and nothing is written -- then one copy in, the device call,
 * one copy out.  frames 0 .. 2^22 per channel (the three-stream pipeline of c1_encode_batch is not used here). */
int c1_encode_modes_batch(c1_ctx *ctx, const float *const *pcm, int channels, int64_t frames, int halo_frames,
                          const c1_encode_options *opts, const uint8_t *modes /* host, frames*channels */, uint8_t *units);

/* ---- encode with the allocation bias supplied per frame and channel: encode() with options.allocationBias set before every
 *      frame (quantizationStage reads it on every call, encoder.js:393) -----------------------------------------------------
 * palette: n_palette (1 .. C1_MAX_BIAS_PALETTE) option sets in HOST memory; bias_index: one byte per sound unit, unit index =
 * frame * channels + channel.  Unit u is encoded exactly as the reference's closure for that channel encodes the frame when
 * options.allocationBias was set, before that call, to the bias behind palette[bias_index[u]].biased_scale_factors.  The bias
 * reaches the bit allocation alone (analysis does not read it, and quantize uses SCALE_FACTORS), so nothing is carried from
 * frame to frame by it: everything else is as in c1_encode_modes_* (modes given) or c1_encode_device (modes NULL).  Every
 * table an encode call accepts is accepted in every entry; an invalid one returns C1_ERR_ARG naming the entry.  Eight entries
 * are what the host keeps derived tables for, so a repeated palette rebuilds nothing.
 * modes non-NULL: the bytes and the domain of c1_encode_modes_*; the entries' transient_threshold and fixed_block_modes are
 * not read.  modes NULL: transient detection or fixed modes as the entries say -- all entries must then agree in
 * fixed_block_modes and in the bit pattern of transient_threshold (else C1_ERR_ARG naming the first entry that differs), and
 * are validated as every encode call validates them.
 * The call always takes the exact analysis (given modes: the front end of c1_encode_modes_device; else the exact kernels of
 * c1_encode_device, the detector as there); unless speculation is 0 the quantization runs in binary32 behind its guard.  The
 * bytes do not depend on the speculation mode, the run length or on how the call is cut into chunks (C1_CHUNK_FRAMES,
 * C1_PIPELINE, C1_OVERLAP).  The units of a chunk are sorted by entry into lists (4 bytes per unit and entry of workspace) and
 * the allocation kernels run once per entry over its list, one chain after the other; c1_ctx_kernel_ms counts the sorting and
 * all chains under "allocate".
 *
 * device-resident: pcm[c] (16-byte aligned), bias_index, modes and units are DEVICE pointers; asynchronous on the context's
 * stream like c1_encode_device and chunked like c1_encode_modes_device; frames 0 .. 2^27 per channel.  A palette whose tables
 * differ from the ones uploaded last synchronises the stream on the host, as a change of options does.  The index bytes are
 * NOT checked: a byte >= n_palette selects entry 0, so no access leaves the buffers; for such a byte the unit's content is
 * unspecified and every other unit is unaffected.  Mode bytes as for c1_encode_modes_device. */
#define C1_MAX_BIAS_PALETTE 8
int c1_encode_biases_device(c1_ctx *ctx, const float *const *pcm, int channels, int64_t frames, int halo_frames,
                            const c1_encode_options *palette /* HOST, n_palette entries */, int n_palette,
                            const uint8_t *bias_index /* device, frames*channels */,
                            const uint8_t *modes /* device, frames*channels, or NULL */, uint8_t *units);
/* host-resident, synchronous: the palette, every index byte (< n_palette) and every mode byte are validated before any device
 * work -- a bad byte returns C1_ERR_ARG naming the frame and the channel (of two), and nothing is written -- then one copy in,
 * the device call, one copy out.  frames 0 .. 2^22 per channel. */
int c1_encode_biases_batch(c1_ctx *ctx, const float *const *pcm, int channels, int64_t frames, int halo_frames,
                           const c1_encode_options *palette, int n_palette, const uint8_t *bias_index /* host */,
                           const uint8_t *modes /* host, or NULL */, uint8_t *units /* host */);

/* ---- encode with the allocation bias of every sound unit chosen from a palette by least coding error ----------------------
 * The reference's allocator (bitallocation.js:74-190) minimises a model of the distortion, biased[sfi] * 2^-bits * size, and
 * never sees the mantissas quantize produces.  This call measures them: one analysis, one allocation per palette entry over
 * every unit, and per (unit u, entry k), in binary64,
 *     D(u,k) = sum_i (c[i] - d_k[i])^2        E(u) = sum_i c[i]^2        i = 0 .. 511
 * where c are the Float32 MDCT coefficients as quantizationStage receives them (encoder.js:365; the exact kernels', whatever
 * the speculation mode) and d_k the Float32 coefficients dequantizationStage (decoder.js:52-98) produces from the sound unit
 * the reference writes for u with allocationBias = entry k's bias: Float32((q * SCALE_FACTORS[sfi]) / range)
 * (quantization.js:65-78) of the mantissas q of quantization.js:34-56, zero where a BFU is at or above the unit's amount or
 * has word length 0.  choice[u] is the smallest k with D(u,k) <= D(u,j) for all j, on the values computed: a NaN never wins,
 * and if every entry's D is NaN the choice is 0.  The order of the sums is fixed (a lane's 8 slots in order, then one tree
 * over the 64 lanes), so the same inputs give the same bits run after run, and entries with identical tables give identical
 * D: the lower index wins.  units[u] are exactly the bytes of c1_encode_biases_* with bias_index[u] = choice[u], packed by
 * the same kernels.  Nothing is carried from frame to frame by the bias or the choice.
 * palette, modes, their validation, the limits on frames, alignment, chunking and the caller's-stream contract are those of
 * c1_encode_biases_device / _batch: modes NULL makes all entries agree in threshold and fixed modes; mode bytes are checked by
 * the batch call and brought into the domain on the device by the device call.  Each output may be NULL (units NULL: measure
 * only, no packing runs); all four NULL is C1_ERR_ARG.  distortion is unit-major: D(u,k) at [u * n_palette + k].  With one
 * entry the call is the report "how well was this coded".  The call always takes the exact analysis; no output depends on
 * the speculation mode, the run length, C1_CHUNK_FRAMES, C1_PIPELINE, C1_OVERLAP or the halo.  Workspace: 32 bytes per unit
 * and entry on top of an encode call's.  c1_ctx_kernel_ms counts the trial allocations under "allocate" and the measuring
 * kernel under "choose". */
int c1_encode_best_bias_device(c1_ctx *ctx, const float *const *pcm, int channels, int64_t frames, int halo_frames,
                               const c1_encode_options *palette /* HOST, n_palette entries */, int n_palette,
                               const uint8_t *modes /* device, frames*channels, or NULL */,
                               uint8_t *units /* device, frames*channels*212, or NULL: measure only */,
                               uint8_t *choice /* device, frames*channels, or NULL */,
                               double *distortion /* device, frames*channels*n_palette (unit-major), or NULL */,
                               double *energy /* device, frames*channels, or NULL */);
/* host-resident, synchronous: every pointer HOST.  The palette, the outputs and every mode byte are validated before the
 * context is looked at or any device work is done (C1_ERR_ARG, nothing written); without a context and without a device the
 * call then returns C1_ERR_NO_DEVICE.  One copy in, the device call, one copy out per output.  frames 0 .. 2^22 per channel. */
int c1_encode_best_bias_batch(c1_ctx *ctx, const float *const *pcm, int channels, int64_t frames, int halo_frames,
                              const c1_encode_options *palette, int n_palette, const uint8_t *modes /* host, or NULL */,
                              uint8_t *units /* host, or NULL */, uint8_t *choice /* host, or NULL */,
                              double *distortion /* host, or NULL */, double *energy /* host, or NULL */);

/* ---- encode with the block modes of every sound unit chosen from candidates by least coding error -------------------------
 * The reference sets the block modes open loop: its transient detector never sees the coded result, and c1_encode_modes_*
 * takes them from a caller who must already know them.  This call measures them.  cand_modes: n_cand (1 ..
 * C1_MAX_MODE_CANDIDATES) distinct mode bytes of the domain of c1_encode_modes_* (low and mid fields 0 or 2, high field 0 or
 * 3, bits 6-7 clear) in HOST memory, in the caller's order; choice indexes them.  Both calls check the bytes (the array is
 * host memory in both): a byte outside the domain, a duplicate, or n_cand outside 1..8 returns C1_ERR_ARG naming the entry,
 * and nothing is written.  Of opts only biased_scale_factors is read; the detector never runs and a stream's detection
 * history is not involved.  Per (unit u, candidate k), in binary64,
 *     D(u,k) = sum_i W(band(i), mode_k(band(i))) * (c_k[i] - d_k[i])^2
 *     E(u,k) = sum_i W(band(i), mode_k(band(i))) * c_k[i]^2                    i = 0 .. 511
 * where c_k are the Float32 MDCT coefficients quantizationStage receives (encoder.js:365) when fixedBlockModes = candidate k
 * was set before the frame, d_k what dequantizationStage (decoder.js:52-98) makes of the sound unit the reference writes for
 * that frame under candidate k and opts' bias (zero where a BFU is at or above the unit's amount or has word length 0), band(i)
 * is low for i < 128, mid for i < 256 and high otherwise, and W is 1 for a band coded long, 1/4 for the low or mid band coded
 * short and 1/2 for the high band coded short: the reference's short transforms carry 4 (low, mid) and 2 (high) times the
 * energy of its long ones for the same signal (mdct.js:215-221), so the weighted error is the PCM error energy up to one
 * constant and the D of different candidates, and of separate calls, are comparable.  A candidate's coefficients are those of
 * the frame whatever modes the frames before it took (applyTailWindowing, encoder.js:309-316, saves the same windowed tail
 * for a long and a short band), so nothing is carried from frame to frame by the choice.  choice[u] is the smallest k with
 * D(u,k) <= D(u,j) for all j, on the values computed: a NaN never wins, and if every D is NaN the choice is 0.
 * modes_out[u] = cand_modes[choice[u]].  The order of the sums is fixed (a lane's 8 BFU-major slots in order, the lane's sum
 * times W -- a power of two, so that is the sum of the weighted terms bit for bit -- then one tree over the 64 lanes), no
 * fused operation is used, and the same inputs give the same bits run after run.  units[u] are exactly the bytes of
 * c1_encode_modes_* with modes[u] = modes_out[u] and the same opts, packed by the same kernels.  Each output may be NULL
 * (units NULL: measure only, no packing runs); all five NULL is C1_ERR_ARG.  distortion and energy are unit-major: D(u,k) at
 * [u * n_cand + k].  With one candidate the call is c1_encode_modes_* under a constant byte plus its quality report.
 * Limits, alignment, chunking, asynchrony and the caller's-stream contract are those of c1_encode_best_bias_device; no output
 * depends on the speculation mode, the run length, C1_CHUNK_FRAMES, C1_PIPELINE, C1_OVERLAP or the halo.  The device path
 * runs the exact analysis at most twice (all long, all short: a band's coefficients and scale-factor indices depend on that
 * band's mode only), one allocation per candidate, and one measuring kernel.  Workspace: 2.2 KB per unit (the second
 * analysis) and 32 bytes per unit and candidate on top of a c1_encode_modes_device call's.  c1_ctx_kernel_ms counts the
 * analyses and the composing of the candidates' side records under "analysis", the trial allocations under "allocate" and
 * the measuring kernel under "choose".
 * A joint search over modes and biases composes from separate calls, because their weighted D are comparable: one
 * measure-only call per bias, the least D per unit over all of them, then one c1_encode_biases_* call with the winning
 * modes and bias_index.  No entry point does it in one call, on purpose: on the CPU model the exhaustive 8 x 8 minimum
 * beats the two-call sequence (best modes at bias 1, then the best bias under them) by 0.15 dB on pink noise with transients,
 * 0.12 dB on white noise and 0.09 dB on a tonal and noise mix, which is not worth sixty-four allocation chains per unit.
 * The larger lever is c1_encode_measured_* below. */
#define C1_MAX_MODE_CANDIDATES 8
int c1_encode_best_modes_device(c1_ctx *ctx, const float *const *pcm, int channels, int64_t frames, int halo_frames,
                                const c1_encode_options *opts, const uint8_t *cand_modes /* HOST, n_cand bytes */, int n_cand,
                                uint8_t *units /* device, frames*channels*212, or NULL: measure only */,
                                uint8_t *choice /* device, frames*channels, or NULL */,
                                uint8_t *modes_out /* device, frames*channels, or NULL: cand_modes[choice[u]] */,
                                double *distortion /* device, frames*channels*n_cand (unit-major), or NULL */,
                                double *energy /* device, frames*channels*n_cand (unit-major), or NULL */);
/* host-resident, synchronous: every pointer HOST.  The candidates and the outputs are validated before the context is looked
 * at or any device work is done (C1_ERR_ARG, nothing written); without a context and without a device the call then returns
 * C1_ERR_NO_DEVICE.  One copy in, the device call, one copy out per output.  frames 0 .. 2^22 per channel. */
int c1_encode_best_modes_batch(c1_ctx *ctx, const float *const *pcm, int channels, int64_t frames, int halo_frames,
                               const c1_encode_options *opts, const uint8_t *cand_modes /* host */, int n_cand,
                               uint8_t *units /* host, or NULL */, uint8_t *choice /* host, or NULL */,
                               uint8_t *modes_out /* host, or NULL */, double *distortion /* host, or NULL */,
                               double *energy /* host, or NULL */);

/* ---- encode with the word lengths of every sound unit allocated by the measured coding error ------------------------------
 * allocateBits (bitallocation.js:74-281) spends the 1696 - 40 - 10 nBfu mantissa bits of a unit by a model of the distortion,
 * biased[sfi] * 2^-bits * size, and never sees the mantissas quantize produces; the bias only bends that model.  This call
 * allocates by the error measured.  OPT-IN, and a new kind of output: the units are NOT those the reference's encoder writes.
 * They are ordinary sound units all the same -- the reference's block modes and scale-factor indices, mantissas that are what
 * quantize (quantization.js:34-56) gives at the chosen word lengths, serializeFrame's layout -- and the reference's decode()
 * reads them.  Every other entry point stays bit-identical to the reference.
 * Definition.  Take unit u with its block modes: modes[u] when given (as for c1_encode_modes_*), else the detector's or the
 * fixed modes of opts.  x are the Float32 MDCT coefficients quantizationStage receives (encoder.js:365; the exact kernels',
 * whatever the speculation mode).  BFU b has SPECS_PER_BFU[b] coefficients x_b[j] at BFU_START_LONG[b] + j, or at
 * BFU_START_SHORT[b] + j when b's band is coded short; sfi[b] = findScaleFactor(x_b), the side record's value; W_b is 1 for a
 * band coded long, 1/4 for the low or mid band coded short and 1/2 for the high band coded short (as for
 * c1_encode_best_modes_*); bits(w) = WORD_LENGTH_BITS[w], w = 0 .. 15.
 *   Error table, in binary64 with no fused operation:
 *     e(b,w) = W_b * sum_j (x_b[j] - d_j)^2, j ascending,  d_j = Float32((q_j * SCALE_FACTORS[sfi[b]]) / range),
 *     q_j from quantize at bits(w); d_j = 0 when w = 0 or sfi[b] = 0.
 *   Greedy for an amount n of BFU_AMOUNTS = 20, 28, .., 52:  budget = 1696 - 40 - 10 n, all wl[b] = 0, used = 0.  A BFU b < n
 *     is eligible when sfi[b] != 0, wl[b] < 15 and cost_b = (bits(wl[b] + 1) - bits(wl[b])) * size_b <= budget - used; its gain
 *     is g_b = (e(b,wl[b]) - e(b,wl[b] + 1)) / cost_b.  Take the eligible b with the largest g_b > 0, the smallest b on a tie,
 *     raise wl[b] by one level and add cost_b to used; stop when no eligible BFU has a positive gain (at most 52 * 15 steps,
 *     whatever the data).  T(n) = sum_{b<n} e(b,wl[b]) + sum_{b>=n} e(b,0), summed in BFU order.  n* is the first amount with
 *     the least T; a NaN never wins.
 *   Fallback to the reference:  (n_R, wl_R) is the reference's record for u under opts (the allocation chain of
 *     c1_encode_device, run once) and T_ref the same sum over it; if that record is allocateBits' own fallback (:132-139: every
 *     scale-factor index written as 0) T_ref = sum_b e(b,0).  taken[u] = 1 if T(n*) < T_ref, else 0 (also when every T is NaN).
 *     The unit is packed from the greedy record when taken, else from the reference's, untouched: T_final <= T_ref for every
 *     unit by construction, and where taken[u] = 0 the bytes are exactly those of c1_encode_modes_* or c1_encode_device.
 * Outputs: distortion[2u] = T_ref, distortion[2u + 1] = T(n*); energy[u] = sum_b W_b sum_j x_b[j]^2 (= sum_b e(b,0) in BFU
 * order); with all-long modes it is c1_encode_best_bias_*'s E within rounding, under a constant byte c1_encode_best_modes_*'s.
 * Each output may be NULL (units NULL: measure only, no packing runs and no record is replaced); all four NULL is C1_ERR_ARG.
 * The same inputs give the same bits run after run.  The call always takes the exact analysis; no output depends on the
 * speculation mode, the run length, C1_CHUNK_FRAMES, C1_PIPELINE, C1_OVERLAP or the halo.  Mode bytes, limits on frames,
 * alignment, chunking, asynchrony and the caller's-stream contract are those of c1_encode_best_bias_device.  No workspace on
 * top of an encode call's.  c1_ctx_kernel_ms counts the new kernel under "measure".
 * Not done: steps of several levels at once (on the CPU model another 0.3 dB at several times the steps), changing scale
 * factors or block modes by this error, perceptual weights. */
int c1_encode_measured_device(c1_ctx *ctx, const float *const *pcm, int channels, int64_t frames, int halo_frames,
                              const c1_encode_options *opts, const uint8_t *modes /* device, frames*channels, or NULL */,
                              uint8_t *units /* device, frames*channels*212, or NULL: measure only */,
                              uint8_t *taken /* device, frames*channels, or NULL */,
                              double *distortion /* device, frames*channels*2: T_ref, T(n*), or NULL */,
                              double *energy /* device, frames*channels, or NULL */);
/* host-resident, synchronous: every pointer HOST.  The options, the outputs and every mode byte are validated before the
 * context is looked at or any device work is done (C1_ERR_ARG, nothing written); without a context and without a device the
 * call then returns C1_ERR_NO_DEVICE.  One copy in, the device call, one copy out per output.  frames 0 .. 2^22 per channel. */
int c1_encode_measured_batch(c1_ctx *ctx, const float *const *pcm, int channels, int64_t frames, int halo_frames,
                             const c1_encode_options *opts, const uint8_t *modes /* host, or NULL */,
                             uint8_t *units /* host, or NULL */, uint8_t *taken /* host, or NULL */,
                             double *distortion /* host, or NULL */, double *energy /* host, or NULL */);

/* ---- the measured allocation with every BFU's scale-factor index chosen by the same error ------------------------------------
 * c1_encode_measured_* keeps every BFU at findScaleFactor's index, the smallest table entry not below the BFU's peak.  quantize
 * clamps to +-range (quantization.js:49-53), so an index a few steps lower clips the few peaks and gives every other coefficient
 * a finer grid; at the short word lengths where most BFUs end up that codes with less error.  This call lets the error decide.
 * OPT-IN like its sibling; the units are ordinary sound units (decode() reads any index 1 .. 63).  Notation as above.
 *   Candidates.  sf_offsets (HOST memory in both calls) holds n_offsets values, 1 <= n_offsets <= C1_MAX_SF_OFFSETS, distinct,
 *     each in -8 .. 8, sf_offsets[0] == 0; otherwise C1_ERR_ARG with the outputs untouched.  For BFU b with s0 =
 *     findScaleFactor(x_b) != 0 candidate k is valid when 1 <= s0 + sf_offsets[k] <= 63.  A BFU with s0 = 0 codes nothing.
 *   Error table.  e_k(b,w) is e(b,w) above with sfi = s0 + sf_offsets[k] in both quantize and the dequantizer (binary64, no
 *     fused operation, j ascending).  e(b,w) = min over the valid k of e_k(b,w); pick(b,w) is the first k, in the order given,
 *     that attains it (a later candidate wins only when its error is strictly smaller).  e(b,0) is unchanged.
 *   Greedy allocation: gains, greedy, totals, the first amount of least T and the NaN rule are those above, over this table.
 *   Fallback.  T_ref is the one above: the sum of e_0 (offset 0, the reference's own indices) over the reference's record.
 *     taken[u] = T(n*) < T_ref; a unit not taken is byte for byte the plain encode's.  No second greedy over the offset-0 table
 *     is run, so T(n*) may now and then exceed c1_encode_measured_*'s (3 of 648 units of the test material).
 *   Packed record of a taken unit.  nBfu and the word lengths are the greedy's; the scale-factor index written for b < nBfu is
 *     s0 + sf_offsets[pick(b, wl[b])] where wl[b] > 0, else s0; the mantissas are quantize at that index and word length.
 * Outputs: shifts[52 u + b] = the offset written for b < nBfu with wl[b] > 0 in a taken unit, 0 everywhere else (also in a
 * measure-only call, where it is what a packing call would write); distortion[2u] = T_ref, distortion[2u + 1] = T(n*); units,
 * taken and energy as above.  Each may be NULL; all five NULL is C1_ERR_ARG.  With units NULL no record of the context is touched.
 * Everything else -- modes, limits, chunking, asynchrony, invariance under the speculation mode, the run length,
 * C1_CHUNK_FRAMES, C1_PIPELINE, C1_OVERLAP and the halo, repeatability, "measure" in c1_ctx_kernel_ms, no workspace on top of an
 * encode call's -- is c1_encode_measured_*'s.  With sf_offsets = {0} every output is bit for bit c1_encode_measured_*'s and
 * shifts is all zero.  The suggested set is {0, -1, 1, -2, -3}: 1.7 to 2.4 dB less error energy than c1_encode_measured_* on
 * the test material; offsets below -3 add 0.03 dB at most. */
#define C1_MAX_SF_OFFSETS 8
int c1_encode_measured_sf_device(c1_ctx *ctx, const float *const *pcm, int channels, int64_t frames, int halo_frames,
                                 const c1_encode_options *opts, const uint8_t *modes /* device, frames*channels, or NULL */,
                                 const int8_t *sf_offsets /* HOST, n_offsets values */, int n_offsets,
                                 uint8_t *units /* device, frames*channels*212, or NULL: measure only */,
                                 uint8_t *taken /* device, frames*channels, or NULL */,
                                 int8_t *shifts /* device, frames*channels*52, or NULL */,
                                 double *distortion /* device, frames*channels*2: T_ref, T(n*), or NULL */,
                                 double *energy /* device, frames*channels, or NULL */);
/* host-resident, synchronous: every pointer HOST.  The options, the offsets, the outputs and every mode byte are validated
 * before the context is looked at or any device work is done (C1_ERR_ARG, nothing written); without a context and without a
 * device the call then returns C1_ERR_NO_DEVICE.  frames 0 .. 2^22 per channel. */
int c1_encode_measured_sf_batch(c1_ctx *ctx, const float *const *pcm, int channels, int64_t frames, int halo_frames,
                                const c1_encode_options *opts, const uint8_t *modes /* host, or NULL */,
                                const int8_t *sf_offsets /* host, n_offsets values */, int n_offsets,
                                uint8_t *units /* host, or NULL */, uint8_t *taken /* host, or NULL */,
                                int8_t *shifts /* host, or NULL */, double *distortion /* host, or NULL */,
                                double *energy /* host, or NULL */);

/* ---- the block modes of every sound unit chosen from candidates by the error of the measured allocation ---------------------
 * c1_encode_best_modes_* ranks its candidates by the error of the reference's allocation under them, and c1_encode_measured_*
 * and c1_encode_measured_sf_* take the block modes as given.  The first ranking is a poor guide to the second: on the test
 * material the candidate of least measured error is not c1_encode_best_modes_*'s in three units of four.  This call joins the
 * two loops.  OPT-IN like c1_encode_measured_*; the units are ordinary sound units.
 *   Arguments.  cand_modes and n_cand are c1_encode_best_modes_*'s exactly (HOST memory, 1 .. C1_MAX_MODE_CANDIDATES distinct
 *     bytes of the domain, checked by both calls, C1_ERR_ARG naming the entry); sf_offsets and n_offsets are
 *     c1_encode_measured_sf_*'s exactly, and {0} gives the plain measured allocation of c1_encode_measured_*.  Of opts only what
 *     c1_encode_measured_* reads under given modes is read.
 *   Definition, by composition.  For unit u and candidate k take what c1_encode_measured_sf_* reports for u under the constant
 *     modes cand_modes[k], the same opts and offsets: T_ref(u,k), T*(u,k) = T(n*), taken(u,k) = T*(u,k) < T_ref(u,k),
 *     energy(u,k), and the record that call would pack.  T_final(u,k) = taken(u,k) ? T*(u,k) : T_ref(u,k).  choice[u] is the
 *     smallest k with T_final(u,k) <= T_final(u,j) for all j, on the values computed: a NaN never wins, and if every T_final is
 *     NaN the choice is 0.  The T of different candidates are comparable because W_b makes each the PCM error energy up to one
 *     constant (c1_encode_best_modes_* above), and a candidate's figures do not depend on the modes of the frames before it.
 *   Outputs.  units[u]: byte for byte what c1_encode_measured_sf_* writes with modes[u] = modes_out[u]; modes_out[u] =
 *     cand_modes[choice[u]]; taken[u] and shifts[52 u + b]: the winner's, as that call defines them; distortion[(u * n_cand + k)
 *     * 2 + 0] = T_ref(u,k), [.. + 1] = T*(u,k); energy[u * n_cand + k] = energy(u,k).  All of them are bit for bit the
 *     per-candidate calls' values: the orders of summation are theirs (slot order within a BFU, BFU order for the totals,
 *     binary64, no fused operation).  Each may be NULL (units NULL: measure only, no packing runs and no record of the context is
 *     touched); all seven NULL is C1_ERR_ARG.  With one candidate the call is c1_encode_measured_sf_* under a constant byte.
 * Limits, alignment, chunking, asynchrony, the caller's-stream contract, repeatability, and invariance under the speculation
 * mode, the run length, C1_CHUNK_FRAMES, C1_PIPELINE, C1_OVERLAP and the halo are c1_encode_best_modes_device's, and so are the
 * front end (the exact analysis at most twice, one trial allocation per candidate) and the workspace.  One kernel then runs the
 * measured allocation under every candidate.  c1_ctx_kernel_ms counts it under "measure", one launch per launch of the chain,
 * the analyses and the composing under "analysis" and the trial allocations under "allocate".
 * Which kernel measures: a launch of at most 8 192 sound units -- of this call or of c1_enc_stream_push_measured_modes -- takes a
 * kernel that spends a workgroup of eight waves on every unit, builds the error table twice (from the all-long and from the
 * all-short analysis) instead of once per candidate and runs the 8 x n_cand greedy chains beside each other; larger launches a
 * wave per unit.  The outputs are the same bits.  C1_MEASURED_WIDE, read when a context is created, overrides this as it does
 * for c1_encode_measured_*: 0 never the workgroup kernel, 1 always.
 * Cost: n_cand greedy passes per unit, about 270 ms each on 2^21 units with five offsets.  This is the library's dearest encode
 * by far.  On 2^21 units it costs 0.67 (two candidates) to 0.88 (eight) of the loop it replaces -- n measure-only calls, the
 * minimum on the host, one final call.  Small launches: at 256 units, eight candidates and five offsets the search takes 0.30 ms
 * in the workgroup kernel against 2.98 ms a wave per unit, and the whole call 1.54 ms against 2.72 ms for that loop (DESIGN.md
 * 6q).
 * Not done: masking weights in this search (each candidate's thresholds come from another spectrum, and nothing has shown
 * their ratios comparable across modes), pruning of candidates.  The streaming form is c1_enc_stream_push_measured_modes.
 * c1_encode_measured_modes_masked_* (below) weighs every candidate with one threshold per unit, from the all-long spectrum. */
int c1_encode_measured_modes_device(c1_ctx *ctx, const float *const *pcm, int channels, int64_t frames, int halo_frames,
                                    const c1_encode_options *opts, const uint8_t *cand_modes /* HOST, n_cand bytes */, int n_cand,
                                    const int8_t *sf_offsets /* HOST, n_offsets values */, int n_offsets,
                                    uint8_t *units /* device, frames*channels*212, or NULL: measure only */,
                                    uint8_t *choice /* device, frames*channels, or NULL */,
                                    uint8_t *modes_out /* device, frames*channels, or NULL: cand_modes[choice[u]] */,
                                    uint8_t *taken /* device, frames*channels, or NULL */,
                                    int8_t *shifts /* device, frames*channels*52, or NULL */,
                                    double *distortion /* device, frames*channels*n_cand*2 (unit-major): T_ref, T(n*), or NULL */,
                                    double *energy /* device, frames*channels*n_cand (unit-major), or NULL */);
/* host-resident, synchronous: every pointer HOST.  The options, the candidates, the offsets and the outputs are validated
 * before the context is looked at or any device work is done (C1_ERR_ARG, nothing written); without a context and without a
 * device the call then returns C1_ERR_NO_DEVICE.  One copy in, the device call, one copy out per output.  frames 0 .. 2^22 per
 * channel. */
int c1_encode_measured_modes_batch(c1_ctx *ctx, const float *const *pcm, int channels, int64_t frames, int halo_frames,
                                   const c1_encode_options *opts, const uint8_t *cand_modes /* host */, int n_cand,
                                   const int8_t *sf_offsets /* host */, int n_offsets,
                                   uint8_t *units /* host, or NULL */, uint8_t *choice /* host, or NULL */,
                                   uint8_t *modes_out /* host, or NULL */, uint8_t *taken /* host, or NULL */,
                                   int8_t *shifts /* host, or NULL */, double *distortion /* host, or NULL */,
                                   double *energy /* host, or NULL */);

/* ---- the measured allocation with every BFU's error weighted by a masking threshold ------------------------------------------
 * c1_encode_measured_sf_* minimises the plain squared error of the coefficients, so its greedy spends bits where the signal is
 * loud.  This call divides every BFU's error by a threshold computed per sound unit from the unit's own spectrum and two tables
 * of the caller's, and minimises that noise-to-mask ratio instead.  OPT-IN like its siblings; the units are ordinary sound
 * units.  The figures are noise-to-mask under this model; nobody has listened to the result.  Notation as above.
 *   Tables (HOST memory in both calls).  mask_floor: 52 values, each finite and within [1e-60, 1e60].  mask_spread: 52 * 52
 *     values, row-major, mask_spread[52 b + c] = masker c onto maskee b, each finite and within [0, 1e60]; or NULL = all zero.
 *     Anything else is C1_ERR_ARG naming the table and the index, with every output untouched.
 *   Weights, per unit, in binary64 with no fused operation:
 *     E_c   = e(c,0), c = 0 .. 51 (W_c * sum_j x_c[j]^2, j ascending)
 *     M_b   = sum_c mask_spread[52 b + c] * E_c, c ascending, each product rounded and then added to a sum that starts at +0.0;
 *             +0.0 with mask_spread NULL
 *     thr_b = M_b > mask_floor[b] ? M_b : mask_floor[b]   (a NaN M_b falls to the floor)
 *     P_b   = 1.0 / thr_b
 *   Error table.  e'_k(b,w) = P_b * e_k(b,w), level 0 included; the multiply is applied to the finished e_k(b,w), after the W_b
 *     multiply.  The minimum over the candidates and pick (first candidate, strictly smaller wins), the gains, the greedy, the
 *     totals, the first amount of least T and the NaN rule are c1_encode_measured_sf_*'s, run on e'.
 *   Fallback.  T_ref = sum_b e'_0(b, wl_ref[b]); taken[u] = T(n*) < T_ref.
 *   Records, shifts, the packing of a taken unit and the bytes of a unit not taken (the plain encode's) are
 *     c1_encode_measured_sf_*'s: the bytes do not reveal the weights.
 * Outputs: distortion holds the weighted T_ref and T(n*); energy = sum_b e'(b,0) in BFU order; weights[52 u + b] = P_b for all
 * 52 BFUs, taken or not, also in a measure-only call; units, taken and shifts as above.  Each may be NULL; all six NULL is
 * C1_ERR_ARG.
 * Consequences.  With mask_floor all 1.0 and mask_spread NULL or all zero, P_b is exactly 1.0 and units, taken, shifts,
 * distortion and energy are bit for bit c1_encode_measured_sf_*'s.  Scaling both tables by 4.0 leaves units, taken and shifts
 * unchanged and multiplies distortion, energy and weights by exactly 0.25.  Everything else -- the offsets' rules, modes,
 * limits, chunking, asynchrony, invariance under the speculation mode, the run length, C1_CHUNK_FRAMES, C1_PIPELINE, C1_OVERLAP
 * and the halo, repeatability, "measure" in c1_ctx_kernel_ms -- is c1_encode_measured_sf_*'s.  The tables are copied into a
 * buffer of the context (22 048 bytes) on the context's stream by every call, behind the work of every earlier call: the
 * caller's arrays are free when the call returns, and no other call reads the buffer. */
int c1_encode_measured_masked_device(c1_ctx *ctx, const float *const *pcm, int channels, int64_t frames, int halo_frames,
                                     const c1_encode_options *opts, const uint8_t *modes /* device, frames*channels, or NULL */,
                                     const int8_t *sf_offsets /* HOST, n_offsets values */, int n_offsets,
                                     const double *mask_floor /* HOST, 52 */, const double *mask_spread /* HOST, 52*52, or NULL */,
                                     uint8_t *units /* device, frames*channels*212, or NULL: measure only */,
                                     uint8_t *taken /* device, frames*channels, or NULL */,
                                     int8_t *shifts /* device, frames*channels*52, or NULL */,
                                     double *distortion /* device, frames*channels*2: weighted T_ref, T(n*), or NULL */,
                                     double *energy /* device, frames*channels, or NULL */,
                                     double *weights /* device, frames*channels*52: P_b, or NULL */);
/* host-resident, synchronous: every pointer HOST.  The options, the offsets, the tables, the outputs and every mode byte are
 * validated before the context is looked at or any device work is done (C1_ERR_ARG, nothing written); without a context and
 * without a device the call then returns C1_ERR_NO_DEVICE.  frames 0 .. 2^22 per channel. */
int c1_encode_measured_masked_batch(c1_ctx *ctx, const float *const *pcm, int channels, int64_t frames, int halo_frames,
                                    const c1_encode_options *opts, const uint8_t *modes /* host, or NULL */,
                                    const int8_t *sf_offsets /* host, n_offsets values */, int n_offsets,
                                    const double *mask_floor /* host, 52 */, const double *mask_spread /* host, 52*52, or NULL */,
                                    uint8_t *units /* host, or NULL */, uint8_t *taken /* host, or NULL */,
                                    int8_t *shifts /* host, or NULL */, double *distortion /* host, or NULL */,
                                    double *energy /* host, or NULL */, double *weights /* host, or NULL */);

/* ---- the measured block-mode search under one masking threshold per unit ------------------------------------------------------
 * c1_encode_measured_masked_* spends a unit's bits by noise-to-mask under the block modes it is given; c1_encode_measured_modes_*
 * chooses the block modes by an unweighted error.  A unit's own-mode thresholds move with the modes (by up to 19.7 dB in one BFU
 * between byte 58 and byte 0 on the test material), so per-candidate thresholds are not comparable.  A masking threshold is a
 * property of the signal, not of the transform chosen to code it: this call computes it once per unit, from the all-long
 * spectrum, and weighs every candidate's error with it.  OPT-IN like every measured call; the figures are noise-to-mask under the
 * model of c1_encode_measured_masked_*, and nobody has listened to the result.
 * New entry points:
 *   c1_encode_measured_modes_masked_device / _batch.  They take c1_encode_measured_modes_*'s arguments, then mask_floor,
 *     mask_spread | NULL, and one more optional output, weights (double[units * 52]).
 *   c1_enc_stream_push_measured_modes_masked, the same extension of c1_enc_stream_push_measured_modes.
 * Tables are validated and uploaded exactly as in c1_encode_measured_masked_*.  They go through check_masking and
 * upload_masking, with the same messages and the same stream-order contract.  mask_floor is required.
 * Weights.  P_b(u) is, bit for bit, the weights row that c1_encode_measured_masked_* reports for unit u under constant modes 0
 * and these tables.  In detail:
 *   E_c = sum_j x_c[j]^2 over the all-long coefficients, j ascending, W = 1.
 *   M_b = sum_c spread[52 b + c] * E_c, c ascending, each product rounded and then added to a sum that starts at +0.0.
 *   thr_b = M_b > floor[b] ? M_b : floor[b].
 *   P_b = 1.0 / thr_b.
 * P_b(u) does not depend on the candidates or on the offsets.
 * Per candidate k.
 *   e'_k(b, w) = P_b * e_k(b, w), where e_k is the error table c1_encode_measured_sf_* builds for u under the constant byte
 *     cand_modes[k].
 *   e_k includes its W_b for short bands.
 *   The multiply is applied to the finished entry, before the strictly-smaller compare over the offsets, as in
 *     c1_encode_measured_masked_*.
 * From there everything is c1_encode_measured_modes_*'s on e':
 *   T_ref(u,k) = sum_b e'_0(b, wl_ref_k[b]) from trial record k.
 *   Gains, greedy, totals, the first amount of least T, the NaN rule, taken(u,k) = T* < T_ref, T_final.
 *   choice[u] is the smallest k of least T_final.  A NaN never wins; all NaN gives 0.
 *   modes_out, and the winner's record, taken, shifts and packing.
 * Outputs.
 *   distortion and energy have c1_encode_measured_modes_*'s shapes and hold the weighted values.
 *   weights holds P_b for all 52 BFUs of every unit.
 *   The units are ordinary sound units.  The bytes do not reveal the weights.
 *   All outputs NULL is C1_ERR_ARG.  units NULL is measure-only, as in c1_encode_measured_modes_*.
 * Stream.
 *   After the push the stream is bit for bit what it is after c1_enc_stream_push_modes(modes_out).
 *   Rows of a stream pushed from its start are the whole-buffer call's.
 *   A rejected call leaves the stream and every output as they were.
 *   What the arguments alone decide is decided before the stream or the context is looked at.
 * Consequences.  With mask_floor all 1.0 and mask_spread NULL or all zero, weights is exactly 1.0 and the other seven outputs are
 * bit for bit c1_encode_measured_modes_*'s.  With cand_modes = {0}, units, taken, shifts, distortion, energy and weights are bit
 * for bit c1_encode_measured_masked_*'s under constant modes 0, and in any candidate set that holds byte 0 that column of
 * distortion and energy is.  weights is the same bits under every candidate set and every offset set: with tables given the
 * front end always makes the all-long analysis, also for sets that never code long.  Scaling both tables by 4.0 leaves units,
 * choice, modes_out, taken and shifts unchanged and multiplies distortion, energy and weights by exactly 0.25.  Limits,
 * chunking, asynchrony, the choice between the wave-per-unit and the workgroup-per-unit kernel (C1_MEASURED_WIDE), invariance
 * under the speculation mode, the run length, C1_CHUNK_FRAMES, C1_PIPELINE, C1_OVERLAP and the halo, repeatability and "measure"
 * in c1_ctx_kernel_ms are c1_encode_measured_modes_*'s.
 * Not done: a c1_encode_signals_* form, meters under shared weights, tonality, temporal masking, anything stereo-aware. */
int c1_encode_measured_modes_masked_device(c1_ctx *ctx, const float *const *pcm, int channels, int64_t frames, int halo_frames,
                                           const c1_encode_options *opts, const uint8_t *cand_modes /* HOST, n_cand bytes */, int n_cand,
                                           const int8_t *sf_offsets /* HOST, n_offsets values */, int n_offsets,
                                           const double *mask_floor /* HOST, 52 */, const double *mask_spread /* HOST, 52*52, or NULL */,
                                           uint8_t *units /* device, frames*channels*212, or NULL: measure only */,
                                           uint8_t *choice /* device, frames*channels, or NULL */,
                                           uint8_t *modes_out /* device, frames*channels, or NULL: cand_modes[choice[u]] */,
                                           uint8_t *taken /* device, frames*channels, or NULL */,
                                           int8_t *shifts /* device, frames*channels*52, or NULL */,
                                           double *distortion /* device, frames*channels*n_cand*2: weighted T_ref, T(n*), or NULL */,
                                           double *energy /* device, frames*channels*n_cand (unit-major), or NULL */,
                                           double *weights /* device, frames*channels*52: P_b, or NULL */);
/* host-resident, synchronous: every pointer HOST.  The options, the candidates, the offsets, the tables and the outputs are
 * validated before the context is looked at or any device work is done (C1_ERR_ARG, nothing written); without a context and
 * without a device the call then returns C1_ERR_NO_DEVICE.  frames 0 .. 2^22 per channel. */
int c1_encode_measured_modes_masked_batch(c1_ctx *ctx, const float *const *pcm, int channels, int64_t frames, int halo_frames,
                                          const c1_encode_options *opts, const uint8_t *cand_modes /* host */, int n_cand,
                                          const int8_t *sf_offsets /* host */, int n_offsets,
                                          const double *mask_floor /* host, 52 */, const double *mask_spread /* host, 52*52, or NULL */,
                                          uint8_t *units /* host, or NULL */, uint8_t *choice /* host, or NULL */,
                                          uint8_t *modes_out /* host, or NULL */, uint8_t *taken /* host, or NULL */,
                                          int8_t *shifts /* host, or NULL */, double *distortion /* host, or NULL */,
                                          double *energy /* host, or NULL */, double *weights /* host, or NULL */);

/* ---- the coding error of given sound units against their PCM -----------------------------------------------------------------
 * The calls above report the measured error of the units they are about to pack.  This call takes sound units that already
 * exist -- the reference's at any bias, the output of any entry point above, a file another encoder wrote, a stream after a bit
 * error -- and scores them with the same yardstick, from the bytes.  It encodes nothing and changes no state.
 * channels 1 or 2, unit index = frame * channels + channel; pcm and the halo as for c1_encode_modes_*.  For unit u:
 *   Fields.  deserializeFrame (serialization.js:111-176) of units[u], exactly as c1_unpack_units reports them: nBfu from
 *     BFU_AMOUNTS, wl 0 .. 15, sfi 0 .. 63, sign-extended mantissas, bits past the unit's end as that call reads them.
 *   Mode byte.  low | mid << 2 | high << 4 of the unit's block_modes.  The host call rejects a unit whose byte is outside the
 *     domain of c1_encode_modes_* (a block mode the encoder never writes): C1_ERR_ARG naming frame, channel (of two) and field,
 *     nothing written.  The device call brings the byte into the domain as the other device entry points do (low and mid: the
 *     byte & 2 and & 8; high 3 when bits 4-5 are both set, else 0).
 *   Coefficients.  x are the Float32 MDCT coefficients quantizationStage receives (encoder.js:365) for that frame under the
 *     unit's own block modes: the exact kernels', whatever the speculation mode.  They do not depend on the modes of the frames
 *     before (see c1_encode_best_modes_*), so halo frames need no units.
 *   Dequantized values.  d is what dequantizationStage (decoder.js:52-98) makes of the fields, c1_dequantize_frames' arithmetic:
 *     Float32((q * SCALE_FACTORS[sfi]) / range); +0 where b >= nBfu, wl = 0 or sfi = 0.
 *   Sums, in binary64 with no fused operation, for all 52 BFUs, with W_b and the BFU geometry of c1_encode_measured_*:
 *     noise[52u + b]  = W_b * sum_j (x_b[j] - d_b[j])^2        signal[52u + b] = W_b * sum_j x_b[j]^2        j ascending
 *     P_b = c1_encode_measured_masked_*'s weight with E_c = signal[52u + c] when mask_floor is given (mask_spread optional), else
 *     exactly 1.0;  weights[52u + b] = P_b
 *     totals[2u] = sum_b P_b * noise[52u + b]     totals[2u + 1] = sum_b P_b * signal[52u + b]     b ascending, each product
 *     rounded before it is added.
 * For the units c1_encode_measured_*, _sf_ and _masked_ write, totals[2u] is their distortion[2u + taken[u]], totals[2u + 1]
 * their energy[u] and weights their weights, bit for bit, under the same tables; for the units of a plain encode totals[2u] is
 * distortion[2u] of a measure-only call.
 * mask_floor, mask_spread: HOST memory in both calls, validated as for c1_encode_measured_masked_* (same messages) and copied
 * into the same buffer of the context under the same stream-order contract.  Every output may be NULL; all four NULL is
 * C1_ERR_ARG, as are weights or mask_spread without mask_floor and a NULL units or pcm with frames to process.  A rejected call
 * writes nothing.  No output depends on the speculation mode, the run length, C1_CHUNK_FRAMES, C1_PIPELINE, C1_OVERLAP, the halo
 * (given the same real history) or on which outputs are asked for, and the same inputs give the same bits.  Non-finite PCM gives
 * non-finite outputs.  No byte pattern of a unit makes any access leave the buffers: every index read from a unit is a masked
 * bit field.
 * device-resident: pcm[c] (16-byte aligned), units (4-byte aligned) and the outputs are DEVICE pointers; limits on frames,
 * chunking, asynchrony and the caller's-stream contract are c1_encode_measured_device's.  Per chunk the units' mode bytes are
 * formed into workspace, the exact analysis under given modes runs as far as the coefficients (no allocation, no packing), then
 * one kernel reads bytes and coefficients back.  c1_ctx_kernel_ms counts that kernel under "meter" and the analysis under
 * "analysis". */
int c1_measure_units_device(c1_ctx *ctx, const float *const *pcm, int channels, int64_t frames, int halo_frames,
                            const uint8_t *units /* device, frames*channels*212 */,
                            const double *mask_floor /* HOST, 52, or NULL: P_b = 1 */, const double *mask_spread /* HOST, 52*52, or NULL */,
                            double *noise /* device, frames*channels*52, or NULL */, double *signal /* device, frames*channels*52, or NULL */,
                            double *totals /* device, frames*channels*2, or NULL */, double *weights /* device, frames*channels*52, or NULL */);
/* host-resident, synchronous: every pointer HOST.  The tables, the outputs and every unit's mode byte are validated before the
 * context is looked at or any device work is done (C1_ERR_ARG, nothing written); without a context and without a device the
 * call then returns C1_ERR_NO_DEVICE.  One copy in, the device call, one copy out per output.  frames 0 .. 2^22 per channel. */
int c1_measure_units_batch(c1_ctx *ctx, const float *const *pcm, int channels, int64_t frames, int halo_frames,
                           const uint8_t *units /* host */, const double *mask_floor /* host, or NULL */,
                           const double *mask_spread /* host, or NULL */, double *noise /* host, or NULL */,
                           double *signal /* host, or NULL */, double *totals /* host, or NULL */, double *weights /* host, or NULL */);

/* ---- the coding error of given sound units under the all-long threshold --------------------------------------------------------
 * c1_measure_units_* forms P_b from the unit's own-mode spectrum, so units coded in different block modes are scored against
 * different thresholds.  c1_encode_measured_modes_masked_* judges every candidate of a unit under one threshold, that of the
 * frame's all-long spectrum; this call scores given units on that scale, from the bytes.  It encodes nothing and changes no state.
 * Arguments, geometry, fields, mode byte (the host call rejects a byte outside the domain, the device call brings it in),
 * coefficients and dequantized values are c1_measure_units_*'s.  For unit u:
 *   noise[52u + b] and signal[52u + b] are exactly c1_measure_units_*'s: the coefficients under the unit's own mode byte, W_b,
 *     j ascending, binary64, nothing fused.
 *   weights[52u + b] = P_b is c1_encode_measured_modes_masked_*'s weight:
 *     x0 are the Float32 MDCT coefficients of the frame under mode byte 0 (all long), the exact kernels';
 *     E_c = sum_j x0_c[j]^2, j ascending, W = 1;
 *     M_b = sum_c mask_spread[52 b + c] * E_c, c ascending, each product rounded, then added to a sum that starts at +0.0; a NULL
 *       mask_spread skips the sum (M_b = +0.0);
 *     thr_b = M_b > mask_floor[b] ? M_b : mask_floor[b]  (a NaN M_b falls to the floor);   P_b = 1.0 / thr_b.
 *     P_b does not depend on the unit's bytes at all.
 *   totals[2u] = sum_b P_b * noise[52u + b]     totals[2u + 1] = sum_b P_b * signal[52u + b]     b ascending, each product
 *     rounded before it is added.
 * For the units c1_encode_measured_modes_masked_* writes, under the same PCM, tables, candidates and offsets, totals[2u] is its
 * distortion[(u * n_cand + choice[u]) * 2 + taken[u]], totals[2u + 1] its energy[u * n_cand + choice[u]] and weights its
 * weights, bit for bit.  For units whose mode byte is 0 every output equals c1_measure_units_*'s under the same tables.
 * mask_floor is required: NULL is C1_ERR_ARG.  mask_floor, mask_spread: HOST memory in both calls, validated as for
 * c1_encode_measured_masked_* (same messages) and copied into the same buffer of the context under the same stream-order
 * contract.  Every output may be NULL; all four NULL is C1_ERR_ARG, as are mask_spread without mask_floor and a NULL units or pcm
 * with frames to process.  In both calls everything the arguments alone decide is decided before the context or a device is looked
 * at, and a rejected call writes nothing.  No output depends on the speculation mode, the run length, C1_CHUNK_FRAMES,
 * C1_PIPELINE, C1_OVERLAP, the halo (given the same real history) or on which outputs are asked for, and the same inputs give the
 * same bits.  Non-finite PCM gives non-finite outputs.  No byte pattern of a unit makes any access leave the buffers.
 * device-resident: pcm[c] (16-byte aligned), units (4-byte aligned) and the outputs are DEVICE pointers; limits on frames,
 * chunking, asynchrony and the caller's-stream contract are c1_measure_units_device's.  Per chunk the exact analysis runs twice
 * from one set of band samples, under the units' modes and all long (the second plane is the mode search's workspace), then one
 * kernel reads bytes and both planes back.  c1_ctx_kernel_ms counts that kernel under "meter" and the analysis under
 * "analysis". */
int c1_measure_units_shared_device(c1_ctx *ctx, const float *const *pcm, int channels, int64_t frames, int halo_frames,
                                   const uint8_t *units /* device, frames*channels*212 */,
                                   const double *mask_floor /* HOST, 52 */, const double *mask_spread /* HOST, 52*52, or NULL */,
                                   double *noise /* device, frames*channels*52, or NULL */, double *signal /* device, frames*channels*52, or NULL */,
                                   double *totals /* device, frames*channels*2, or NULL */, double *weights /* device, frames*channels*52, or NULL */);
/* host-resident, synchronous: every pointer HOST.  The tables, the outputs and every unit's mode byte are validated before the
 * context is looked at or any device work is done (C1_ERR_ARG, nothing written); without a context and without a device the
 * call then returns C1_ERR_NO_DEVICE.  One copy in, the device call, one copy out per output.  frames 0 .. 2^22 per channel. */
int c1_measure_units_shared_batch(c1_ctx *ctx, const float *const *pcm, int channels, int64_t frames, int halo_frames,
                                  const uint8_t *units /* host */, const double *mask_floor /* host */,
                                  const double *mask_spread /* host, or NULL */, double *noise /* host, or NULL */,
                                  double *signal /* host, or NULL */, double *totals /* host, or NULL */, double *weights /* host, or NULL */);

/* ---- the error of the decoded PCM of given sound units against their PCM, per 32 samples ---------------------------------------
 * c1_measure_units_* compares coefficients; this call compares what a listener gets: it decodes the units exactly as
 * c1_decode_device does and reports how far the decoded PCM is from the PCM that went in, per unit and per 32-sample segment, in
 * one launch.  No decoded PCM is written anywhere; it encodes nothing and changes no state.
 *   Geometry.  channels 1 or 2, unit index u = frame * channels + channel.
 *   PCM and its halo.  pcm[c] is planar Float32; halo_frames (0 .. 2) whole frames of real PCM sit in front of the pointers, as
 *     for c1_encode_modes_*; samples before that are zero.  Only the last 266 samples of history are ever read.
 *   Unit halo.  halo_units (0 or 1): the unit(s) of frame -1 precede `units`, as for c1_decode_device; otherwise the decoder
 *     starts from a fresh pool.
 *   Decoded PCM.  y[c][t], t = 0 .. 512 * frames - 1, is the Float32 PCM c1_decode_device writes for these units, channels,
 *     frames and halo_units under C1_DECODE_EXACT, bit for bit: the exact (binary64) decoder under every decode model of the
 *     context (c1_ctx_set_decode_model); the meter has no binary32 form.
 *   Delayed input.  x[c][t] = pcm[c][t - 266] (the codec delay); zero where t - 266 < -512 * halo_frames.
 *   Sums, in binary64 with no fused operation.  For unit u (frame f, channel c) and segment s = 0 .. 15, t = 512 f + 32 s + i,
 *     i ascending over 0 .. 31:   e = (double)y - (double)x
 *     noise[16u + s] = sum_i e * e          signal[16u + s] = sum_i x * x
 *     each square rounded before it is added, each sum starting from +0;
 *     totals[2u] = sum_s noise[16u + s]     totals[2u + 1] = sum_s signal[16u + s]     s ascending.
 *     Segment s of frame f covers the input samples 512 f + 32 s - 266 .. 512 f + 32 s - 266 + 31.
 * Any of noise, signal, totals may be NULL; all three NULL is C1_ERR_ARG, as are a NULL units or pcm with frames to process and
 * channels, frames, halo_frames or halo_units out of range.  These are decided before the context is looked at, and a rejected
 * call writes nothing.  frames == 0 is success with nothing written.
 * No output depends on the run length, chunking, the halos (given the same real history), the decode-precision setting or on
 * which outputs are asked for, and the same inputs give the same bits.  Non-finite PCM gives non-finite noise and signal in the
 * segments it falls in (and the unit's totals), and nowhere else.  No byte pattern of a unit makes any access leave the buffers
 * (c1_decode_device's property).  No PCM read lies before pcm[c] - 512 * halo_frames or at or after pcm[c] + 512 * frames - 266.
 * device-resident: pcm[c] (16-byte aligned), units (4-byte aligned) and the outputs are DEVICE pointers; asynchronous on the
 * context's stream under c1_decode_device's caller's-stream contract; frames 0 .. 2^22 per channel; no workspace and so no
 * chunking.  c1_ctx_kernel_ms counts the kernel under "meter_pcm". */
int c1_measure_pcm_device(c1_ctx *ctx, const float *const *pcm, int channels, int64_t frames, int halo_frames,
                          const uint8_t *units /* device, frames*channels*212 */, int halo_units,
                          double *noise /* device, frames*channels*16, or NULL */, double *signal /* device, frames*channels*16, or NULL */,
                          double *totals /* device, frames*channels*2, or NULL */);
/* host-resident, synchronous: every pointer HOST.  The arguments are validated before the context is looked at or any device
 * work is done (C1_ERR_ARG, nothing written); without a context and without a device the call then returns C1_ERR_NO_DEVICE.
 * One copy in, the device call, one copy out per output; batches longer than the context's chunk length (C1_CHUNK_FRAMES) go in
 * chunks, each with its halos taken from the batch itself, and the result equals the unchunked one bit for bit.  frames
 * 0 .. 2^22 per channel. */
int c1_measure_pcm_batch(c1_ctx *ctx, const float *const *pcm, int channels, int64_t frames, int halo_frames,
                         const uint8_t *units /* host */, int halo_units, double *noise /* host, or NULL */,
                         double *signal /* host, or NULL */, double *totals /* host, or NULL */);

/* The same batch sharded over several devices of this host (the hot loop of processor.js:119-136 has no
 * dependency between frames beyond a bounded PCM history): contiguous frame ranges, one per entry of `devices`, each
 * encoded by its own host thread on a context of that device from its 2 frames of real PCM history; no collective, the
 * ranges land in `units` by frame index.  A device may be listed more than once (each entry gets its own context).
 * Contexts come from a process-wide pool: created on first use, leased to one call at a time (concurrent calls get their
 * own), made anew after c1_set_tables().  Every shard streams its range in chunks as c1_encode_batch does.
 * Bit-identical to c1_encode_batch on a fresh context. */
int c1_encode_batch_multi(const int *devices, int n_devices, const float *const *pcm, int channels, int64_t frames,
                          int halo_frames, const c1_encode_options *opts, uint8_t *units);
/* decode twin: every range starts from the unit(s) of the frame before it.  It takes no context and has no decode model: the
 * exact decoder always (c1_ctx_set_decode_model) */
int c1_decode_batch_multi(const int *devices, int n_devices, const uint8_t *units, int channels, int64_t frames,
                          int halo_units, float *const *pcm);

/* Page-locked host memory for the *_batch calls.  c1_encode_batch / c1_decode_batch stream a batch of more than
 * 65 536 frames per channel in chunks: upload of chunk i+1, kernels of chunk i and download of chunk i-1 overlap on
 * three streams.  From buffers in memory from c1_host_alloc (or otherwise registered with HIP) the PCIe link then runs
 * at its pinned-memory rate (12.9 M stereo frames/s on one MI355X host); from pageable buffers the runtime stages the
 * copies and the same calls reach 91 % of that (11.7 M; whole-batch copy, compute, copy managed 8.1 M). */
int c1_host_alloc(size_t bytes, void **out);
int c1_host_free(void *p);

/* ---- decode: replaces the decode() frame closure body, decoder.js:408-411
 *      (dequantizationStage :52-98, imdctStage :116-330, qmfSynthesisStage :349-389)
 *      plus deserializeFrame (serialization.js:111-176), batched ----------------------------- */
int c1_decode_device(c1_ctx *ctx, const uint8_t *units, int channels, int64_t frames,
                     int halo_units, float *const *pcm);
int c1_decode_batch(c1_ctx *ctx, const uint8_t *units, int channels, int64_t frames,
                    int halo_units, float *const *pcm);

/* ---- stateful streams: what one encode()/decode() closure + its BufferPool is
 *      (encoder.js:438-441, buffers.js:7-81).  The stream keeps the PCM / unit history on the
 *      device, so successive calls continue the same stream bit for bit. ---------------------- */
typedef struct c1_enc_stream c1_enc_stream;
typedef struct c1_dec_stream c1_dec_stream;
int c1_enc_stream_create(c1_ctx *ctx, int channels, const c1_encode_options *opts, c1_enc_stream **out);
int c1_enc_stream_push(c1_enc_stream *s, const float *const *pcm /* host */, int64_t frames,
                       uint8_t *units /* host, frames*channels*212 */);
int c1_enc_stream_destroy(c1_enc_stream *s);
/* The options of every channel from the next push on, as the reference's encode() reads its EncoderOptions on every call
 * (encoder.js:131-140, :393): validated as c1_enc_stream_create validates them; an invalid call leaves the stream as it was.
 * The stream goes on bit for bit as the reference's closure does under the same option changes.  What it carries across a
 * change is the PCM history (QMF delays and the MDCT overlap are functions of it, whatever the block modes) and the detection
 * history, which only detection writes: under fixed modes it stays at the magnitudes of the last frame detection ran on, or at
 * a fresh pool's zeros when there was none.  So a switch from detection to fixed modes keeps the bands of the last pushed frame
 * on the device, and the first frame pushed after a switch back to detection is encoded by the stage kernels
 * (c1_select_block_modes against those bands or zeros, then c1_mdct_batch, c1_quantize_frames, c1_pack_units); the rest of
 * that push, and every other push, takes the usual path.  One nuance on that first frame: for non-finite bands the stage
 * selector follows the reference's Math.max / Math.min, where the encoder's detector clamps, so there it follows the
 * reference.  Setting the options a stream already has changes nothing. */
int c1_enc_stream_set_options(c1_enc_stream *s, const c1_encode_options *opts);
/* c1_enc_stream_push with the block modes of the pushed frames given (mode bytes as for c1_encode_modes_batch, validated the
 * same way: an invalid byte returns C1_ERR_ARG and leaves the stream as it was).  The stream continues bit for bit as the
 * reference's closure does when fixedBlockModes is set frame by frame for these frames and then put back to what the stream's
 * options say; the stream's options do not change.  On a stream under detection the frames behave like a temporary switch to
 * fixed modes: the detection history stays at the last frame detection ran on (c1_enc_stream_get_state: transient_mags is
 * unchanged by these frames), and the first frame of the next ordinary push is detected against it, by the mechanism described
 * under c1_enc_stream_set_options.  On a stream under fixed modes the frames simply take the given modes. */
int c1_enc_stream_push_modes(c1_enc_stream *s, const float *const *pcm /* host */, int64_t frames,
                             const uint8_t *modes /* host, frames*channels */, uint8_t *units /* host, frames*channels*212 */);
/* c1_enc_stream_push (modes NULL) or c1_enc_stream_push_modes (modes given) with the allocation bias of every pushed unit taken
 * from a palette, as in c1_encode_biases_batch and validated the same way (an invalid call leaves the stream as it was).  Of
 * the entries only biased_scale_factors is read: with modes NULL the stream's own options decide threshold and block modes.
 * The stream's options do not change, and the bias is not state: c1_enc_stream_get_state afterwards is what it is after the
 * same push without a palette.  The frames a stream encodes one at a time (the first two after c1_enc_stream_set_state, the
 * first after a switch back to detection) allocate under their own unit's entry too. */
int c1_enc_stream_push_biases(c1_enc_stream *s, const float *const *pcm /* host */, int64_t frames,
                              const c1_encode_options *palette, int n_palette, const uint8_t *bias_index /* host, frames*channels */,
                              const uint8_t *modes /* host, frames*channels, or NULL */, uint8_t *units /* host */);
/* c1_enc_stream_push (modes NULL) or c1_enc_stream_push_modes (modes given) with the word lengths, and optionally the scale-factor
 * indices, of every pushed unit allocated by the measured coding error: the streaming form of c1_encode_measured_*,
 * c1_encode_measured_sf_* and c1_encode_measured_masked_*, which are nested bit for bit (flat tables give the sf call, the single
 * offset 0 the plain one).  The call the push behaves as follows from its arguments:
 *     mask_floor   sf_offsets
 *     non-NULL     non-NULL     c1_encode_measured_masked_* with those offsets
 *     non-NULL     NULL         c1_encode_measured_masked_* with the single offset 0; n_offsets must be 0
 *     NULL         non-NULL     c1_encode_measured_sf_*
 *     NULL         NULL         c1_encode_measured_*; n_offsets must be 0
 * Definition.  The analysis of the pushed frames, their block modes and the record the reference's allocation chain leaves per
 * unit are exactly what c1_enc_stream_push computes for the same PCM on the same stream (c1_enc_stream_push_modes when modes is
 * given).  On top of that record every unit is the per-unit function defined above for c1_encode_measured_masked_*, word for
 * word: weights, error table, candidates and pick, gains, greedy, totals, the first amount of least T, the NaN rule, the fallback
 * against T_ref, the records of a taken unit and its packing.  This holds for every frame of the push, including the ones a
 * stream encodes one at a time (the first two after c1_enc_stream_set_state, the first after a switch back to detection).
 * The measured allocation keeps no state: after the push c1_enc_stream_get_state, the detection history and the count of pushed
 * frames are bit for bit what they are after the plain push of the same PCM, so plain, modes, biases and measured pushes may be
 * mixed freely on one stream.
 * Arguments.  Every pointer is HOST memory.  units is required; taken (frames*channels), shifts (frames*channels*52),
 * distortion (frames*channels*2), energy (frames*channels) and weights (frames*channels*52) may each be NULL and have the shapes
 * and meanings of the *_batch calls.  shifts without offsets is written as zeros.  mask_spread without mask_floor, weights
 * without mask_floor and n_offsets != 0 with sf_offsets NULL are C1_ERR_ARG; the offsets and the tables are validated as in the
 * whole-buffer calls, with the same messages; the stream's options are validated as those calls validate theirs; the mode bytes
 * as c1_enc_stream_push_modes validates them.  What the arguments alone decide is decided before the stream is looked at.  A
 * rejected call leaves the stream and every output as they were.  frames 0 .. 2^22 per call.  The tables are uploaded as in
 * c1_encode_measured_masked_device, under the same stream-order contract.  "measure" in c1_ctx_kernel_ms counts the step.
 * Which kernel measures: a launch of at most 8 192 sound units -- of this call or of the whole-buffer calls above -- takes a kernel
 * that spends a workgroup on every unit, larger ones a wave; the outputs are the same bits.  C1_MEASURED_WIDE, read when a context
 * is created, overrides this: 0 never the workgroup kernel, 1 always. */
int c1_enc_stream_push_measured(c1_enc_stream *s, const float *const *pcm /* host */, int64_t frames,
                                const uint8_t *modes /* host, frames*channels, or NULL */,
                                const int8_t *sf_offsets /* host, n_offsets values, or NULL */, int n_offsets,
                                const double *mask_floor /* host, 52, or NULL */, const double *mask_spread /* host, 52*52, or NULL */,
                                uint8_t *units /* host, frames*channels*212 */, uint8_t *taken /* host, or NULL */,
                                int8_t *shifts /* host, or NULL */, double *distortion /* host, or NULL */,
                                double *energy /* host, or NULL */, double *weights /* host, or NULL */);
/* The block modes of the pushed frames chosen from candidates by the error of the measured allocation: the streaming form of
 * c1_encode_measured_modes_* (above), OPT-IN like it.
 * Definition, by composition.  For unit u and candidate k the figures (T_ref, T*, taken, energy) are what
 * c1_enc_stream_push_measured(modes = the constant cand_modes[k], sf_offsets, no tables) reports for the same PCM on a twin stream
 * in the same state; choice, modes_out and T_final are c1_encode_measured_modes_*'s; units, taken and shifts are byte for byte
 * c1_enc_stream_push_measured(modes = modes_out)'s.  After the push the stream is bit for bit what it is after
 * c1_enc_stream_push_modes of the same PCM -- c1_enc_stream_get_state, the detection history and the count of pushed frames: the
 * QMF delay lines and the MDCT overlap do not depend on the modes, and on a stream under detection the frames behave as a
 * temporary switch to fixed modes.  So for a stream pushed from its start the rows are those of c1_encode_measured_modes_batch
 * over the whole signal, whatever the stream's block-mode options are, and all kinds of push mix freely on one stream.  The
 * first two frames after c1_enc_stream_set_state run that call's front end on the restored pools (the from-state analysis under
 * all-long and all-short modes, the pools advanced once); there is no detection frame and no switch frame.
 * Arguments.  Every pointer is HOST memory.  units is required; choice, modes_out, taken (frames*channels), shifts
 * (frames*channels*52), distortion (frames*channels*n_cand*2) and energy (frames*channels*n_cand) may each be NULL and have the
 * shapes and meanings of c1_encode_measured_modes_batch.  sf_offsets NULL with n_offsets 0 gives the plain measured allocation
 * (shifts is then zeros); n_offsets != 0 with sf_offsets NULL is C1_ERR_ARG.  The candidates and the offsets are validated as in
 * the whole-buffer call, with the same messages, the stream's options as that call validates its own.  What the arguments alone
 * decide is decided before the stream is looked at.  A rejected call leaves the stream and every output as they were.  frames
 * 0 .. 2^22 per call.  "measure" in c1_ctx_kernel_ms counts the search, one launch per launch of the chain. */
int c1_enc_stream_push_measured_modes(c1_enc_stream *s, const float *const *pcm /* host */, int64_t frames,
                                      const uint8_t *cand_modes /* host, n_cand bytes */, int n_cand,
                                      const int8_t *sf_offsets /* host, n_offsets values, or NULL */, int n_offsets,
                                      uint8_t *units /* host, frames*channels*212 */, uint8_t *choice /* host, or NULL */,
                                      uint8_t *modes_out /* host, or NULL */, uint8_t *taken /* host, or NULL */,
                                      int8_t *shifts /* host, or NULL */, double *distortion /* host, or NULL */,
                                      double *energy /* host, or NULL */);
/* c1_enc_stream_push_measured_modes under one masking threshold per unit: the streaming form of
 * c1_encode_measured_modes_masked_* (above), whose definition holds word for word.  mask_floor is required; the tables are
 * validated and uploaded as in c1_encode_measured_masked_device, with the same messages and the same stream-order contract.
 * weights (frames*channels*52) may be NULL like every output but units.  Everything else -- the stream afterwards, the first
 * two frames after c1_enc_stream_set_state, the order of validation, a rejected call -- is c1_enc_stream_push_measured_modes'. */
int c1_enc_stream_push_measured_modes_masked(c1_enc_stream *s, const float *const *pcm /* host */, int64_t frames,
                                             const uint8_t *cand_modes /* host, n_cand bytes */, int n_cand,
                                             const int8_t *sf_offsets /* host, n_offsets values, or NULL */, int n_offsets,
                                             const double *mask_floor /* host, 52 */, const double *mask_spread /* host, 52*52, or NULL */,
                                             uint8_t *units /* host, frames*channels*212 */, uint8_t *choice /* host, or NULL */,
                                             uint8_t *modes_out /* host, or NULL */, uint8_t *taken /* host, or NULL */,
                                             int8_t *shifts /* host, or NULL */, double *distortion /* host, or NULL */,
                                             double *energy /* host, or NULL */, double *weights /* host, or NULL */);
int c1_dec_stream_create(c1_ctx *ctx, int channels, c1_dec_stream **out);
int c1_dec_stream_push(c1_dec_stream *s, const uint8_t *units /* host */, int64_t frames,
                       float *const *pcm /* host */);
int c1_dec_stream_destroy(c1_dec_stream *s);
/* decode() over frame fields (below, c1_decode_fields_*) on the same stream: one frame per channel, unit index = frame *
 * channels + channel in every array.  Continues the stream c1_dec_stream_push decodes: any interleaving of unit pushes and
 * field pushes decodes exactly as one call over the concatenated frames would (the decoded state after a frame is a function
 * of that frame alone).  The domain is validated as c1_decode_fields_batch validates it; frames 0 .. 2^20 per call. */
int c1_dec_stream_push_fields(c1_dec_stream *s, int64_t frames, const int32_t *nbfu, const int32_t *block_modes,
                              const int32_t *sfi, const int32_t *wl, const int32_t *quantized, float *const *pcm /* host */);

/* ---- stream state in the reference's BufferPool layout (codec/core/buffers.js:30-72).  In the reference a stream IS its
 *      pool: encode(options, pool) and decode(pool) continue from whatever the pool holds (encoder.js:438-441), so a pool can
 *      be checkpointed, copied to fork a stream, or handed to another worker.  These two structs are that state, one per
 *      channel, and the entry points below read it, write it and encode / decode from it.  Finite values only, denormals
 *      and -0 included; every value is honoured bit for bit, also state no PCM or unit history could have produced. ------- */
typedef struct c1_enc_state {   /* 483 floats = 1932 bytes */
  float qmf_low[46];            /* qmfDelays.lowBand:  the last 46 inputs of the first QMF stage (encoder.js:66)          */
  float qmf_mid[46];            /* qmfDelays.midBand:  the last 46 inputs of the second stage (:75)                       */
  float qmf_high[39];           /* qmfDelays.highBand: the last 39 high-band samples, its delay (:84-90)                  */
  float mdct_overlap[3][32];    /* mdctOverlap: W[i] * the last 32 samples of every band (:309-316)                       */
  float transient_mags[256];    /* transientDetection, 64 | 64 | 128: performFFT's magnitudes of the last frame detection
                                   ran on (:142); untouched by frames under fixed block modes (:130-132)                 */
} c1_enc_state;
typedef struct c1_dec_state {   /* 179 floats = 716 bytes */
  float qmf_low[46], qmf_mid[46], qmf_high[39];   /* the decoder's qmfDelays, as c1_qmf_synthesis_batch's comment defines them */
  float imdct_tail[3][16];      /* the last 16 entries of imdctOverlap[band], the only ones that carry (c1_imdct_batch's comment) */
} c1_dec_state;

/* The frame closures over explicit pools, batched: the reference's encode(options, pool)(frame) and decode(pool)(unit) for n
 * independent pools at once.  Pool i encodes pcm[i*512 ..] from in[i] into units[i*212 ..] and leaves its pool in out[i]
 * (decode: units[i*212 ..] from in[i] into pcm[i*512 ..]).  out may be in (in place) or NULL; n == 0 writes nothing.  All
 * pools share opts: detection -- the frame's magnitudes are compared with in[i].transient_mags and written to out[i] -- or
 * fixed block modes, any mix of long and short, under which transient_mags passes through unchanged (encoder.js:130-132);
 * any supported allocation bias.  Number model: encode, the reference's always (binary64 operations, binary32 at every
 * typed-array store), nothing is speculated; decode, the reference's under the decode models C1_DECODE_EXACT and
 * C1_DECODE_BINARY32_BULK, and binary32 under C1_DECODE_BINARY32 (c1_ctx_set_decode_model): PCM and out[i] are then what
 * c1_decode_device computes in binary32 for the same unit after the same history, bit for bit.  C1_ERR_ARG for a NULL pointer
 * or n out of range. */
/* device pointers, asynchronous on the context's stream (the caller's-stream contract above); n 0 .. 2^27; pcm 16-byte
 * aligned, units (decode) and states 4-byte aligned.  The state is not checked: for non-finite entries the output is unspecified, and no access leaves the buffers. */
int c1_encode_frames_from_states_device(c1_ctx *ctx, int64_t n, const float *pcm, const c1_enc_state *in,
                                        const c1_encode_options *opts, uint8_t *units, c1_enc_state *out);
int c1_decode_frames_from_states_device(c1_ctx *ctx, int64_t n, const uint8_t *units, const c1_dec_state *in, float *pcm,
                                        c1_dec_state *out);
/* host pointers, synchronous; n 0 .. 2^20.  A non-finite state entry is C1_ERR_ARG, naming its pool and field. */
int c1_encode_frames_from_states(c1_ctx *ctx, int64_t n, const float *pcm, const c1_enc_state *in,
                                 const c1_encode_options *opts, uint8_t *units, c1_enc_state *out);
int c1_decode_frames_from_states(c1_ctx *ctx, int64_t n, const uint8_t *units, const c1_dec_state *in, float *pcm,
                                 c1_dec_state *out);

/* n independent mono signals of any lengths, each from its own pool, in one call: what n reference closures produce.  Signal i
 * owns frames [frame_offsets[i], frame_offsets[i+1]) of one concatenated PCM buffer (512 floats per frame) and the same unit
 * indices of one concatenated unit buffer (212 bytes per unit).  frame_offsets has n + 1 entries, starts at 0 and never
 * decreases; a signal may be empty.  All signals share opts.  Signal i starts from in[i], or from a fresh pool (all zeros)
 * when in is NULL; out[i] receives the pool the reference holds after the signal's last frame.  out may be NULL or in (in
 * place).  An empty signal writes no units and out[i] = in[i] bit for bit (zeros when in is NULL).  Under fixed block modes
 * transient_mags passes from in[i] to out[i] unchanged (encoder.js:130-132); under detection it holds the magnitudes of the
 * signal's last frame.  A stereo file is two signals: the reference's channels are independent closures (processor.js:119-136).
 * The bytes do not depend on the speculation mode, on how the library chunks the work, or on the neighbouring signals.
 * How: the concatenation runs once through c1_encode_device / c1_decode_device as one mono stream; then the
 * first two frames of every signal (decode: the first frame) are computed again from in[i] by the from-state kernels, and the
 * pools are rebuilt from the last two frames (decode: the last unit) as c1_*_stream_get_state rebuilds them.
 * Decode models (c1_ctx_set_decode_model).  C1_DECODE_BINARY32_BULK applies to the bulk of a decode call; the first frame
 * of every signal and the pools written to out are still computed in the reference's number model (binary64 operations,
 * binary32 at every typed-array store): that frame is bit-identical to the reference.  Under C1_DECODE_BINARY32 the bulk, the
 * first frames and the pools are all binary32: every signal is, bit for bit, its own c1_decode_device call under that model
 * (from in[i]: the continuation of the binary32 stream in[i] came from). */
/* device pointers -- pcm, units, in, out -- but frame_offsets, a HOST pointer that is read before the call returns.
 * Asynchronous on the context's stream (the caller's-stream contract above).  n 0 .. 2^20, frame_offsets[n] 0 .. 2^27; pcm
 * 16-byte aligned, units and states 4-byte aligned.  The states are not checked, as in c1_encode_frames_from_states_device.
 * A second signals call on the same context waits on the host until the first one's index lists have been uploaded. */
int c1_encode_signals_device(c1_ctx *ctx, int64_t n, const int64_t *frame_offsets, const float *pcm, const c1_enc_state *in,
                             const c1_encode_options *opts, uint8_t *units, c1_enc_state *out);
int c1_decode_signals_device(c1_ctx *ctx, int64_t n, const int64_t *frame_offsets, const uint8_t *units, const c1_dec_state *in,
                             float *pcm, c1_dec_state *out);
/* host pointers, synchronous; frame_offsets[n] 0 .. 2^22.  C1_ERR_ARG for a non-finite state entry, naming its signal and
 * field, for frame_offsets that do not start at 0, decrease or pass the limits, and for a NULL frame_offsets, opts, or (with
 * frames to process) pcm or units.  A rejected call writes nothing. */
int c1_encode_signals(c1_ctx *ctx, int64_t n, const int64_t *frame_offsets, const float *pcm, const c1_enc_state *in,
                      const c1_encode_options *opts, uint8_t *units, c1_enc_state *out);
int c1_decode_signals(c1_ctx *ctx, int64_t n, const int64_t *frame_offsets, const uint8_t *units, const c1_dec_state *in,
                      float *pcm, c1_dec_state *out);

/* c1_encode_signals* with the measured allocation: layout, pools, in / out and empty signals as above; the
 * measured arguments as in c1_enc_stream_push_measured -- tables and / or offsets select the masked, the sf or the plain
 * definition, tables alone mean the single offset 0, shifts without offsets are zeros; mask_spread or weights without mask_floor,
 * and n_offsets != 0 without offsets, are C1_ERR_ARG.  The per-unit outputs are indexed by frame of the concatenation: taken one
 * entry per unit, shifts 52, distortion 2, energy 1, weights 52; each may be NULL, and so may units, as long as one output is
 * asked for.  modes: NULL, or one byte per frame of the concatenation (the domain of c1_enc_stream_push_modes); every frame then
 * behaves as under fixed block modes of its byte, the detector does not run, transient_mags passes from in[i] to out[i], and the
 * threshold and fixed modes of opts are not read.
 * Definition, by composition: the rows of signal i -- units and all five outputs, doubles as bit patterns -- are what
 * c1_enc_stream_push_measured reports for signal i's frames in one push on a mono stream created with opts and restored to in[i]
 * with c1_enc_stream_set_state (or fresh), under the same modes rows, offsets and tables, and out[i] is that stream's
 * c1_enc_stream_get_state.  Nothing depends on the neighbouring signals, on chunking, on the speculation mode, or on which
 * measuring kernel a launch takes.
 * How: the concatenation runs once as c1_encode_measured_*_device runs it; the first two frames of every signal are computed
 * again from in[i] with the measured step between allocation and packing, and one launch moves their rows to their places.
 * C1_SIGNAL_STARTS (read when the context is created) selects how: 0 in two passes of the from-state kernel, frame 1 from the pool
 * frame 0 left (with modes: once per mode byte present, at most eight times); 1 in one pass of a kernel that keeps that pool
 * on the chip; unset: two passes (DESIGN.md 6r has the measurements behind that).  The bits are the same.
 * Device form: device pointers but frame_offsets, sf_offsets, mask_floor and mask_spread, which are HOST pointers read before the
 * call returns.  Asynchronous on the context's stream under the contracts of c1_encode_signals_device and
 * c1_encode_measured_masked_device; with modes on the two-pass route the call reads the mode bytes back and waits for the
 * stream.  Limits, the tighter of the two calls composed: n 0 .. 2^20, frame_offsets[n] 0 .. 2^27; pcm 16-byte aligned; units,
 * states and shifts 4-byte, distortion, energy and weights 8-byte aligned.  States and mode bytes are not checked (a byte outside
 * the domain is brought into it). */
int c1_encode_signals_measured_device(c1_ctx *ctx, int64_t n, const int64_t *frame_offsets /* host */, const float *pcm,
                                      const c1_enc_state *in, const c1_encode_options *opts, const uint8_t *modes,
                                      const int8_t *sf_offsets /* host */, int n_offsets, const double *mask_floor /* host */,
                                      const double *mask_spread /* host */, uint8_t *units, c1_enc_state *out, uint8_t *taken,
                                      int8_t *shifts, double *distortion, double *energy, double *weights);
/* host pointers, synchronous; frame_offsets[n] 0 .. 2^22.  What the arguments alone decide is decided first and needs neither a
 * context nor a device: the measured arguments, the options, frame_offsets, a mode byte outside the domain (naming its frame), a
 * non-finite state entry (naming its signal and field), all outputs NULL.  A rejected call writes nothing. */
int c1_encode_signals_measured(c1_ctx *ctx, int64_t n, const int64_t *frame_offsets, const float *pcm, const c1_enc_state *in,
                               const c1_encode_options *opts, const uint8_t *modes, const int8_t *sf_offsets, int n_offsets,
                               const double *mask_floor, const double *mask_spread, uint8_t *units, c1_enc_state *out,
                               uint8_t *taken, int8_t *shifts, double *distortion, double *energy, double *weights);

/* c1_encode_signals* with the measured block-mode search: layout, pools, in / out (NULL, or in place) and empty
 * signals as in c1_encode_signals*, frame_offsets with n + 1 entries, a stereo file two signals.  cand_modes, n_cand (1 to 8
 * distinct bytes of the domain), sf_offsets and n_offsets are c1_enc_stream_push_measured_modes': sf_offsets NULL with n_offsets 0
 * is the search over the plain measured allocation, and shifts is then zeros; n_offsets != 0 without offsets is C1_ERR_ARG.  The
 * per-unit outputs have c1_encode_measured_modes_*'s shapes, indexed by frame of the concatenation: choice, modes_out and taken
 * one entry per unit, shifts 52, distortion 2 * n_cand (unit-major), energy n_cand; each may be NULL, and so may units, as long as
 * one output is asked for.  There are no masking tables: each candidate's thresholds would come from a different spectrum, and
 * nothing has shown their ratios comparable across modes.
 * Definition, by composition: the rows of signal i -- units and all six outputs, doubles as bit patterns -- are what
 * c1_enc_stream_push_measured_modes reports for signal i's frames in one push on a mono stream created with opts and restored to
 * in[i] with c1_enc_stream_set_state (or fresh), under the same candidates and offsets, and out[i] is that stream's
 * c1_enc_stream_get_state: what a stream holds after c1_enc_stream_push_modes of modes_out, transient_mags passing from in[i] to
 * out[i].  Of opts only what the measured calls read under given modes is read: neither the threshold nor the fixed modes.
 * Nothing depends on the neighbouring signals, on chunking, on the speculation mode, on C1_SIGNAL_STARTS or on which measuring
 * kernel a launch takes (C1_MEASURED_WIDE).
 * How: the concatenation runs once as c1_encode_measured_modes_device runs it; the first two frames of every signal are computed
 * again from in[i] -- the from-state kernel under all-long and under all-short options, the allocation chain per candidate, the
 * search, packing -- frame 1 from the pool frame 0 left, and one launch per chunk of rows moves their units and outputs to their
 * places.  Both settings of C1_SIGNAL_STARTS take this two-pass route.
 * Device form: device pointers but frame_offsets, cand_modes and sf_offsets, which are HOST pointers read before the call
 * returns.  Asynchronous on the context's stream under the contracts of c1_encode_signals_device and
 * c1_encode_measured_modes_device.  Limits, the tighter of the calls composed: n 0 .. 2^20, frame_offsets[n] 0 .. 2^27; pcm
 * 16-byte aligned; units, states and shifts 4-byte, distortion and energy 8-byte aligned.  States are not checked. */
int c1_encode_signals_measured_modes_device(c1_ctx *ctx, int64_t n, const int64_t *frame_offsets /* host */, const float *pcm,
                                            const c1_enc_state *in, const c1_encode_options *opts, const uint8_t *cand_modes /* host */,
                                            int n_cand, const int8_t *sf_offsets /* host */, int n_offsets, uint8_t *units,
                                            c1_enc_state *out, uint8_t *choice, uint8_t *modes_out, uint8_t *taken, int8_t *shifts,
                                            double *distortion, double *energy);
/* host pointers, synchronous; frame_offsets[n] 0 .. 2^22.  What the arguments alone decide is decided first and needs neither a
 * context nor a device: the candidates, the offsets, the options, frame_offsets, a non-finite state entry (naming its signal and
 * field), all outputs NULL.  A rejected call writes nothing. */
int c1_encode_signals_measured_modes(c1_ctx *ctx, int64_t n, const int64_t *frame_offsets, const float *pcm, const c1_enc_state *in,
                                     const c1_encode_options *opts, const uint8_t *cand_modes, int n_cand, const int8_t *sf_offsets,
                                     int n_offsets, uint8_t *units, c1_enc_state *out, uint8_t *choice, uint8_t *modes_out,
                                     uint8_t *taken, int8_t *shifts, double *distortion, double *energy);

/* Snapshot and restore of a stream: host pointers, `channels` entries.  get_state returns what the reference's pool would hold
 * after the same calls -- pushes, option changes and earlier restores; every field zero on a fresh stream.  transient_mags is
 * the spectrum of the last frame detection ran on: the last pushed frame while detection is on, the kept frame after a switch
 * to fixed modes, the restored values verbatim when nothing was detected since a restore, zeros when detection never ran.
 * set_state replaces the whole state of every channel, also mid-stream: whatever PCM, unit or field history the stream held
 * stops counting, and the following pushes (units or fields, in any interleaving; under later c1_enc_stream_set_options calls
 * too) continue as the reference continues from that pool.  set_state then get_state returns the same bits.  A non-finite
 * entry is C1_ERR_ARG and leaves the stream as it was.  How: the two frames after an encoder restore, and the frame after a
 * decoder restore, run through the from-state kernels; from then on the stream's own PCM / unit history is real again
 * (all state after a frame is a function of that frame and the 138 samples before it; the decoder's, of that
 * frame's unit alone).
 * Decode models (c1_ctx_set_decode_model): a decoder stream reads its context's model at every call.  Under C1_DECODE_BINARY32
 * pushes of units and of fields, in any interleaving and after a restore, all compute in binary32 and give the bits of one
 * c1_decode_device call over the whole stream; under the other two models everything but the plain unit push is exact.
 * get_state returns the pool the last frame left under the model that decoded it.  When the model went to or from
 * C1_DECODE_BINARY32 between two pushes, the next push continues from that pool as after set_state: every frame is the
 * from-state frame (c1_decode_frames_from_states) under the model in force, from the pool the frame before it left. */
int c1_enc_stream_get_state(c1_enc_stream *s, c1_enc_state *out);
int c1_enc_stream_set_state(c1_enc_stream *s, const c1_enc_state *in);
int c1_dec_stream_get_state(c1_dec_stream *s, c1_dec_state *out);
int c1_dec_stream_set_state(c1_dec_stream *s, const c1_dec_state *in);

/* ---- device-resident synthetic input for measurement ------------- */
enum { C1_SIGNAL_WHITE = 0, C1_SIGNAL_PINK_BURSTS = 1, C1_SIGNAL_MIXED = 2, C1_SIGNAL_PARTIALS = 3 };
/* Fills pcm (DEVICE pointer, frames*512 floats) with a signal of the given statistics.  Every 512-
 * frame segment restarts xorshift32 from a seed derived from (seed, segment), so segments are
 * generated in parallel; segment 0 with seed s reproduces the first 512 frames of the generators
 * in BASELINE.md section 4 exactly (the parity subset).  C1_SIGNAL_MIXED is the synthetic corpus of BASELINE configs[3]:
 * 512-frame segments cycling white noise, pink noise with bursts, stationary partials with slow amplitude modulation
 * and quiet white noise; C1_SIGNAL_PARTIALS is the tonal segment kind alone (parity subsets of both are checked by
 * copying the generated PCM back to the host). */
int c1_generate_device(c1_ctx *ctx, int signal, uint32_t seed, int64_t frames, float *pcm);

/* ---- the data formats either side of the path -------------- */
/* WAV PCM ingest, bin/cli.js:367-404 (WavReader._processFrameBuffer / _sampleToFloat): little-endian
 * interleaved integer PCM (bits = 16, 24 or 32) -> planar float32, value / 2^(bits-1).  Device pointers. */
int c1_pcm_from_int_device(c1_ctx *ctx, const void *interleaved, int bits, int channels,
                           int64_t samples_per_channel, float *const *pcm);
/* 16-bit WAV output, codec/io/processor.js:368-447: clamp to [-1,1], negative * 32768, positive * 32767,
 * DataView.setInt16 truncation; planar float32 -> little-endian interleaved int16.  Device pointers. */
int c1_pcm_to_int16_device(c1_ctx *ctx, const float *const *pcm, int channels,
                           int64_t samples_per_channel, int16_t *interleaved);
/* WAV body <-> sound units in one host call (what the reference's CLI does around the codec: WavReader ->
 * frameBufferToFrames -> encode, bin/cli.js:367-404, codec/io/processor.js:246-276; and decode -> createWavBlob,
 * processor.js:349-447).  The integer PCM crosses PCIe (half the bytes of float32 for 16 bit) and is converted on
 * the device; batches are streamed in chunks, at the pinned rate when the host buffers are page-locked.
 * samples_per_channel need not be a multiple of 512: the last frame is zero padded as frameBufferToFrames does.
 * units: ceil(samples_per_channel / 512) * channels * 212 bytes. */
int c1_encode_wav_batch(c1_ctx *ctx, const void *interleaved, int bits, int channels, int64_t samples_per_channel,
                        const c1_encode_options *opts, uint8_t *units);
/* decode `frames` frames to 16-bit interleaved PCM: frames * 512 * channels int16 */
int c1_decode_wav16_batch(c1_ctx *ctx, const uint8_t *units, int channels, int64_t frames, int16_t *interleaved);
/* AeaFile.createHeader, codec/io/serialization.js:190-211 (host side; the units a batch call returns are
 * already the AEA body: header + units is the whole file).  title is UTF-8, truncated to 255 bytes. */
int c1_aea_header(const char *title, uint32_t unit_count, int channels, uint8_t out[2048]);

/* ---- the single-stage functions the reference exports next to encode()/decode() (codec/index.js:30-35,42).  Host
 *      pointers, synchronous; the arithmetic runs on the device in the reference's own number model.  They serve
 *      applications that import these names; the hot path itself never calls them (it quantizes inside the packing kernel
 *      and transforms inside the analysis kernels). ------------------------------------------------------------------- */
/* quantize, codec/coding/quantization.js:34-56: out[i] = ToInt32(clamp(((x norm) +- 0.5) | 0)), norm = range / SCALE_FACTORS[sfi];
 * zeros when bits or sfi is 0.  range is the reference's (1 << (bits - 1)) - 1: an int32 shift with the count mod 32, the
 * "- 1" in binary64, so every int bits_per_sample is accepted with the reference's meaning (range 0 at 1 and 33; at 32 it
 * is -2147483649, the clamps cross and every output is 2147483647).  Deviation: scale_factor_index outside 0..63 is
 * C1_ERR_ARG, where the reference reads SCALE_FACTORS[sfi] as undefined and produces NaN or 0. */
int c1_quantize(c1_ctx *ctx, const float *coefficients, int n, int scale_factor_index, int bits_per_sample, int32_t *out);
/* dequantize, quantization.js:65-78: Float32((q SCALE_FACTORS[sfi]) / range), range and the argument domain as for c1_quantize */
int c1_dequantize(c1_ctx *ctx, const int32_t *quantized, int n, int scale_factor_index, int bits_per_sample, float *out);
/* FFT.fft, codec/transforms/fft.js:14-68: in place on real[n], imag[n], n a power of two; w = (cos, sin)(-2 pi / stride) for
 * stride = 2, 4, .., n as the HOST's Math.cos / Math.sin give them (log2(n) pairs; the reference computes them per call, :37-39) */
int c1_fft(c1_ctx *ctx, float *real, float *imag, int n, const double *w);
/* qmfAnalysisStage, codec/pipeline/encoder.js:57-96, for `frames` consecutive frames of one channel: pcm = (halo_frames + frames)
 * * 512 samples, the first halo_frames (0..2) being the stream's history (zero history = a fresh BufferPool); bands =
 * frames * 512 floats, low128 | mid128 | high256 (the high band behind its 39-sample delay) per frame */
int c1_qmf_analysis_batch(c1_ctx *ctx, const float *pcm, int64_t frames, int halo_frames, float *bands);
/* mdctStage, encoder.js:170-349, from band samples: bands = (halo_frames + frames) * 512 floats as above, the first frame (when
 * halo_frames = 1) being the previous frame of the stream, whose band tails make mdctOverlap (:309-316; none: a fresh pool's zero
 * overlap); block_modes = frames * 3 (0 long, else short); coefs = frames * 512 (as quantizationStage receives them);
 * bands_windowed (optional) = frames * 512: the band arrays as the reference leaves them, windowed in place (:244,292,314) */
int c1_mdct_batch(c1_ctx *ctx, const float *bands, int64_t frames, int halo_frames, const int32_t *block_modes, float *coefs,
                  float *bands_windowed);

/* The decoder's pipeline stages (codec/pipeline/decoder.js:52-389) and deserializeFrame, for `frames` (0 .. 2^20) consecutive
 * frames of one channel.  Host pointers, synchronous, like the two calls above; the reference's number model (binary64
 * operations, binary32 at every typed-array store) under every decode model: c1_ctx_set_decode_model and
 * c1_ctx_set_decode_precision do not reach the single-stage exports, which have no binary32 form.
 * "Frame fields", int32 arrays per batch: nbfu[frames] (nBfu); block_modes[frames*3] (the three band modes); sfi[frames*52]
 * and wl[frames*52] (scale-factor and word-length index per BFU); quantized[frames*512] (BFU after BFU, SPECS_PER_BFU[b]
 * values each: slot order, where a long band's coefficients also sit). */
/* deserializeFrame, serialization.js:111-176: units = frames*212 bytes -> frame fields.  Entries the reference leaves unset
 * -- sfi and wl of BFUs at or above nBfu, quantized of those BFUs and of BFUs with word length 0 -- come back as zeros. */
int c1_unpack_units(c1_ctx *ctx, const uint8_t *units, int64_t frames, int32_t *nbfu, int32_t *block_modes, int32_t *sfi,
                    int32_t *wl, int32_t *quantized);
/* dequantizationStage, decoder.js:52-98: frame fields -> coefs = frames*512 floats (as imdctStage receives them).  Any nBfu
 * 0..52; for the BFUs below it any wl 0..15 (0: the BFU stays zero) and sfi 0..63 (0: zero, quantization.js:66-68), anything
 * else is C1_ERR_ARG; entries at or above nBfu are not read.  Mantissas are any int32, not clamped:
 * Float32((q * SCALE_FACTORS[sfi]) / ((1 << (bits - 1)) - 1)).  A band is long only when its mode is exactly 0 (:82); its
 * BFUs then sit at BFU_START_LONG, else at BFU_START_SHORT. */
int c1_dequantize_frames(c1_ctx *ctx, int64_t frames, const int32_t *nbfu, const int32_t *block_modes, const int32_t *sfi,
                         const int32_t *wl, const int32_t *quantized, float *coefs);
/* imdctStage, decoder.js:116-330: coefs = (halo_frames + frames) * 512 floats and block_modes = (halo_frames + frames) * 3
 * (0 long, any other value short), the first halo_frames (0 or 1) being the stream's previous frame -> bands = frames * 512
 * floats, low128 | mid128 | high256 per frame (the three arrays qmfSynthesisStage receives).  History: imdctOverlap
 * (buffers.js:63-67, 256 | 256 | 512 floats) carries into the next frame only its last 16 entries per band, which are the
 * last 16 IMDCT samples of the band (:227-230, :296-300): a function of the previous frame's coefficients and modes alone.
 * Without a halo the call starts from a fresh BufferPool's zero overlap. */
int c1_imdct_batch(c1_ctx *ctx, const float *coefs, int64_t frames, int halo_frames, const int32_t *block_modes, float *bands);
/* qmfSynthesisStage, decoder.js:349-389: bands = (halo_frames + frames) * 512 floats as above, the first halo_frames (0 or 1)
 * being the previous frame's -> pcm = frames * 512 samples.  History: qmfDelays (buffers.js:29-33) = highBand, the last 39
 * samples of the previous frame's high band; midBand, the last 46 interleaved (low + mid) / 2, (low - mid) / 2 inputs of
 * stage 2; lowBand, the last 46 inputs of stage 1, made from the previous frame's low and mid bands (samples 93..127)
 * and high band.  All are functions of the previous frame's bands alone; without a halo they are a fresh pool's zeros. */
int c1_qmf_synthesis_batch(c1_ctx *ctx, const float *bands, int64_t frames, int halo_frames, float *pcm);

/* The encoder's two middle-to-last pipeline stages (codec/pipeline/encoder.js:111-152, :365-418), which with
 * c1_qmf_analysis_batch (qmfAnalysisStage) and c1_mdct_batch (mdctStage) make up encode() (:438-450).  For `frames` (0 .. 2^20)
 * consecutive frames of one channel; host pointers, synchronous; the reference's number model always.  Both return C1_ERR_ARG
 * for a bad halo, a NULL pointer or NULL opts; frames == 0 writes nothing. */
/* blockSelectorStage, encoder.js:111-152 (detection branch).  bands = (halo_frames + frames) * 512 floats, low128 | mid128 |
 * high256 as qmfAnalysisStage returns them (unwindowed); halo_frames 0 or 1: the bands whose magnitudes are the pool's
 * transientDetection (the last frame detection ran on), none = a fresh pool's zero magnitudes.  threshold =
 * options.transientThresholdLow, any double (NaN: nothing is transient).  block_modes = frames * 3 int32: per band 0, or
 * 2 | 2 | 3 when its score > threshold (:143). */
int c1_select_block_modes(c1_ctx *ctx, const float *bands, int64_t frames, int halo_frames, double threshold,
                          int32_t *block_modes);
/* quantizationStage, encoder.js:365-418.  coefs = frames * 512 floats as mdctStage returns them, any bit pattern;
 * block_modes = frames * 3, any int32 (0 long, anything else short); opts->biased_scale_factors = allocationBias's table
 * (threshold and fixed modes are not read).  Out: frame fields as c1_unpack_units writes them -- nbfu, sfi and wl of the
 * BFUs below nBfu (sfi as findScaleFactor gave it, also where wl is 0), quantized; zeros at and above nBfu and where wl is 0.
 * findScaleFactor's maximum skips NaN (signalling or quiet), so +-Inf gives 63 and -0 and denormals give 0; quantize gives 0
 * for +-Inf and NaN.  allocateBits' fallback (:132-139, no finite total) gives nBfu 20 with every index 0.  The bit
 * allocation runs on scratch of the call, not on the context's encode workspace. */
int c1_quantize_frames(c1_ctx *ctx, const float *coefs, int64_t frames, const int32_t *block_modes,
                       const c1_encode_options *opts, int32_t *nbfu, int32_t *sfi, int32_t *wl, int32_t *quantized);
/* serializeFrame, codec/io/serialization.js:41-98, the inverse of c1_unpack_units: frame fields in the layout c1_unpack_units
 * writes and c1_quantize_frames returns -> units = frames*212 bytes.  frames 0 .. 2^20 of one channel; host pointers,
 * synchronous; frames == 0 writes nothing.  C1_ERR_ARG for a NULL pointer, frames out of range, or an nbfu outside 0..52
 * (the layout holds 52 BFUs).  Every other value is any int32 and takes the reference's meaning:
 *   header: ((2 - m0) << 14) | ((2 - m1) << 12) | ((3 - m2) << 10) | (idx << 5) in wrapping uint32 arithmetic, truncated
 *     to 16 bits, big-endian; idx = the position of nbfu in BFU_AMOUNTS, or -1, which sets bits 5..15.  Out-of-range
 *     modes make the fields overlap (nbfu 19, modes 0,0,0: 0xffe0; nbfu 20, modes 1,-2,7: 0xf000).
 *   from bit 16: nbfu 4-bit fields wl & 15, then nbfu 6-bit fields sfi & 63.
 *   mantissas: for b < nbfu in BFU order, SPECS_PER_BFU[b] fields of WORD_LENGTH_BITS[wl] = wl + 1 bits, value q & mask,
 *     when wl is 1..15.  A wl outside 0..15 still writes its 4 bits wl & 15 but no mantissas (WORD_LENGTH_BITS[wl] is
 *     undefined there).
 *   truncation: bits past bit 1696 are dropped, also the tail of a field that straddles it (packBits stops at the end of
 *     the buffer, bitstream.js:15-38); then bytes 209..211 are zeroed.  Bits after the end of the stream are zero. */
int c1_pack_units(c1_ctx *ctx, int64_t frames, const int32_t *nbfu, const int32_t *block_modes, const int32_t *sfi,
                  const int32_t *wl, const int32_t *quantized, uint8_t *units);

/* The decision functions of codec/analysis/transient.js (performFFT, detectTransient) and codec/coding/bitallocation.js
 * (findScaleFactor, allocateBits), which the encoder runs at the codec's fixed shapes, for any shapes and values, batched over
 * `problems` (0 .. 2^20) independent problems.  Host pointers, synchronous; the reference's number model (binary64 operations
 * in its index order, binary32 at every typed-array store).  Input values are doubles as JavaScript reads them; variable-length
 * inputs are concatenated, with offsets[problems + 1] starting at 0 and non-decreasing (problem p owns values
 * [offsets[p], offsets[p + 1])), at most 2^28 values per call.  C1_ERR_ARG for a NULL pointer or a range outside these. */
/* performFFT, transient.js:17-35: the first min(length, fft_size) samples of each problem rounded to binary32 (real.set),
 * zero padding, FFT.fft with w as for c1_fft (log2(fft_size) pairs from the host's Math.cos / Math.sin), then
 * Float32(Math.sqrt(re*re + im*im)) of bins 0 .. fft_size/2 - 1 -> magnitudes = problems * (fft_size / 2) floats.  fft_size is a
 * power of two 1 .. 2^22 (1 writes nothing, as Float32Array(1 / 2) is empty); problems * fft_size <= 2^26.  Deviation: any
 * other fft_size is C1_ERR_ARG (the reference's FFT does not define it). */
int c1_perform_fft(c1_ctx *ctx, const double *samples, const int64_t *offsets, int64_t problems, int fft_size, const double *w,
                   float *magnitudes);
/* detectTransient, transient.js:44-226: currentCoeffs and prevCoeffs of any lengths (cur_offsets, prev_offsets).  has_prev
 * (NULL: every problem has one) = 0 is a falsy prevCoeffs: false, score NaN.  A read of prevCoeffs past its end is undefined
 * (NaN in flux and energy); extra previous bins count in its flatness and high-frequency ratio only.  Math.max / Math.min
 * propagate NaN, and `Math.sqrt(e) || 1e-6` also replaces a NaN.  Math.log1p(10) is the installed tables' log1p_10.
 * transient[p] = score > thresholds[p] (a NaN score never is); scores[p] = the score (a test tap). */
int c1_detect_transients(c1_ctx *ctx, const double *cur, const int64_t *cur_offsets, const double *prev, const int64_t *prev_offsets,
                         const uint8_t *has_prev, const double *thresholds, int64_t problems, uint8_t *transient, double *scores);
/* findScaleFactor, bitallocation.js:290-299: max |v| over the first `lengths[p]` values (a read past the array is undefined and,
 * like NaN, never raises the maximum; lengths <= 0 read nothing), then 0 for a zero maximum, else
 * clamp(ceil(3 (Math.log2(max) + 21)), 0, 63) with V8's Math.log2 (c1_libm_device fn 4): +Inf gives 63. */
int c1_find_scale_factors(c1_ctx *ctx, const double *values, const int64_t *offsets, const int64_t *lengths, int64_t problems,
                          int32_t *indices);
/* allocateBits, bitallocation.js:74-288: per problem max_bfu_counts[p] (0..52) BFUs; BFU i (p*52 + i) has bfu_sizes (any int32,
 * bfuSizes[i] | 0) and bfu_lengths values at data + bfu_offsets (entries at and above max_bfu_counts[p] are not read, nor those
 * of size 0).  A BFU shorter than its size reads undefined past its end; a negative size reads nothing.  biased_scale_factors =
 * the 64 entries of buildBiasedScaleFactorTable(allocationBias), any doubles.  Out per problem: bfu_count; allocation[52] (the
 * first bfu_count word lengths, zeros behind); scale_factor_indices[52] (the first maxBfuCount, zeros behind); fallback = 1
 * when no candidate total is < +Inf (bfuCount 20, zero word lengths, 52 zero indices; :132-139).  Deviation: maxBfuCount
 * above 52 is C1_ERR_ARG. */
int c1_allocate_bits(c1_ctx *ctx, const double *data, int64_t data_len, const int64_t *bfu_offsets, const int32_t *bfu_lengths,
                     const int32_t *bfu_sizes, const int32_t *max_bfu_counts, int64_t problems, const double *biased_scale_factors,
                     int32_t *bfu_count, int32_t *allocation, int32_t *scale_factor_indices, uint8_t *fallback);

/* The decode() frame closure (codec/pipeline/decoder.js:408-411: dequantizationStage, imdctStage, qmfSynthesisStage) over frame
 * fields in the layout c1_unpack_units writes, in one device launch: what the reference's decode() computes for a frameData
 * object, also for fields serializeFrame would not carry (an nBfu outside BFU_AMOUNTS, band modes other than 0 and the
 * short codes, mantissas beyond their word length).  channels 1 or 2; unit index = frame * channels + channel in every array
 * (the interleave of c1_unpack_units over stereo units).  halo_frames 0 or 1: one frame of fields per channel precedes each
 * pointer, the stream's previous frame, whose fields rebuild imdctOverlap and qmfDelays; without one the state is a fresh
 * BufferPool's zeros.  pcm[c] = frames * 512 samples.
 * Number model: the reference's (binary64 operations, binary32 at every typed-array store) under the decode models
 * C1_DECODE_EXACT and C1_DECODE_BINARY32_BULK.  Under C1_DECODE_BINARY32 (c1_ctx_set_decode_model) the binary32 unit decoder's,
 * operation for operation: dequantization is Float32(q * Float32(Float32(SCALE_FACTORS[sfi]) * Float32(1 / range))), the
 * product also for sfi 0 (a zero with q's sign) and +0 for word length 0, and the later stages run in binary32; the fields
 * c1_unpack_units makes of sound units then decode to the bits c1_decode_device gives for the units under that model, and
 * fields no unit can carry stay within its error against the exact decode.  c1_dec_stream_push_fields follows
 * the same rule.  Exact dequantization is Float32((q * SCALE_FACTORS[sfi]) / ((1 << (bits - 1)) - 1)) for any int32 q, with the
 * semantics of c1_dequantize_frames: entries at or above nBfu are never read, nor are the mantissas of BFUs with word length 0,
 * and a band is long only when its mode is exactly 0.
 * Domain: nbfu 0..52; below nbfu, wl 0..15 and sfi 0..63; block modes and mantissas any int32. */
/* device pointers, asynchronous on the context's stream; frames 0 .. 2^27 per channel; quantized 16-byte aligned, pcm[c]
 * 16-byte aligned.  Fields outside the domain are not checked here: the output is then unspecified, but every read stays in
 * bounds for any int32 value (nbfu is clamped to 0..52, wl & 15 and sfi & 63 are what is read). */
int c1_decode_fields_device(c1_ctx *ctx, int channels, int64_t frames, int halo_frames, const int32_t *nbfu,
                            const int32_t *block_modes, const int32_t *sfi, const int32_t *wl, const int32_t *quantized,
                            float *const *pcm);
/* host pointers, synchronous; frames 0 .. 2^20 per channel.  Validates the domain over the halo and the frames first:
 * C1_ERR_ARG naming the frame (-1 for the halo; and the channel when channels is 2) and the BFU, worded as
 * c1_dequantize_frames words it; also for a bad halo, a NULL pointer or frames out of range. */
int c1_decode_fields_batch(c1_ctx *ctx, int channels, int64_t frames, int halo_frames, const int32_t *nbfu,
                           const int32_t *block_modes, const int32_t *sfi, const int32_t *wl, const int32_t *quantized,
                           float *const *pcm);

/* ---- stage taps for bring-up and stage-level parity tests (device pointers) ---------------- */
/* bands: frames*channels*512 floats (low128|mid128|high256 per unit index, before windowing);
 * coefs: same shape (MDCT coefficients as quantizationStage receives them);
 * side:  frames*channels*64 bytes: sfi[52], modes byte (m0|m1<<2|m2<<4);  any of the three may be NULL */
int c1_encode_stages_device(c1_ctx *ctx, const float *const *pcm, int channels, int64_t frames,
                            int halo_frames, const c1_encode_options *opts, float *bands,
                            float *coefs, uint8_t *side, uint8_t *alloc /* frames*channels*32 or NULL */);

/* Stage taps of the transient detector (transient.js:17-226, blockSelectorStage encoder.js:111-152), device pointers:
 * mags:  frames*channels*256 floats, performFFT's magnitude spectra of the three bands (64 | 64 | 128 per unit index);
 * modes: frames*channels bytes, the block modes the detector chose (m0 | m1<<2 | m2<<4).  opts must ask for detection
 * (fixed_block_modes {-1,-1,-1}).  Either pointer may be NULL. */
int c1_detect_stages_device(c1_ctx *ctx, const float *const *pcm, int channels, int64_t frames, int halo_frames,
                            const c1_encode_options *opts, float *mags, uint8_t *modes);

/* Test tap of the detector's decisions.  scores: frames*channels*3*2 doubles, per unit and band {lo, hi}: with
 * speculative != 0 the interval the binary32 detector derives for calculateTransientScore (transient.js:197-226), else
 * the reference's score twice.  modes: frames*channels bytes (after the exact recheck of the open units);
 * open_units: one uint32 on the device, the number of units whose interval contained the threshold.  Device pointers,
 * any of them may be NULL. */
int c1_detect_scores_device(c1_ctx *ctx, const float *const *pcm, int channels, int64_t frames, int halo_frames,
                            const c1_encode_options *opts, int speculative, double *scores, uint8_t *modes,
                            uint32_t *open_units);
/* Test tap: the speculative detector's binary32 magnitude spectra (mags: frames*channels*256 floats, laid out as
 * c1_detect_stages_device's) and the bound it claims on the l2 distance of each band's spectrum from the reference's
 * (bounds: frames*channels*3 floats).  Device pointers. */
int c1_detect_spec_mags_device(c1_ctx *ctx, const float *const *pcm, int channels, int64_t frames, int halo_frames,
                               float *mags, float *bounds);
/* Test tap: the device's binary32 log2 (v_log_f32), which the speculative detector's flatness sums use, against
 * binary64 log2 over the bit patterns [first_bits, first_bits + count) of normal positive numbers.  out (host):
 * out[0] = max |r - log2 x| / |log2 x| in units of 2^-24 over the x with |log2 x| >= 2^-6, out[1] = max |r - log2 x|
 * over the others. */
int c1_log2f_error_device(c1_ctx *ctx, uint32_t first_bits, uint64_t count, double *out);

/* Test tap: Math.log (fn 0), Math.exp (1), Math.log1p (2), Math.log10 (3) as the reference's engine evaluates them and as
 * the detector's kernels use them (transient.js:129, :137, :185, :211; V8 src/base/ieee754.cc = fdlibm, not correctly
 * rounded, so the algorithm itself is part of the parity contract), and Math.log2 (4) as c1_find_scale_factors uses it
 * (bitallocation.js:297).  in, out: n doubles, device pointers. */
int c1_libm_device(c1_ctx *ctx, int fn, const double *in, double *out, int64_t n);

/* Test tap of the bit allocation (allocateBits, bitallocation.js:74-142).  The library runs the greedy heap only for the
 * candidate BFU counts that a lower bound on their total distortion does not exclude; this call shows both sides of
 * that comparison.  side: units*64 bytes as above (sfi[52] of every unit); out: units*16 doubles = the totals of the
 * eight candidates {20,28,32,36,40,44,48,52} as calculateTotalDistortion returns them (:157-190), then the seven lower
 * bounds, then (slot 15) the index of the candidate the pruned production path chose, -1 for the fallback.  Device
 * pointers.  tests/test_gpu_alloc_bound.py checks bound <= total everywhere and choice == brute-force minimum. */
int c1_alloc_bounds_device(c1_ctx *ctx, const uint8_t *side, int64_t units, const c1_encode_options *opts, double *out);

/* The speculative binary32 analysis on its own (diagnostics; tests/test_gpu_spec.py checks the bound with it):
 * coefs: frames*channels*512 floats = the binary32 coefficients; eps: frames*channels*4 floats = the proven bound on
 * |coefficient - reference coefficient| for bands 0, 1, 2 and a flag word (non-zero bit pattern: a scale-factor
 * index was not certain); side as above.  Fixed block modes [0,0,0] only (C1_ERR_ARG otherwise). */
int c1_spec_stages_device(c1_ctx *ctx, const float *const *pcm, int channels, int64_t frames, int halo_frames,
                          const c1_encode_options *opts, float *coefs, float *eps, uint8_t *side);

/* Test tap of the speculative quantizer on its own (k_pack<.., SPEC>: quantization.js:34-56 in binary32 behind the guard
 * band of DESIGN.md 3b, serializeFrame serialization.js:41-98).  The caller supplies what the analysis and allocation
 * kernels would: coefs units*512 floats (coefficient order of quantizationStage), eps units*4 floats (bounds of bands
 * 0..2; flag word: bit 0 = a scale-factor index is open), side units*64 bytes (sfi[52], modes byte), alloc units*32 bytes
 * (52 word-length nibbles, low nibble first; last dword: fallback flag bit 27, BFU-amount index bits 28..30).  Out:
 * units_out units*212 bytes, and lists = 8 + 3*units uint32: [0] [1] [2] the lengths of the redo, reallocation and
 * re-analysis lists, which start at 8, 8 + units and 8 + 2*units.  Device pointers.  tests/test_gpu_pack_guard.py
 * checks kernel == CPU model (tests/model/pack_model.c) on coefficients built to sit on the guard band's edge. */
int c1_pack_spec_tap_device(c1_ctx *ctx, const float *coefs, const float *eps, const uint8_t *side, const uint8_t *alloc,
                            int64_t units, int all_long, uint8_t *units_out, uint32_t *lists);

#ifdef __cplusplus
}
#endif
#endif /* CARTA1_HIP_H */
