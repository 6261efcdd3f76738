// carta1_napi.cc -- thin N-API addon over the C ABI of include/carta1_hip.h.
// One JavaScript function per C entry point; no codec logic lives here.  Batch calls come in a
// synchronous form and an asynchronous one (napi_async_work on the libuv pool, resolving a Promise)
// so encodeAeaPcm / decodeAeaPcm stay async like the reference's (codec/io/processor.js:597,628).
#include <node_api.h>

#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../../include/carta1_hip.h"

#define NAPI_OK(call)                                                     \
  do {                                                                    \
    if ((call) != napi_ok) {                                              \
      napi_throw_error(env, nullptr, "N-API call failed: " #call);        \
      return nullptr;                                                     \
    }                                                                     \
  } while (0)

namespace {

napi_value throw_c1(napi_env env, int rc) {
  std::string msg = std::string("carta1_hip: ") + c1_last_error();
  napi_throw_error(env, rc == C1_ERR_NO_DEVICE ? "C1_ERR_NO_DEVICE" : (rc == C1_ERR_ARG ? "C1_ERR_ARG" : "C1_ERR_HIP"), msg.c_str());
  return nullptr;
}

bool get_args(napi_env env, napi_callback_info info, size_t want, napi_value *argv) {
  size_t argc = want;
  if (napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr) != napi_ok || argc < want) {
    napi_throw_type_error(env, nullptr, "wrong number of arguments");
    return false;
  }
  return true;
}

template <typename T>
bool get_external(napi_env env, napi_value v, T **out) {
  void *p = nullptr;
  if (napi_get_value_external(env, v, &p) != napi_ok || !p) {
    napi_throw_type_error(env, nullptr, "expected a native handle");
    return false;
  }
  *out = static_cast<T *>(p);
  return true;
}

bool get_typed(napi_env env, napi_value v, napi_typedarray_type want, void **data, size_t *len) {
  napi_typedarray_type t;
  napi_value ab;
  size_t off;
  bool is = false;
  if (napi_is_typedarray(env, v, &is) != napi_ok || !is ||
      napi_get_typedarray_info(env, v, &t, len, data, &ab, &off) != napi_ok || t != want) {
    napi_throw_type_error(env, nullptr, "typed array of the wrong kind");
    return false;
  }
  return true;
}

// options arrive as one Float64Array(68): biased[64], threshold, mode0, mode1, mode2
bool get_options(napi_env env, napi_value v, c1_encode_options *o) {
  void *d;
  size_t n;
  if (!get_typed(env, v, napi_float64_array, &d, &n)) return false;
  if (n != 68) { napi_throw_type_error(env, nullptr, "options must be a Float64Array(68)"); return false; }
  const double *p = static_cast<const double *>(d);
  memset(o, 0, sizeof *o);
  memcpy(o->biased_scale_factors, p, 64 * sizeof(double));
  o->transient_threshold = p[64];
  for (int b = 0; b < 3; b++) o->fixed_block_modes[b] = (int32_t)p[65 + b];
  return true;
}

bool get_channels(napi_env env, napi_value arr, std::vector<float *> *ptrs, size_t *samples) {
  uint32_t n = 0;
  bool is = false;
  if (napi_is_array(env, arr, &is) != napi_ok || !is || napi_get_array_length(env, arr, &n) != napi_ok || n < 1 || n > 2) {
    napi_throw_type_error(env, nullptr, "channels must be an array of one or two Float32Array");
    return false;
  }
  for (uint32_t c = 0; c < n; c++) {
    napi_value e;
    void *d;
    size_t len;
    if (napi_get_element(env, arr, c, &e) != napi_ok || !get_typed(env, e, napi_float32_array, &d, &len)) return false;
    if (c == 0) *samples = len;
    else if (len != *samples) { napi_throw_type_error(env, nullptr, "channels must have equal length"); return false; }
    ptrs->push_back(static_cast<float *>(d));
  }
  return true;
}

// ArrayBuffer of `bytes` bytes.  Large PCM buffers come from page-locked memory (c1_host_alloc) so that the batch calls
// stream them over PCIe in overlapping chunks; they are released by the garbage collector (c1_host_free).
constexpr size_t kPinnedThreshold = (size_t)32768 * 512 * 4;   // one streaming chunk of one channel
void free_pinned(napi_env, void *data, void *) { c1_host_free(data); }
bool make_buffer(napi_env env, size_t bytes, bool pinned, void **data, napi_value *ab) {
  if (pinned && bytes > 0) {
    void *p = nullptr;
    if (c1_host_alloc(bytes, &p) == C1_OK && p) {
      if (napi_create_external_arraybuffer(env, p, bytes, free_pinned, nullptr, ab) == napi_ok) { *data = p; return true; }
      c1_host_free(p);
    }
  }
  return napi_create_arraybuffer(env, bytes, data, ab) == napi_ok;
}
napi_value make_u8(napi_env env, size_t n, uint8_t **data) {
  napi_value ab, ta;
  void *p;
  if (!make_buffer(env, n, false, &p, &ab) || napi_create_typedarray(env, napi_uint8_array, n, ab, 0, &ta) != napi_ok) return nullptr;
  *data = static_cast<uint8_t *>(p);
  return ta;
}
napi_value make_f32(napi_env env, size_t n, float **data) {
  napi_value ab, ta;
  void *p;
  if (!make_buffer(env, n * 4, n * 4 > kPinnedThreshold, &p, &ab) || napi_create_typedarray(env, napi_float32_array, n, ab, 0, &ta) != napi_ok) return nullptr;
  *data = static_cast<float *>(p);
  return ta;
}

// allocPinned(bytes) -> ArrayBuffer in page-locked memory: PCM placed there is uploaded at the pinned PCIe rate
napi_value AllocPinned(napi_env env, napi_callback_info info) {
  napi_value argv[1];
  if (!get_args(env, info, 1, argv)) return nullptr;
  int64_t bytes = 0;
  NAPI_OK(napi_get_value_int64(env, argv[0], &bytes));
  if (bytes < 0) { napi_throw_range_error(env, nullptr, "bytes must be >= 0"); return nullptr; }
  void *p = nullptr;
  const int rc = c1_host_alloc((size_t)bytes, &p);
  if (rc) return throw_c1(env, rc);
  napi_value ab;
  if (bytes == 0) { NAPI_OK(napi_create_arraybuffer(env, 0, &p, &ab)); return ab; }
  if (napi_create_external_arraybuffer(env, p, (size_t)bytes, free_pinned, nullptr, &ab) != napi_ok) {
    c1_host_free(p);
    napi_throw_error(env, nullptr, "allocation failed");
    return nullptr;
  }
  return ab;
}

// ---- library ---------------------------------------------------------------------------------------
napi_value DeviceCount(napi_env env, napi_callback_info) {
  int n = 0;
  const int rc = c1_device_count(&n);
  if (rc) return throw_c1(env, rc);
  napi_value v;
  NAPI_OK(napi_create_int32(env, n, &v));
  return v;
}
napi_value AbiVersion(napi_env env, napi_callback_info) {
  napi_value v;
  NAPI_OK(napi_create_int32(env, c1_abi_version(), &v));
  return v;
}
// tables travel as one Float64Array in the field order of c1_tables
napi_value GetDefaultTables(napi_env env, napi_callback_info) {
  c1_tables t;
  const int rc = c1_get_default_tables(&t);
  if (rc) return throw_c1(env, rc);
  napi_value ab, ta;
  void *p;
  const size_t n = sizeof(c1_tables) / sizeof(double);
  NAPI_OK(napi_create_arraybuffer(env, sizeof t, &p, &ab));
  memcpy(p, &t, sizeof t);
  NAPI_OK(napi_create_typedarray(env, napi_float64_array, n, ab, 0, &ta));
  return ta;
}
napi_value SetTables(napi_env env, napi_callback_info info) {
  napi_value argv[1];
  if (!get_args(env, info, 1, argv)) return nullptr;
  napi_valuetype vt;
  NAPI_OK(napi_typeof(env, argv[0], &vt));
  int rc;
  if (vt == napi_null || vt == napi_undefined) rc = c1_set_tables(nullptr);
  else {
    void *d;
    size_t n;
    if (!get_typed(env, argv[0], napi_float64_array, &d, &n)) return nullptr;
    if (n != sizeof(c1_tables) / sizeof(double)) { napi_throw_type_error(env, nullptr, "tables: wrong length"); return nullptr; }
    c1_tables t;
    memcpy(&t, d, sizeof t);
    rc = c1_set_tables(&t);
  }
  if (rc) return throw_c1(env, rc);
  return nullptr;
}

// ---- contexts ---------------------------------------------------------------------------------------
void FinalizeCtx(napi_env, void *data, void *) { c1_ctx_destroy(static_cast<c1_ctx *>(data)); }
napi_value CtxCreate(napi_env env, napi_callback_info info) {
  napi_value argv[1];
  if (!get_args(env, info, 1, argv)) return nullptr;
  int32_t dev = 0;
  NAPI_OK(napi_get_value_int32(env, argv[0], &dev));
  c1_ctx *ctx = nullptr;
  const int rc = c1_ctx_create(dev, nullptr, &ctx);
  if (rc) return throw_c1(env, rc);
  napi_value ext;
  NAPI_OK(napi_create_external(env, ctx, FinalizeCtx, nullptr, &ext));
  return ext;
}
// ctxSetDecodeModel(ctx, model): c1_ctx_set_decode_model (0 exact, 1 binary32 in the unit-walking kernel, 2 binary32 throughout)
napi_value CtxSetDecodeModel(napi_env env, napi_callback_info info) {
  napi_value argv[2];
  if (!get_args(env, info, 2, argv)) return nullptr;
  c1_ctx *ctx;
  if (!get_external(env, argv[0], &ctx)) return nullptr;
  int32_t model = 0;
  NAPI_OK(napi_get_value_int32(env, argv[1], &model));
  const int rc = c1_ctx_set_decode_model(ctx, model);
  if (rc) return throw_c1(env, rc);
  return nullptr;
}

// ---- batches ------------------------------------------------------------------------------------------
// encodeBatch(ctx, [Float32Array...], haloFrames, options) -> Uint8Array(frames*channels*212)
napi_value EncodeBatch(napi_env env, napi_callback_info info) {
  napi_value argv[4];
  if (!get_args(env, info, 4, argv)) return nullptr;
  c1_ctx *ctx;
  std::vector<float *> ch;
  size_t samples = 0;
  int32_t halo = 0;
  c1_encode_options o;
  if (!get_external(env, argv[0], &ctx) || !get_channels(env, argv[1], &ch, &samples)) return nullptr;
  NAPI_OK(napi_get_value_int32(env, argv[2], &halo));
  if (!get_options(env, argv[3], &o)) return nullptr;
  if (samples % 512 || (int64_t)(samples / 512) < halo) { napi_throw_type_error(env, nullptr, "PCM length must be a multiple of 512"); return nullptr; }
  const int64_t frames = (int64_t)(samples / 512) - halo;
  uint8_t *units;
  napi_value out = make_u8(env, (size_t)frames * ch.size() * C1_UNIT_BYTES, &units);
  if (!out) { napi_throw_error(env, nullptr, "allocation failed"); return nullptr; }
  const float *p[2] = {ch[0] + (size_t)halo * 512, ch.size() > 1 ? ch[1] + (size_t)halo * 512 : nullptr};
  const int rc = c1_encode_batch(ctx, p, (int)ch.size(), frames, halo, &o, units);
  if (rc) return throw_c1(env, rc);
  return out;
}

// encodeBatchModes(ctx, [Float32Array...], haloFrames, options, Uint8Array modes) -> Uint8Array(frames*channels*212):
// c1_encode_modes_batch, one mode byte per sound unit (frame-major, channels interleaved); of the options only the bias is used
napi_value EncodeBatchModes(napi_env env, napi_callback_info info) {
  napi_value argv[5];
  if (!get_args(env, info, 5, argv)) return nullptr;
  c1_ctx *ctx;
  std::vector<float *> ch;
  size_t samples = 0, n_modes = 0;
  int32_t halo = 0;
  c1_encode_options o;
  void *modes;
  if (!get_external(env, argv[0], &ctx) || !get_channels(env, argv[1], &ch, &samples)) return nullptr;
  NAPI_OK(napi_get_value_int32(env, argv[2], &halo));
  if (!get_options(env, argv[3], &o) || !get_typed(env, argv[4], napi_uint8_array, &modes, &n_modes)) return nullptr;
  if (samples % 512 || (int64_t)(samples / 512) < halo) { napi_throw_type_error(env, nullptr, "PCM length must be a multiple of 512"); return nullptr; }
  const int64_t frames = (int64_t)(samples / 512) - halo;
  if (n_modes != (size_t)frames * ch.size()) { napi_throw_type_error(env, nullptr, "modes: one byte per frame and channel"); return nullptr; }
  uint8_t *units;
  napi_value out = make_u8(env, (size_t)frames * ch.size() * C1_UNIT_BYTES, &units);
  if (!out) { napi_throw_error(env, nullptr, "allocation failed"); return nullptr; }
  const float *p[2] = {ch[0] + (size_t)halo * 512, ch.size() > 1 ? ch[1] + (size_t)halo * 512 : nullptr};
  const int rc = c1_encode_modes_batch(ctx, p, (int)ch.size(), frames, halo, &o, static_cast<const uint8_t *>(modes), units);
  if (rc) return throw_c1(env, rc);
  return out;
}

// encodeBatchBiases(ctx, [Float32Array...], haloFrames, Float64Array(68 * n) palette, Uint8Array index, Uint8Array modes | null)
// -> Uint8Array(frames*channels*212): c1_encode_biases_batch, n = 1..8 option sets laid out like `options` one after the other,
// one palette index and (optionally) one mode byte per sound unit (frame-major, channels interleaved)
napi_value EncodeBatchBiases(napi_env env, napi_callback_info info) {
  napi_value argv[6];
  if (!get_args(env, info, 6, argv)) return nullptr;
  c1_ctx *ctx;
  std::vector<float *> ch;
  size_t samples = 0, n_index = 0, n_modes = 0, n_pal = 0;
  int32_t halo = 0;
  void *index, *modes = nullptr, *pal;
  if (!get_external(env, argv[0], &ctx) || !get_channels(env, argv[1], &ch, &samples)) return nullptr;
  NAPI_OK(napi_get_value_int32(env, argv[2], &halo));
  if (!get_typed(env, argv[3], napi_float64_array, &pal, &n_pal) || !get_typed(env, argv[4], napi_uint8_array, &index, &n_index)) return nullptr;
  if (n_pal == 0 || n_pal % 68 || n_pal / 68 > C1_MAX_BIAS_PALETTE) { napi_throw_range_error(env, nullptr, "palette must hold 1 to 8 option sets of 68 doubles"); return nullptr; }
  napi_valuetype mt;
  NAPI_OK(napi_typeof(env, argv[5], &mt));
  const bool have_modes = mt != napi_null && mt != napi_undefined;
  if (have_modes && !get_typed(env, argv[5], napi_uint8_array, &modes, &n_modes)) return nullptr;
  if (samples % 512 || (int64_t)(samples / 512) < halo) { napi_throw_type_error(env, nullptr, "PCM length must be a multiple of 512"); return nullptr; }
  const int64_t frames = (int64_t)(samples / 512) - halo;
  if (n_index != (size_t)frames * ch.size() || (have_modes && n_modes != n_index)) { napi_throw_type_error(env, nullptr, "index and modes: one byte per frame and channel"); return nullptr; }
  std::vector<c1_encode_options> palette(n_pal / 68);
  const double *p64 = static_cast<const double *>(pal);
  for (size_t k = 0; k < palette.size(); k++) {
    memset(&palette[k], 0, sizeof palette[k]);
    memcpy(palette[k].biased_scale_factors, p64 + 68 * k, 64 * sizeof(double));
    palette[k].transient_threshold = p64[68 * k + 64];
    for (int b = 0; b < 3; b++) palette[k].fixed_block_modes[b] = (int32_t)p64[68 * k + 65 + b];
  }
  uint8_t *units;
  napi_value out = make_u8(env, (size_t)frames * ch.size() * C1_UNIT_BYTES, &units);
  if (!out) { napi_throw_error(env, nullptr, "allocation failed"); return nullptr; }
  const float *p[2] = {ch[0] + (size_t)halo * 512, ch.size() > 1 ? ch[1] + (size_t)halo * 512 : nullptr};
  const int rc = c1_encode_biases_batch(ctx, p, (int)ch.size(), frames, halo, palette.data(), (int)palette.size(), static_cast<const uint8_t *>(index),
                                        have_modes ? static_cast<const uint8_t *>(modes) : nullptr, units);
  if (rc) return throw_c1(env, rc);
  return out;
}

// encodeBestBias(ctx, [Float32Array...], haloFrames, Float64Array(68 * n) palette, Uint8Array modes | null)
// -> { units: Uint8Array(frames*channels*212), choice: Uint8Array(frames*channels), distortion: Float64Array(frames*channels*n)
// (unit-major), energy: Float64Array(frames*channels) }: c1_encode_best_bias_batch, the palette laid out as for encodeBatchBiases
napi_value EncodeBestBias(napi_env env, napi_callback_info info) {
  napi_value argv[5];
  if (!get_args(env, info, 5, argv)) return nullptr;
  c1_ctx *ctx;
  std::vector<float *> ch;
  size_t samples = 0, n_modes = 0, n_pal = 0;
  int32_t halo = 0;
  void *modes = nullptr, *pal;
  if (!get_external(env, argv[0], &ctx) || !get_channels(env, argv[1], &ch, &samples)) return nullptr;
  NAPI_OK(napi_get_value_int32(env, argv[2], &halo));
  if (!get_typed(env, argv[3], napi_float64_array, &pal, &n_pal)) return nullptr;
  if (n_pal == 0 || n_pal % 68 || n_pal / 68 > C1_MAX_BIAS_PALETTE) { napi_throw_range_error(env, nullptr, "palette must hold 1 to 8 option sets of 68 doubles"); return nullptr; }
  napi_valuetype mt;
  NAPI_OK(napi_typeof(env, argv[4], &mt));
  const bool have_modes = mt != napi_null && mt != napi_undefined;
  if (have_modes && !get_typed(env, argv[4], napi_uint8_array, &modes, &n_modes)) return nullptr;
  if (samples % 512 || (int64_t)(samples / 512) < halo) { napi_throw_type_error(env, nullptr, "PCM length must be a multiple of 512"); return nullptr; }
  const int64_t frames = (int64_t)(samples / 512) - halo;
  const size_t n_units = (size_t)frames * ch.size();
  if (have_modes && n_modes != n_units) { napi_throw_type_error(env, nullptr, "modes: one byte per frame and channel"); return nullptr; }
  std::vector<c1_encode_options> palette(n_pal / 68);
  const double *p64 = static_cast<const double *>(pal);
  for (size_t k = 0; k < palette.size(); k++) {
    memset(&palette[k], 0, sizeof palette[k]);
    memcpy(palette[k].biased_scale_factors, p64 + 68 * k, 64 * sizeof(double));
    palette[k].transient_threshold = p64[68 * k + 64];
    for (int b = 0; b < 3; b++) palette[k].fixed_block_modes[b] = (int32_t)p64[68 * k + 65 + b];
  }
  uint8_t *units, *choice;
  napi_value out_units = make_u8(env, n_units * C1_UNIT_BYTES, &units), out_choice = make_u8(env, n_units, &choice);
  if (!out_units || !out_choice) { napi_throw_error(env, nullptr, "allocation failed"); return nullptr; }
  napi_value ab_d, ab_e, out_dist, out_energy;
  void *dist, *energy;
  NAPI_OK(napi_create_arraybuffer(env, n_units * palette.size() * sizeof(double), &dist, &ab_d));
  NAPI_OK(napi_create_typedarray(env, napi_float64_array, n_units * palette.size(), ab_d, 0, &out_dist));
  NAPI_OK(napi_create_arraybuffer(env, n_units * sizeof(double), &energy, &ab_e));
  NAPI_OK(napi_create_typedarray(env, napi_float64_array, n_units, ab_e, 0, &out_energy));
  const float *p[2] = {ch[0] + (size_t)halo * 512, ch.size() > 1 ? ch[1] + (size_t)halo * 512 : nullptr};
  const int rc = c1_encode_best_bias_batch(ctx, p, (int)ch.size(), frames, halo, palette.data(), (int)palette.size(),
                                           have_modes ? static_cast<const uint8_t *>(modes) : nullptr, units, choice,
                                           static_cast<double *>(dist), static_cast<double *>(energy));
  if (rc) return throw_c1(env, rc);
  napi_value obj;
  NAPI_OK(napi_create_object(env, &obj));
  NAPI_OK(napi_set_named_property(env, obj, "units", out_units));
  NAPI_OK(napi_set_named_property(env, obj, "choice", out_choice));
  NAPI_OK(napi_set_named_property(env, obj, "distortion", out_dist));
  NAPI_OK(napi_set_named_property(env, obj, "energy", out_energy));
  return obj;
}

// encodeBestModes(ctx, [Float32Array...], haloFrames, options, Uint8Array candidates)
// -> { units: Uint8Array(frames*channels*212), choice, modes: Uint8Array(frames*channels), distortion, energy:
// Float64Array(frames*channels*n) (unit-major) }: c1_encode_best_modes_batch, n = 1..8 distinct mode bytes; of the options only
// the bias is used
napi_value EncodeBestModes(napi_env env, napi_callback_info info) {
  napi_value argv[5];
  if (!get_args(env, info, 5, argv)) return nullptr;
  c1_ctx *ctx;
  std::vector<float *> ch;
  size_t samples = 0, n_cand = 0;
  int32_t halo = 0;
  c1_encode_options o;
  void *cand;
  if (!get_external(env, argv[0], &ctx) || !get_channels(env, argv[1], &ch, &samples)) return nullptr;
  NAPI_OK(napi_get_value_int32(env, argv[2], &halo));
  if (!get_options(env, argv[3], &o) || !get_typed(env, argv[4], napi_uint8_array, &cand, &n_cand)) return nullptr;
  if (n_cand < 1 || n_cand > C1_MAX_MODE_CANDIDATES) { napi_throw_range_error(env, nullptr, "candidates must hold 1 to 8 mode bytes"); return nullptr; }
  if (samples % 512 || (int64_t)(samples / 512) < halo) { napi_throw_type_error(env, nullptr, "PCM length must be a multiple of 512"); return nullptr; }
  const int64_t frames = (int64_t)(samples / 512) - halo;
  const size_t n_units = (size_t)frames * ch.size();
  uint8_t *units, *choice, *modes;
  napi_value out_units = make_u8(env, n_units * C1_UNIT_BYTES, &units), out_choice = make_u8(env, n_units, &choice), out_modes = make_u8(env, n_units, &modes);
  if (!out_units || !out_choice || !out_modes) { napi_throw_error(env, nullptr, "allocation failed"); return nullptr; }
  napi_value ab_d, ab_e, out_dist, out_energy;
  void *dist, *energy;
  NAPI_OK(napi_create_arraybuffer(env, n_units * n_cand * sizeof(double), &dist, &ab_d));
  NAPI_OK(napi_create_typedarray(env, napi_float64_array, n_units * n_cand, ab_d, 0, &out_dist));
  NAPI_OK(napi_create_arraybuffer(env, n_units * n_cand * sizeof(double), &energy, &ab_e));
  NAPI_OK(napi_create_typedarray(env, napi_float64_array, n_units * n_cand, ab_e, 0, &out_energy));
  const float *p[2] = {ch[0] + (size_t)halo * 512, ch.size() > 1 ? ch[1] + (size_t)halo * 512 : nullptr};
  const int rc = c1_encode_best_modes_batch(ctx, p, (int)ch.size(), frames, halo, &o, static_cast<const uint8_t *>(cand), (int)n_cand, units, choice,
                                            modes, static_cast<double *>(dist), static_cast<double *>(energy));
  if (rc) return throw_c1(env, rc);
  napi_value obj;
  NAPI_OK(napi_create_object(env, &obj));
  NAPI_OK(napi_set_named_property(env, obj, "units", out_units));
  NAPI_OK(napi_set_named_property(env, obj, "choice", out_choice));
  NAPI_OK(napi_set_named_property(env, obj, "modes", out_modes));
  NAPI_OK(napi_set_named_property(env, obj, "distortion", out_dist));
  NAPI_OK(napi_set_named_property(env, obj, "energy", out_energy));
  return obj;
}

// encodeMeasured(ctx, [Float32Array...], haloFrames, options, Uint8Array modes | null)
// -> { units: Uint8Array(frames*channels*212), taken: Uint8Array(frames*channels), distortion: Float64Array(frames*channels*2)
// (per unit: the reference record's error, the greedy allocation's), energy: Float64Array(frames*channels) }:
// c1_encode_measured_batch
napi_value EncodeMeasured(napi_env env, napi_callback_info info) {
  napi_value argv[5];
  if (!get_args(env, info, 5, argv)) return nullptr;
  c1_ctx *ctx;
  std::vector<float *> ch;
  size_t samples = 0, n_modes = 0;
  int32_t halo = 0;
  c1_encode_options o;
  void *modes = nullptr;
  if (!get_external(env, argv[0], &ctx) || !get_channels(env, argv[1], &ch, &samples)) return nullptr;
  NAPI_OK(napi_get_value_int32(env, argv[2], &halo));
  if (!get_options(env, argv[3], &o)) return nullptr;
  napi_valuetype mt;
  NAPI_OK(napi_typeof(env, argv[4], &mt));
  const bool have_modes = mt != napi_null && mt != napi_undefined;
  if (have_modes && !get_typed(env, argv[4], napi_uint8_array, &modes, &n_modes)) return nullptr;
  if (samples % 512 || (int64_t)(samples / 512) < halo) { napi_throw_type_error(env, nullptr, "PCM length must be a multiple of 512"); return nullptr; }
  const int64_t frames = (int64_t)(samples / 512) - halo;
  const size_t n_units = (size_t)frames * ch.size();
  if (have_modes && n_modes != n_units) { napi_throw_type_error(env, nullptr, "modes: one byte per frame and channel"); return nullptr; }
  uint8_t *units, *taken;
  napi_value out_units = make_u8(env, n_units * C1_UNIT_BYTES, &units), out_taken = make_u8(env, n_units, &taken);
  if (!out_units || !out_taken) { napi_throw_error(env, nullptr, "allocation failed"); return nullptr; }
  napi_value ab_d, ab_e, out_dist, out_energy;
  void *dist, *energy;
  NAPI_OK(napi_create_arraybuffer(env, n_units * 2 * sizeof(double), &dist, &ab_d));
  NAPI_OK(napi_create_typedarray(env, napi_float64_array, n_units * 2, ab_d, 0, &out_dist));
  NAPI_OK(napi_create_arraybuffer(env, n_units * sizeof(double), &energy, &ab_e));
  NAPI_OK(napi_create_typedarray(env, napi_float64_array, n_units, ab_e, 0, &out_energy));
  const float *p[2] = {ch[0] + (size_t)halo * 512, ch.size() > 1 ? ch[1] + (size_t)halo * 512 : nullptr};
  const int rc = c1_encode_measured_batch(ctx, p, (int)ch.size(), frames, halo, &o, have_modes ? static_cast<const uint8_t *>(modes) : nullptr,
                                          units, taken, static_cast<double *>(dist), static_cast<double *>(energy));
  if (rc) return throw_c1(env, rc);
  napi_value obj;
  NAPI_OK(napi_create_object(env, &obj));
  NAPI_OK(napi_set_named_property(env, obj, "units", out_units));
  NAPI_OK(napi_set_named_property(env, obj, "taken", out_taken));
  NAPI_OK(napi_set_named_property(env, obj, "distortion", out_dist));
  NAPI_OK(napi_set_named_property(env, obj, "energy", out_energy));
  return obj;
}

// encodeMeasuredSf(ctx, [Float32Array...], haloFrames, options, Uint8Array modes | null, Int8Array offsets)
// -> encodeMeasured's object and shifts: Int8Array(frames*channels*52), the offset written per BFU: c1_encode_measured_sf_batch
napi_value EncodeMeasuredSf(napi_env env, napi_callback_info info) {
  napi_value argv[6];
  if (!get_args(env, info, 6, argv)) return nullptr;
  c1_ctx *ctx;
  std::vector<float *> ch;
  size_t samples = 0, n_modes = 0, n_offsets = 0;
  int32_t halo = 0;
  c1_encode_options o;
  void *modes = nullptr, *offsets = nullptr;
  if (!get_external(env, argv[0], &ctx) || !get_channels(env, argv[1], &ch, &samples)) return nullptr;
  NAPI_OK(napi_get_value_int32(env, argv[2], &halo));
  if (!get_options(env, argv[3], &o)) return nullptr;
  napi_valuetype mt;
  NAPI_OK(napi_typeof(env, argv[4], &mt));
  const bool have_modes = mt != napi_null && mt != napi_undefined;
  if (have_modes && !get_typed(env, argv[4], napi_uint8_array, &modes, &n_modes)) return nullptr;
  if (!get_typed(env, argv[5], napi_int8_array, &offsets, &n_offsets)) return nullptr;
  if (samples % 512 || (int64_t)(samples / 512) < halo) { napi_throw_type_error(env, nullptr, "PCM length must be a multiple of 512"); return nullptr; }
  const int64_t frames = (int64_t)(samples / 512) - halo;
  const size_t n_units = (size_t)frames * ch.size();
  if (have_modes && n_modes != n_units) { napi_throw_type_error(env, nullptr, "modes: one byte per frame and channel"); return nullptr; }
  if (n_offsets > 64) n_offsets = 64;                           // the library's own check names the limit
  uint8_t *units, *taken;
  napi_value out_units = make_u8(env, n_units * C1_UNIT_BYTES, &units), out_taken = make_u8(env, n_units, &taken);
  if (!out_units || !out_taken) { napi_throw_error(env, nullptr, "allocation failed"); return nullptr; }
  napi_value ab_s, ab_d, ab_e, out_shifts, out_dist, out_energy;
  void *shifts, *dist, *energy;
  NAPI_OK(napi_create_arraybuffer(env, n_units * 52, &shifts, &ab_s));
  NAPI_OK(napi_create_typedarray(env, napi_int8_array, n_units * 52, ab_s, 0, &out_shifts));
  NAPI_OK(napi_create_arraybuffer(env, n_units * 2 * sizeof(double), &dist, &ab_d));
  NAPI_OK(napi_create_typedarray(env, napi_float64_array, n_units * 2, ab_d, 0, &out_dist));
  NAPI_OK(napi_create_arraybuffer(env, n_units * sizeof(double), &energy, &ab_e));
  NAPI_OK(napi_create_typedarray(env, napi_float64_array, n_units, ab_e, 0, &out_energy));
  const float *p[2] = {ch[0] + (size_t)halo * 512, ch.size() > 1 ? ch[1] + (size_t)halo * 512 : nullptr};
  const int rc = c1_encode_measured_sf_batch(ctx, p, (int)ch.size(), frames, halo, &o, have_modes ? static_cast<const uint8_t *>(modes) : nullptr,
                                             static_cast<const int8_t *>(offsets), (int)n_offsets, units, taken, static_cast<int8_t *>(shifts),
                                             static_cast<double *>(dist), static_cast<double *>(energy));
  if (rc) return throw_c1(env, rc);
  napi_value obj;
  NAPI_OK(napi_create_object(env, &obj));
  NAPI_OK(napi_set_named_property(env, obj, "units", out_units));
  NAPI_OK(napi_set_named_property(env, obj, "taken", out_taken));
  NAPI_OK(napi_set_named_property(env, obj, "shifts", out_shifts));
  NAPI_OK(napi_set_named_property(env, obj, "distortion", out_dist));
  NAPI_OK(napi_set_named_property(env, obj, "energy", out_energy));
  return obj;
}

// encodeMeasuredModes(ctx, [Float32Array...], haloFrames, options, Uint8Array candidates, Int8Array offsets)
// -> { units: Uint8Array(frames*channels*212), choice, modes, taken: Uint8Array(frames*channels), shifts:
// Int8Array(frames*channels*52), distortion: Float64Array(frames*channels*n*2) (unit-major: T_ref, T(n*) per candidate), energy:
// Float64Array(frames*channels*n) }: c1_encode_measured_modes_batch, n = 1..8 distinct mode bytes
napi_value EncodeMeasuredModes(napi_env env, napi_callback_info info) {
  napi_value argv[6];
  if (!get_args(env, info, 6, argv)) return nullptr;
  c1_ctx *ctx;
  std::vector<float *> ch;
  size_t samples = 0, n_cand = 0, n_offsets = 0;
  int32_t halo = 0;
  c1_encode_options o;
  void *cand = nullptr, *offsets = nullptr;
  if (!get_external(env, argv[0], &ctx) || !get_channels(env, argv[1], &ch, &samples)) return nullptr;
  NAPI_OK(napi_get_value_int32(env, argv[2], &halo));
  if (!get_options(env, argv[3], &o) || !get_typed(env, argv[4], napi_uint8_array, &cand, &n_cand)) return nullptr;
  if (!get_typed(env, argv[5], napi_int8_array, &offsets, &n_offsets)) return nullptr;
  if (n_cand < 1 || n_cand > C1_MAX_MODE_CANDIDATES) { napi_throw_range_error(env, nullptr, "candidates must hold 1 to 8 mode bytes"); return nullptr; }
  if (samples % 512 || (int64_t)(samples / 512) < halo) { napi_throw_type_error(env, nullptr, "PCM length must be a multiple of 512"); return nullptr; }
  if (n_offsets > 64) n_offsets = 64;                           // the library's own check names the limit
  const int64_t frames = (int64_t)(samples / 512) - halo;
  const size_t n_units = (size_t)frames * ch.size();
  uint8_t *units, *choice, *modes, *taken;
  napi_value out_units = make_u8(env, n_units * C1_UNIT_BYTES, &units), out_choice = make_u8(env, n_units, &choice),
             out_modes = make_u8(env, n_units, &modes), out_taken = make_u8(env, n_units, &taken);
  if (!out_units || !out_choice || !out_modes || !out_taken) { napi_throw_error(env, nullptr, "allocation failed"); return nullptr; }
  napi_value ab_s, ab_d, ab_e, out_shifts, out_dist, out_energy;
  void *shifts, *dist, *energy;
  NAPI_OK(napi_create_arraybuffer(env, n_units * 52, &shifts, &ab_s));
  NAPI_OK(napi_create_typedarray(env, napi_int8_array, n_units * 52, ab_s, 0, &out_shifts));
  NAPI_OK(napi_create_arraybuffer(env, n_units * n_cand * 2 * sizeof(double), &dist, &ab_d));
  NAPI_OK(napi_create_typedarray(env, napi_float64_array, n_units * n_cand * 2, ab_d, 0, &out_dist));
  NAPI_OK(napi_create_arraybuffer(env, n_units * n_cand * sizeof(double), &energy, &ab_e));
  NAPI_OK(napi_create_typedarray(env, napi_float64_array, n_units * n_cand, ab_e, 0, &out_energy));
  const float *p[2] = {ch[0] + (size_t)halo * 512, ch.size() > 1 ? ch[1] + (size_t)halo * 512 : nullptr};
  const int rc = c1_encode_measured_modes_batch(ctx, p, (int)ch.size(), frames, halo, &o, static_cast<const uint8_t *>(cand), (int)n_cand,
                                                static_cast<const int8_t *>(offsets), (int)n_offsets, units, choice, modes, taken,
                                                static_cast<int8_t *>(shifts), static_cast<double *>(dist), static_cast<double *>(energy));
  if (rc) return throw_c1(env, rc);
  napi_value obj;
  NAPI_OK(napi_create_object(env, &obj));
  NAPI_OK(napi_set_named_property(env, obj, "units", out_units));
  NAPI_OK(napi_set_named_property(env, obj, "choice", out_choice));
  NAPI_OK(napi_set_named_property(env, obj, "modes", out_modes));
  NAPI_OK(napi_set_named_property(env, obj, "taken", out_taken));
  NAPI_OK(napi_set_named_property(env, obj, "shifts", out_shifts));
  NAPI_OK(napi_set_named_property(env, obj, "distortion", out_dist));
  NAPI_OK(napi_set_named_property(env, obj, "energy", out_energy));
  return obj;
}

// encodeMeasuredMasked(ctx, [Float32Array...], haloFrames, options, Uint8Array modes | null, Int8Array offsets, Float64Array floor,
// Float64Array spread | null) -> encodeMeasuredSf's object and weights: Float64Array(frames*channels*52), the reciprocal masking
// threshold of every BFU: c1_encode_measured_masked_batch
napi_value EncodeMeasuredMasked(napi_env env, napi_callback_info info) {
  napi_value argv[8];
  if (!get_args(env, info, 8, argv)) return nullptr;
  c1_ctx *ctx;
  std::vector<float *> ch;
  size_t samples = 0, n_modes = 0, n_offsets = 0, n_floor = 0, n_spread = 0;
  int32_t halo = 0;
  c1_encode_options o;
  void *modes = nullptr, *offsets = nullptr, *floor = nullptr, *spread = nullptr;
  if (!get_external(env, argv[0], &ctx) || !get_channels(env, argv[1], &ch, &samples)) return nullptr;
  NAPI_OK(napi_get_value_int32(env, argv[2], &halo));
  if (!get_options(env, argv[3], &o)) return nullptr;
  napi_valuetype mt, st;
  NAPI_OK(napi_typeof(env, argv[4], &mt));
  NAPI_OK(napi_typeof(env, argv[7], &st));
  const bool have_modes = mt != napi_null && mt != napi_undefined, have_spread = st != napi_null && st != napi_undefined;
  if (have_modes && !get_typed(env, argv[4], napi_uint8_array, &modes, &n_modes)) return nullptr;
  if (!get_typed(env, argv[5], napi_int8_array, &offsets, &n_offsets)) return nullptr;
  if (!get_typed(env, argv[6], napi_float64_array, &floor, &n_floor)) return nullptr;
  if (have_spread && !get_typed(env, argv[7], napi_float64_array, &spread, &n_spread)) return nullptr;
  if (n_floor != 52 || (have_spread && n_spread != 52 * 52)) { napi_throw_type_error(env, nullptr, "masking: floor holds 52 values, spread 52 * 52"); return nullptr; }
  if (samples % 512 || (int64_t)(samples / 512) < halo) { napi_throw_type_error(env, nullptr, "PCM length must be a multiple of 512"); return nullptr; }
  const int64_t frames = (int64_t)(samples / 512) - halo;
  const size_t n_units = (size_t)frames * ch.size();
  if (have_modes && n_modes != n_units) { napi_throw_type_error(env, nullptr, "modes: one byte per frame and channel"); return nullptr; }
  if (n_offsets > 64) n_offsets = 64;                           // the library's own check names the limit
  uint8_t *units, *taken;
  napi_value out_units = make_u8(env, n_units * C1_UNIT_BYTES, &units), out_taken = make_u8(env, n_units, &taken);
  if (!out_units || !out_taken) { napi_throw_error(env, nullptr, "allocation failed"); return nullptr; }
  napi_value ab_s, ab_d, ab_e, ab_w, out_shifts, out_dist, out_energy, out_weights;
  void *shifts, *dist, *energy, *weights;
  NAPI_OK(napi_create_arraybuffer(env, n_units * 52, &shifts, &ab_s));
  NAPI_OK(napi_create_typedarray(env, napi_int8_array, n_units * 52, ab_s, 0, &out_shifts));
  NAPI_OK(napi_create_arraybuffer(env, n_units * 2 * sizeof(double), &dist, &ab_d));
  NAPI_OK(napi_create_typedarray(env, napi_float64_array, n_units * 2, ab_d, 0, &out_dist));
  NAPI_OK(napi_create_arraybuffer(env, n_units * sizeof(double), &energy, &ab_e));
  NAPI_OK(napi_create_typedarray(env, napi_float64_array, n_units, ab_e, 0, &out_energy));
  NAPI_OK(napi_create_arraybuffer(env, n_units * 52 * sizeof(double), &weights, &ab_w));
  NAPI_OK(napi_create_typedarray(env, napi_float64_array, n_units * 52, ab_w, 0, &out_weights));
  const float *p[2] = {ch[0] + (size_t)halo * 512, ch.size() > 1 ? ch[1] + (size_t)halo * 512 : nullptr};
  const int rc = c1_encode_measured_masked_batch(ctx, p, (int)ch.size(), frames, halo, &o, have_modes ? static_cast<const uint8_t *>(modes) : nullptr,
                                                 static_cast<const int8_t *>(offsets), (int)n_offsets, static_cast<const double *>(floor),
                                                 have_spread ? static_cast<const double *>(spread) : nullptr, units, taken,
                                                 static_cast<int8_t *>(shifts), static_cast<double *>(dist), static_cast<double *>(energy),
                                                 static_cast<double *>(weights));
  if (rc) return throw_c1(env, rc);
  napi_value obj;
  NAPI_OK(napi_create_object(env, &obj));
  NAPI_OK(napi_set_named_property(env, obj, "units", out_units));
  NAPI_OK(napi_set_named_property(env, obj, "taken", out_taken));
  NAPI_OK(napi_set_named_property(env, obj, "shifts", out_shifts));
  NAPI_OK(napi_set_named_property(env, obj, "distortion", out_dist));
  NAPI_OK(napi_set_named_property(env, obj, "energy", out_energy));
  NAPI_OK(napi_set_named_property(env, obj, "weights", out_weights));
  return obj;
}

// encodeMeasuredModesMasked(ctx, [Float32Array...], haloFrames, options, Uint8Array candidates, Int8Array offsets, Float64Array floor,
// Float64Array spread | null) -> encodeMeasuredModes' object (distortion and energy weighted) and weights:
// Float64Array(frames*channels*52), the one reciprocal masking threshold per unit and BFU that weighs every candidate:
// c1_encode_measured_modes_masked_batch
napi_value EncodeMeasuredModesMasked(napi_env env, napi_callback_info info) {
  napi_value argv[8];
  if (!get_args(env, info, 8, argv)) return nullptr;
  c1_ctx *ctx;
  std::vector<float *> ch;
  size_t samples = 0, n_cand = 0, n_offsets = 0, n_floor = 0, n_spread = 0;
  int32_t halo = 0;
  c1_encode_options o;
  void *cand = nullptr, *offsets = nullptr, *floor = nullptr, *spread = nullptr;
  if (!get_external(env, argv[0], &ctx) || !get_channels(env, argv[1], &ch, &samples)) return nullptr;
  NAPI_OK(napi_get_value_int32(env, argv[2], &halo));
  if (!get_options(env, argv[3], &o) || !get_typed(env, argv[4], napi_uint8_array, &cand, &n_cand)) return nullptr;
  if (!get_typed(env, argv[5], napi_int8_array, &offsets, &n_offsets)) return nullptr;
  napi_valuetype st;
  NAPI_OK(napi_typeof(env, argv[7], &st));
  const bool have_spread = st != napi_null && st != napi_undefined;
  if (!get_typed(env, argv[6], napi_float64_array, &floor, &n_floor)) return nullptr;
  if (have_spread && !get_typed(env, argv[7], napi_float64_array, &spread, &n_spread)) return nullptr;
  if (n_floor != 52 || (have_spread && n_spread != 52 * 52)) { napi_throw_type_error(env, nullptr, "masking: floor holds 52 values, spread 52 * 52"); return nullptr; }
  if (n_cand < 1 || n_cand > C1_MAX_MODE_CANDIDATES) { napi_throw_range_error(env, nullptr, "candidates must hold 1 to 8 mode bytes"); return nullptr; }
  if (samples % 512 || (int64_t)(samples / 512) < halo) { napi_throw_type_error(env, nullptr, "PCM length must be a multiple of 512"); return nullptr; }
  if (n_offsets > 64) n_offsets = 64;                           // the library's own check names the limit
  const int64_t frames = (int64_t)(samples / 512) - halo;
  const size_t n_units = (size_t)frames * ch.size();
  uint8_t *units, *choice, *modes, *taken;
  napi_value out_units = make_u8(env, n_units * C1_UNIT_BYTES, &units), out_choice = make_u8(env, n_units, &choice),
             out_modes = make_u8(env, n_units, &modes), out_taken = make_u8(env, n_units, &taken);
  if (!out_units || !out_choice || !out_modes || !out_taken) { napi_throw_error(env, nullptr, "allocation failed"); return nullptr; }
  napi_value ab_s, ab_d, ab_e, ab_w, out_shifts, out_dist, out_energy, out_weights;
  void *shifts, *dist, *energy, *weights;
  NAPI_OK(napi_create_arraybuffer(env, n_units * 52, &shifts, &ab_s));
  NAPI_OK(napi_create_typedarray(env, napi_int8_array, n_units * 52, ab_s, 0, &out_shifts));
  NAPI_OK(napi_create_arraybuffer(env, n_units * n_cand * 2 * sizeof(double), &dist, &ab_d));
  NAPI_OK(napi_create_typedarray(env, napi_float64_array, n_units * n_cand * 2, ab_d, 0, &out_dist));
  NAPI_OK(napi_create_arraybuffer(env, n_units * n_cand * sizeof(double), &energy, &ab_e));
  NAPI_OK(napi_create_typedarray(env, napi_float64_array, n_units * n_cand, ab_e, 0, &out_energy));
  NAPI_OK(napi_create_arraybuffer(env, n_units * 52 * sizeof(double), &weights, &ab_w));
  NAPI_OK(napi_create_typedarray(env, napi_float64_array, n_units * 52, ab_w, 0, &out_weights));
  const float *p[2] = {ch[0] + (size_t)halo * 512, ch.size() > 1 ? ch[1] + (size_t)halo * 512 : nullptr};
  const int rc = c1_encode_measured_modes_masked_batch(ctx, p, (int)ch.size(), frames, halo, &o, static_cast<const uint8_t *>(cand), (int)n_cand,
                                                       static_cast<const int8_t *>(offsets), (int)n_offsets, static_cast<const double *>(floor),
                                                       have_spread ? static_cast<const double *>(spread) : nullptr, units, choice, modes, taken,
                                                       static_cast<int8_t *>(shifts), static_cast<double *>(dist), static_cast<double *>(energy),
                                                       static_cast<double *>(weights));
  if (rc) return throw_c1(env, rc);
  napi_value obj;
  NAPI_OK(napi_create_object(env, &obj));
  NAPI_OK(napi_set_named_property(env, obj, "units", out_units));
  NAPI_OK(napi_set_named_property(env, obj, "choice", out_choice));
  NAPI_OK(napi_set_named_property(env, obj, "modes", out_modes));
  NAPI_OK(napi_set_named_property(env, obj, "taken", out_taken));
  NAPI_OK(napi_set_named_property(env, obj, "shifts", out_shifts));
  NAPI_OK(napi_set_named_property(env, obj, "distortion", out_dist));
  NAPI_OK(napi_set_named_property(env, obj, "energy", out_energy));
  NAPI_OK(napi_set_named_property(env, obj, "weights", out_weights));
  return obj;
}

// measureUnits(ctx, [Float32Array...], haloFrames, Uint8Array units, Float64Array floor | null, Float64Array spread | null)
// -> { noise, signal: Float64Array(frames*channels*52), totals: Float64Array(frames*channels*2), weights: Float64Array(frames*
// channels*52), with tables only }: the coding error of given sound units against their PCM, c1_measure_units_batch; shared: under
// the all-long threshold, c1_measure_units_shared_batch (the library requires the floor)
static napi_value measure_units_call(napi_env env, napi_callback_info info, bool shared) {
  napi_value argv[6];
  if (!get_args(env, info, 6, argv)) return nullptr;
  c1_ctx *ctx;
  std::vector<float *> ch;
  size_t samples = 0, n_bytes = 0, n_floor = 0, n_spread = 0;
  int32_t halo = 0;
  void *units = nullptr, *floor = nullptr, *spread = nullptr;
  if (!get_external(env, argv[0], &ctx) || !get_channels(env, argv[1], &ch, &samples)) return nullptr;
  NAPI_OK(napi_get_value_int32(env, argv[2], &halo));
  if (!get_typed(env, argv[3], napi_uint8_array, &units, &n_bytes)) return nullptr;
  napi_valuetype ft, st;
  NAPI_OK(napi_typeof(env, argv[4], &ft));
  NAPI_OK(napi_typeof(env, argv[5], &st));
  const bool have_floor = ft != napi_null && ft != napi_undefined, have_spread = st != napi_null && st != napi_undefined;
  if (have_floor && !get_typed(env, argv[4], napi_float64_array, &floor, &n_floor)) return nullptr;
  if (have_spread && !get_typed(env, argv[5], napi_float64_array, &spread, &n_spread)) return nullptr;
  if ((have_floor && n_floor != 52) || (have_spread && n_spread != 52 * 52)) { napi_throw_type_error(env, nullptr, "masking: floor holds 52 values, spread 52 * 52"); return nullptr; }
  if (samples % 512 || (int64_t)(samples / 512) < halo) { napi_throw_type_error(env, nullptr, "PCM length must be a multiple of 512"); return nullptr; }
  const int64_t frames = (int64_t)(samples / 512) - halo;
  const size_t n_units = (size_t)frames * ch.size();
  if (n_bytes != n_units * C1_UNIT_BYTES) { napi_throw_type_error(env, nullptr, "units: 212 bytes per frame and channel"); return nullptr; }
  const char *const names[4] = {"noise", "signal", "totals", "weights"};
  const size_t width[4] = {52, 52, 2, 52};
  napi_value arrays[4];
  void *data[4] = {nullptr, nullptr, nullptr, nullptr};
  const int n_out = have_floor ? 4 : 3;
  for (int k = 0; k < n_out; k++) {
    napi_value ab;
    NAPI_OK(napi_create_arraybuffer(env, n_units * width[k] * sizeof(double), &data[k], &ab));
    NAPI_OK(napi_create_typedarray(env, napi_float64_array, n_units * width[k], ab, 0, &arrays[k]));
  }
  const float *p[2] = {ch[0] + (size_t)halo * 512, ch.size() > 1 ? ch[1] + (size_t)halo * 512 : nullptr};
  const int rc = (shared ? c1_measure_units_shared_batch : c1_measure_units_batch)(
      ctx, p, (int)ch.size(), frames, halo, static_cast<const uint8_t *>(units), have_floor ? static_cast<const double *>(floor) : nullptr,
      have_spread ? static_cast<const double *>(spread) : nullptr, static_cast<double *>(data[0]), static_cast<double *>(data[1]),
      static_cast<double *>(data[2]), static_cast<double *>(data[3]));
  if (rc) return throw_c1(env, rc);
  napi_value obj;
  NAPI_OK(napi_create_object(env, &obj));
  for (int k = 0; k < n_out; k++) NAPI_OK(napi_set_named_property(env, obj, names[k], arrays[k]));
  return obj;
}
napi_value MeasureUnits(napi_env env, napi_callback_info info) { return measure_units_call(env, info, false); }
// measureUnitsShared: the same arguments and result, the weights from the frame's all-long spectrum
napi_value MeasureUnitsShared(napi_env env, napi_callback_info info) { return measure_units_call(env, info, true); }

// measurePcm(ctx, [Float32Array...], haloFrames, Uint8Array units, haloUnits) -> { noise, signal: Float64Array(frames*channels*16),
// totals: Float64Array(frames*channels*2) }: the error of the decoded PCM of given sound units against their PCM, per 32 samples,
// c1_measure_pcm_batch.  units holds the haloUnits unit(s) of frame -1 first
napi_value MeasurePcm(napi_env env, napi_callback_info info) {
  napi_value argv[5];
  if (!get_args(env, info, 5, argv)) return nullptr;
  c1_ctx *ctx;
  std::vector<float *> ch;
  size_t samples = 0, n_bytes = 0;
  int32_t halo = 0, halo_units = 0;
  void *units = nullptr;
  if (!get_external(env, argv[0], &ctx) || !get_channels(env, argv[1], &ch, &samples)) return nullptr;
  NAPI_OK(napi_get_value_int32(env, argv[2], &halo));
  if (!get_typed(env, argv[3], napi_uint8_array, &units, &n_bytes)) return nullptr;
  NAPI_OK(napi_get_value_int32(env, argv[4], &halo_units));
  if (halo < 0 || halo > 2 || halo_units < 0 || halo_units > 1) { napi_throw_type_error(env, nullptr, "haloFrames must be 0 .. 2 and haloUnits 0 or 1"); return nullptr; }
  if (samples % 512 || (int64_t)(samples / 512) < halo) { napi_throw_type_error(env, nullptr, "PCM length must be a multiple of 512"); return nullptr; }
  const int64_t frames = (int64_t)(samples / 512) - halo;
  const size_t n_units = (size_t)frames * ch.size(), halo_bytes = (size_t)halo_units * ch.size() * C1_UNIT_BYTES;
  if (n_bytes != n_units * C1_UNIT_BYTES + halo_bytes) { napi_throw_type_error(env, nullptr, "units: 212 bytes per frame and channel, the halo unit(s) first"); return nullptr; }
  const char *const names[3] = {"noise", "signal", "totals"};
  const size_t width[3] = {16, 16, 2};
  napi_value arrays[3];
  void *data[3] = {nullptr, nullptr, nullptr};
  for (int k = 0; k < 3; k++) {
    napi_value ab;
    NAPI_OK(napi_create_arraybuffer(env, n_units * width[k] * sizeof(double), &data[k], &ab));
    NAPI_OK(napi_create_typedarray(env, napi_float64_array, n_units * width[k], ab, 0, &arrays[k]));
  }
  const float *p[2] = {ch[0] + (size_t)halo * 512, ch.size() > 1 ? ch[1] + (size_t)halo * 512 : nullptr};
  const int rc = c1_measure_pcm_batch(ctx, p, (int)ch.size(), frames, halo, static_cast<const uint8_t *>(units) + halo_bytes, halo_units,
                                      static_cast<double *>(data[0]), static_cast<double *>(data[1]), static_cast<double *>(data[2]));
  if (rc) return throw_c1(env, rc);
  napi_value obj;
  NAPI_OK(napi_create_object(env, &obj));
  for (int k = 0; k < 3; k++) NAPI_OK(napi_set_named_property(env, obj, names[k], arrays[k]));
  return obj;
}

// decodeBatch(ctx, Uint8Array units, channels, haloUnits) -> [Float32Array...]
napi_value DecodeBatch(napi_env env, napi_callback_info info) {
  napi_value argv[4];
  if (!get_args(env, info, 4, argv)) return nullptr;
  c1_ctx *ctx;
  void *d;
  size_t n;
  int32_t channels = 1, halo = 0;
  if (!get_external(env, argv[0], &ctx) || !get_typed(env, argv[1], napi_uint8_array, &d, &n)) return nullptr;
  NAPI_OK(napi_get_value_int32(env, argv[2], &channels));
  NAPI_OK(napi_get_value_int32(env, argv[3], &halo));
  if (channels < 1 || channels > 2 || n % ((size_t)channels * C1_UNIT_BYTES)) { napi_throw_type_error(env, nullptr, "units: wrong length"); return nullptr; }
  const int64_t frames = (int64_t)(n / ((size_t)channels * C1_UNIT_BYTES)) - halo;
  if (frames < 0) { napi_throw_type_error(env, nullptr, "units shorter than the halo"); return nullptr; }
  napi_value arr;
  NAPI_OK(napi_create_array_with_length(env, channels, &arr));
  float *p[2] = {nullptr, nullptr};
  for (int c = 0; c < channels; c++) {
    napi_value ta = make_f32(env, (size_t)frames * 512, &p[c]);
    if (!ta) { napi_throw_error(env, nullptr, "allocation failed"); return nullptr; }
    NAPI_OK(napi_set_element(env, arr, c, ta));
  }
  const int rc = c1_decode_batch(ctx, static_cast<const uint8_t *>(d) + (size_t)halo * channels * C1_UNIT_BYTES, channels, frames, halo, p);
  if (rc) return throw_c1(env, rc);
  return arr;
}

// n independent mono signals from fresh pools in one call (c1_encode_signals / c1_decode_signals).  frameOffsets: Float64Array of
// n + 1 whole numbers, signal i owns frames [frameOffsets[i], frameOffsets[i + 1]) of the concatenated PCM / units.
bool get_frame_offsets(napi_env env, napi_value v, std::vector<int64_t> *off) {
  void *d;
  size_t n;
  if (!get_typed(env, v, napi_float64_array, &d, &n)) return false;
  if (n < 1) { napi_throw_type_error(env, nullptr, "frameOffsets must hold n + 1 entries"); return false; }
  const double *p = static_cast<const double *>(d);
  for (size_t i = 0; i < n; i++) {
    if (!(p[i] >= 0 && p[i] <= 4503599627370496.0) || p[i] != (double)(int64_t)p[i]) {
      napi_throw_type_error(env, nullptr, "frameOffsets must be whole numbers >= 0");
      return false;
    }
    off->push_back((int64_t)p[i]);
  }
  return true;
}
// encodeSignals(ctx, Float32Array pcm, Float64Array frameOffsets, options) -> Uint8Array(frames * 212)
napi_value EncodeSignals(napi_env env, napi_callback_info info) {
  napi_value argv[4];
  if (!get_args(env, info, 4, argv)) return nullptr;
  c1_ctx *ctx;
  void *d;
  size_t samples;
  std::vector<int64_t> off;
  c1_encode_options o;
  if (!get_external(env, argv[0], &ctx) || !get_typed(env, argv[1], napi_float32_array, &d, &samples) ||
      !get_frame_offsets(env, argv[2], &off) || !get_options(env, argv[3], &o)) return nullptr;
  if (samples % 512 || (uint64_t)off.back() != samples / 512) { napi_throw_type_error(env, nullptr, "pcm must hold frameOffsets[n] frames of 512 samples"); return nullptr; }
  uint8_t *units;
  napi_value out = make_u8(env, (samples / 512) * C1_UNIT_BYTES, &units);
  if (!out) { napi_throw_error(env, nullptr, "allocation failed"); return nullptr; }
  const int rc = c1_encode_signals(ctx, (int64_t)off.size() - 1, off.data(), static_cast<const float *>(d), nullptr, &o, units, nullptr);
  if (rc) return throw_c1(env, rc);
  return out;
}
// encodeSignalsMeasured(ctx, Float32Array pcm, Float64Array frameOffsets, options, Int8Array offsets | null, Float64Array floor |
// null, Float64Array spread | null) -> Uint8Array(frames * 212): encodeSignals with the measured allocation of encodeMeasured
// (offsets and tables null), encodeMeasuredSf (offsets) or encodeMeasuredMasked (tables; without offsets the single offset 0),
// every signal from a fresh pool: c1_encode_signals_measured
napi_value EncodeSignalsMeasured(napi_env env, napi_callback_info info) {
  napi_value argv[7];
  if (!get_args(env, info, 7, argv)) return nullptr;
  c1_ctx *ctx;
  void *d;
  size_t samples, n[3] = {0, 0, 0};
  void *data[3] = {nullptr, nullptr, nullptr};
  std::vector<int64_t> off;
  c1_encode_options o;
  if (!get_external(env, argv[0], &ctx) || !get_typed(env, argv[1], napi_float32_array, &d, &samples) ||
      !get_frame_offsets(env, argv[2], &off) || !get_options(env, argv[3], &o)) return nullptr;
  const napi_typedarray_type kinds[3] = {napi_int8_array, napi_float64_array, napi_float64_array};
  for (int k = 0; k < 3; k++) {
    napi_valuetype t;
    NAPI_OK(napi_typeof(env, argv[4 + k], &t));
    if (t != napi_null && t != napi_undefined && !get_typed(env, argv[4 + k], kinds[k], &data[k], &n[k])) return nullptr;
  }
  if ((data[1] && n[1] != 52) || (data[2] && n[2] != 52 * 52)) { napi_throw_type_error(env, nullptr, "masking: floor holds 52 values, spread 52 * 52"); return nullptr; }
  if (samples % 512 || (uint64_t)off.back() != samples / 512) { napi_throw_type_error(env, nullptr, "pcm must hold frameOffsets[n] frames of 512 samples"); return nullptr; }
  if (n[0] > 64) n[0] = 64;                                     // the library's own check names the limit
  uint8_t *units;
  napi_value out = make_u8(env, (samples / 512) * C1_UNIT_BYTES, &units);
  if (!out) { napi_throw_error(env, nullptr, "allocation failed"); return nullptr; }
  const int rc = c1_encode_signals_measured(ctx, (int64_t)off.size() - 1, off.data(), static_cast<const float *>(d), nullptr, &o, nullptr,
                                            static_cast<const int8_t *>(data[0]), data[0] ? (int)n[0] : 0, static_cast<const double *>(data[1]),
                                            static_cast<const double *>(data[2]), units, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
  if (rc) return throw_c1(env, rc);
  return out;
}
// encodeSignalsMeasuredModes(ctx, Float32Array pcm, Float64Array frameOffsets, options, Uint8Array candidates, Int8Array offsets |
// null) -> Uint8Array(frames * 212): encodeSignals with the measured block-mode search of encodeMeasuredModes (offsets null: the
// plain measured allocation), every signal from a fresh pool: c1_encode_signals_measured_modes
napi_value EncodeSignalsMeasuredModes(napi_env env, napi_callback_info info) {
  napi_value argv[6];
  if (!get_args(env, info, 6, argv)) return nullptr;
  c1_ctx *ctx;
  void *d, *cand = nullptr, *offsets = nullptr;
  size_t samples, n_cand = 0, n_offsets = 0;
  std::vector<int64_t> off;
  c1_encode_options o;
  if (!get_external(env, argv[0], &ctx) || !get_typed(env, argv[1], napi_float32_array, &d, &samples) ||
      !get_frame_offsets(env, argv[2], &off) || !get_options(env, argv[3], &o) ||
      !get_typed(env, argv[4], napi_uint8_array, &cand, &n_cand)) return nullptr;
  napi_valuetype t;
  NAPI_OK(napi_typeof(env, argv[5], &t));
  if (t != napi_null && t != napi_undefined && !get_typed(env, argv[5], napi_int8_array, &offsets, &n_offsets)) return nullptr;
  if (n_cand < 1 || n_cand > C1_MAX_MODE_CANDIDATES) { napi_throw_range_error(env, nullptr, "candidates must hold 1 to 8 mode bytes"); return nullptr; }
  if (samples % 512 || (uint64_t)off.back() != samples / 512) { napi_throw_type_error(env, nullptr, "pcm must hold frameOffsets[n] frames of 512 samples"); return nullptr; }
  if (n_offsets > 64) n_offsets = 64;                           // the library's own check names the limit
  uint8_t *units;
  napi_value out = make_u8(env, (samples / 512) * C1_UNIT_BYTES, &units);
  if (!out) { napi_throw_error(env, nullptr, "allocation failed"); return nullptr; }
  const int rc = c1_encode_signals_measured_modes(ctx, (int64_t)off.size() - 1, off.data(), static_cast<const float *>(d), nullptr, &o,
                                                  static_cast<const uint8_t *>(cand), (int)n_cand, static_cast<const int8_t *>(offsets),
                                                  offsets ? (int)n_offsets : 0, units, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                                  nullptr);
  if (rc) return throw_c1(env, rc);
  return out;
}
// decodeSignals(ctx, Uint8Array units, Float64Array frameOffsets) -> Float32Array(frames * 512)
napi_value DecodeSignals(napi_env env, napi_callback_info info) {
  napi_value argv[3];
  if (!get_args(env, info, 3, argv)) return nullptr;
  c1_ctx *ctx;
  void *d;
  size_t bytes;
  std::vector<int64_t> off;
  if (!get_external(env, argv[0], &ctx) || !get_typed(env, argv[1], napi_uint8_array, &d, &bytes) || !get_frame_offsets(env, argv[2], &off)) return nullptr;
  if (bytes % C1_UNIT_BYTES || (uint64_t)off.back() != bytes / C1_UNIT_BYTES) { napi_throw_type_error(env, nullptr, "units must hold frameOffsets[n] units of 212 bytes"); return nullptr; }
  float *pcm;
  napi_value out = make_f32(env, (bytes / C1_UNIT_BYTES) * 512, &pcm);
  if (!out) { napi_throw_error(env, nullptr, "allocation failed"); return nullptr; }
  const int rc = c1_decode_signals(ctx, (int64_t)off.size() - 1, off.data(), static_cast<const uint8_t *>(d), nullptr, pcm, nullptr);
  if (rc) return throw_c1(env, rc);
  return out;
}

// encodeWavBatch(ctx, Int16Array | Uint8Array wavBody, bits, channels, options) -> Uint8Array units
// (c1_encode_wav_batch: interleaved little-endian integer PCM converted on the device, ragged tail zero padded)
napi_value EncodeWavBatch(napi_env env, napi_callback_info info) {
  napi_value argv[5];
  if (!get_args(env, info, 5, argv)) return nullptr;
  c1_ctx *ctx;
  if (!get_external(env, argv[0], &ctx)) return nullptr;
  bool is_ta = false;
  NAPI_OK(napi_is_typedarray(env, argv[1], &is_ta));
  if (!is_ta) { napi_throw_type_error(env, nullptr, "wav body must be an Int16Array or a Uint8Array"); return nullptr; }
  napi_typedarray_type tt;
  size_t len = 0, off = 0;
  void *data = nullptr;
  napi_value ab;
  NAPI_OK(napi_get_typedarray_info(env, argv[1], &tt, &len, &data, &ab, &off));
  if (tt != napi_int16_array && tt != napi_uint8_array) { napi_throw_type_error(env, nullptr, "wav body must be an Int16Array or a Uint8Array"); return nullptr; }
  const size_t bytes = tt == napi_int16_array ? len * 2 : len;
  int32_t bits = 16, channels = 1;
  NAPI_OK(napi_get_value_int32(env, argv[2], &bits));
  NAPI_OK(napi_get_value_int32(env, argv[3], &channels));
  c1_encode_options o;
  if (!get_options(env, argv[4], &o)) return nullptr;
  if ((bits != 16 && bits != 24 && bits != 32) || channels < 1 || channels > 2 || bytes % ((size_t)channels * (bits / 8))) {
    napi_throw_type_error(env, nullptr, "wav body: bits must be 16, 24 or 32, channels 1 or 2, and the length a whole number of samples");
    return nullptr;
  }
  const int64_t samples = (int64_t)(bytes / ((size_t)channels * (bits / 8)));
  const int64_t frames = (samples + 511) / 512;
  uint8_t *units;
  napi_value out = make_u8(env, (size_t)frames * channels * C1_UNIT_BYTES, &units);
  if (!out) { napi_throw_error(env, nullptr, "allocation failed"); return nullptr; }
  const int rc = c1_encode_wav_batch(ctx, data, bits, channels, samples, &o, units);
  if (rc) return throw_c1(env, rc);
  return out;
}

// decodeWav16Batch(ctx, Uint8Array units, channels) -> Int16Array (interleaved, frames * 512 * channels)
napi_value DecodeWav16Batch(napi_env env, napi_callback_info info) {
  napi_value argv[3];
  if (!get_args(env, info, 3, argv)) return nullptr;
  c1_ctx *ctx;
  void *d;
  size_t n;
  int32_t channels = 1;
  if (!get_external(env, argv[0], &ctx) || !get_typed(env, argv[1], napi_uint8_array, &d, &n)) return nullptr;
  NAPI_OK(napi_get_value_int32(env, argv[2], &channels));
  if (channels < 1 || channels > 2 || n % ((size_t)channels * C1_UNIT_BYTES)) { napi_throw_type_error(env, nullptr, "units: wrong length"); return nullptr; }
  const int64_t frames = (int64_t)(n / ((size_t)channels * C1_UNIT_BYTES));
  const size_t count = (size_t)frames * 512 * channels;
  napi_value ab, ta;
  void *p;
  if (!make_buffer(env, count * 2, count * 2 > kPinnedThreshold, &p, &ab) || napi_create_typedarray(env, napi_int16_array, count, ab, 0, &ta) != napi_ok) {
    napi_throw_error(env, nullptr, "allocation failed");
    return nullptr;
  }
  const int rc = c1_decode_wav16_batch(ctx, static_cast<const uint8_t *>(d), channels, frames, static_cast<int16_t *>(p));
  if (rc) return throw_c1(env, rc);
  return ta;
}

// ---- asynchronous batches: the typed arrays are kept alive by references while the work runs ----------
struct AsyncJob {
  napi_async_work work = nullptr;
  napi_deferred deferred = nullptr;
  napi_ref keep[4] = {nullptr, nullptr, nullptr, nullptr};
  int nkeep = 0;
  c1_ctx *ctx = nullptr;
  std::vector<int> devices;          // non-empty: the *_multi entry points (one context per entry, owned by the library)
  bool encode = true;
  int channels = 1, halo = 0;
  int64_t frames = 0;
  c1_encode_options opts;
  const float *in[2] = {nullptr, nullptr};
  float *outp[2] = {nullptr, nullptr};
  const uint8_t *units_in = nullptr;
  uint8_t *units_out = nullptr;
  napi_ref result = nullptr;
  int rc = 0;
  std::string err;
};
void AsyncExecute(napi_env, void *data) {
  AsyncJob *j = static_cast<AsyncJob *>(data);
  if (!j->devices.empty())
    j->rc = j->encode ? c1_encode_batch_multi(j->devices.data(), (int)j->devices.size(), j->in, j->channels, j->frames, j->halo, &j->opts, j->units_out)
                      : c1_decode_batch_multi(j->devices.data(), (int)j->devices.size(), j->units_in, j->channels, j->frames, j->halo, j->outp);
  else
    j->rc = j->encode ? c1_encode_batch(j->ctx, j->in, j->channels, j->frames, j->halo, &j->opts, j->units_out)
                      : c1_decode_batch(j->ctx, j->units_in, j->channels, j->frames, j->halo, j->outp);
  if (j->rc) j->err = c1_last_error();   // thread-local: read it on the worker thread
}
void AsyncComplete(napi_env env, napi_status, void *data) {
  AsyncJob *j = static_cast<AsyncJob *>(data);
  if (j->rc) {
    napi_value msg, e;
    napi_create_string_utf8(env, ("carta1_hip: " + j->err).c_str(), NAPI_AUTO_LENGTH, &msg);
    napi_create_error(env, nullptr, msg, &e);
    napi_reject_deferred(env, j->deferred, e);
  } else {
    napi_value v;
    napi_get_reference_value(env, j->result, &v);
    napi_resolve_deferred(env, j->deferred, v);
  }
  for (int i = 0; i < j->nkeep; i++) napi_delete_reference(env, j->keep[i]);
  napi_delete_reference(env, j->result);
  napi_delete_async_work(env, j->work);
  delete j;
}
napi_value start_job(napi_env env, AsyncJob *j, const char *name) {
  napi_value promise, rname;
  if (napi_create_promise(env, &j->deferred, &promise) != napi_ok ||
      napi_create_string_utf8(env, name, NAPI_AUTO_LENGTH, &rname) != napi_ok ||
      napi_create_async_work(env, nullptr, rname, AsyncExecute, AsyncComplete, j, &j->work) != napi_ok ||
      napi_queue_async_work(env, j->work) != napi_ok) {
    delete j;
    napi_throw_error(env, nullptr, "could not queue async work");
    return nullptr;
  }
  return promise;
}
// argv[0]: a context, or (multi) an array of device indices
bool get_ctx_or_devices(napi_env env, napi_value v, AsyncJob *j) {
  bool is_array = false;
  if (napi_is_array(env, v, &is_array) != napi_ok) return false;
  if (!is_array) return get_external(env, v, &j->ctx);
  uint32_t n = 0;
  if (napi_get_array_length(env, v, &n) != napi_ok || n < 1 || n > 64) return false;
  for (uint32_t i = 0; i < n; i++) {
    napi_value e;
    int32_t d = 0;
    if (napi_get_element(env, v, i, &e) != napi_ok || napi_get_value_int32(env, e, &d) != napi_ok) return false;
    j->devices.push_back(d);
  }
  return true;
}
// keep `v` alive until the job is done; false (and an exception) when the engine cannot reference it -- the job must
// then not start: its buffers could be collected under it
bool keep_alive(napi_env env, AsyncJob *j, napi_value v) {
  napi_ref r = nullptr;
  if (napi_create_reference(env, v, 1, &r) != napi_ok || !r) {
    napi_throw_error(env, nullptr, "carta1: cannot reference an argument of the asynchronous call");
    return false;
  }
  j->keep[j->nkeep++] = r;
  return true;
}
void drop_job(napi_env env, AsyncJob *j) {
  for (int i = 0; i < j->nkeep; i++) if (j->keep[i]) napi_delete_reference(env, j->keep[i]);
  if (j->result) napi_delete_reference(env, j->result);
  delete j;
}

napi_value EncodeBatchAsync(napi_env env, napi_callback_info info) {
  napi_value argv[4];
  if (!get_args(env, info, 4, argv)) return nullptr;
  AsyncJob *j = new AsyncJob();
  std::vector<float *> ch;
  size_t samples = 0;
  int32_t halo = 0;
  if (!get_ctx_or_devices(env, argv[0], j) || !get_channels(env, argv[1], &ch, &samples) ||
      napi_get_value_int32(env, argv[2], &halo) != napi_ok || !get_options(env, argv[3], &j->opts) ||
      samples % 512 || (int64_t)(samples / 512) < halo) {
    delete j;
    bool pending = false;
    napi_is_exception_pending(env, &pending);
    if (!pending) napi_throw_type_error(env, nullptr, "bad arguments");
    return nullptr;
  }
  j->encode = true;
  j->channels = (int)ch.size();
  j->halo = halo;
  j->frames = (int64_t)(samples / 512) - halo;
  for (size_t c = 0; c < ch.size(); c++) j->in[c] = ch[c] + (size_t)halo * 512;
  napi_value out = make_u8(env, (size_t)j->frames * ch.size() * C1_UNIT_BYTES, &j->units_out);
  if (!out || (j->frames > 0 && !j->units_out)) {
    delete j;
    napi_throw_error(env, nullptr, "could not allocate the result");
    return nullptr;
  }
  // the context (or device list) and the input arrays must outlive the job
  if (!keep_alive(env, j, argv[0]) || !keep_alive(env, j, argv[1])) { drop_job(env, j); return nullptr; }
  if (napi_create_reference(env, out, 1, &j->result) != napi_ok) { j->result = nullptr; drop_job(env, j); napi_throw_error(env, nullptr, "carta1: cannot reference the result"); return nullptr; }
  return start_job(env, j, "carta1.encodeBatch");
}
napi_value DecodeBatchAsync(napi_env env, napi_callback_info info) {
  napi_value argv[4];
  if (!get_args(env, info, 4, argv)) return nullptr;
  AsyncJob *j = new AsyncJob();
  void *d;
  size_t n;
  int32_t channels = 1, halo = 0;
  if (!get_ctx_or_devices(env, argv[0], j) || !get_typed(env, argv[1], napi_uint8_array, &d, &n) ||
      napi_get_value_int32(env, argv[2], &channels) != napi_ok || napi_get_value_int32(env, argv[3], &halo) != napi_ok ||
      channels < 1 || channels > 2 || n % ((size_t)channels * C1_UNIT_BYTES) ||
      (int64_t)(n / ((size_t)channels * C1_UNIT_BYTES)) < halo) {
    delete j;
    bool pending = false;
    napi_is_exception_pending(env, &pending);
    if (!pending) napi_throw_type_error(env, nullptr, "bad arguments");
    return nullptr;
  }
  j->encode = false;
  j->channels = channels;
  j->halo = halo;
  j->frames = (int64_t)(n / ((size_t)channels * C1_UNIT_BYTES)) - halo;
  j->units_in = static_cast<const uint8_t *>(d) + (size_t)halo * channels * C1_UNIT_BYTES;
  napi_value arr;
  napi_create_array_with_length(env, channels, &arr);
  for (int c = 0; c < channels; c++) {
    napi_value ta = make_f32(env, (size_t)j->frames * 512, &j->outp[c]);
    if (!ta || (j->frames > 0 && !j->outp[c])) {
      delete j;
      napi_throw_error(env, nullptr, "could not allocate the result");
      return nullptr;
    }
    napi_set_element(env, arr, c, ta);
  }
  if (!keep_alive(env, j, argv[0]) || !keep_alive(env, j, argv[1])) { drop_job(env, j); return nullptr; }   // context and units outlive the job
  if (napi_create_reference(env, arr, 1, &j->result) != napi_ok) { j->result = nullptr; drop_job(env, j); napi_throw_error(env, nullptr, "carta1: cannot reference the result"); return nullptr; }
  return start_job(env, j, "carta1.decodeBatch");
}

// ---- stateful streams: the native half of one encode()/decode() closure --------------------------------
void FinalizeEnc(napi_env, void *data, void *) { c1_enc_stream_destroy(static_cast<c1_enc_stream *>(data)); }
void FinalizeDec(napi_env, void *data, void *) { c1_dec_stream_destroy(static_cast<c1_dec_stream *>(data)); }
napi_value EncStreamCreate(napi_env env, napi_callback_info info) {
  napi_value argv[3];
  if (!get_args(env, info, 3, argv)) return nullptr;
  c1_ctx *ctx;
  int32_t channels = 1;
  c1_encode_options o;
  if (!get_external(env, argv[0], &ctx)) return nullptr;
  NAPI_OK(napi_get_value_int32(env, argv[1], &channels));
  if (!get_options(env, argv[2], &o)) return nullptr;
  c1_enc_stream *s = nullptr;
  const int rc = c1_enc_stream_create(ctx, channels, &o, &s);
  if (rc) return throw_c1(env, rc);
  napi_value ext;
  NAPI_OK(napi_create_external(env, s, FinalizeEnc, nullptr, &ext));
  // keep the context alive as long as the stream is
  napi_ref ref;
  napi_create_reference(env, argv[0], 1, &ref);
  return ext;
}
napi_value EncStreamPush(napi_env env, napi_callback_info info) {
  napi_value argv[2];
  if (!get_args(env, info, 2, argv)) return nullptr;
  c1_enc_stream *s;
  std::vector<float *> ch;
  size_t samples = 0;
  if (!get_external(env, argv[0], &s) || !get_channels(env, argv[1], &ch, &samples)) return nullptr;
  if (samples % 512) { napi_throw_type_error(env, nullptr, "PCM length must be a multiple of 512"); return nullptr; }
  const int64_t frames = (int64_t)(samples / 512);
  uint8_t *units;
  napi_value out = make_u8(env, (size_t)frames * ch.size() * C1_UNIT_BYTES, &units);
  const float *p[2] = {ch[0], ch.size() > 1 ? ch[1] : nullptr};
  const int rc = c1_enc_stream_push(s, p, frames, units);
  if (rc) return throw_c1(env, rc);
  return out;
}
// encStreamPushMeasured(stream, [Float32Array...], Int8Array offsets | null, Float64Array floor | null, Float64Array spread | null)
// -> Uint8Array units: encStreamPush with the measured allocation of encodeMeasured (offsets and tables null), encodeMeasuredSf
// (offsets) or encodeMeasuredMasked (tables; without offsets the single offset 0): c1_enc_stream_push_measured
napi_value EncStreamPushMeasured(napi_env env, napi_callback_info info) {
  napi_value argv[5];
  if (!get_args(env, info, 5, argv)) return nullptr;
  c1_enc_stream *s;
  std::vector<float *> ch;
  size_t samples = 0, n[3] = {0, 0, 0};
  void *data[3] = {nullptr, nullptr, nullptr};
  if (!get_external(env, argv[0], &s) || !get_channels(env, argv[1], &ch, &samples)) return nullptr;
  const napi_typedarray_type kinds[3] = {napi_int8_array, napi_float64_array, napi_float64_array};
  for (int k = 0; k < 3; k++) {
    napi_valuetype t;
    NAPI_OK(napi_typeof(env, argv[2 + k], &t));
    if (t != napi_null && t != napi_undefined && !get_typed(env, argv[2 + k], kinds[k], &data[k], &n[k])) return nullptr;
  }
  if ((data[1] && n[1] != 52) || (data[2] && n[2] != 52 * 52)) { napi_throw_type_error(env, nullptr, "masking: floor holds 52 values, spread 52 * 52"); return nullptr; }
  if (samples % 512) { napi_throw_type_error(env, nullptr, "PCM length must be a multiple of 512"); return nullptr; }
  if (n[0] > 64) n[0] = 64;                                     // the library's own check names the limit
  const int64_t frames = (int64_t)(samples / 512);
  uint8_t *units;
  napi_value out = make_u8(env, (size_t)frames * ch.size() * C1_UNIT_BYTES, &units);
  const float *p[2] = {ch[0], ch.size() > 1 ? ch[1] : nullptr};
  const int rc = c1_enc_stream_push_measured(s, p, frames, nullptr, static_cast<const int8_t *>(data[0]), data[0] ? (int)n[0] : 0,
                                             static_cast<const double *>(data[1]), static_cast<const double *>(data[2]), units, nullptr,
                                             nullptr, nullptr, nullptr, nullptr);
  if (rc) return throw_c1(env, rc);
  return out;
}
// encStreamPushMeasuredModes(stream, [Float32Array...], Uint8Array candidates, Int8Array offsets | null) -> Uint8Array units:
// encStreamPush with the block modes of every unit chosen among the candidates by the measured allocation's final error, as
// encodeMeasuredModes chooses them (offsets null: the plain measured allocation): c1_enc_stream_push_measured_modes
napi_value EncStreamPushMeasuredModes(napi_env env, napi_callback_info info) {
  napi_value argv[4];
  if (!get_args(env, info, 4, argv)) return nullptr;
  c1_enc_stream *s;
  std::vector<float *> ch;
  size_t samples = 0, n_cand = 0, n_off = 0;
  void *cand = nullptr, *off = nullptr;
  if (!get_external(env, argv[0], &s) || !get_channels(env, argv[1], &ch, &samples)) return nullptr;
  if (!get_typed(env, argv[2], napi_uint8_array, &cand, &n_cand)) return nullptr;
  napi_valuetype t;
  NAPI_OK(napi_typeof(env, argv[3], &t));
  if (t != napi_null && t != napi_undefined && !get_typed(env, argv[3], napi_int8_array, &off, &n_off)) return nullptr;
  if (samples % 512) { napi_throw_type_error(env, nullptr, "PCM length must be a multiple of 512"); return nullptr; }
  if (n_cand > 64) n_cand = 64;                                 // the library's own checks name the limits
  if (n_off > 64) n_off = 64;
  const int64_t frames = (int64_t)(samples / 512);
  uint8_t *units;
  napi_value out = make_u8(env, (size_t)frames * ch.size() * C1_UNIT_BYTES, &units);
  const float *p[2] = {ch[0], ch.size() > 1 ? ch[1] : nullptr};
  const int rc = c1_enc_stream_push_measured_modes(s, p, frames, static_cast<const uint8_t *>(cand), (int)n_cand,
                                                   static_cast<const int8_t *>(off), off ? (int)n_off : 0, units, nullptr, nullptr, nullptr,
                                                   nullptr, nullptr, nullptr);
  if (rc) return throw_c1(env, rc);
  return out;
}
// encStreamPushMeasuredModesMasked(stream, [Float32Array...], Uint8Array candidates, Int8Array offsets | null, Float64Array floor,
// Float64Array spread | null) -> Uint8Array units: encStreamPushMeasuredModes with every candidate weighed by one masking
// threshold per unit, as encodeMeasuredModesMasked chooses: c1_enc_stream_push_measured_modes_masked
napi_value EncStreamPushMeasuredModesMasked(napi_env env, napi_callback_info info) {
  napi_value argv[6];
  if (!get_args(env, info, 6, argv)) return nullptr;
  c1_enc_stream *s;
  std::vector<float *> ch;
  size_t samples = 0, n_cand = 0, n_off = 0, n_floor = 0, n_spread = 0;
  void *cand = nullptr, *off = nullptr, *floor = nullptr, *spread = nullptr;
  if (!get_external(env, argv[0], &s) || !get_channels(env, argv[1], &ch, &samples)) return nullptr;
  if (!get_typed(env, argv[2], napi_uint8_array, &cand, &n_cand)) return nullptr;
  napi_valuetype t;
  NAPI_OK(napi_typeof(env, argv[3], &t));
  if (t != napi_null && t != napi_undefined && !get_typed(env, argv[3], napi_int8_array, &off, &n_off)) return nullptr;
  if (!get_typed(env, argv[4], napi_float64_array, &floor, &n_floor)) return nullptr;
  NAPI_OK(napi_typeof(env, argv[5], &t));
  if (t != napi_null && t != napi_undefined && !get_typed(env, argv[5], napi_float64_array, &spread, &n_spread)) return nullptr;
  if (n_floor != 52 || (spread && n_spread != 52 * 52)) { napi_throw_type_error(env, nullptr, "masking: floor holds 52 values, spread 52 * 52"); return nullptr; }
  if (samples % 512) { napi_throw_type_error(env, nullptr, "PCM length must be a multiple of 512"); return nullptr; }
  if (n_cand > 64) n_cand = 64;                                 // the library's own checks name the limits
  if (n_off > 64) n_off = 64;
  const int64_t frames = (int64_t)(samples / 512);
  uint8_t *units;
  napi_value out = make_u8(env, (size_t)frames * ch.size() * C1_UNIT_BYTES, &units);
  const float *p[2] = {ch[0], ch.size() > 1 ? ch[1] : nullptr};
  const int rc = c1_enc_stream_push_measured_modes_masked(s, p, frames, static_cast<const uint8_t *>(cand), (int)n_cand,
                                                          static_cast<const int8_t *>(off), off ? (int)n_off : 0,
                                                          static_cast<const double *>(floor), static_cast<const double *>(spread), units,
                                                          nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
  if (rc) return throw_c1(env, rc);
  return out;
}
// encStreamSetOptions(stream, packedOptions): the options of the next push on (c1_enc_stream_set_options)
napi_value EncStreamSetOptions(napi_env env, napi_callback_info info) {
  napi_value argv[2];
  if (!get_args(env, info, 2, argv)) return nullptr;
  c1_enc_stream *s;
  c1_encode_options o;
  if (!get_external(env, argv[0], &s) || !get_options(env, argv[1], &o)) return nullptr;
  const int rc = c1_enc_stream_set_options(s, &o);
  if (rc) return throw_c1(env, rc);
  return nullptr;
}
// Stream state in the reference's BufferPool layout (c1_enc_state / c1_dec_state, include/carta1_hip.h) as one Float32Array of
// channels * 483 (encoder) or channels * 179 (decoder) floats, the fields of each channel back to back; core/buffers.js gives
// them the reference's names.
// encStreamGetState(stream, channels) / decStreamGetState(stream, channels) -> Float32Array
template <typename Stream, typename State, int (*Get)(Stream *, State *)>
napi_value StreamGetState(napi_env env, napi_callback_info info) {
  napi_value argv[2];
  if (!get_args(env, info, 2, argv)) return nullptr;
  Stream *s;
  int32_t channels = 1;
  if (!get_external(env, argv[0], &s)) return nullptr;
  NAPI_OK(napi_get_value_int32(env, argv[1], &channels));
  if (channels < 1 || channels > C1_MAX_CHANNELS) { napi_throw_type_error(env, nullptr, "channels must be 1 or 2"); return nullptr; }
  float *p = nullptr;
  napi_value out = make_f32(env, (size_t)channels * (sizeof(State) / sizeof(float)), &p);
  if (!out || !p) { napi_throw_error(env, nullptr, "could not allocate the result"); return nullptr; }
  const int rc = Get(s, reinterpret_cast<State *>(p));
  if (rc) return throw_c1(env, rc);
  return out;
}
// encStreamSetState(stream, channels, Float32Array) / decStreamSetState(stream, channels, Float32Array)
template <typename Stream, typename State, int (*Set)(Stream *, const State *)>
napi_value StreamSetState(napi_env env, napi_callback_info info) {
  napi_value argv[3];
  if (!get_args(env, info, 3, argv)) return nullptr;
  Stream *s;
  int32_t channels = 1;
  void *d;
  size_t n;
  if (!get_external(env, argv[0], &s)) return nullptr;
  NAPI_OK(napi_get_value_int32(env, argv[1], &channels));
  if (!get_typed(env, argv[2], napi_float32_array, &d, &n)) return nullptr;
  if (channels < 1 || channels > C1_MAX_CHANNELS || n != (size_t)channels * (sizeof(State) / sizeof(float))) {
    napi_throw_type_error(env, nullptr, "state: wrong length");
    return nullptr;
  }
  const int rc = Set(s, static_cast<const State *>(d));
  if (rc) return throw_c1(env, rc);
  return nullptr;
}
napi_value DecStreamCreate(napi_env env, napi_callback_info info) {
  napi_value argv[2];
  if (!get_args(env, info, 2, argv)) return nullptr;
  c1_ctx *ctx;
  int32_t channels = 1;
  if (!get_external(env, argv[0], &ctx)) return nullptr;
  NAPI_OK(napi_get_value_int32(env, argv[1], &channels));
  c1_dec_stream *s = nullptr;
  const int rc = c1_dec_stream_create(ctx, channels, &s);
  if (rc) return throw_c1(env, rc);
  napi_value ext;
  NAPI_OK(napi_create_external(env, s, FinalizeDec, nullptr, &ext));
  napi_ref ref;
  napi_create_reference(env, argv[0], 1, &ref);
  return ext;
}
napi_value DecStreamPush(napi_env env, napi_callback_info info) {
  napi_value argv[3];
  if (!get_args(env, info, 3, argv)) return nullptr;
  c1_dec_stream *s;
  void *d;
  size_t n;
  int32_t channels = 1;
  if (!get_external(env, argv[0], &s) || !get_typed(env, argv[1], napi_uint8_array, &d, &n)) return nullptr;
  NAPI_OK(napi_get_value_int32(env, argv[2], &channels));
  if (channels < 1 || channels > 2 || n % ((size_t)channels * C1_UNIT_BYTES)) { napi_throw_type_error(env, nullptr, "units: wrong length"); return nullptr; }
  const int64_t frames = (int64_t)(n / ((size_t)channels * C1_UNIT_BYTES));
  napi_value arr;
  NAPI_OK(napi_create_array_with_length(env, channels, &arr));
  float *p[2] = {nullptr, nullptr};
  for (int c = 0; c < channels; c++) {
    napi_value ta = make_f32(env, (size_t)frames * 512, &p[c]);
    NAPI_OK(napi_set_element(env, arr, c, ta));
  }
  const int rc = c1_dec_stream_push(s, static_cast<const uint8_t *>(d), frames, p);
  if (rc) return throw_c1(env, rc);
  return arr;
}
// frame fields (Int32Array nbfu, blockModes, sfi, wl, quantized; unit index frame * channels + channel) of whole frames:
// the frame count, or -1 after throwing
int64_t get_fields(napi_env env, const napi_value *argv, int32_t channels, int32_t halo, const int32_t **f, const char *what) {
  void *a[5];
  size_t n[5];
  for (int i = 0; i < 5; i++) if (!get_typed(env, argv[i], napi_int32_array, &a[i], &n[i])) return -1;
  const size_t units = n[0];
  if (channels < 1 || channels > 2 || units % (size_t)channels || n[1] != 3 * units || n[2] != 52 * units || n[3] != 52 * units ||
      n[4] != 512 * units || halo < 0 || (size_t)halo * channels > units) {
    std::string msg = std::string(what) + ": nBfu, 3 block modes, 52 sfi, 52 wl and 512 mantissas per frame and channel";
    napi_throw_type_error(env, nullptr, msg.c_str());
    return -1;
  }
  static const size_t per[5] = {1, 3, 52, 52, 512};
  for (int i = 0; i < 5; i++) f[i] = static_cast<const int32_t *>(a[i]) + per[i] * (size_t)halo * channels;
  return (int64_t)(units / channels) - halo;
}
napi_value pcm_array(napi_env env, int32_t channels, int64_t frames, float **p) {
  napi_value arr;
  if (napi_create_array_with_length(env, channels, &arr) != napi_ok) return nullptr;
  for (int c = 0; c < channels; c++) {
    napi_value ta = make_f32(env, (size_t)frames * 512, &p[c]);
    if (!ta || napi_set_element(env, arr, c, ta) != napi_ok) return nullptr;
  }
  return arr;
}
// (ctx, Int32Array nbfu, blockModes, sfi, wl, quantized, channels, haloFrames) -> [Float32Array pcm per channel]
napi_value DecodeFieldsBatch(napi_env env, napi_callback_info info) {
  napi_value argv[8];
  if (!get_args(env, info, 8, argv)) return nullptr;
  c1_ctx *ctx;
  int32_t channels = 1, halo = 0;
  if (!get_external(env, argv[0], &ctx)) return nullptr;
  NAPI_OK(napi_get_value_int32(env, argv[6], &channels));
  NAPI_OK(napi_get_value_int32(env, argv[7], &halo));
  const int32_t *f[5];
  const int64_t frames = get_fields(env, argv + 1, channels, halo, f, "decodeFieldsBatch");
  if (frames < 0) return nullptr;
  float *p[2] = {nullptr, nullptr};
  napi_value arr = pcm_array(env, channels, frames, p);
  if (!arr) { napi_throw_error(env, nullptr, "allocation failed"); return nullptr; }
  const int rc = c1_decode_fields_batch(ctx, channels, frames, halo, f[0], f[1], f[2], f[3], f[4], p);
  if (rc) return throw_c1(env, rc);
  return arr;
}
// (stream, Int32Array nbfu, blockModes, sfi, wl, quantized, channels) -> [Float32Array pcm per channel]
napi_value DecStreamPushFields(napi_env env, napi_callback_info info) {
  napi_value argv[7];
  if (!get_args(env, info, 7, argv)) return nullptr;
  c1_dec_stream *s;
  int32_t channels = 1;
  if (!get_external(env, argv[0], &s)) return nullptr;
  NAPI_OK(napi_get_value_int32(env, argv[6], &channels));
  const int32_t *f[5];
  const int64_t frames = get_fields(env, argv + 1, channels, 0, f, "decStreamPushFields");
  if (frames < 0) return nullptr;
  float *p[2] = {nullptr, nullptr};
  napi_value arr = pcm_array(env, channels, frames, p);
  if (!arr) { napi_throw_error(env, nullptr, "allocation failed"); return nullptr; }
  const int rc = c1_dec_stream_push_fields(s, frames, f[0], f[1], f[2], f[3], f[4], p);
  if (rc) return throw_c1(env, rc);
  return arr;
}

// ---- the single-stage functions of the reference's export surface (codec/index.js:30-35,42) ---------------------------
napi_value Quantize(napi_env env, napi_callback_info info) {      // (ctx, Float32Array, sfi, bits) -> Int32Array
  napi_value argv[4];
  if (!get_args(env, info, 4, argv)) return nullptr;
  c1_ctx *ctx; void *d; size_t n; int32_t sfi = 0, bits = 0;
  if (!get_external(env, argv[0], &ctx) || !get_typed(env, argv[1], napi_float32_array, &d, &n)) return nullptr;
  NAPI_OK(napi_get_value_int32(env, argv[2], &sfi));
  NAPI_OK(napi_get_value_int32(env, argv[3], &bits));
  napi_value ab, ta; void *q;
  NAPI_OK(napi_create_arraybuffer(env, n * 4, &q, &ab));
  NAPI_OK(napi_create_typedarray(env, napi_int32_array, n, ab, 0, &ta));
  const int rc = c1_quantize(ctx, static_cast<const float *>(d), (int)n, sfi, bits, static_cast<int32_t *>(q));
  if (rc) return throw_c1(env, rc);
  return ta;
}
napi_value Dequantize(napi_env env, napi_callback_info info) {    // (ctx, Int32Array, sfi, bits) -> Float32Array
  napi_value argv[4];
  if (!get_args(env, info, 4, argv)) return nullptr;
  c1_ctx *ctx; void *d; size_t n; int32_t sfi = 0, bits = 0;
  if (!get_external(env, argv[0], &ctx) || !get_typed(env, argv[1], napi_int32_array, &d, &n)) return nullptr;
  NAPI_OK(napi_get_value_int32(env, argv[2], &sfi));
  NAPI_OK(napi_get_value_int32(env, argv[3], &bits));
  float *x;
  napi_value out = make_f32(env, n, &x);
  const int rc = c1_dequantize(ctx, static_cast<const int32_t *>(d), (int)n, sfi, bits, x);
  if (rc) return throw_c1(env, rc);
  return out;
}
napi_value Fft(napi_env env, napi_callback_info info) {           // (ctx, real, imag, Float64Array w) in place
  napi_value argv[4];
  if (!get_args(env, info, 4, argv)) return nullptr;
  c1_ctx *ctx; void *re, *im, *w; size_t n, n2, nw;
  if (!get_external(env, argv[0], &ctx) || !get_typed(env, argv[1], napi_float32_array, &re, &n) ||
      !get_typed(env, argv[2], napi_float32_array, &im, &n2) || !get_typed(env, argv[3], napi_float64_array, &w, &nw)) return nullptr;
  size_t stages = 0;
  while (((size_t)1 << stages) < n) stages++;
  if (n2 != n || nw < 2 * stages) { napi_throw_type_error(env, nullptr, "fft: real, imag of equal length and log2(n) twiddle pairs"); return nullptr; }
  const int rc = c1_fft(ctx, static_cast<float *>(re), static_cast<float *>(im), (int)n, static_cast<const double *>(w));
  if (rc) return throw_c1(env, rc);
  napi_value undef;
  napi_get_undefined(env, &undef);
  return undef;
}
napi_value QmfAnalysis(napi_env env, napi_callback_info info) {   // (ctx, Float32Array pcm incl. halo, haloFrames) -> Float32Array bands
  napi_value argv[3];
  if (!get_args(env, info, 3, argv)) return nullptr;
  c1_ctx *ctx; void *d; size_t n; int32_t halo = 0;
  if (!get_external(env, argv[0], &ctx) || !get_typed(env, argv[1], napi_float32_array, &d, &n)) return nullptr;
  NAPI_OK(napi_get_value_int32(env, argv[2], &halo));
  if (n % 512 || halo < 0 || (size_t)halo > n / 512) { napi_throw_type_error(env, nullptr, "qmfAnalysis: whole frames of 512 samples"); return nullptr; }
  const int64_t frames = (int64_t)(n / 512) - halo;
  float *b;
  napi_value out = make_f32(env, (size_t)frames * 512, &b);
  const int rc = c1_qmf_analysis_batch(ctx, static_cast<const float *>(d), frames, halo, b);
  if (rc) return throw_c1(env, rc);
  return out;
}
napi_value MdctFromBands(napi_env env, napi_callback_info info) { // (ctx, Float32Array bands incl. halo, haloFrames, Int32Array modes) -> [coefs, bandsWindowed]
  napi_value argv[4];
  if (!get_args(env, info, 4, argv)) return nullptr;
  c1_ctx *ctx; void *d, *m; size_t n, nm; int32_t halo = 0;
  if (!get_external(env, argv[0], &ctx) || !get_typed(env, argv[1], napi_float32_array, &d, &n)) return nullptr;
  NAPI_OK(napi_get_value_int32(env, argv[2], &halo));
  if (!get_typed(env, argv[3], napi_int32_array, &m, &nm)) return nullptr;
  if (n % 512 || halo < 0 || halo > 1 || (size_t)halo > n / 512 || nm != 3 * (n / 512 - (size_t)halo)) { napi_throw_type_error(env, nullptr, "mdctFromBands: whole frames and three block modes per frame"); return nullptr; }
  const int64_t frames = (int64_t)(n / 512) - halo;
  float *c, *bw;
  napi_value coefs = make_f32(env, (size_t)frames * 512, &c), windowed = make_f32(env, (size_t)frames * 512, &bw), arr;
  const int rc = c1_mdct_batch(ctx, static_cast<const float *>(d), frames, halo, static_cast<const int32_t *>(m), c, bw);
  if (rc) return throw_c1(env, rc);
  NAPI_OK(napi_create_array_with_length(env, 2, &arr));
  NAPI_OK(napi_set_element(env, arr, 0, coefs));
  NAPI_OK(napi_set_element(env, arr, 1, windowed));
  return arr;
}

// the decoder's pipeline stages, one channel (c1_unpack_units, c1_dequantize_frames, c1_imdct_batch, c1_qmf_synthesis_batch)
napi_value UnpackUnits(napi_env env, napi_callback_info info) {   // (ctx, Uint8Array units) -> [nbfu, blockModes, sfi, wl, quantized] Int32Arrays
  napi_value argv[2];
  if (!get_args(env, info, 2, argv)) return nullptr;
  c1_ctx *ctx; void *u; size_t n;
  if (!get_external(env, argv[0], &ctx) || !get_typed(env, argv[1], napi_uint8_array, &u, &n)) return nullptr;
  if (n % C1_UNIT_BYTES) { napi_throw_type_error(env, nullptr, "unpackUnits: whole units of 212 bytes"); return nullptr; }
  const size_t frames = n / C1_UNIT_BYTES, per[5] = {1, 3, 52, 52, 512};
  napi_value arr, out[5];
  void *p[5];
  for (int i = 0; i < 5; i++) {
    napi_value ab;
    NAPI_OK(napi_create_arraybuffer(env, frames * per[i] * 4 + 4, &p[i], &ab));
    NAPI_OK(napi_create_typedarray(env, napi_int32_array, frames * per[i], ab, 0, &out[i]));
  }
  const int rc = c1_unpack_units(ctx, static_cast<const uint8_t *>(u), (int64_t)frames, static_cast<int32_t *>(p[0]), static_cast<int32_t *>(p[1]),
                                 static_cast<int32_t *>(p[2]), static_cast<int32_t *>(p[3]), static_cast<int32_t *>(p[4]));
  if (rc) return throw_c1(env, rc);
  NAPI_OK(napi_create_array_with_length(env, 5, &arr));
  for (int i = 0; i < 5; i++) NAPI_OK(napi_set_element(env, arr, i, out[i]));
  return arr;
}
napi_value SelectBlockModes(napi_env env, napi_callback_info info) {  // (ctx, Float32Array bands incl. halo, haloFrames, threshold) -> Int32Array modes
  napi_value argv[4];
  if (!get_args(env, info, 4, argv)) return nullptr;
  c1_ctx *ctx; void *d; size_t n; int32_t halo = 0; double threshold = 0;
  if (!get_external(env, argv[0], &ctx) || !get_typed(env, argv[1], napi_float32_array, &d, &n)) return nullptr;
  NAPI_OK(napi_get_value_int32(env, argv[2], &halo));
  NAPI_OK(napi_get_value_double(env, argv[3], &threshold));
  if (n % 512 || halo < 0 || halo > 1 || (size_t)halo > n / 512) { napi_throw_type_error(env, nullptr, "selectBlockModes: whole frames of 512 band samples, halo 0 or 1"); return nullptr; }
  const int64_t frames = (int64_t)(n / 512) - halo;
  napi_value ab, out;
  void *m;
  NAPI_OK(napi_create_arraybuffer(env, (size_t)frames * 3 * 4 + 4, &m, &ab));
  NAPI_OK(napi_create_typedarray(env, napi_int32_array, (size_t)frames * 3, ab, 0, &out));
  const int rc = c1_select_block_modes(ctx, static_cast<const float *>(d), frames, halo, threshold, static_cast<int32_t *>(m));
  if (rc) return throw_c1(env, rc);
  return out;
}
napi_value QuantizeFrames(napi_env env, napi_callback_info info) {  // (ctx, Float32Array coefs, Int32Array modes, Float64Array(68) options) -> {nbfu, sfi, wl, quantized}
  napi_value argv[4];
  if (!get_args(env, info, 4, argv)) return nullptr;
  c1_ctx *ctx; void *c, *m; size_t n, nm;
  if (!get_external(env, argv[0], &ctx) || !get_typed(env, argv[1], napi_float32_array, &c, &n) ||
      !get_typed(env, argv[2], napi_int32_array, &m, &nm)) return nullptr;
  c1_encode_options o;
  if (!get_options(env, argv[3], &o)) return nullptr;
  if (n % 512 || nm != 3 * (n / 512)) { napi_throw_type_error(env, nullptr, "quantizeFrames: whole frames of 512 coefficients and three block modes per frame"); return nullptr; }
  const size_t frames = n / 512, per[4] = {1, 52, 52, 512};
  static const char *const names[4] = {"nbfu", "sfi", "wl", "quantized"};
  napi_value obj, out[4];
  void *p[4];
  for (int i = 0; i < 4; i++) {
    napi_value ab;
    NAPI_OK(napi_create_arraybuffer(env, frames * per[i] * 4 + 4, &p[i], &ab));
    NAPI_OK(napi_create_typedarray(env, napi_int32_array, frames * per[i], ab, 0, &out[i]));
  }
  const int rc = c1_quantize_frames(ctx, static_cast<const float *>(c), (int64_t)frames, static_cast<const int32_t *>(m), &o,
                                    static_cast<int32_t *>(p[0]), static_cast<int32_t *>(p[1]), static_cast<int32_t *>(p[2]),
                                    static_cast<int32_t *>(p[3]));
  if (rc) return throw_c1(env, rc);
  NAPI_OK(napi_create_object(env, &obj));
  for (int i = 0; i < 4; i++) NAPI_OK(napi_set_named_property(env, obj, names[i], out[i]));
  return obj;
}
napi_value PackUnits(napi_env env, napi_callback_info info) {  // (ctx, Int32Array nbfu, blockModes, sfi, wl, quantized) -> Uint8Array units
  napi_value argv[6];
  if (!get_args(env, info, 6, argv)) return nullptr;
  c1_ctx *ctx; void *a[5]; size_t n[5];
  if (!get_external(env, argv[0], &ctx)) return nullptr;
  for (int i = 0; i < 5; i++) if (!get_typed(env, argv[1 + i], napi_int32_array, &a[i], &n[i])) return nullptr;
  const size_t frames = n[0];
  if (n[1] != 3 * frames || n[2] != 52 * frames || n[3] != 52 * frames || n[4] != 512 * frames) {
    napi_throw_type_error(env, nullptr, "packUnits: nBfu, 3 block modes, 52 sfi, 52 wl and 512 mantissas per frame");
    return nullptr;
  }
  napi_value ab, out;
  void *u;
  NAPI_OK(napi_create_arraybuffer(env, frames * C1_UNIT_BYTES + 4, &u, &ab));
  NAPI_OK(napi_create_typedarray(env, napi_uint8_array, frames * C1_UNIT_BYTES, ab, 0, &out));
  const int rc = c1_pack_units(ctx, (int64_t)frames, static_cast<const int32_t *>(a[0]), static_cast<const int32_t *>(a[1]),
                               static_cast<const int32_t *>(a[2]), static_cast<const int32_t *>(a[3]), static_cast<const int32_t *>(a[4]),
                               static_cast<uint8_t *>(u));
  if (rc) return throw_c1(env, rc);
  return out;
}
napi_value DequantizeFrames(napi_env env, napi_callback_info info) {  // (ctx, Int32Array nbfu, blockModes, sfi, wl, quantized) -> Float32Array coefs
  napi_value argv[6];
  if (!get_args(env, info, 6, argv)) return nullptr;
  c1_ctx *ctx; void *a[5]; size_t n[5];
  if (!get_external(env, argv[0], &ctx)) return nullptr;
  for (int i = 0; i < 5; i++) if (!get_typed(env, argv[1 + i], napi_int32_array, &a[i], &n[i])) return nullptr;
  const size_t frames = n[0];
  if (n[1] != 3 * frames || n[2] != 52 * frames || n[3] != 52 * frames || n[4] != 512 * frames) {
    napi_throw_type_error(env, nullptr, "dequantizeFrames: nBfu, 3 block modes, 52 sfi, 52 wl and 512 mantissas per frame");
    return nullptr;
  }
  float *c;
  napi_value out = make_f32(env, frames * 512, &c);
  const int rc = c1_dequantize_frames(ctx, (int64_t)frames, static_cast<const int32_t *>(a[0]), static_cast<const int32_t *>(a[1]),
                                      static_cast<const int32_t *>(a[2]), static_cast<const int32_t *>(a[3]), static_cast<const int32_t *>(a[4]), c);
  if (rc) return throw_c1(env, rc);
  return out;
}
napi_value Imdct(napi_env env, napi_callback_info info) {  // (ctx, Float32Array coefs incl. halo, haloFrames, Int32Array modes incl. halo) -> Float32Array bands
  napi_value argv[4];
  if (!get_args(env, info, 4, argv)) return nullptr;
  c1_ctx *ctx; void *d, *m; size_t n, nm; int32_t halo = 0;
  if (!get_external(env, argv[0], &ctx) || !get_typed(env, argv[1], napi_float32_array, &d, &n)) return nullptr;
  NAPI_OK(napi_get_value_int32(env, argv[2], &halo));
  if (!get_typed(env, argv[3], napi_int32_array, &m, &nm)) return nullptr;
  if (n % 512 || halo < 0 || (size_t)halo > n / 512 || nm != 3 * (n / 512)) { napi_throw_type_error(env, nullptr, "imdct: whole frames and three block modes per frame"); return nullptr; }
  const int64_t frames = (int64_t)(n / 512) - halo;
  float *b;
  napi_value out = make_f32(env, (size_t)frames * 512, &b);
  const int rc = c1_imdct_batch(ctx, static_cast<const float *>(d), frames, halo, static_cast<const int32_t *>(m), b);
  if (rc) return throw_c1(env, rc);
  return out;
}
napi_value QmfSynthesis(napi_env env, napi_callback_info info) {  // (ctx, Float32Array bands incl. halo, haloFrames) -> Float32Array pcm
  napi_value argv[3];
  if (!get_args(env, info, 3, argv)) return nullptr;
  c1_ctx *ctx; void *d; size_t n; int32_t halo = 0;
  if (!get_external(env, argv[0], &ctx) || !get_typed(env, argv[1], napi_float32_array, &d, &n)) return nullptr;
  NAPI_OK(napi_get_value_int32(env, argv[2], &halo));
  if (n % 512 || halo < 0 || (size_t)halo > n / 512) { napi_throw_type_error(env, nullptr, "qmfSynthesis: whole frames of 512 samples"); return nullptr; }
  const int64_t frames = (int64_t)(n / 512) - halo;
  float *p;
  napi_value out = make_f32(env, (size_t)frames * 512, &p);
  const int rc = c1_qmf_synthesis_batch(ctx, static_cast<const float *>(d), frames, halo, p);
  if (rc) return throw_c1(env, rc);
  return out;
}

// ---- the decision functions of analysis/transient.js and coding/bitallocation.js, one problem per call ----
napi_value PerformFft(napi_env env, napi_callback_info info) {    // (ctx, Float64Array samples, fftSize, Float64Array w) -> Float32Array(fftSize / 2)
  napi_value argv[4];
  if (!get_args(env, info, 4, argv)) return nullptr;
  c1_ctx *ctx; void *x, *w; size_t n, nw; int32_t size = 0;
  if (!get_external(env, argv[0], &ctx) || !get_typed(env, argv[1], napi_float64_array, &x, &n) ||
      !get_typed(env, argv[3], napi_float64_array, &w, &nw)) return nullptr;
  NAPI_OK(napi_get_value_int32(env, argv[2], &size));
  size_t stages = 0;
  while (size > 0 && ((size_t)1 << stages) < (size_t)size) stages++;
  if (nw < 2 * stages) { napi_throw_type_error(env, nullptr, "performFFT: log2(fftSize) twiddle pairs"); return nullptr; }
  const int64_t off[2] = {0, (int64_t)n};
  float *mag;
  napi_value out = make_f32(env, size > 1 ? (size_t)size / 2 : 0, &mag);
  const int rc = c1_perform_fft(ctx, static_cast<const double *>(x), off, 1, size, static_cast<const double *>(w), mag);
  if (rc) return throw_c1(env, rc);
  return out;
}
napi_value DetectTransient(napi_env env, napi_callback_info info) {  // (ctx, Float64Array cur, Float64Array prev, threshold) -> [transient, score]
  napi_value argv[4];
  if (!get_args(env, info, 4, argv)) return nullptr;
  c1_ctx *ctx; void *c, *p; size_t nc, np; double thr = 0;
  if (!get_external(env, argv[0], &ctx) || !get_typed(env, argv[1], napi_float64_array, &c, &nc) ||
      !get_typed(env, argv[2], napi_float64_array, &p, &np)) return nullptr;
  NAPI_OK(napi_get_value_double(env, argv[3], &thr));
  const int64_t co[2] = {0, (int64_t)nc}, po[2] = {0, (int64_t)np};
  uint8_t flag = 0;
  double score = 0;
  const int rc = c1_detect_transients(ctx, static_cast<const double *>(c), co, static_cast<const double *>(p), po, nullptr, &thr, 1, &flag, &score);
  if (rc) return throw_c1(env, rc);
  napi_value arr, b, sc;
  NAPI_OK(napi_create_array_with_length(env, 2, &arr));
  NAPI_OK(napi_get_boolean(env, flag != 0, &b));
  NAPI_OK(napi_create_double(env, score, &sc));
  NAPI_OK(napi_set_element(env, arr, 0, b));
  NAPI_OK(napi_set_element(env, arr, 1, sc));
  return arr;
}
napi_value FindScaleFactor(napi_env env, napi_callback_info info) {  // (ctx, Float64Array values, length as a double integer) -> number
  napi_value argv[3];
  if (!get_args(env, info, 3, argv)) return nullptr;
  c1_ctx *ctx; void *v; size_t n; int64_t len = 0;
  if (!get_external(env, argv[0], &ctx) || !get_typed(env, argv[1], napi_float64_array, &v, &n)) return nullptr;
  NAPI_OK(napi_get_value_int64(env, argv[2], &len));
  const int64_t off[2] = {0, (int64_t)n};
  int32_t idx = 0;
  const int rc = c1_find_scale_factors(ctx, static_cast<const double *>(v), off, &len, 1, &idx);
  if (rc) return throw_c1(env, rc);
  napi_value r;
  NAPI_OK(napi_create_int32(env, idx, &r));
  return r;
}
// (ctx, Float64Array data, Int32Array offsets[52], Int32Array lengths[52], Int32Array sizes[52], maxBfuCount, Float64Array(64) table)
//   -> [bfuCount, Int32Array allocation(52), Int32Array scaleFactorIndices(52), fallback]
napi_value AllocateBits(napi_env env, napi_callback_info info) {
  napi_value argv[7];
  if (!get_args(env, info, 7, argv)) return nullptr;
  c1_ctx *ctx; void *d, *o, *l, *z, *t; size_t nd, no, nl, nz, nt; int32_t mb = 0;
  if (!get_external(env, argv[0], &ctx) || !get_typed(env, argv[1], napi_float64_array, &d, &nd) ||
      !get_typed(env, argv[2], napi_int32_array, &o, &no) || !get_typed(env, argv[3], napi_int32_array, &l, &nl) ||
      !get_typed(env, argv[4], napi_int32_array, &z, &nz) || !get_typed(env, argv[6], napi_float64_array, &t, &nt)) return nullptr;
  NAPI_OK(napi_get_value_int32(env, argv[5], &mb));
  if (no != 52 || nl != 52 || nz != 52 || nt != 64) { napi_throw_type_error(env, nullptr, "allocateBits: 52 offsets, lengths and sizes and a 64-entry table"); return nullptr; }
  int64_t off[52];
  for (int i = 0; i < 52; i++) off[i] = static_cast<const int32_t *>(o)[i];
  napi_value arr, ab, wl, sf, cnt, fb;
  void *pw, *ps;
  NAPI_OK(napi_create_arraybuffer(env, 52 * 4, &pw, &ab));
  NAPI_OK(napi_create_typedarray(env, napi_int32_array, 52, ab, 0, &wl));
  NAPI_OK(napi_create_arraybuffer(env, 52 * 4, &ps, &ab));
  NAPI_OK(napi_create_typedarray(env, napi_int32_array, 52, ab, 0, &sf));
  int32_t count = 0;
  uint8_t fallback = 0;
  const int rc = c1_allocate_bits(ctx, static_cast<const double *>(d), (int64_t)nd, off, static_cast<const int32_t *>(l),
                                  static_cast<const int32_t *>(z), &mb, 1, static_cast<const double *>(t), &count,
                                  static_cast<int32_t *>(pw), static_cast<int32_t *>(ps), &fallback);
  if (rc) return throw_c1(env, rc);
  NAPI_OK(napi_create_array_with_length(env, 4, &arr));
  NAPI_OK(napi_create_int32(env, count, &cnt));
  NAPI_OK(napi_get_boolean(env, fallback != 0, &fb));
  NAPI_OK(napi_set_element(env, arr, 0, cnt));
  NAPI_OK(napi_set_element(env, arr, 1, wl));
  NAPI_OK(napi_set_element(env, arr, 2, sf));
  NAPI_OK(napi_set_element(env, arr, 3, fb));
  return arr;
}
napi_value Init(napi_env env, napi_value exports) {
  const napi_property_descriptor props[] = {
      {"abiVersion", nullptr, AbiVersion, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"deviceCount", nullptr, DeviceCount, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"getDefaultTables", nullptr, GetDefaultTables, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"setTables", nullptr, SetTables, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"ctxCreate", nullptr, CtxCreate, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"ctxSetDecodeModel", nullptr, CtxSetDecodeModel, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"allocPinned", nullptr, AllocPinned, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"encodeBatch", nullptr, EncodeBatch, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"encodeBatchModes", nullptr, EncodeBatchModes, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"encodeBatchBiases", nullptr, EncodeBatchBiases, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"encodeBestBias", nullptr, EncodeBestBias, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"encodeBestModes", nullptr, EncodeBestModes, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"encodeMeasured", nullptr, EncodeMeasured, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"encodeMeasuredSf", nullptr, EncodeMeasuredSf, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"encodeMeasuredModes", nullptr, EncodeMeasuredModes, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"encodeMeasuredModesMasked", nullptr, EncodeMeasuredModesMasked, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"encodeMeasuredMasked", nullptr, EncodeMeasuredMasked, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"measureUnits", nullptr, MeasureUnits, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"measureUnitsShared", nullptr, MeasureUnitsShared, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"measurePcm", nullptr, MeasurePcm, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"decodeBatch", nullptr, DecodeBatch, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"encodeWavBatch", nullptr, EncodeWavBatch, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"decodeWav16Batch", nullptr, DecodeWav16Batch, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"encodeBatchAsync", nullptr, EncodeBatchAsync, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"decodeBatchAsync", nullptr, DecodeBatchAsync, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"encodeSignals", nullptr, EncodeSignals, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"encodeSignalsMeasured", nullptr, EncodeSignalsMeasured, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"encodeSignalsMeasuredModes", nullptr, EncodeSignalsMeasuredModes, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"decodeSignals", nullptr, DecodeSignals, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"encStreamCreate", nullptr, EncStreamCreate, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"encStreamPush", nullptr, EncStreamPush, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"encStreamPushMeasured", nullptr, EncStreamPushMeasured, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"encStreamPushMeasuredModes", nullptr, EncStreamPushMeasuredModes, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"encStreamPushMeasuredModesMasked", nullptr, EncStreamPushMeasuredModesMasked, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"encStreamSetOptions", nullptr, EncStreamSetOptions, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"encStreamGetState", nullptr, StreamGetState<c1_enc_stream, c1_enc_state, c1_enc_stream_get_state>, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"encStreamSetState", nullptr, StreamSetState<c1_enc_stream, c1_enc_state, c1_enc_stream_set_state>, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"decStreamGetState", nullptr, StreamGetState<c1_dec_stream, c1_dec_state, c1_dec_stream_get_state>, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"decStreamSetState", nullptr, StreamSetState<c1_dec_stream, c1_dec_state, c1_dec_stream_set_state>, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"decStreamCreate", nullptr, DecStreamCreate, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"decStreamPush", nullptr, DecStreamPush, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"decStreamPushFields", nullptr, DecStreamPushFields, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"decodeFieldsBatch", nullptr, DecodeFieldsBatch, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"quantize", nullptr, Quantize, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"dequantize", nullptr, Dequantize, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"fft", nullptr, Fft, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"qmfAnalysis", nullptr, QmfAnalysis, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"mdctFromBands", nullptr, MdctFromBands, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"selectBlockModes", nullptr, SelectBlockModes, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"quantizeFrames", nullptr, QuantizeFrames, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"unpackUnits", nullptr, UnpackUnits, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"dequantizeFrames", nullptr, DequantizeFrames, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"packUnits", nullptr, PackUnits, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"imdct", nullptr, Imdct, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"qmfSynthesis", nullptr, QmfSynthesis, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"performFFT", nullptr, PerformFft, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"detectTransient", nullptr, DetectTransient, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"findScaleFactor", nullptr, FindScaleFactor, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"allocateBits", nullptr, AllocateBits, nullptr, nullptr, nullptr, napi_default, nullptr},
  };
  napi_define_properties(env, exports, sizeof props / sizeof props[0], props);
  return exports;
}

}  // namespace

NAPI_MODULE(NODE_GYP_MODULE_NAME, Init)
