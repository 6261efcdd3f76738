"""Host-side mirror (Python) of the reference interface around the hot path.

Mirrors, with the same names / argument meaning / error behaviour:
  EncoderOptions            codec/core/options.js:11-164
  encode_aea_pcm            encodeAeaPcm   codec/io/processor.js:597-617
  decode_aea_pcm            decodeAeaPcm   codec/io/processor.js:628-654
  EncoderStream / DecoderStream   one encode()/decode() closure + its BufferPool
                            (codec/pipeline/encoder.js:438-450, decoder.js:408-411)
  serialize_frame / deserialize_frame   codec/io/serialization.js:41-176 (host-side format code)
All arithmetic of the hot path runs on the GPU through libcarta1_hip.so (carta1_amd/capi.py); there
is no CPU fallback.  The JavaScript host with the reference's exact API is carta1_amd/js.
"""
import ctypes as C
import math
import struct

import numpy as np

from . import capi

AEA_HEADER_SIZE = 2048          # codec/core/constants.js:12-16
AEA_MAGIC = bytes([0x00, 0x08, 0x00, 0x00])
AEA_TITLE_OFFSET, AEA_TITLE_SIZE = 4, 256
AEA_FRAME_COUNT_OFFSET, AEA_CHANNEL_COUNT_OFFSET = 260, 264
BFU_AMOUNTS = (20, 28, 32, 36, 40, 44, 48, 52)
SPECS_PER_BFU = (8, 8, 8, 8, 4, 4, 4, 4, 8, 8, 8, 8, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6, 7, 7, 7, 7, 9, 9, 9, 9,
                 10, 10, 10, 10, 12, 12, 12, 12, 12, 12, 12, 12, 20, 20, 20, 20, 20, 20, 20, 20)
WORD_LENGTH_BITS = (0, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16)


_BIASED = None


def packaged_biased_table(bias):
    """pow(SCALE_FACTORS, bias) as V8 computed it, for the biases carta1_amd/biased_tables.json holds; else None"""
    global _BIASED
    if _BIASED is None:
        import json
        import os
        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'biased_tables.json')
        raw = json.load(open(path))['biased_scale_factors_f64']
        _BIASED = {float(k): [struct.unpack('>d', bytes.fromhex(h))[0] for h in v] for k, v in raw.items()}
    return _BIASED.get(float(bias))


class EncoderOptions:
    """codec/core/options.js: same keys, defaults, ranges and error messages."""
    _RANGES = {'transientThresholdLow': (0.01, 2), 'transientThresholdMid': (0.01, 3),
               'transientThresholdHigh': (0.01, 4), 'allocationBias': (0.0, 5.0)}

    def __init__(self, options=None, biased_table=None):
        self.values = {'transientThresholdLow': 1.0, 'transientThresholdMid': 1.5, 'transientThresholdHigh': 2.0,
                       'allocationBias': 1.0, 'fixedBlockModes': None}
        self.biased_table = biased_table   # optional explicit pow(SCALE_FACTORS, bias) table (64 doubles)
        for k, v in (options or {}).items():
            if k in self.values:
                self.set_value(k, v)

    def set_value(self, key, value):
        if key not in self.values:
            raise ValueError('Unknown option: %s' % key)
        if key in self._RANGES:
            lo, hi = self._RANGES[key]
            if value < lo or value > hi:
                raise ValueError('Value for %s must be between %s and %s, got %s' % (key, lo, hi, value))
        self.values[key] = value

    def __getattr__(self, name):
        vals = self.__dict__.get('values', {})
        if name in vals:
            return vals[name]
        raise AttributeError(name)

    def to_c(self):
        """c1_encode_options.  The biased table is pow(SCALE_FACTORS[i], bias) (bitallocation.js:46-61) as the
        reference's engine computes it; Math.pow is not correctly rounded and differs between engines, so
        the package carries the tables V8 produced for the biases 0, 0.25, 0.5, 1, 1.5, 2, 3.3 and 5
        (carta1_amd/biased_tables.json, generated from the golden vectors).  Any other bias falls back to libm's pow,
        whose last bit may differ from V8's ("parity unpinned" for those) -- pass biased_table to pin it; the JavaScript
        host always uses its own engine's Math.pow.  Bias 1 is SCALE_FACTORS itself (bitallocation.js:51-53): the table
        installed with c1_set_tables at the time to_c() runs, which c1_default_encode_options copies.  A context keeps the
        tables it was created with (its quantization norms, window, transforms), so for a context created before a later
        c1_set_tables, pass biased_table= its own SCALE_FACTORS (c1_get_default_tables, or the table installed then);
        otherwise its allocation would weigh with the newer engine's table."""
        o = capi.EncodeOptions()
        capi.check(capi.load().c1_default_encode_options(C.byref(o)))
        bias = float(self.values['allocationBias'])
        table = self.biased_table
        if table is None and bias != 1.0:
            table = packaged_biased_table(bias)
        if table is not None:
            for i in range(64):
                o.biased_scale_factors[i] = float(table[i])
        elif bias != 1.0:
            sf = [o.biased_scale_factors[i] for i in range(64)]
            for i in range(64):
                o.biased_scale_factors[i] = math.pow(sf[i], bias)
        o.transient_threshold = float(self.values['transientThresholdLow'])   # encoder.js:137-141
        fm = self.values['fixedBlockModes']
        if fm is not None and len(fm) != 3:
            raise ValueError('fixedBlockModes must have 3 entries, got %d' % len(fm))
        for b in range(3):
            o.fixed_block_modes[b] = int(fm[b]) if fm is not None else -1
        return o


class Context:
    """One c1_ctx: a device, a stream, tables and workspace on it."""

    def __init__(self, device=0, stream=None):
        """stream: a hipStream_t as an integer (torch: `torch.cuda.Stream().cuda_stream`), or None for a stream of the
        context's own.  On a caller's stream every *_device call is ordered like a kernel launch on it: after everything
        queued before it, and finished with every buffer, inputs included, for everything queued after it.  The library
        never destroys that stream (close() waits for the context's work on it), and several contexts may share one.
        The trap: a zero handle means "own stream", and torch's legacy default stream has the handle 0, so
        `Context(0, stream=torch.cuda.current_stream().cuda_stream)` outside a `torch.cuda.stream(...)` block gives a
        context whose work is NOT ordered with the default stream's; synchronise by hand or use a stream of your own."""
        self._h = C.c_void_p()
        capi.check(capi.load().c1_ctx_create(int(device), C.c_void_p(stream) if stream else None, C.byref(self._h)))
        self.device = device

    def close(self):
        if self._h:
            capi.load().c1_ctx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def synchronize(self):
        capi.check(capi.load().c1_ctx_synchronize(self._h))

    def set_profiling(self, on):
        capi.check(capi.load().c1_ctx_set_profiling(self._h, 1 if on else 0))

    def kernel_ms(self, name):
        ms, n = C.c_double(0), C.c_int(0)
        capi.check(capi.load().c1_ctx_kernel_ms(self._h, name.encode(), C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def set_speculation(self, mode):
        """0 = exact kernels only, 1 = material-local (default: runs the predictor rejects go to the exact kernels),
        2 = always speculate (include/carta1_hip.h)."""
        capi.check(capi.load().c1_ctx_set_speculation(self._h, int(mode)))

    def set_decode_precision(self, binary32):
        """False (default): bit-identical to the reference; True: binary32 arithmetic, PCM within rounding noise."""
        capi.check(capi.load().c1_ctx_set_decode_precision(self._h, 1 if binary32 else 0))

    def set_decode_model(self, model):
        """DECODE_EXACT (0, default): bit-identical to the reference on every entry.  DECODE_BINARY32_BULK (1): what
        set_decode_precision(True) selects: the unit-walking kernel in binary32, everything decoded from frame fields or
        from decoder states exact.  DECODE_BINARY32 (2): every decode entry of the context, DecoderStream included, in
        that kernel's binary32 arithmetic: the same units give the same bits through any of them."""
        capi.check(capi.load().c1_ctx_set_decode_model(self._h, int(model)))

    @property
    def decode_model(self):
        m = C.c_int(0)
        capi.check(capi.load().c1_ctx_get_decode_model(self._h, C.byref(m)))
        return m.value

    def speculation_stats(self, reset=False):
        """(units encoded through the speculative pass, units among them redone by the exact kernels)."""
        u, r = C.c_uint64(0), C.c_uint64(0)
        capi.check(capi.load().c1_ctx_speculation_stats(self._h, C.byref(u), C.byref(r), 1 if reset else 0))
        return u.value, r.value

    def speculation_deferred(self):
        """units whose runs the speculative analysis handed to the exact kernels (material-local mode)"""
        u = C.c_uint64(0)
        capi.check(capi.load().c1_ctx_speculation_deferred(self._h, C.byref(u)))
        return int(u.value)

    # ---- host-resident batches ------------------------------------------------------------------
    def quantization_stats(self):
        """(units whose exact coefficients were quantized in binary32 with the guard band, units packed again in binary64)"""
        u, r = C.c_uint64(0), C.c_uint64(0)
        capi.check(capi.load().c1_ctx_quantization_stats(self._h, C.byref(u), C.byref(r)))
        return int(u.value), int(r.value)

    def detection_stats(self):
        """(units whose block modes the speculative transient detector decided, units among them rechecked exactly)"""
        u, r = C.c_uint64(0), C.c_uint64(0)
        capi.check(capi.load().c1_ctx_detection_stats(self._h, C.byref(u), C.byref(r)))
        return int(u.value), int(r.value)

    def encode(self, channels, options=None, halo_frames=0, out=None):
        """channels: list of 1 or 2 float32 arrays, each (halo_frames + frames) * 512 samples.
        Returns uint8 [frames * nch, 212], units interleaved L,R.  `out`: optional preallocated result (when it
        and the channels come from pinned_empty() the batch is streamed over PCIe in overlapping chunks)."""
        opts = (options or EncoderOptions()).to_c()
        chans = [np.ascontiguousarray(c, dtype=np.float32) for c in channels]
        n = len(chans[0])
        if any(len(c) != n for c in chans) or n % 512:
            raise ValueError('channels must have equal length, a multiple of 512')
        frames = n // 512 - halo_frames
        if out is None:
            units = np.zeros((max(frames, 0) * len(chans), 212), dtype=np.uint8)
        else:
            units = out
            if units.dtype != np.uint8 or not units.flags['C_CONTIGUOUS'] or units.size != max(frames, 0) * len(chans) * 212:
                raise ValueError('out must be a contiguous uint8 array of frames * channels * 212 bytes')
            units = units.reshape(-1, 212)
        ptrs = capi.ptr_array([c.ctypes.data + halo_frames * 512 * 4 for c in chans])
        capi.check(capi.load().c1_encode_batch(self._h, ptrs, len(chans), frames, halo_frames, C.byref(opts),
                                               units.ctypes.data))
        return units

    def encode_modes(self, channels, modes, options=None, halo_frames=0, out=None):
        """encode() with the block modes of every frame given: what the reference's closure produces with
        options.fixedBlockModes set before each frame (the detector does not run).  channels and `out` as for encode();
        modes: uint8 [frames, nch] or flat (frame-major, channels interleaved), one byte m0 | m1 << 2 | m2 << 4 per sound
        unit as pack_block_modes() makes them and the detector taps return them.  Of `options` only the allocation bias
        (or biased table) is used.  A byte outside the domain raises ValueError naming frame, channel and field."""
        opts = (options or EncoderOptions()).to_c()
        chans = [np.ascontiguousarray(c, dtype=np.float32) for c in channels]
        n = len(chans[0])
        if any(len(c) != n for c in chans) or n % 512:
            raise ValueError('channels must have equal length, a multiple of 512')
        frames = n // 512 - halo_frames
        m = check_block_modes(modes, max(frames, 0), len(chans))
        if out is None:
            units = np.zeros((max(frames, 0) * len(chans), 212), dtype=np.uint8)
        else:
            units = out
            if units.dtype != np.uint8 or not units.flags['C_CONTIGUOUS'] or units.size != max(frames, 0) * len(chans) * 212:
                raise ValueError('out must be a contiguous uint8 array of frames * channels * 212 bytes')
            units = units.reshape(-1, 212)
        ptrs = capi.ptr_array([c.ctypes.data + halo_frames * 512 * 4 for c in chans])
        capi.check(capi.load().c1_encode_modes_batch(self._h, ptrs, len(chans), frames, halo_frames, C.byref(opts),
                                                     m.ctypes.data, units.ctypes.data))
        return units

    def encode_biases(self, channels, biases, modes=None, options=None, halo_frames=0, out=None):
        """encode() with the allocation bias of every frame given: what the reference's closure produces with
        options.allocationBias set before each frame.  channels, `out` as for encode(); biases: one value per frame (all
        channels) or [frames, nch], each in allocationBias's range.  The distinct values (at most MAX_BIAS_PALETTE, else
        ValueError) become the call's palette, their tables made as EncoderOptions.to_c() makes them.  modes: None (detection
        or fixed modes as `options` say) or mode bytes as for encode_modes().  The allocationBias of `options` is not used."""
        chans = [np.ascontiguousarray(c, dtype=np.float32) for c in channels]
        n = len(chans[0])
        if any(len(c) != n for c in chans) or n % 512:
            raise ValueError('channels must have equal length, a multiple of 512')
        frames = n // 512 - halo_frames
        palette, index = bias_palette(biases, max(frames, 0), len(chans), options)
        m = None if modes is None else check_block_modes(modes, max(frames, 0), len(chans))
        if out is None:
            units = np.zeros((max(frames, 0) * len(chans), 212), dtype=np.uint8)
        else:
            units = out
            if units.dtype != np.uint8 or not units.flags['C_CONTIGUOUS'] or units.size != max(frames, 0) * len(chans) * 212:
                raise ValueError('out must be a contiguous uint8 array of frames * channels * 212 bytes')
            units = units.reshape(-1, 212)
        ptrs = capi.ptr_array([c.ctypes.data + halo_frames * 512 * 4 for c in chans])
        capi.check(capi.load().c1_encode_biases_batch(self._h, ptrs, len(chans), frames, halo_frames, palette, len(palette),
                                                      index.ctypes.data, None if m is None else m.ctypes.data, units.ctypes.data))
        return units

    def encode_best_bias(self, channels, biases, modes=None, options=None, halo_frames=0, return_distortion=False):
        """encode() with the allocation bias of every sound unit chosen among `biases` by least coding error: the sum over the
        unit's 512 MDCT coefficients of (c - d)^2, d what the decoder's dequantizationStage makes of the unit (c1_encode_best_bias_batch).
        biases: 1 .. MAX_BIAS_PALETTE distinct values in the caller's order (choice indexes it), or EncoderOptions that carry
        explicit tables (candidate_palette).  modes, options, halo_frames as for encode_biases().  Returns (units, choice uint8
        [units]), and with return_distortion (units, choice, distortion float64 [units, n], energy float64 [units]); units of
        one candidate are what encode() / encode_modes() give under it."""
        chans = [np.ascontiguousarray(c, dtype=np.float32) for c in channels]
        n = len(chans[0])
        if any(len(c) != n for c in chans) or n % 512:
            raise ValueError('channels must have equal length, a multiple of 512')
        frames = max(n // 512 - halo_frames, 0)
        palette, count = candidate_palette(biases, options)
        m = None if modes is None else check_block_modes(modes, frames, len(chans))
        units = np.zeros((frames * len(chans), 212), dtype=np.uint8)
        choice = np.zeros(frames * len(chans), dtype=np.uint8)
        dist = np.zeros((frames * len(chans), count), dtype=np.float64) if return_distortion else None
        energy = np.zeros(frames * len(chans), dtype=np.float64) if return_distortion else None
        ptrs = capi.ptr_array([c.ctypes.data + halo_frames * 512 * 4 for c in chans])
        capi.check(capi.load().c1_encode_best_bias_batch(self._h, ptrs, len(chans), n // 512 - halo_frames, halo_frames, palette, count,
                                                         None if m is None else m.ctypes.data, units.ctypes.data, choice.ctypes.data,
                                                         None if dist is None else dist.ctypes.data,
                                                         None if energy is None else energy.ctypes.data))
        return (units, choice, dist, energy) if return_distortion else (units, choice)

    def encode_best_modes(self, channels, candidates, options=None, halo_frames=0, return_distortion=False):
        """encode() with the block modes of every sound unit chosen among `candidates` by least coding error: the sum over the
        unit's 512 MDCT coefficients of W * (c - d)^2, d what the decoder's dequantizationStage makes of the unit and W the
        transform's scaling (1 long, 1/4 low or mid short, 1/2 high short), so that candidates compare as their PCM error does
        (c1_encode_best_modes_batch).  candidates: 1 .. MAX_MODE_CANDIDATES distinct mode bytes or triples as
        pack_block_modes() takes them, in the caller's order (choice indexes it); ValueError for a duplicate or a candidate
        outside the domain of encode_modes().  Of `options` only the allocation bias (or biased table) is used.  Returns
        (units, choice uint8 [units], modes uint8 [units]), and with return_distortion also distortion and energy, float64
        [units, n]; units are what encode_modes() gives under `modes`."""
        opts = (options or EncoderOptions()).to_c()
        chans = [np.ascontiguousarray(c, dtype=np.float32) for c in channels]
        n = len(chans[0])
        if any(len(c) != n for c in chans) or n % 512:
            raise ValueError('channels must have equal length, a multiple of 512')
        frames = max(n // 512 - halo_frames, 0)
        cand = mode_candidates(candidates)
        count = len(cand)
        units = np.zeros((frames * len(chans), 212), dtype=np.uint8)
        choice = np.zeros(frames * len(chans), dtype=np.uint8)
        modes = np.zeros(frames * len(chans), dtype=np.uint8)
        dist = np.zeros((frames * len(chans), count), dtype=np.float64) if return_distortion else None
        energy = np.zeros((frames * len(chans), count), dtype=np.float64) if return_distortion else None
        ptrs = capi.ptr_array([c.ctypes.data + halo_frames * 512 * 4 for c in chans])
        capi.check(capi.load().c1_encode_best_modes_batch(self._h, ptrs, len(chans), n // 512 - halo_frames, halo_frames, C.byref(opts),
                                                          cand.ctypes.data, count, units.ctypes.data, choice.ctypes.data, modes.ctypes.data,
                                                          None if dist is None else dist.ctypes.data,
                                                          None if energy is None else energy.ctypes.data))
        return (units, choice, modes, dist, energy) if return_distortion else (units, choice, modes)

    def encode_measured(self, channels, modes=None, options=None, halo_frames=0, return_distortion=False, scale_factor_offsets=None,
                        return_shifts=False, masking=None, return_weights=False):
        """encode() with the word lengths of every sound unit allocated by the measured coding error instead of the reference's
        model of it (c1_encode_measured_batch; opt-in: the units are not the reference encoder's, but ordinary sound units with
        its block modes and scale factors that its decode() reads).  Per unit a greedy allocation over the W-weighted error of
        every (BFU, word length) is compared with the reference's own record; taken[u] = 1 where the greedy one codes with less
        error and was packed, 0 where the unit is byte for byte encode()'s / encode_modes()'s.  modes: None (detection or fixed
        modes as `options` say) or mode bytes as for encode_modes().  Returns (units, taken uint8 [units]), and with
        return_distortion (units, taken, distortion float64 [units, 2]: the reference record's error and the greedy one's,
        energy float64 [units]).
        scale_factor_offsets (c1_encode_measured_sf_batch): 1 to 8 distinct offsets within -8..8, the first 0, e.g.
        SCALE_FACTOR_OFFSETS.  Every BFU's scale-factor index is then chosen, per word length, among findScaleFactor's plus
        each offset by the same error, and a taken unit carries the chosen indices.  None: the call above, untouched.
        return_shifts (needs the offsets): shifts int8 [units, 52], the offset written per BFU and 0 where none was, follows
        taken in the result.
        masking (c1_encode_measured_masked_batch): True for the packaged tables (MASKING_DEFAULT) or a (floor [52], spread
        [52, 52] or None) pair, see check_masking.  Every BFU's error is then divided by a masking threshold computed per unit
        from the unit's own spectrum and these tables; distortion and energy are the weighted ones.  Without offsets the
        offsets are (0,).  None: the calls above, untouched.  return_weights (needs masking): weights float64 [units, 52], the
        reciprocal threshold of every BFU, ends the result."""
        opts = (options or EncoderOptions()).to_c()
        chans = [np.ascontiguousarray(c, dtype=np.float32) for c in channels]
        n = len(chans[0])
        if any(len(c) != n for c in chans) or n % 512:
            raise ValueError('channels must have equal length, a multiple of 512')
        frames = max(n // 512 - halo_frames, 0)
        m = None if modes is None else check_block_modes(modes, frames, len(chans))
        if return_shifts and scale_factor_offsets is None:
            raise ValueError('return_shifts needs scale_factor_offsets')
        if return_weights and masking is None:
            raise ValueError('return_weights needs masking')
        mask = None if masking is None else check_masking(masking)
        if return_shifts and mask is not None and scale_factor_offsets is None:
            raise ValueError('return_shifts needs scale_factor_offsets')
        offs = None if scale_factor_offsets is None else check_scale_factor_offsets(scale_factor_offsets)
        if mask is not None and offs is None:
            offs = check_scale_factor_offsets((0,))
        units = np.zeros((frames * len(chans), 212), dtype=np.uint8)
        taken = np.zeros(frames * len(chans), dtype=np.uint8)
        dist = np.zeros((frames * len(chans), 2), dtype=np.float64) if return_distortion else None
        energy = np.zeros(frames * len(chans), dtype=np.float64) if return_distortion else None
        ptrs = capi.ptr_array([c.ctypes.data + halo_frames * 512 * 4 for c in chans])
        if mask is not None:
            shifts = np.zeros((frames * len(chans), 52), dtype=np.int8) if return_shifts else None
            weights = np.zeros((frames * len(chans), 52), dtype=np.float64) if return_weights else None
            capi.check(capi.load().c1_encode_measured_masked_batch(
                self._h, ptrs, len(chans), n // 512 - halo_frames, halo_frames, C.byref(opts), None if m is None else m.ctypes.data,
                offs.ctypes.data, len(offs), mask[0].ctypes.data, None if mask[1] is None else mask[1].ctypes.data, units.ctypes.data,
                taken.ctypes.data, None if shifts is None else shifts.ctypes.data, None if dist is None else dist.ctypes.data,
                None if energy is None else energy.ctypes.data, None if weights is None else weights.ctypes.data))
            out = (units, taken) + ((shifts,) if return_shifts else ())
            out = out + (dist, energy) if return_distortion else out
            return out + (weights,) if return_weights else out
        if offs is not None:
            shifts = np.zeros((frames * len(chans), 52), dtype=np.int8) if return_shifts else None
            capi.check(capi.load().c1_encode_measured_sf_batch(self._h, ptrs, len(chans), n // 512 - halo_frames, halo_frames, C.byref(opts),
                                                               None if m is None else m.ctypes.data, offs.ctypes.data, len(offs),
                                                               units.ctypes.data, taken.ctypes.data,
                                                               None if shifts is None else shifts.ctypes.data,
                                                               None if dist is None else dist.ctypes.data,
                                                               None if energy is None else energy.ctypes.data))
            out = (units, taken) + ((shifts,) if return_shifts else ())
            return out + (dist, energy) if return_distortion else out
        capi.check(capi.load().c1_encode_measured_batch(self._h, ptrs, len(chans), n // 512 - halo_frames, halo_frames, C.byref(opts),
                                                        None if m is None else m.ctypes.data, units.ctypes.data, taken.ctypes.data,
                                                        None if dist is None else dist.ctypes.data,
                                                        None if energy is None else energy.ctypes.data))
        return (units, taken, dist, energy) if return_distortion else (units, taken)

    def encode_measured_modes(self, channels, candidates, options=None, halo_frames=0, scale_factor_offsets=None,
                              return_distortion=False, return_shifts=False, masking=None, return_weights=False):
        """encode_measured() with the block modes of every sound unit chosen among `candidates` by the final error of the measured
        allocation under each (c1_encode_measured_modes_batch; opt-in like encode_measured()).  candidates: as for
        encode_best_modes(); scale_factor_offsets: as for encode_measured(), None for the plain measured allocation (offsets
        (0,)).  Per (unit, candidate) the figures are those of encode_measured(modes=constant byte, ...); the candidate of least
        T_final = taken ? T(n*) : T_ref wins, the first on a tie.  Of `options` only the allocation bias (or biased table) is used.
        Returns (units, choice uint8 [units], modes uint8 [units], taken uint8 [units]), then with return_shifts shifts int8
        [units, 52] (the winner's), then with return_distortion distortion float64 [units, n, 2] (T_ref, T(n*)) and energy
        float64 [units, n]; units are what encode_measured(modes=modes, ...) gives.  The dearest encode of the library: one
        greedy allocation per unit and candidate.
        masking (c1_encode_measured_modes_masked_batch): True for the packaged tables or a (floor, spread or None) pair, as for
        encode_measured().  Every candidate's errors are then divided by ONE masking threshold per unit and BFU, computed from the
        unit's all-long spectrum whatever the candidates (the weights encode_measured(modes=zeros, masking=...) reports), so the
        weighted T_final of the candidates are comparable; distortion and energy are the weighted ones.  None: the call above,
        untouched.  return_weights (needs masking): weights float64 [units, 52] ends the result."""
        opts = (options or EncoderOptions()).to_c()
        chans = [np.ascontiguousarray(c, dtype=np.float32) for c in channels]
        n = len(chans[0])
        if any(len(c) != n for c in chans) or n % 512:
            raise ValueError('channels must have equal length, a multiple of 512')
        frames = max(n // 512 - halo_frames, 0)
        cand = mode_candidates(candidates)
        count = len(cand)
        if return_weights and masking is None:
            raise ValueError('return_weights needs masking')
        mask = None if masking is None else check_masking(masking)
        offs = check_scale_factor_offsets((0,) if scale_factor_offsets is None else scale_factor_offsets)
        total = frames * len(chans)
        units = np.zeros((total, 212), dtype=np.uint8)
        choice = np.zeros(total, dtype=np.uint8)
        modes = np.zeros(total, dtype=np.uint8)
        taken = np.zeros(total, dtype=np.uint8)
        shifts = np.zeros((total, 52), dtype=np.int8) if return_shifts else None
        dist = np.zeros((total, count, 2), dtype=np.float64) if return_distortion else None
        energy = np.zeros((total, count), dtype=np.float64) if return_distortion else None
        ptrs = capi.ptr_array([c.ctypes.data + halo_frames * 512 * 4 for c in chans])
        if mask is not None:
            weights = np.zeros((total, 52), dtype=np.float64) if return_weights else None
            capi.check(capi.load().c1_encode_measured_modes_masked_batch(
                self._h, ptrs, len(chans), n // 512 - halo_frames, halo_frames, C.byref(opts), cand.ctypes.data, count, offs.ctypes.data,
                len(offs), mask[0].ctypes.data, None if mask[1] is None else mask[1].ctypes.data, units.ctypes.data, choice.ctypes.data,
                modes.ctypes.data, taken.ctypes.data, None if shifts is None else shifts.ctypes.data,
                None if dist is None else dist.ctypes.data, None if energy is None else energy.ctypes.data,
                None if weights is None else weights.ctypes.data))
            out = (units, choice, modes, taken) + ((shifts,) if return_shifts else ())
            out = out + (dist, energy) if return_distortion else out
            return out + (weights,) if return_weights else out
        capi.check(capi.load().c1_encode_measured_modes_batch(
            self._h, ptrs, len(chans), n // 512 - halo_frames, halo_frames, C.byref(opts), cand.ctypes.data, count, offs.ctypes.data,
            len(offs), units.ctypes.data, choice.ctypes.data, modes.ctypes.data, taken.ctypes.data,
            None if shifts is None else shifts.ctypes.data, None if dist is None else dist.ctypes.data,
            None if energy is None else energy.ctypes.data))
        out = (units, choice, modes, taken) + ((shifts,) if return_shifts else ())
        return out + (dist, energy) if return_distortion else out

    def measure_units(self, channels, units, masking=None, halo_frames=0, return_weights=False, threshold_from='own'):
        """The coding error of sound units that already exist against their PCM (c1_measure_units_batch): any encoder's units,
        scored from the bytes with the yardstick of encode_measured().  channels: the PCM as for encode() (halo_frames frames of
        real history first); units: uint8 [frames * channels, 212], unit index = frame * channels + channel, every unit's block
        modes inside the domain of encode_modes() (ValueError naming frame, channel and field).  Returns (noise float64 [units,
        52], signal float64 [units, 52], totals float64 [units, 2]): per BFU the W-weighted squared error of the dequantized
        unit against the exact coefficients under the unit's own block modes and the W-weighted energy of those, and their sums
        over the BFUs.  masking: None, or as for encode_measured() -- totals are then the sums weighted by every BFU's reciprocal
        masking threshold, which return_weights (needs masking) appends as weights float64 [units, 52].  threshold_from: 'own'
        forms those thresholds from the unit's spectrum under its own block modes; 'long' (needs masking) from the frame's
        all-long spectrum, the one threshold per unit of encode_measured_modes(masking=...) under which units coded in different
        modes compare (c1_measure_units_shared_batch); noise and signal are the same either way."""
        shared = check_threshold_from(threshold_from, masking)
        chans = [np.ascontiguousarray(c, dtype=np.float32) for c in channels]
        n = len(chans[0])
        if any(len(c) != n for c in chans) or n % 512:
            raise ValueError('channels must have equal length, a multiple of 512')
        frames = max(n // 512 - halo_frames, 0)
        u = check_measured_units(units, frames, len(chans))
        if return_weights and masking is None:
            raise ValueError('return_weights needs masking')
        mask = None if masking is None else check_masking(masking)
        noise = np.zeros((frames * len(chans), 52), dtype=np.float64)
        signal = np.zeros((frames * len(chans), 52), dtype=np.float64)
        totals = np.zeros((frames * len(chans), 2), dtype=np.float64)
        weights = np.zeros((frames * len(chans), 52), dtype=np.float64) if return_weights else None
        ptrs = capi.ptr_array([c.ctypes.data + halo_frames * 512 * 4 for c in chans])
        call = capi.load().c1_measure_units_shared_batch if shared else capi.load().c1_measure_units_batch
        capi.check(call(
            self._h, ptrs, len(chans), n // 512 - halo_frames, halo_frames, u.ctypes.data,
            None if mask is None else mask[0].ctypes.data, None if mask is None or mask[1] is None else mask[1].ctypes.data,
            noise.ctypes.data, signal.ctypes.data, totals.ctypes.data, None if weights is None else weights.ctypes.data))
        return (noise, signal, totals, weights) if return_weights else (noise, signal, totals)

    def measure_pcm(self, channels, units, halo_frames=0, halo_units=0):
        """The error of the decoded PCM of sound units against the PCM they were made from (c1_measure_pcm_batch), per unit and
        per 32-sample segment.  channels: the PCM as for encode() (halo_frames frames of real history first); units: uint8
        [(halo_units + frames) * channels, 212], unit index = frame * channels + channel, the unit(s) of frame -1 first when
        halo_units is 1 (the decoder starts from a fresh pool otherwise).  Returns (noise float64 [units, 16], signal float64
        [units, 16], totals float64 [units, 2]): with y the exact decode of the units and x the input PCM_DELAY = 266 samples
        earlier (zero before the history given), noise[u, s] = sum (y - x)^2 and signal[u, s] = sum x^2 over the samples 32 s ..
        32 s + 31 of the unit's frame, and totals[u] their sums over the segments."""
        chans = [np.ascontiguousarray(c) for c in channels]
        if len(chans) not in (1, 2):
            raise ValueError('channels must be 1 or 2 arrays')
        if any(c.dtype != np.float32 or c.ndim != 1 for c in chans):
            raise ValueError('channels must be one-dimensional float32 arrays')
        n = len(chans[0])
        if any(len(c) != n for c in chans) or n % 512:
            raise ValueError('channels must have equal length, a multiple of 512')
        if halo_frames not in (0, 1, 2) or n // 512 < halo_frames:
            raise ValueError('halo_frames must be 0, 1 or 2 frames of the PCM given')
        if halo_units not in (0, 1):
            raise ValueError('halo_units must be 0 or 1')
        frames = n // 512 - halo_frames
        u = check_pcm_units(units, frames + halo_units, len(chans))
        noise = np.zeros((frames * len(chans), PCM_SEGMENTS), dtype=np.float64)
        signal = np.zeros((frames * len(chans), PCM_SEGMENTS), dtype=np.float64)
        totals = np.zeros((frames * len(chans), 2), dtype=np.float64)
        ptrs = capi.ptr_array([c.ctypes.data + halo_frames * 512 * 4 for c in chans])
        capi.check(capi.load().c1_measure_pcm_batch(self._h, ptrs, len(chans), frames, halo_frames,
                                                    u.ctypes.data + halo_units * len(chans) * 212, halo_units,
                                                    noise.ctypes.data, signal.ctypes.data, totals.ctypes.data))
        return noise, signal, totals

    def decode(self, units, channels, halo_units=0, out=None):
        """units: uint8 [(halo_units + frames) * channels, 212].  Returns a list of float32 arrays (`out`: optional
        preallocated list of them, see encode())."""
        u = np.ascontiguousarray(units, dtype=np.uint8).reshape(-1, 212)
        frames = u.shape[0] // channels - halo_units
        if out is None:
            outs = [np.zeros(max(frames, 0) * 512, dtype=np.float32) for _ in range(channels)]
        else:
            outs = list(out)
            if len(outs) != channels or any(o.dtype != np.float32 or not o.flags['C_CONTIGUOUS'] or o.size != max(frames, 0) * 512 for o in outs):
                raise ValueError('out must be one contiguous float32 array of frames * 512 samples per channel')
        ptrs = capi.ptr_array([o.ctypes.data for o in outs])
        capi.check(capi.load().c1_decode_batch(self._h, u.ctypes.data + halo_units * channels * 212, channels,
                                               frames, halo_units, ptrs))
        return outs

    # ---- device-resident (raw device pointers, e.g. torch tensor .data_ptr()) ---------------------
    def encode_device(self, pcm_ptrs, frames, units_ptr, options=None, halo_frames=0, c_options=None):
        opts = c_options if c_options is not None else (options or EncoderOptions()).to_c()
        capi.check(capi.load().c1_encode_device(self._h, capi.ptr_array(pcm_ptrs), len(pcm_ptrs), frames, halo_frames,
                                                C.byref(opts), C.c_void_p(units_ptr)))

    def encode_modes_device(self, pcm_ptrs, frames, modes_ptr, units_ptr, options=None, halo_frames=0):
        """c1_encode_modes_device: modes_ptr = frames * channels mode bytes on the device (not checked: a byte outside the
        domain gives an unspecified unit, never an access outside the buffers)."""
        opts = (options or EncoderOptions()).to_c()
        capi.check(capi.load().c1_encode_modes_device(self._h, capi.ptr_array(pcm_ptrs), len(pcm_ptrs), frames, halo_frames,
                                                      C.byref(opts), C.c_void_p(modes_ptr), C.c_void_p(units_ptr)))

    def encode_biases_device(self, pcm_ptrs, frames, palette_options, index_ptr, units_ptr, modes_ptr=None, halo_frames=0):
        """c1_encode_biases_device: palette_options = 1 .. MAX_BIAS_PALETTE EncoderOptions (an entry may carry its own
        biased_table); index_ptr = frames * channels palette indices on the device (not checked: a byte outside the palette
        selects entry 0); modes_ptr = mode bytes on the device as for encode_modes_device, or None."""
        palette = palette_array([o.to_c() for o in palette_options])
        capi.check(capi.load().c1_encode_biases_device(self._h, capi.ptr_array(pcm_ptrs), len(pcm_ptrs), frames, halo_frames,
                                                       palette, len(palette_options), C.c_void_p(index_ptr),
                                                       C.c_void_p(modes_ptr) if modes_ptr else None, C.c_void_p(units_ptr)))

    def encode_best_bias_device(self, pcm_ptrs, frames, palette_options, units_ptr=None, choice_ptr=None, distortion_ptr=None,
                                energy_ptr=None, modes_ptr=None, halo_frames=0):
        """c1_encode_best_bias_device: palette_options = 1 .. MAX_BIAS_PALETTE EncoderOptions; outputs on the device, each may be
        None (units_ptr None: measure only), not all; distortion is float64 [units, n], energy float64 [units], choice uint8
        [units]; modes_ptr = mode bytes on the device as for encode_modes_device, or None."""
        palette = palette_array([o.to_c() for o in palette_options])
        vp = lambda p: C.c_void_p(p) if p else None
        capi.check(capi.load().c1_encode_best_bias_device(self._h, capi.ptr_array(pcm_ptrs), len(pcm_ptrs), frames, halo_frames,
                                                          palette, len(palette_options), vp(modes_ptr), vp(units_ptr), vp(choice_ptr),
                                                          vp(distortion_ptr), vp(energy_ptr)))

    def encode_best_modes_device(self, pcm_ptrs, frames, candidates, units_ptr=None, choice_ptr=None, modes_ptr=None,
                                 distortion_ptr=None, energy_ptr=None, options=None, halo_frames=0):
        """c1_encode_best_modes_device: candidates = 1 .. MAX_MODE_CANDIDATES distinct mode bytes or triples (host; checked by
        the library: C1_ERR_ARG); outputs on the device, each may be None (units_ptr None: measure only), not all; choice and
        modes are uint8 [units], distortion and energy float64 [units, n]."""
        opts = (options or EncoderOptions()).to_c()
        cand = mode_candidates(candidates, check=False)
        vp = lambda p: C.c_void_p(p) if p else None
        capi.check(capi.load().c1_encode_best_modes_device(self._h, capi.ptr_array(pcm_ptrs), len(pcm_ptrs), frames, halo_frames,
                                                           C.byref(opts), cand.ctypes.data, len(cand), vp(units_ptr), vp(choice_ptr),
                                                           vp(modes_ptr), vp(distortion_ptr), vp(energy_ptr)))

    def encode_measured_modes_device(self, pcm_ptrs, frames, candidates, units_ptr=None, choice_ptr=None, modes_ptr=None, taken_ptr=None,
                                     shifts_ptr=None, distortion_ptr=None, energy_ptr=None, options=None, halo_frames=0,
                                     scale_factor_offsets=None, masking=None, weights_ptr=None):
        """c1_encode_measured_modes_device: candidates as for encode_best_modes_device and scale_factor_offsets as for
        encode_measured_device (host values; checked by the library: C1_ERR_ARG), None for offsets (0,); outputs on the device,
        each may be None (units_ptr None: measure only), not all; choice, modes and taken are uint8 [units], shifts int8 [units,
        52], distortion float64 [units, n, 2] and energy float64 [units, n].  masking (host values, as for encode_measured_modes):
        c1_encode_measured_modes_masked_device, and weights_ptr = float64 [units, 52] on the device, or None."""
        opts = (options or EncoderOptions()).to_c()
        cand = mode_candidates(candidates, check=False)
        offs = check_scale_factor_offsets((0,) if scale_factor_offsets is None else scale_factor_offsets, check=False)
        vp = lambda p: C.c_void_p(p) if p else None
        if masking is not None:
            mask = check_masking(masking, check=False)                             # the library's own check decides
            capi.check(capi.load().c1_encode_measured_modes_masked_device(
                self._h, capi.ptr_array(pcm_ptrs), len(pcm_ptrs), frames, halo_frames, C.byref(opts), cand.ctypes.data if len(cand) else None,
                len(cand), offs.ctypes.data if len(offs) else None, len(offs), mask[0].ctypes.data,
                None if mask[1] is None else mask[1].ctypes.data, vp(units_ptr), vp(choice_ptr), vp(modes_ptr), vp(taken_ptr), vp(shifts_ptr),
                vp(distortion_ptr), vp(energy_ptr), vp(weights_ptr)))
            return
        if weights_ptr:
            raise ValueError('weights_ptr needs masking')
        capi.check(capi.load().c1_encode_measured_modes_device(
            self._h, capi.ptr_array(pcm_ptrs), len(pcm_ptrs), frames, halo_frames, C.byref(opts), cand.ctypes.data if len(cand) else None,
            len(cand), offs.ctypes.data if len(offs) else None, len(offs), vp(units_ptr), vp(choice_ptr), vp(modes_ptr), vp(taken_ptr),
            vp(shifts_ptr), vp(distortion_ptr), vp(energy_ptr)))

    def encode_measured_device(self, pcm_ptrs, frames, units_ptr=None, taken_ptr=None, distortion_ptr=None, energy_ptr=None,
                               modes_ptr=None, options=None, halo_frames=0, scale_factor_offsets=None, shifts_ptr=None, masking=None,
                               weights_ptr=None):
        """c1_encode_measured_device: outputs on the device, each may be None (units_ptr None: measure only), not all; taken is
        uint8 [units], distortion float64 [units, 2], energy float64 [units]; modes_ptr = mode bytes on the device as for
        encode_modes_device, or None.  scale_factor_offsets (host values, as for encode_measured): c1_encode_measured_sf_device,
        and shifts_ptr = int8 [units, 52] on the device, or None.  masking (host values, as for encode_measured):
        c1_encode_measured_masked_device, offsets (0,) when none are given, and weights_ptr = float64 [units, 52] on the device, or
        None."""
        opts = (options or EncoderOptions()).to_c()
        vp = lambda p: C.c_void_p(p) if p else None
        if masking is not None:
            mask = check_masking(masking, check=False)                             # the library's own check decides
            offs = check_scale_factor_offsets((0,) if scale_factor_offsets is None else scale_factor_offsets, check=False)
            capi.check(capi.load().c1_encode_measured_masked_device(
                self._h, capi.ptr_array(pcm_ptrs), len(pcm_ptrs), frames, halo_frames, C.byref(opts), vp(modes_ptr),
                offs.ctypes.data if len(offs) else None, len(offs), mask[0].ctypes.data, None if mask[1] is None else mask[1].ctypes.data,
                vp(units_ptr), vp(taken_ptr), vp(shifts_ptr), vp(distortion_ptr), vp(energy_ptr), vp(weights_ptr)))
            return
        if weights_ptr:
            raise ValueError('weights_ptr needs masking')
        if scale_factor_offsets is not None:
            offs = check_scale_factor_offsets(scale_factor_offsets, check=False)   # the library's own check decides
            capi.check(capi.load().c1_encode_measured_sf_device(self._h, capi.ptr_array(pcm_ptrs), len(pcm_ptrs), frames, halo_frames,
                                                                C.byref(opts), vp(modes_ptr), offs.ctypes.data if len(offs) else None,
                                                                len(offs), vp(units_ptr), vp(taken_ptr), vp(shifts_ptr),
                                                                vp(distortion_ptr), vp(energy_ptr)))
            return
        if shifts_ptr:
            raise ValueError('shifts_ptr needs scale_factor_offsets')
        capi.check(capi.load().c1_encode_measured_device(self._h, capi.ptr_array(pcm_ptrs), len(pcm_ptrs), frames, halo_frames,
                                                         C.byref(opts), vp(modes_ptr), vp(units_ptr), vp(taken_ptr),
                                                         vp(distortion_ptr), vp(energy_ptr)))

    def measure_units_device(self, pcm_ptrs, frames, units_ptr, noise_ptr=None, signal_ptr=None, totals_ptr=None, weights_ptr=None,
                             masking=None, halo_frames=0, threshold_from='own'):
        """c1_measure_units_device: units_ptr = frames * channels sound units on the device (4-byte aligned; the block modes are
        not checked: a unit outside the domain is measured under the byte brought into it, never with an access outside the
        buffers); outputs on the device, each may be None, not all: noise, signal and weights float64 [units, 52], totals
        float64 [units, 2].  masking (host values, as for measure_units); weights_ptr needs it (the library's own check).
        threshold_from as for measure_units: 'long' (needs masking) takes c1_measure_units_shared_device."""
        shared = check_threshold_from(threshold_from, masking)
        vp = lambda p: C.c_void_p(p) if p else None
        mask = None if masking is None else check_masking(masking, check=False)   # the library's own check decides
        call = capi.load().c1_measure_units_shared_device if shared else capi.load().c1_measure_units_device
        capi.check(call(
            self._h, capi.ptr_array(pcm_ptrs), len(pcm_ptrs), frames, halo_frames, vp(units_ptr),
            None if mask is None else mask[0].ctypes.data, None if mask is None or mask[1] is None else mask[1].ctypes.data,
            vp(noise_ptr), vp(signal_ptr), vp(totals_ptr), vp(weights_ptr)))

    def measure_pcm_device(self, pcm_ptrs, frames, units_ptr, noise_ptr=None, signal_ptr=None, totals_ptr=None, halo_frames=0,
                           halo_units=0):
        """c1_measure_pcm_device: pcm_ptrs = frame 0 of every channel on the device (16-byte aligned, halo_frames frames of
        real PCM before it), units_ptr = unit 0 of frames * channels sound units on the device (4-byte aligned, the unit(s) of
        frame -1 before it when halo_units is 1); outputs on the device, each may be None, not all: noise and signal float64
        [units, 16], totals float64 [units, 2]."""
        vp = lambda p: C.c_void_p(p) if p else None
        capi.check(capi.load().c1_measure_pcm_device(self._h, capi.ptr_array(pcm_ptrs), len(pcm_ptrs), frames, halo_frames,
                                                     vp(units_ptr), halo_units, vp(noise_ptr), vp(signal_ptr), vp(totals_ptr)))

    def decode_device(self, units_ptr, channels, frames, pcm_ptrs, halo_units=0):
        capi.check(capi.load().c1_decode_device(self._h, C.c_void_p(units_ptr), channels, frames, halo_units,
                                                capi.ptr_array(pcm_ptrs)))

    def decode_fields_device(self, field_ptrs, channels, frames, pcm_ptrs, halo_frames=0):
        """c1_decode_fields_device: field_ptrs = device pointers (nbfu, block_modes, sfi, wl, quantized) of frame 0, the halo's
        fields (halo_frames 0 or 1) just before them; unit index frame * channels + channel.  Fields outside the domain of
        include/carta1_hip.h are not checked here."""
        capi.check(capi.load().c1_decode_fields_device(self._h, channels, frames, halo_frames,
                                                       *[C.c_void_p(int(p)) for p in field_ptrs], capi.ptr_array(pcm_ptrs)))

    def generate_device(self, signal, seed, frames, pcm_ptr):
        capi.check(capi.load().c1_generate_device(self._h, signal, seed, frames, C.c_void_p(pcm_ptr)))

    def encode_wav(self, raw, bits, channels, options=None, out=None):
        """raw: the body of a WAV file (interleaved little-endian integer PCM, bits = 16, 24 or 32) as bytes or a
        uint8 array.  Returns uint8 [ceil(samples / 512) * channels, 212].  Conversion happens on the device."""
        opts = (options or EncoderOptions()).to_c()
        buf = np.frombuffer(raw, dtype=np.uint8) if not isinstance(raw, np.ndarray) else np.ascontiguousarray(raw).view(np.uint8).reshape(-1)
        bps = bits // 8
        if buf.size % (bps * channels):
            raise ValueError('raw length is not a whole number of %d-bit %d-channel samples' % (bits, channels))
        samples = buf.size // (bps * channels)
        frames = (samples + 511) // 512
        units = out if out is not None else np.zeros((frames * channels, 212), dtype=np.uint8)
        if units.dtype != np.uint8 or not units.flags['C_CONTIGUOUS'] or units.size != frames * channels * 212:
            raise ValueError('out must be a contiguous uint8 array of frames * channels * 212 bytes')
        capi.check(capi.load().c1_encode_wav_batch(self._h, buf.ctypes.data, bits, channels, samples, C.byref(opts), units.ctypes.data))
        return units.reshape(-1, 212)

    def decode_wav16(self, units, channels, out=None):
        """units: uint8 [frames * channels, 212].  Returns int16 [frames * 512, channels] (a 16-bit WAV body)."""
        u = np.ascontiguousarray(units, dtype=np.uint8).reshape(-1, 212)
        frames = u.shape[0] // channels
        pcm = out if out is not None else np.zeros((frames * 512, channels), dtype=np.int16)
        if pcm.dtype != np.int16 or not pcm.flags['C_CONTIGUOUS'] or pcm.size != frames * 512 * channels:
            raise ValueError('out must be a contiguous int16 array of frames * 512 * channels samples')
        capi.check(capi.load().c1_decode_wav16_batch(self._h, u.ctypes.data, channels, frames, pcm.ctypes.data))
        return pcm

    def pcm_from_int_device(self, src_ptr, bits, channels, samples, pcm_ptrs):
        capi.check(capi.load().c1_pcm_from_int_device(self._h, C.c_void_p(src_ptr), bits, channels, samples, capi.ptr_array(pcm_ptrs)))

    def pcm_to_int16_device(self, pcm_ptrs, samples, dst_ptr):
        capi.check(capi.load().c1_pcm_to_int16_device(self._h, capi.ptr_array(pcm_ptrs), len(pcm_ptrs), samples, C.c_void_p(dst_ptr)))

    def encode_stages_device(self, pcm_ptrs, frames, bands_ptr, coefs_ptr, side_ptr, alloc_ptr, options=None,
                             halo_frames=0):
        opts = (options or EncoderOptions()).to_c()
        capi.check(capi.load().c1_encode_stages_device(
            self._h, capi.ptr_array(pcm_ptrs), len(pcm_ptrs), frames, halo_frames, C.byref(opts),
            C.c_void_p(bands_ptr), C.c_void_p(coefs_ptr), C.c_void_p(side_ptr), C.c_void_p(alloc_ptr)))

    def detect_stages_device(self, pcm_ptrs, frames, mags_ptr, modes_ptr, options=None, halo_frames=0):
        """The transient detector's magnitude spectra (256 floats per unit) and chosen block modes (1 byte per unit)."""
        opts = (options or EncoderOptions()).to_c()
        capi.check(capi.load().c1_detect_stages_device(
            self._h, capi.ptr_array(pcm_ptrs), len(pcm_ptrs), frames, halo_frames, C.byref(opts),
            C.c_void_p(mags_ptr), C.c_void_p(modes_ptr)))

    def detect_scores_device(self, pcm_ptrs, frames, scores_ptr, modes_ptr, open_ptr, options=None, halo_frames=0, speculative=True):
        """Per unit and band {lo, hi}: the speculative detector's interval for the transient score, or the reference's
        score twice; the block modes after the exact recheck; how many units the interval left open."""
        opts = (options or EncoderOptions()).to_c()
        capi.check(capi.load().c1_detect_scores_device(
            self._h, capi.ptr_array(pcm_ptrs), len(pcm_ptrs), frames, halo_frames, C.byref(opts), 1 if speculative else 0,
            C.c_void_p(scores_ptr), C.c_void_p(modes_ptr), C.c_void_p(open_ptr)))

    def detect_spec_mags_device(self, pcm_ptrs, frames, mags_ptr, bounds_ptr, halo_frames=0):
        """The speculative detector's binary32 magnitude spectra (256 floats per unit) and the bound per band (3 floats per unit)."""
        capi.check(capi.load().c1_detect_spec_mags_device(
            self._h, capi.ptr_array(pcm_ptrs), len(pcm_ptrs), frames, halo_frames, C.c_void_p(mags_ptr), C.c_void_p(bounds_ptr)))

    def log2f_error(self, first_bits, count):
        """(max relative error in units of 2^-24, max absolute error near 1) of the device's binary32 log2 over a range of bit patterns"""
        out = (C.c_double * 2)()
        capi.check(capi.load().c1_log2f_error_device(self._h, first_bits, count, out))
        return float(out[0]), float(out[1])

    def libm_device(self, fn, in_ptr, out_ptr, n):
        """Math.log / exp / log1p / log10 (fn 0..3) as the detector's kernels evaluate them, and Math.log2 (fn 4) as
        find_scale_factor does, on n device doubles."""
        capi.check(capi.load().c1_libm_device(self._h, fn, C.c_void_p(in_ptr), C.c_void_p(out_ptr), n))

    def alloc_bounds_device(self, side_ptr, units, out_ptr, options=None):
        """Totals of the eight candidate BFU counts and the lower bounds the allocation prunes with (16 doubles per unit)."""
        opts = (options or EncoderOptions()).to_c()
        capi.check(capi.load().c1_alloc_bounds_device(self._h, C.c_void_p(side_ptr), units, C.byref(opts), C.c_void_p(out_ptr)))

    def spec_stages_device(self, pcm_ptrs, frames, coefs_ptr, eps_ptr, side_ptr, options=None, halo_frames=0):
        """The speculative binary32 analysis alone: coefficients, their proven error bounds, scale-factor indices."""
        opts = (options or EncoderOptions({'fixedBlockModes': [0, 0, 0]})).to_c()
        capi.check(capi.load().c1_spec_stages_device(
            self._h, capi.ptr_array(pcm_ptrs), len(pcm_ptrs), frames, halo_frames, C.byref(opts),
            C.c_void_p(coefs_ptr), C.c_void_p(eps_ptr), C.c_void_p(side_ptr)))

    # ---- the single-stage functions the reference exports (codec/index.js:30-35,42), host arrays ----------------
    def quantize(self, coefficients, scale_factor_index, bits_per_sample):
        """quantize, codec/coding/quantization.js:34-56 -> int32 array.  Every int32 bits_per_sample has the reference's
        meaning; scale_factor_index outside 0..63 is C1_ERR_ARG, a non-int32 argument ValueError"""
        _check_quantize_args(scale_factor_index, bits_per_sample)
        x = np.ascontiguousarray(coefficients, dtype=np.float32)
        out = np.zeros(x.size, dtype=np.int32)
        capi.check(capi.load().c1_quantize(self._h, x.ctypes.data, x.size, int(scale_factor_index), int(bits_per_sample), out.ctypes.data))
        return out

    def dequantize(self, quantized, scale_factor_index, bits_per_sample):
        """dequantize, quantization.js:65-78 -> float32 array; arguments as for quantize"""
        _check_quantize_args(scale_factor_index, bits_per_sample)
        q = np.ascontiguousarray(quantized, dtype=np.int32)
        out = np.zeros(q.size, dtype=np.float32)
        capi.check(capi.load().c1_dequantize(self._h, q.ctypes.data, q.size, int(scale_factor_index), int(bits_per_sample), out.ctypes.data))
        return out

    def fft(self, real, imag, w):
        """FFT.fft, codec/transforms/fft.js:14-68, in place on two contiguous float32 arrays; w: (cos, sin)(-2 pi / stride) for
        stride = 2, 4, .., n as the reference's engine computes them (float64, log2(n) pairs)"""
        if real.dtype != np.float32 or imag.dtype != np.float32 or not real.flags['C_CONTIGUOUS'] or not imag.flags['C_CONTIGUOUS'] or real.size != imag.size:
            raise ValueError('fft works in place on two contiguous float32 arrays of equal length')
        w = np.ascontiguousarray(w, dtype=np.float64)
        capi.check(capi.load().c1_fft(self._h, real.ctypes.data, imag.ctypes.data, real.size, w.ctypes.data))

    # ---- the decision functions of codec/analysis/transient.js and codec/coding/bitallocation.js, batched over independent
    # problems of any shape (include/carta1_hip.h, c1_perform_fft .. c1_allocate_bits).  Values are read as float64.

    def perform_fft(self, samples, fft_size, w=None):
        """performFFT, transient.js:17-35, per problem: samples = a sequence of 1-D arrays (any lengths) or a 2-D array ->
        float32 [problems, fft_size // 2] magnitudes.  fft_size: a power of two 1 .. 2^22.  w: (cos, sin)(-2 pi / stride) for
        stride = 2 .. fft_size, log2(fft_size) pairs as the reference's engine computes them; default this process's math.cos /
        math.sin, which may differ from V8's in the last bit"""
        if not isinstance(fft_size, int) or fft_size < 1 or fft_size & (fft_size - 1) or fft_size > 1 << 22:
            raise ValueError('perform_fft: fftSize must be a power of two 1 .. 2^22, got %r' % (fft_size,))
        stages = fft_size.bit_length() - 1
        if w is None:
            w = [f(-2 * math.pi / (2 << s)) for s in range(stages) for f in (math.cos, math.sin)]
        w = np.ascontiguousarray(w, dtype=np.float64)
        if w.size != 2 * stages:
            raise ValueError('perform_fft: w must hold log2(fftSize) pairs')
        rows = list(samples)
        out = np.zeros((len(rows), fft_size // 2), dtype=np.float32)
        step = max(1, (1 << 22) // fft_size)                  # problems per call: re / im scratch of 32 MiB
        for a in range(0, len(rows), step):
            vals, off = _ragged(rows[a:a + step])
            capi.check(capi.load().c1_perform_fft(self._h, vals.ctypes.data, off.ctypes.data, off.size - 1, fft_size, w.ctypes.data,
                                                  out[a:a + step].ctypes.data))
        return out

    def detect_transient(self, current, previous, threshold):
        """detectTransient, transient.js:44-226, per problem: current / previous = sequences of 1-D arrays of any lengths
        (previous[p] None: a falsy prevCoeffs, never transient); threshold a float or one per problem -> (bool [problems],
        float64 scores [problems], NaN where previous is None)"""
        cur = list(current)
        prev = list(previous)
        if len(prev) != len(cur):
            raise ValueError('detect_transient: one previous frame (or None) per current frame')
        thr = np.ascontiguousarray(np.broadcast_to(np.asarray(threshold, dtype=np.float64), (len(cur),)))
        has = np.array([q is not None for q in prev], dtype=np.uint8)
        cv, co = _ragged(cur)
        pv, po = _ragged([q if q is not None else () for q in prev])
        flag = np.zeros(len(cur), dtype=np.uint8)
        score = np.zeros(len(cur), dtype=np.float64)
        capi.check(capi.load().c1_detect_transients(self._h, cv.ctypes.data, co.ctypes.data, pv.ctypes.data, po.ctypes.data,
                                                    has.ctypes.data, thr.ctypes.data, len(cur), flag.ctypes.data, score.ctypes.data))
        return flag.astype(bool), score

    def find_scale_factor(self, values, lengths=None):
        """findScaleFactor, bitallocation.js:290-299, per problem: values = a sequence of 1-D arrays; lengths = `length` per
        problem (default each array's own; past the end reads undefined, <= 0 gives 0) -> int32 [problems]"""
        rows = list(values)
        vals, off = _ragged(rows)
        n = np.diff(off) if lengths is None else np.ascontiguousarray(lengths, dtype=np.int64)
        if n.size != len(rows):
            raise ValueError('find_scale_factor: one length per problem')
        n = np.ascontiguousarray(n, dtype=np.int64)
        out = np.zeros(len(rows), dtype=np.int32)
        capi.check(capi.load().c1_find_scale_factors(self._h, vals.ctypes.data, off.ctypes.data, n.ctypes.data, len(rows), out.ctypes.data))
        return out

    def allocate_bits(self, bfu_data, bfu_sizes, max_bfu_count, allocation_bias=1.0, biased_table=None):
        """allocateBits, bitallocation.js:74-142, per problem.  bfu_data: a float array [problems, 52, L] (every BFU L values)
        or a sequence (per problem) of sequences of 1-D arrays (BFU i's values, any length); bfu_sizes int [problems, 52]
        (bfuSizes[i] | 0); max_bfu_count 0..52, an int or one per problem.  The table is pow(SCALE_FACTORS, allocation_bias)
        as EncoderOptions.to_c() builds it (allocation_bias 0 .. 5), or biased_table (64 doubles, any values).  -> dict: bfu_count int32 [problems], allocation
        int32 [problems, 52] (the first bfu_count entries are the reference's array), scale_factor_indices int32
        [problems, 52] (the first max_bfu_count entries, or 52 zeros on the fallback), fallback bool [problems]"""
        sizes = np.ascontiguousarray(bfu_sizes, dtype=np.int32).reshape(-1, 52)
        n = sizes.shape[0]
        mb = np.ascontiguousarray(np.broadcast_to(np.asarray(max_bfu_count, dtype=np.int32), (n,)))
        if isinstance(bfu_data, np.ndarray):
            d = np.ascontiguousarray(bfu_data, dtype=np.float64).reshape(n, 52, -1)
            per = d.shape[2]
            data = d.reshape(-1)
            offs = (np.arange(n * 52, dtype=np.int64) * per).reshape(n, 52)
            lens = np.full((n, 52), per, dtype=np.int32)
        else:
            rows = list(bfu_data)
            if len(rows) != n:
                raise ValueError('allocate_bits: one BFU list per problem')
            flat = [np.ascontiguousarray(b, dtype=np.float64).reshape(-1) for r in rows for b in list(r)[:52]]
            data = np.concatenate(flat) if flat else np.zeros(0)
            offs = np.zeros((n, 52), dtype=np.int64)
            lens = np.zeros((n, 52), dtype=np.int32)
            pos = k = 0
            for p, r in enumerate(rows):
                for i in range(min(len(r), 52)):
                    offs[p, i], lens[p, i] = pos, flat[k].size
                    pos += flat[k].size
                    k += 1
        table = biased_table
        if table is None:
            o = EncoderOptions({'allocationBias': allocation_bias}).to_c()
            table = [o.biased_scale_factors[i] for i in range(64)]
        table = np.ascontiguousarray(table, dtype=np.float64)
        if table.size != 64:
            raise ValueError('allocate_bits: the biased table holds 64 entries')
        res = {'bfu_count': np.zeros(n, dtype=np.int32), 'allocation': np.zeros((n, 52), dtype=np.int32),
               'scale_factor_indices': np.zeros((n, 52), dtype=np.int32), 'fallback': np.zeros(n, dtype=np.uint8)}
        capi.check(capi.load().c1_allocate_bits(self._h, data.ctypes.data, data.size, offs.ctypes.data, lens.ctypes.data,
                                                sizes.ctypes.data, mb.ctypes.data, n, table.ctypes.data, res['bfu_count'].ctypes.data,
                                                res['allocation'].ctypes.data, res['scale_factor_indices'].ctypes.data,
                                                res['fallback'].ctypes.data))
        res['fallback'] = res['fallback'].astype(bool)
        return res

    def qmf_analysis(self, pcm, halo_frames=0):
        """qmfAnalysisStage, codec/pipeline/encoder.js:57-96: pcm = (halo_frames + frames) * 512 samples of one channel
        -> float32 [frames, 512] (low128 | mid128 | high256)"""
        x = np.ascontiguousarray(pcm, dtype=np.float32)
        frames = x.size // 512 - halo_frames
        out = np.zeros((max(frames, 0), 512), dtype=np.float32)
        capi.check(capi.load().c1_qmf_analysis_batch(self._h, x.ctypes.data, frames, halo_frames, out.ctypes.data))
        return out

    def mdct(self, bands, block_modes, halo_frames=0):
        """mdctStage, encoder.js:170-349: bands float32 [(halo_frames + frames), 512], block_modes int [frames, 3]
        -> (coefficients [frames, 512], the bands as the reference leaves them [frames, 512])"""
        b = np.ascontiguousarray(bands, dtype=np.float32).reshape(-1, 512)
        frames = b.shape[0] - halo_frames
        m = np.ascontiguousarray(block_modes, dtype=np.int32).reshape(-1)
        if m.size != 3 * frames:
            raise ValueError('block_modes must hold three entries per frame')
        co = np.zeros((frames, 512), dtype=np.float32)
        bw = np.zeros((frames, 512), dtype=np.float32)
        capi.check(capi.load().c1_mdct_batch(self._h, b.ctypes.data, frames, halo_frames, m.ctypes.data, co.ctypes.data, bw.ctypes.data))
        return co, bw

    def select_block_modes(self, bands, threshold=1.0, halo_frames=0):
        """blockSelectorStage's detection branch, encoder.js:111-152: bands float32 [(halo_frames + frames), 512] as qmf_analysis
        returns them (the first halo_frames rows: the last frame detection ran on) -> int32 [frames, 3], per band 0 or
        2 | 2 | 3 when its transient score > threshold (options.transientThresholdLow, any float)"""
        b = np.ascontiguousarray(bands, dtype=np.float32).reshape(-1, 512)
        frames = b.shape[0] - halo_frames
        out = np.zeros((max(frames, 0), 3), dtype=np.int32)
        capi.check(capi.load().c1_select_block_modes(self._h, b.ctypes.data, frames, halo_frames, float(threshold), out.ctypes.data))
        return out

    def quantize_frames(self, coefs, block_modes, options=None):
        """quantizationStage, encoder.js:365-418: coefs float32 [frames, 512] as mdct returns them, block_modes int [frames, 3]
        (0 long, anything else short) -> the dict unpack_units returns (block_modes echoed), so that dequantize_frames takes
        it as it stands.  options: EncoderOptions; only allocationBias (its biased table, as encode uses it) is read."""
        c = np.ascontiguousarray(coefs, dtype=np.float32).reshape(-1, 512)
        frames = c.shape[0]
        m = np.ascontiguousarray(block_modes, dtype=np.int32).reshape(-1, 3)
        if m.shape[0] != frames:
            raise ValueError('block_modes must hold three entries per frame of coefs')
        opts = (options or EncoderOptions()).to_c()
        out = {k: np.zeros((frames,) + shape, dtype=np.int32) for k, shape in self.FIELD_SHAPES if k != 'block_modes'}
        capi.check(capi.load().c1_quantize_frames(self._h, c.ctypes.data, frames, m.ctypes.data, C.byref(opts), out['nbfu'].ctypes.data,
                                                   out['sfi'].ctypes.data, out['wl'].ctypes.data, out['quantized'].ctypes.data))
        out['block_modes'] = m.copy()
        return {k: out[k] for k, _ in self.FIELD_SHAPES}

    def pack_units(self, fields):
        """serializeFrame, serialization.js:41-98, over consecutive frames of one channel: a dict of frame fields as
        unpack_units and quantize_frames return it (FIELD_SHAPES) -> uint8 [frames, 212].  nbfu must be 0..52; every other
        value is any int32 and takes the reference's meaning (include/carta1_hip.h, c1_pack_units)."""
        frames = int(np.asarray(fields['nbfu']).size)
        arrs = []
        for k, shape in self.FIELD_SHAPES:
            a = np.ascontiguousarray(fields[k], dtype=np.int32)
            if a.size != frames * int(np.prod(shape, dtype=np.int64)):
                raise ValueError('%s must hold %s entries per frame' % (k, shape or 1))
            arrs.append(a)
        out = np.zeros((frames, 212), dtype=np.uint8)
        capi.check(capi.load().c1_pack_units(self._h, frames, *[a.ctypes.data for a in arrs], out.ctypes.data))
        return out

    # ---- the decoder's pipeline stages (codec/pipeline/decoder.js:52-389, serialization.js:111-176), one channel ------------
    FIELD_SHAPES = (('nbfu', ()), ('block_modes', (3,)), ('sfi', (52,)), ('wl', (52,)), ('quantized', (512,)))

    def unpack_units(self, units):
        """deserializeFrame, serialization.js:111-176, over consecutive units of one channel: uint8 [frames, 212] -> dict of
        int32 arrays nbfu [frames], block_modes [frames, 3], sfi / wl [frames, 52], quantized [frames, 512] (BFU order);
        entries the reference leaves unset are zeros"""
        u = np.ascontiguousarray(units, dtype=np.uint8).reshape(-1, capi.UNIT_BYTES)
        frames = u.shape[0]
        out = {k: np.zeros((frames,) + shape, dtype=np.int32) for k, shape in self.FIELD_SHAPES}
        capi.check(capi.load().c1_unpack_units(self._h, u.ctypes.data, frames, *[out[k].ctypes.data for k, _ in self.FIELD_SHAPES]))
        return out

    def decode_fields(self, fields, channels=1, halo_frames=0):
        """decode() over frame fields (c1_decode_fields_batch): a dict as unpack_units / quantize_frames return it, with
        (halo_frames + frames) * channels units in the order frame * channels + channel (the first halo_frames frames: the
        stream's previous frame) -> a list of float32 arrays of frames * 512 samples, one per channel, as decode returns"""
        arrs = _field_arrays(fields)
        units = arrs[0].size
        if units % channels:
            raise ValueError('the fields must hold whole frames of %d channel(s)' % channels)
        frames = units // channels - halo_frames
        outs = [np.zeros(max(frames, 0) * 512, dtype=np.float32) for _ in range(channels)]
        capi.check(capi.load().c1_decode_fields_batch(self._h, channels, frames, halo_frames,
                                                      *[a.ctypes.data + 4 * halo_frames * channels * int(np.prod(shape, dtype=np.int64))
                                                        for a, (_, shape) in zip(arrs, self.FIELD_SHAPES)],
                                                      capi.ptr_array([o.ctypes.data for o in outs])))
        return outs

    def dequantize_frames(self, fields):
        """dequantizationStage, decoder.js:52-98: a dict of frame fields as unpack_units returns it -> float32 [frames, 512]"""
        frames = int(np.asarray(fields['nbfu']).size)
        arrs = []
        for k, shape in self.FIELD_SHAPES:
            a = np.ascontiguousarray(fields[k], dtype=np.int32)
            if a.size != frames * int(np.prod(shape, dtype=np.int64)):
                raise ValueError('%s must hold %s entries per frame' % (k, shape or 1))
            arrs.append(a)
        out = np.zeros((frames, 512), dtype=np.float32)
        capi.check(capi.load().c1_dequantize_frames(self._h, frames, *[a.ctypes.data for a in arrs], out.ctypes.data))
        return out

    def imdct(self, coefs, block_modes, halo_frames=0):
        """imdctStage, decoder.js:116-330: coefs float32 [(halo_frames + frames), 512], block_modes int [(halo_frames + frames), 3]
        (the first halo_frames rows: the stream's previous frame) -> bands float32 [frames, 512] (low128 | mid128 | high256)"""
        c = np.ascontiguousarray(coefs, dtype=np.float32).reshape(-1, 512)
        frames = c.shape[0] - halo_frames
        m = np.ascontiguousarray(block_modes, dtype=np.int32).reshape(-1)
        if m.size != 3 * c.shape[0]:
            raise ValueError('block_modes must hold three entries per frame of coefs')
        out = np.zeros((max(frames, 0), 512), dtype=np.float32)
        capi.check(capi.load().c1_imdct_batch(self._h, c.ctypes.data, frames, halo_frames, m.ctypes.data, out.ctypes.data))
        return out

    def qmf_synthesis(self, bands, halo_frames=0):
        """qmfSynthesisStage, decoder.js:349-389: bands float32 [(halo_frames + frames), 512] -> PCM float32 [frames, 512]"""
        b = np.ascontiguousarray(bands, dtype=np.float32).reshape(-1, 512)
        frames = b.shape[0] - halo_frames
        out = np.zeros((max(frames, 0), 512), dtype=np.float32)
        capi.check(capi.load().c1_qmf_synthesis_batch(self._h, b.ctypes.data, frames, halo_frames, out.ctypes.data))
        return out

    def encode_frames_from_states(self, pcm, states, options=None, in_place=False):
        """encode(options, pool)(frame) for n independent pools: pcm (n, 512) float32, states (n, 483) float32 rows laid out
        as capi.EncState (qmf_low 46 | qmf_mid 46 | qmf_high 39 | mdct_overlap 3 x 32 | transient_mags 64 | 64 | 128).
        Returns (units (n, 212) uint8, states after the frame (n, 483)); in_place overwrites `states` instead of returning a
        new array.  Non-finite state raises."""
        x = np.ascontiguousarray(pcm, dtype=np.float32).reshape(-1, 512)
        st = _state_rows(states, capi.ENC_STATE_FLOATS, x.shape[0])
        out = st if in_place else np.empty_like(st)
        units = np.zeros((x.shape[0], 212), dtype=np.uint8)
        opts = (options or EncoderOptions()).to_c()
        capi.check(capi.load().c1_encode_frames_from_states(self._h, x.shape[0], x.ctypes.data, st.ctypes.data, C.byref(opts),
                                                            units.ctypes.data, out.ctypes.data))
        return units, out

    def decode_frames_from_states(self, units, states, in_place=False):
        """decode(pool)(unit) for n independent pools: units (n, 212) uint8, states (n, 179) float32 rows laid out as
        capi.DecState (qmf_low 46 | qmf_mid 46 | qmf_high 39 | imdct_tail 3 x 16).  Returns (pcm (n, 512) float32, states
        after the frame (n, 179))."""
        u = np.ascontiguousarray(units, dtype=np.uint8).reshape(-1, 212)
        st = _state_rows(states, capi.DEC_STATE_FLOATS, u.shape[0])
        out = st if in_place else np.empty_like(st)
        pcm = np.zeros((u.shape[0], 512), dtype=np.float32)
        capi.check(capi.load().c1_decode_frames_from_states(self._h, u.shape[0], u.ctypes.data, st.ctypes.data, pcm.ctypes.data,
                                                            out.ctypes.data))
        return pcm, out

    # ---- n signals of any lengths, each from its own pool, in one call (include/carta1_hip.h, c1_*_signals*) ----
    def encode_signals(self, signals, options=None, states=None, return_states=False, in_place=False):
        """signals: a list of float32 arrays, each one mono signal (zero padded to whole frames, as encode_pcm pads).  Signal i
        is encoded as its own stream from states[i] ((n, 483) float32 rows laid out as capi.EncState; None: fresh pools).
        Returns a list of (frames_i, 212) uint8 arrays, and with return_states the (n, 483) pools after every signal's last
        frame as well; in_place writes those into `states`.  An empty signal gives no units and its pool unchanged."""
        pcm, off = signals_layout([pad_signal(x) for x in signals])
        n = off.size - 1
        st = None if states is None else _state_rows(states, capi.ENC_STATE_FLOATS, n)
        if in_place and st is None:
            raise ValueError('in_place needs states')
        out = st if in_place else (np.zeros((n, capi.ENC_STATE_FLOATS), dtype=np.float32) if return_states else None)
        units = np.zeros((int(off[-1]), 212), dtype=np.uint8)
        opts = (options or EncoderOptions()).to_c()
        capi.check(capi.load().c1_encode_signals(self._h, n, off.ctypes.data_as(C.POINTER(C.c_int64)), pcm.ctypes.data,
                                                 st.ctypes.data if st is not None else None, C.byref(opts), units.ctypes.data,
                                                 out.ctypes.data if out is not None else None))
        res = split_rows(units, off)
        return (res, out) if (return_states or in_place) else res

    def decode_signals(self, units_list, states=None, return_states=False, in_place=False):
        """units_list: a list of (frames_i, 212) uint8 arrays, each one mono signal's sound units; states: (n, 179) float32 rows
        laid out as capi.DecState, or None for fresh pools.  Returns a list of float32 arrays of frames_i * 512 samples, and
        with return_states the (n, 179) pools after every signal's last unit."""
        rows = [np.ascontiguousarray(u, dtype=np.uint8).reshape(-1, 212) for u in units_list]
        off = np.zeros(len(rows) + 1, dtype=np.int64)
        if rows:
            off[1:] = np.cumsum([r.shape[0] for r in rows])
        u = np.concatenate(rows) if rows else np.zeros((0, 212), dtype=np.uint8)
        u = np.ascontiguousarray(u)
        n = len(rows)
        st = None if states is None else _state_rows(states, capi.DEC_STATE_FLOATS, n)
        if in_place and st is None:
            raise ValueError('in_place needs states')
        out = st if in_place else (np.zeros((n, capi.DEC_STATE_FLOATS), dtype=np.float32) if return_states else None)
        pcm = np.zeros(int(off[-1]) * 512, dtype=np.float32)
        capi.check(capi.load().c1_decode_signals(self._h, n, off.ctypes.data_as(C.POINTER(C.c_int64)), u.ctypes.data,
                                                 st.ctypes.data if st is not None else None, pcm.ctypes.data,
                                                 out.ctypes.data if out is not None else None))
        res = [pcm[int(off[i]) * 512:int(off[i + 1]) * 512] for i in range(n)]
        return (res, out) if (return_states or in_place) else res

    def encode_signals_device(self, frame_offsets, pcm_ptr, units_ptr, states_ptr=None, out_states_ptr=None, options=None,
                              c_options=None):
        """raw device pointers (e.g. torch tensor .data_ptr()); frame_offsets: n + 1 host integers.  Asynchronous on the
        context's stream."""
        off = np.ascontiguousarray(frame_offsets, dtype=np.int64)
        opts = c_options if c_options is not None else (options or EncoderOptions()).to_c()
        capi.check(capi.load().c1_encode_signals_device(
            self._h, off.size - 1, off.ctypes.data_as(C.POINTER(C.c_int64)), C.c_void_p(pcm_ptr),
            C.c_void_p(states_ptr) if states_ptr else None, C.byref(opts), C.c_void_p(units_ptr),
            C.c_void_p(out_states_ptr) if out_states_ptr else None))

    def encode_signals_measured(self, signals, modes=None, options=None, states=None, return_states=False, in_place=False,
                                scale_factor_offsets=None, masking=None, return_distortion=False, return_shifts=False,
                                return_weights=False):
        """encode_signals() with the measured allocation of encode_measured() (c1_encode_signals_measured): signal i's rows are
        what EncoderStream.push_measured reports for it in one push on a mono stream restored to states[i] (or fresh).  modes:
        None, or one array of mode bytes per signal, one byte per frame (as for encode_modes()).  scale_factor_offsets, masking,
        the return_* flags and their ValueErrors are encode_measured()'s.  Returns per-signal lists in encode_measured()'s result
        order -- (units, taken[, shifts][, distortion, energy][, weights]) -- and last, with return_states or in_place, the
        (n, 483) pools after every signal's last frame."""
        pcm, off = signals_layout([pad_signal(x) for x in signals])
        n = off.size - 1
        total = int(off[-1])
        st = None if states is None else _state_rows(states, capi.ENC_STATE_FLOATS, n)
        if in_place and st is None:
            raise ValueError('in_place needs states')
        m = None
        if modes is not None:
            if len(modes) != n:
                raise ValueError('modes must hold one array of mode bytes per signal: %d arrays for %d signals' % (len(modes), n))
            rows = [check_block_modes(modes[i], int(off[i + 1] - off[i]), 1).reshape(-1) for i in range(n)]
            m = np.ascontiguousarray(np.concatenate(rows) if rows else np.zeros(0, dtype=np.uint8), dtype=np.uint8)
        if return_shifts and scale_factor_offsets is None:
            raise ValueError('return_shifts needs scale_factor_offsets')
        if return_weights and masking is None:
            raise ValueError('return_weights needs masking')
        mask = None if masking is None else check_masking(masking)
        offs = None if scale_factor_offsets is None else check_scale_factor_offsets(scale_factor_offsets)
        out = st if in_place else (np.zeros((n, capi.ENC_STATE_FLOATS), dtype=np.float32) if return_states else None)
        units = np.zeros((total, 212), dtype=np.uint8)
        taken = np.zeros(total, dtype=np.uint8)
        shifts = np.zeros((total, 52), dtype=np.int8) if return_shifts else None
        dist = np.zeros((total, 2), dtype=np.float64) if return_distortion else None
        energy = np.zeros(total, dtype=np.float64) if return_distortion else None
        weights = np.zeros((total, 52), dtype=np.float64) if return_weights else None
        opts = (options or EncoderOptions()).to_c()
        data = lambda a: None if a is None else a.ctypes.data
        capi.check(capi.load().c1_encode_signals_measured(
            self._h, n, off.ctypes.data_as(C.POINTER(C.c_int64)), pcm.ctypes.data, data(st), C.byref(opts), data(m), data(offs),
            0 if offs is None else len(offs), None if mask is None else mask[0].ctypes.data, None if mask is None else data(mask[1]),
            units.ctypes.data, data(out), taken.ctypes.data, data(shifts), data(dist), data(energy), data(weights)))
        res = (split_rows(units, off), split_rows(taken, off)) + ((split_rows(shifts, off),) if return_shifts else ())
        res = res + (split_rows(dist, off), split_rows(energy, off)) if return_distortion else res
        res = res + (split_rows(weights, off),) if return_weights else res
        return res + (out,) if (return_states or in_place) else res

    def encode_signals_measured_device(self, frame_offsets, pcm_ptr, units_ptr=None, states_ptr=None, out_states_ptr=None, options=None,
                                       modes_ptr=None, scale_factor_offsets=None, masking=None, taken_ptr=None, shifts_ptr=None,
                                       distortion_ptr=None, energy_ptr=None, weights_ptr=None):
        """c1_encode_signals_measured_device: raw device pointers as for encode_signals_device; frame_offsets, the offsets and the
        masking tables are host values (as for encode_measured_device, the library's own checks decide).  Every output may be
        None, not all; modes_ptr = one mode byte per frame of the concatenation on the device, or None.  Asynchronous on the
        context's stream."""
        off = np.ascontiguousarray(frame_offsets, dtype=np.int64)
        opts = (options or EncoderOptions()).to_c()
        vp = lambda p: C.c_void_p(p) if p else None
        mask = None if masking is None else check_masking(masking, check=False)
        offs = None if scale_factor_offsets is None else check_scale_factor_offsets(scale_factor_offsets, check=False)
        capi.check(capi.load().c1_encode_signals_measured_device(
            self._h, off.size - 1, off.ctypes.data_as(C.POINTER(C.c_int64)), vp(pcm_ptr), vp(states_ptr), C.byref(opts), vp(modes_ptr),
            offs.ctypes.data if offs is not None and len(offs) else None, 0 if offs is None else len(offs),
            None if mask is None else mask[0].ctypes.data, None if mask is None or mask[1] is None else mask[1].ctypes.data,
            vp(units_ptr), vp(out_states_ptr), vp(taken_ptr), vp(shifts_ptr), vp(distortion_ptr), vp(energy_ptr), vp(weights_ptr)))

    def encode_signals_measured_modes(self, signals, candidates, options=None, states=None, return_states=False, in_place=False,
                                      scale_factor_offsets=None, return_distortion=False, return_shifts=False):
        """encode_signals() with the measured block-mode search of encode_measured_modes() (c1_encode_signals_measured_modes):
        signal i's rows are what EncoderStream.push_measured_modes reports for it in one push on a mono stream restored to
        states[i] (or fresh).  candidates, scale_factor_offsets (None: the plain measured allocation), the return_* flags and
        their ValueErrors are encode_measured_modes()'s.  Returns per-signal lists in encode_measured_modes()'s result order --
        (units, choice, modes, taken[, shifts][, distortion, energy]) -- and last, with return_states or in_place, the (n, 483)
        pools after every signal's last frame."""
        pcm, off = signals_layout([pad_signal(x) for x in signals])
        n = off.size - 1
        total = int(off[-1])
        st = None if states is None else _state_rows(states, capi.ENC_STATE_FLOATS, n)
        if in_place and st is None:
            raise ValueError('in_place needs states')
        cand = mode_candidates(candidates)
        count = len(cand)
        offs = None if scale_factor_offsets is None else check_scale_factor_offsets(scale_factor_offsets)
        out = st if in_place else (np.zeros((n, capi.ENC_STATE_FLOATS), dtype=np.float32) if return_states else None)
        units = np.zeros((total, 212), dtype=np.uint8)
        choice = np.zeros(total, dtype=np.uint8)
        modes = np.zeros(total, dtype=np.uint8)
        taken = np.zeros(total, dtype=np.uint8)
        shifts = np.zeros((total, 52), dtype=np.int8) if return_shifts else None
        dist = np.zeros((total, count, 2), dtype=np.float64) if return_distortion else None
        energy = np.zeros((total, count), dtype=np.float64) if return_distortion else None
        opts = (options or EncoderOptions()).to_c()
        data = lambda a: None if a is None else a.ctypes.data
        capi.check(capi.load().c1_encode_signals_measured_modes(
            self._h, n, off.ctypes.data_as(C.POINTER(C.c_int64)), pcm.ctypes.data, data(st), C.byref(opts), cand.ctypes.data, count,
            data(offs), 0 if offs is None else len(offs), units.ctypes.data, data(out), choice.ctypes.data, modes.ctypes.data,
            taken.ctypes.data, data(shifts), data(dist), data(energy)))
        res = (split_rows(units, off), split_rows(choice, off), split_rows(modes, off), split_rows(taken, off))
        res = res + (split_rows(shifts, off),) if return_shifts else res
        res = res + (split_rows(dist, off), split_rows(energy, off)) if return_distortion else res
        return res + (out,) if (return_states or in_place) else res

    def encode_signals_measured_modes_device(self, frame_offsets, pcm_ptr, candidates, units_ptr=None, states_ptr=None,
                                             out_states_ptr=None, options=None, scale_factor_offsets=None, choice_ptr=None,
                                             modes_ptr=None, taken_ptr=None, shifts_ptr=None, distortion_ptr=None, energy_ptr=None):
        """c1_encode_signals_measured_modes_device: raw device pointers as for encode_signals_device; frame_offsets, the
        candidates and the offsets are host values (as for encode_measured_modes_device, the library's own checks decide; None
        for no offsets).  Every output may be None, not all; choice, modes and taken are uint8 [frames], shifts int8 [frames,
        52], distortion float64 [frames, n, 2] and energy float64 [frames, n].  Asynchronous on the context's stream."""
        off = np.ascontiguousarray(frame_offsets, dtype=np.int64)
        opts = (options or EncoderOptions()).to_c()
        vp = lambda p: C.c_void_p(p) if p else None
        cand = mode_candidates(candidates, check=False)
        offs = None if scale_factor_offsets is None else check_scale_factor_offsets(scale_factor_offsets, check=False)
        capi.check(capi.load().c1_encode_signals_measured_modes_device(
            self._h, off.size - 1, off.ctypes.data_as(C.POINTER(C.c_int64)), vp(pcm_ptr), vp(states_ptr), C.byref(opts),
            cand.ctypes.data if len(cand) else None, len(cand), offs.ctypes.data if offs is not None and len(offs) else None,
            0 if offs is None else len(offs), vp(units_ptr), vp(out_states_ptr), vp(choice_ptr), vp(modes_ptr), vp(taken_ptr),
            vp(shifts_ptr), vp(distortion_ptr), vp(energy_ptr)))

    def decode_signals_device(self, frame_offsets, units_ptr, pcm_ptr, states_ptr=None, out_states_ptr=None):
        off = np.ascontiguousarray(frame_offsets, dtype=np.int64)
        capi.check(capi.load().c1_decode_signals_device(
            self._h, off.size - 1, off.ctypes.data_as(C.POINTER(C.c_int64)), C.c_void_p(units_ptr),
            C.c_void_p(states_ptr) if states_ptr else None, C.c_void_p(pcm_ptr),
            C.c_void_p(out_states_ptr) if out_states_ptr else None))

    def pack_spec_tap_device(self, coefs_ptr, eps_ptr, side_ptr, alloc_ptr, units, units_out_ptr, lists_ptr, all_long=True):
        """Test tap: the speculative quantizer + packer on caller-supplied coefficients, bounds and records (device pointers)."""
        capi.check(capi.load().c1_pack_spec_tap_device(
            self._h, C.c_void_p(coefs_ptr), C.c_void_p(eps_ptr), C.c_void_p(side_ptr), C.c_void_p(alloc_ptr), units,
            1 if all_long else 0, C.c_void_p(units_out_ptr), C.c_void_p(lists_ptr)))


def encode_multi(channels, options=None, devices=(0,), out=None):
    """c1_encode_batch_multi: the batch sharded over `devices` (contiguous frame ranges, one host thread and context
    per entry, no collective).  channels: a stream from its start.  Same bytes as one device produces.
    out: a C-contiguous uint8 array of frames * channels * 212 bytes to write into (as Context.encode takes)."""
    opts = (options or EncoderOptions()).to_c()
    chans = [np.ascontiguousarray(c, dtype=np.float32) for c in channels]
    n = len(chans[0])
    if any(len(c) != n for c in chans) or n % 512:
        raise ValueError('channels must have equal length, a multiple of 512')
    frames = n // 512
    if out is None:
        units = np.zeros((frames * len(chans), 212), dtype=np.uint8)
    else:
        units = out
        if units.dtype != np.uint8 or not units.flags.c_contiguous or units.size != frames * len(chans) * 212:
            raise ValueError('out must be a C-contiguous uint8 array of frames * channels * 212 bytes')
    devs = (C.c_int * len(devices))(*[int(d) for d in devices])
    capi.check(capi.load().c1_encode_batch_multi(devs, len(devices), capi.ptr_array([c.ctypes.data for c in chans]),
                                                 len(chans), frames, 0, C.byref(opts), units.ctypes.data))
    return units


def decode_multi(units, channels, devices=(0,), out=None):
    """c1_decode_batch_multi: units of a stream from its start -> list of float32 arrays (out: such a list to write into)."""
    u = np.ascontiguousarray(units, dtype=np.uint8).reshape(-1, 212)
    frames = u.shape[0] // channels
    if out is None:
        outs = [np.zeros(frames * 512, dtype=np.float32) for _ in range(channels)]
    else:
        outs = list(out)
        if len(outs) != channels or any(o.dtype != np.float32 or not o.flags.c_contiguous or o.size != frames * 512 for o in outs):
            raise ValueError('out must be one C-contiguous float32 array of frames * 512 samples per channel')
    devs = (C.c_int * len(devices))(*[int(d) for d in devices])
    capi.check(capi.load().c1_decode_batch_multi(devs, len(devices), u.ctypes.data, channels, frames, 0,
                                                 capi.ptr_array([o.ctypes.data for o in outs])))
    return outs


class EncoderStream:
    """What one encode() closure per channel + BufferPool is in the reference: push frames, get units,
    state carried on the device between calls."""

    def __init__(self, ctx, channels=1, options=None):
        self._ctx, self.channels = ctx, channels
        self._h = C.c_void_p()
        opts = (options or EncoderOptions()).to_c()
        capi.check(capi.load().c1_enc_stream_create(ctx._h, channels, C.byref(opts), C.byref(self._h)))

    def push(self, channels, modes=None, biases=None):
        """modes: None, or the block modes of the pushed frames (uint8 [frames, nch] or flat, as for
        Context.encode_modes): those frames are encoded as the reference encodes them with fixedBlockModes set frame by
        frame and put back afterwards; the stream's options and its detection history stay as they are.
        biases: None, or the allocation bias of the pushed frames (one per frame or [frames, nch], as for
        Context.encode_biases): those frames allocate as the reference does with allocationBias set frame by frame; the
        stream's options stay as they are."""
        chans = [np.ascontiguousarray(c, dtype=np.float32) for c in channels]
        if len(chans) != self.channels:
            raise ValueError('expected %d channels' % self.channels)
        frames = len(chans[0]) // 512
        units = np.zeros((frames * self.channels, 212), dtype=np.uint8)
        ptrs = capi.ptr_array([c.ctypes.data for c in chans])
        if biases is not None:
            palette, index = bias_palette(biases, frames, self.channels, None)
            m = None if modes is None else check_block_modes(modes, frames, self.channels)
            capi.check(capi.load().c1_enc_stream_push_biases(self._h, ptrs, frames, palette, len(palette), index.ctypes.data,
                                                             None if m is None else m.ctypes.data, units.ctypes.data))
        elif modes is None:
            capi.check(capi.load().c1_enc_stream_push(self._h, ptrs, frames, units.ctypes.data))
        else:
            m = check_block_modes(modes, frames, self.channels)
            capi.check(capi.load().c1_enc_stream_push_modes(self._h, ptrs, frames, m.ctypes.data, units.ctypes.data))
        return units

    def push_measured(self, channels, modes=None, scale_factor_offsets=None, masking=None, return_distortion=False,
                      return_shifts=False, return_weights=False):
        """push() with the word lengths (and, with scale_factor_offsets, the scale-factor indices) of every pushed unit
        allocated by the measured coding error: Context.encode_measured on a live stream (c1_enc_stream_push_measured).  The
        analysis, the block modes and the reference's own record per unit are push()'s (push(modes=...)'s when modes is
        given); the measured allocation keeps no state, so the stream afterwards is what it is after the plain push and the
        kinds of push may be mixed.  modes, scale_factor_offsets, masking, the return_* flags, their ValueErrors and the
        result -- (units, taken[, shifts][, distortion, energy][, weights]) -- are Context.encode_measured's."""
        chans = [np.ascontiguousarray(c, dtype=np.float32) for c in channels]
        if len(chans) != self.channels:
            raise ValueError('expected %d channels' % self.channels)
        n = len(chans[0])
        if any(len(c) != n for c in chans) or n % 512:
            raise ValueError('channels must have equal length, a multiple of 512')
        frames = n // 512
        m = None if modes is None else check_block_modes(modes, frames, self.channels)
        if return_shifts and scale_factor_offsets is None:
            raise ValueError('return_shifts needs scale_factor_offsets')
        if return_weights and masking is None:
            raise ValueError('return_weights needs masking')
        mask = None if masking is None else check_masking(masking)
        offs = None if scale_factor_offsets is None else check_scale_factor_offsets(scale_factor_offsets)
        count = frames * self.channels
        units = np.zeros((count, 212), dtype=np.uint8)
        taken = np.zeros(count, dtype=np.uint8)
        shifts = np.zeros((count, 52), dtype=np.int8) if return_shifts else None
        dist = np.zeros((count, 2), dtype=np.float64) if return_distortion else None
        energy = np.zeros(count, dtype=np.float64) if return_distortion else None
        weights = np.zeros((count, 52), dtype=np.float64) if return_weights else None
        data = lambda a: None if a is None else a.ctypes.data
        capi.check(capi.load().c1_enc_stream_push_measured(
            self._h, capi.ptr_array([c.ctypes.data for c in chans]), frames, data(m), data(offs), 0 if offs is None else len(offs),
            None if mask is None else mask[0].ctypes.data, None if mask is None else data(mask[1]), units.ctypes.data,
            taken.ctypes.data, data(shifts), data(dist), data(energy), data(weights)))
        out = (units, taken) + ((shifts,) if return_shifts else ())
        out = out + (dist, energy) if return_distortion else out
        return out + (weights,) if return_weights else out

    def push_measured_modes(self, channels, candidates, scale_factor_offsets=None, return_distortion=False, return_shifts=False,
                            masking=None, return_weights=False):
        """push_measured() with the block modes of every pushed unit chosen among `candidates` by the final error of the measured
        allocation under each: Context.encode_measured_modes on a live stream (c1_enc_stream_push_measured_modes).  Per (unit,
        candidate) the figures are push_measured(modes=constant byte, ...)'s on a twin stream; the units are
        push_measured(modes=modes, ...)'s, and the stream afterwards is what it is after push(modes=modes), so the kinds of push
        may be mixed.  For a stream pushed from its start the rows are Context.encode_measured_modes' over the whole signal.
        candidates, scale_factor_offsets, the return_* flags, their ValueErrors and the result -- (units, choice, modes,
        taken[, shifts][, distortion, energy]) -- are Context.encode_measured_modes'.  masking and return_weights are that call's
        too (c1_enc_stream_push_measured_modes_masked): one masking threshold per unit weighs every candidate, and weights ends
        the result; None takes the call above, untouched."""
        chans = [np.ascontiguousarray(c, dtype=np.float32) for c in channels]
        if len(chans) != self.channels:
            raise ValueError('expected %d channels' % self.channels)
        n = len(chans[0])
        if any(len(c) != n for c in chans) or n % 512:
            raise ValueError('channels must have equal length, a multiple of 512')
        frames = n // 512
        cand = mode_candidates(candidates)
        count = len(cand)
        if return_weights and masking is None:
            raise ValueError('return_weights needs masking')
        mask = None if masking is None else check_masking(masking)
        offs = None if scale_factor_offsets is None else check_scale_factor_offsets(scale_factor_offsets)
        total = frames * self.channels
        units = np.zeros((total, 212), dtype=np.uint8)
        choice = np.zeros(total, dtype=np.uint8)
        modes = np.zeros(total, dtype=np.uint8)
        taken = np.zeros(total, dtype=np.uint8)
        shifts = np.zeros((total, 52), dtype=np.int8) if return_shifts else None
        dist = np.zeros((total, count, 2), dtype=np.float64) if return_distortion else None
        energy = np.zeros((total, count), dtype=np.float64) if return_distortion else None
        data = lambda a: None if a is None else a.ctypes.data
        if mask is not None:
            weights = np.zeros((total, 52), dtype=np.float64) if return_weights else None
            capi.check(capi.load().c1_enc_stream_push_measured_modes_masked(
                self._h, capi.ptr_array([c.ctypes.data for c in chans]), frames, cand.ctypes.data, count, data(offs),
                0 if offs is None else len(offs), mask[0].ctypes.data, data(mask[1]), units.ctypes.data, choice.ctypes.data,
                modes.ctypes.data, taken.ctypes.data, data(shifts), data(dist), data(energy), data(weights)))
            out = (units, choice, modes, taken) + ((shifts,) if return_shifts else ())
            out = out + (dist, energy) if return_distortion else out
            return out + (weights,) if return_weights else out
        capi.check(capi.load().c1_enc_stream_push_measured_modes(
            self._h, capi.ptr_array([c.ctypes.data for c in chans]), frames, cand.ctypes.data, count, data(offs),
            0 if offs is None else len(offs), units.ctypes.data, choice.ctypes.data, modes.ctypes.data, taken.ctypes.data, data(shifts),
            data(dist), data(energy)))
        out = (units, choice, modes, taken) + ((shifts,) if return_shifts else ())
        return out + (dist, energy) if return_distortion else out

    def set_options(self, options):
        """The options of every channel from the next push on, as the reference's encode() reads them on every call; the
        stream goes on (include/carta1_hip.h, c1_enc_stream_set_options).  Invalid options raise and change nothing."""
        opts = options.to_c()
        capi.check(capi.load().c1_enc_stream_set_options(self._h, C.byref(opts)))

    def get_state(self):
        """The stream's state in the reference's BufferPool layout: a (channels, 483) float32 array, one capi.EncState per
        row -- what the reference's pool would hold after the same pushes, option changes and restores (zeros when fresh)."""
        out = np.zeros((self.channels, capi.ENC_STATE_FLOATS), dtype=np.float32)
        capi.check(capi.load().c1_enc_stream_get_state(self._h, out.ctypes.data))
        return out

    def set_state(self, states):
        """Replace the whole state of every channel, also mid-stream; the following pushes continue as the reference's
        encode() continues from that pool.  states: (channels, 483) float32 (or anything np.asarray turns into it, a ctypes
        array of capi.EncState included).  Non-finite entries raise and leave the stream as it was."""
        st = _state_rows(states, capi.ENC_STATE_FLOATS, self.channels)
        capi.check(capi.load().c1_enc_stream_set_state(self._h, st.ctypes.data))

    def close(self):
        if self._h:
            capi.load().c1_enc_stream_destroy(self._h)
            self._h = C.c_void_p()


class DecoderStream:
    def __init__(self, ctx, channels=1):
        self._ctx, self.channels = ctx, channels
        self._h = C.c_void_p()
        capi.check(capi.load().c1_dec_stream_create(ctx._h, channels, C.byref(self._h)))

    def push(self, units):
        u = np.ascontiguousarray(units, dtype=np.uint8).reshape(-1, 212)
        frames = u.shape[0] // self.channels
        outs = [np.zeros(frames * 512, dtype=np.float32) for _ in range(self.channels)]
        capi.check(capi.load().c1_dec_stream_push(self._h, u.ctypes.data, frames,
                                                  capi.ptr_array([o.ctypes.data for o in outs])))
        return outs

    def push_fields(self, fields):
        """frame fields (the dict unpack_units returns, unit index frame * channels + channel) continuing the same stream as
        push: any interleaving of the two decodes as one call over all frames would"""
        arrs = _field_arrays(fields)
        frames = arrs[0].size // self.channels
        if arrs[0].size != frames * self.channels:
            raise ValueError('the fields must hold whole frames of %d channel(s)' % self.channels)
        outs = [np.zeros(frames * 512, dtype=np.float32) for _ in range(self.channels)]
        capi.check(capi.load().c1_dec_stream_push_fields(self._h, frames, *[a.ctypes.data for a in arrs],
                                                         capi.ptr_array([o.ctypes.data for o in outs])))
        return outs

    def get_state(self):
        """(channels, 179) float32, one capi.DecState per row: the decoder half of the reference's pool after the same pushes"""
        out = np.zeros((self.channels, capi.DEC_STATE_FLOATS), dtype=np.float32)
        capi.check(capi.load().c1_dec_stream_get_state(self._h, out.ctypes.data))
        return out

    def set_state(self, states):
        """Replace the decoder state of every channel; unit and field pushes continue from it, in any interleaving"""
        st = _state_rows(states, capi.DEC_STATE_FLOATS, self.channels)
        capi.check(capi.load().c1_dec_stream_set_state(self._h, st.ctypes.data))

    def close(self):
        if self._h:
            capi.load().c1_dec_stream_destroy(self._h)
            self._h = C.c_void_p()


# ---- AEA container: codec/io/serialization.js:182-254 -------------------------------------------------
# ---- block modes as bytes: m0 | m1 << 2 | m2 << 4, the detector taps' format and c1_encode_modes_*'s ------------------
_MODE_FIELDS = ('low', 'mid', 'high')


def pack_block_modes(triples):
    """[n, 3] (or one triple) of block modes as blockSelectorStage returns them -> uint8 [n] mode bytes."""
    t = np.asarray(triples, dtype=np.int64).reshape(-1, 3)
    if ((t < 0) | (t > 3)).any():
        raise ValueError('block modes must be 0..3')
    return (t[:, 0] | (t[:, 1] << 2) | (t[:, 2] << 4)).astype(np.uint8)


def unpack_block_modes(mode_bytes):
    """uint8 mode bytes (any shape) -> int array [n, 3]: low, mid, high field of each."""
    b = np.asarray(mode_bytes, dtype=np.uint8).reshape(-1).astype(np.int64)
    return np.stack([b & 3, (b >> 2) & 3, (b >> 4) & 3], axis=1)


def check_block_modes(modes, frames, channels):
    """modes as a contiguous uint8 array of frames * channels bytes, every one inside blockSelectorStage's domain (low and
    mid field 0 or 2, high field 0 or 3, bits 6-7 clear); ValueError naming the first offender's frame, channel and field."""
    m = np.ascontiguousarray(modes)
    if m.dtype != np.uint8:
        if m.size and ((m < 0) | (m > 255)).any():
            raise ValueError('mode bytes must be 0..255')
        m = m.astype(np.uint8)
    m = m.reshape(-1)
    if m.size != frames * channels:
        raise ValueError('modes must hold frames * channels = %d bytes, got %d' % (frames * channels, m.size))
    bad = np.flatnonzero(((m & 0xC5) != 0) | (((m & 0x30) != 0) & ((m & 0x30) != 0x30)))
    if bad.size:
        i = int(bad[0])
        b = int(m[i])
        where = 'frame %d, channel %d' % (i // channels, i % channels) if channels == 2 else 'frame %d' % i
        for k, name in enumerate(_MODE_FIELDS):
            f, other = (b >> (2 * k)) & 3, 3 if k == 2 else 2
            if f not in (0, other):
                raise ValueError('%s: %s field of mode byte 0x%02x is %d, not 0 or %d' % (where, name, b, f, other))
        raise ValueError('%s: bits 6-7 of mode byte 0x%02x are set' % (where, b))
    return m


# ---- the block modes per sound unit chosen among candidates (c1_encode_best_modes_*) ------------------------------------
MAX_MODE_CANDIDATES = 8


def mode_candidates(candidates, check=True):
    """the candidates of Context.encode_best_modes -> uint8 mode bytes in the caller's order.  An entry is a mode byte or a
    triple as pack_block_modes() takes it.  check: ValueError for none, for more than MAX_MODE_CANDIDATES, for an entry
    outside the domain of encode_modes() (naming it) and for a byte given twice; without it the library's own check decides."""
    out = []
    for v in list(candidates):
        if isinstance(v, (int, np.integer)):
            if not 0 <= int(v) <= 255:
                raise ValueError('mode bytes must be 0..255')
            out.append(int(v))
        else:
            out.append(int(pack_block_modes(v)[0]) if np.asarray(v).size == 3 else -1)
            if out[-1] < 0:
                raise ValueError('a candidate must be a mode byte or a triple of block modes')
    if check:
        if not 1 <= len(out) <= MAX_MODE_CANDIDATES:
            raise ValueError('between 1 and %d candidate block modes per call, got %d' % (MAX_MODE_CANDIDATES, len(out)))
        for i, b in enumerate(out):
            for k, name in enumerate(_MODE_FIELDS):
                f, other = (b >> (2 * k)) & 3, 3 if k == 2 else 2
                if f not in (0, other):
                    raise ValueError('candidate %d: %s field of mode byte 0x%02x is %d, not 0 or %d' % (i, name, b, f, other))
            if b & 0xC0:
                raise ValueError('candidate %d: bits 6-7 of mode byte 0x%02x are set' % (i, b))
            if b in out[:i]:
                raise ValueError('candidate %d: mode byte 0x%02x is given twice' % (i, b))
    return np.ascontiguousarray(out, dtype=np.uint8).reshape(-1)


# ---- the scale-factor index of every BFU chosen among findScaleFactor + offset (c1_encode_measured_sf_*) ------------------
MAX_SCALE_FACTOR_OFFSETS = 8
SCALE_FACTOR_OFFSETS = (0, -1, 1, -2, -3)       # the suggested set: offsets below -3 add 0.03 dB at most


def check_scale_factor_offsets(offsets, check=True):
    """the offsets of Context.encode_measured(scale_factor_offsets=...) -> int8 array in the caller's order.  check: ValueError
    for none, for more than MAX_SCALE_FACTOR_OFFSETS, for a value outside -8..8, for a value given twice and for a first value
    other than 0; without it the library's own check decides."""
    out = [int(v) for v in list(offsets)]
    if any(not -128 <= v <= 127 for v in out):
        raise ValueError('scale-factor offsets must be within -8..8')
    if check:
        if not 1 <= len(out) <= MAX_SCALE_FACTOR_OFFSETS:
            raise ValueError('between 1 and %d scale-factor offsets per call, got %d' % (MAX_SCALE_FACTOR_OFFSETS, len(out)))
        for i, v in enumerate(out):
            if not -8 <= v <= 8:
                raise ValueError('scale-factor offset %d is %d, outside -8..8' % (i, v))
            if v in out[:i]:
                raise ValueError('scale-factor offset %d: %d is given twice' % (i, v))
        if out[0] != 0:
            raise ValueError('the first scale-factor offset must be 0 (the reference\'s own index), got %d' % out[0])
    return np.ascontiguousarray(out, dtype=np.int8).reshape(-1)


# ---- every BFU's error weighted by a masking threshold (c1_encode_measured_masked_*) ---------------------------------------
_MASKING = None


def _packaged_masking():
    """carta1_amd/masking_default.json (tools/make_masking_tables.py): (floor float64 [52], spread float64 [52, 52]), read-only"""
    global _MASKING
    if _MASKING is None:
        import json
        import os
        raw = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'masking_default.json')))
        val = lambda h: struct.unpack('>d', bytes.fromhex(h))[0]
        floor = np.array([val(h) for h in raw['floor_f64']], dtype=np.float64)
        spread = np.array([[val(h) for h in row] for row in raw['spread_f64']], dtype=np.float64)
        floor.setflags(write=False)
        spread.setflags(write=False)
        _MASKING = (floor, spread)
    return _MASKING


MASKING_DEFAULT = _packaged_masking()             # Schroeder spreading on the Bark scale, Terhardt's threshold in quiet


def check_masking(masking, check=True):
    """the masking of Context.encode_measured(masking=...) -> (floor float64 [52], spread float64 [52, 52] or None), contiguous.
    masking: True (the packaged tables) or a (floor, spread or None) pair.  check: ValueError naming the table and the index for a
    floor that is not finite and within [1e-60, 1e60] or a spread entry that is not finite and within [0, 1e60]; without it
    the library's own check decides."""
    if masking is True:
        masking = _packaged_masking()
    if masking is False or masking is None or len(masking) != 2:
        raise ValueError('masking must be True or a (floor, spread) pair')
    floor = np.ascontiguousarray(masking[0], dtype=np.float64).reshape(-1)
    spread = None if masking[1] is None else np.ascontiguousarray(masking[1], dtype=np.float64)
    if floor.size != 52:
        raise ValueError('masking: the floor must hold 52 values, got %d' % floor.size)
    if spread is not None:
        if spread.size != 52 * 52:
            raise ValueError('masking: the spread must hold 52 x 52 values, got %d' % spread.size)
        spread = spread.reshape(52, 52)
    if check:
        bad = np.flatnonzero(~((floor >= 1e-60) & (floor <= 1e60)))
        if bad.size:
            raise ValueError('masking: mask_floor[%d] = %r is outside [1e-60, 1e60]' % (bad[0], float(floor[bad[0]])))
        if spread is not None:
            bad = np.flatnonzero(~((spread.reshape(-1) >= 0.0) & (spread.reshape(-1) <= 1e60)))
            if bad.size:
                raise ValueError('masking: mask_spread[%d] = %r is outside [0, 1e60]' % (bad[0], float(spread.reshape(-1)[bad[0]])))
    return floor, spread


# ---- the coding error of given sound units (c1_measure_units_*) --------------------------------------------------------------
def check_threshold_from(threshold_from, masking):
    """threshold_from of Context.measure_units -> True for 'long' (c1_measure_units_shared_*), False for 'own'.  ValueError for
    anything else and for 'long' without masking: the all-long threshold is made of the tables."""
    if threshold_from not in ('own', 'long'):
        raise ValueError("threshold_from must be 'own' or 'long', got %r" % (threshold_from,))
    if threshold_from == 'long' and masking is None:
        raise ValueError("threshold_from='long' needs masking")
    return threshold_from == 'long'


def check_measured_units(units, frames, channels):
    """the units of Context.measure_units -> contiguous uint8 [frames * channels, 212].  ValueError for another size and for the
    first unit whose block modes (deserializeFrame's: 2, 2 and 3 minus the fields of the first six bits) are outside the
    domain of encode_modes(), naming its frame, channel and field."""
    u = np.ascontiguousarray(units)
    if u.dtype != np.uint8:
        raise ValueError('units must be uint8')
    if u.size != frames * channels * 212:
        raise ValueError('units must hold frames * channels = %d sound units of 212 bytes, got %d bytes' % (frames * channels, u.size))
    u = u.reshape(-1, 212)
    first = u[:, 0].astype(np.int64)
    m = np.stack([2 - ((first >> 6) & 3), 2 - ((first >> 4) & 3), 3 - ((first >> 2) & 3)], axis=1)
    ok = ((m[:, 0] == 0) | (m[:, 0] == 2)) & ((m[:, 1] == 0) | (m[:, 1] == 2)) & ((m[:, 2] == 0) | (m[:, 2] == 3))
    bad = np.flatnonzero(~ok)
    if bad.size:
        i = int(bad[0])
        where = 'frame %d, channel %d' % (i // channels, i % channels) if channels == 2 else 'frame %d' % i
        for k, name in enumerate(_MODE_FIELDS):
            other = 3 if k == 2 else 2
            if int(m[i, k]) not in (0, other):
                raise ValueError('%s: %s block mode of the unit is %d, not 0 or %d' % (where, name, int(m[i, k]), other))
    return u


# ---- the decoded PCM error of given sound units (c1_measure_pcm_*) ----------------------------------------------------------
PCM_DELAY = 266       # samples between a sample going into encode() and coming out of decode()
PCM_SEGMENTS = 16     # 32-sample segments of a frame


def check_pcm_units(units, count, channels):
    """the units of Context.measure_pcm -> contiguous uint8 [count * channels, 212]; ValueError for another dtype or size.  Any
    bytes are units to the decoder: nothing else is checked."""
    u = np.ascontiguousarray(units)
    if u.dtype != np.uint8:
        raise ValueError('units must be uint8')
    if u.size != count * channels * 212:
        raise ValueError('units must hold (halo_units + frames) * channels = %d sound units of 212 bytes, got %d bytes'
                         % (count * channels, u.size))
    return u.reshape(-1, 212)


# ---- the allocation bias per sound unit: a palette of option sets and one index byte per unit (c1_encode_biases_*) -----
MAX_BIAS_PALETTE = 8


def palette_array(c_options):
    """capi.EncodeOptions instances -> the contiguous array c1_encode_biases_* take"""
    arr = (capi.EncodeOptions * max(len(c_options), 1))()
    for k, o in enumerate(c_options):
        C.memmove(C.byref(arr[k]), C.byref(o), C.sizeof(capi.EncodeOptions))
    return arr


def bias_palette(biases, frames, channels, options=None):
    """biases: `frames` values (every channel of a frame takes the frame's) or frames * channels ([frames, nch] or flat,
    frame-major) -> (palette array, uint8 index [frames * channels]).  The palette holds the distinct values in ascending
    order, each an EncoderOptions of `options`' other values with that allocationBias (so each is range-checked as
    allocationBias is); more than MAX_BIAS_PALETTE distinct values raise ValueError."""
    b = np.ascontiguousarray(biases, dtype=np.float64).reshape(-1)
    if b.size == frames and channels != 1:
        b = np.repeat(b, channels)
    if b.size != frames * channels:
        raise ValueError('biases must hold frames = %d or frames * channels = %d values, got %d' % (frames, frames * channels, b.size))
    if np.isnan(b).any():
        raise ValueError('biases must not be NaN')
    values, index = (np.unique(b, return_inverse=True) if b.size else (np.array([1.0]), np.zeros(0, dtype=np.int64)))
    if len(values) > MAX_BIAS_PALETTE:
        raise ValueError('at most %d distinct allocation biases per call, got %d' % (MAX_BIAS_PALETTE, len(values)))
    base = dict(options.values) if options is not None else {}
    entries = []
    for v in values:
        o = EncoderOptions(base)
        o.set_value('allocationBias', float(v))
        entries.append(o.to_c())
    return palette_array(entries), np.ascontiguousarray(index.reshape(-1), dtype=np.uint8)


def candidate_palette(biases, options=None):
    """the candidates of Context.encode_best_bias -> (palette array, count).  biases: 1 .. MAX_BIAS_PALETTE entries in the
    caller's order, each a number (an EncoderOptions of `options`' other values with that allocationBias, range-checked as
    allocationBias is) or an EncoderOptions (taken as it is: it may carry an explicit table).  ValueError for none, for more
    than MAX_BIAS_PALETTE, for NaN and for a numeric bias given twice."""
    items = list(biases)
    if not 1 <= len(items) <= MAX_BIAS_PALETTE:
        raise ValueError('between 1 and %d candidate biases per call, got %d' % (MAX_BIAS_PALETTE, len(items)))
    base = dict(options.values) if options is not None else {}
    entries, seen = [], set()
    for v in items:
        if isinstance(v, EncoderOptions):
            entries.append(v.to_c())
            continue
        v = float(v)
        if v != v:
            raise ValueError('candidate biases must not be NaN')
        if v in seen:
            raise ValueError('candidate bias %r is given twice' % v)
        seen.add(v)
        o = EncoderOptions(base)
        o.set_value('allocationBias', v)
        entries.append(o.to_c())
    return palette_array(entries), len(entries)


def aea_header(title='', frame_count=0, channel_count=1):
    h = bytearray(AEA_HEADER_SIZE)
    h[0:4] = AEA_MAGIC
    t = title.encode('utf-8')[:AEA_TITLE_SIZE - 1]
    h[AEA_TITLE_OFFSET:AEA_TITLE_OFFSET + len(t)] = t
    struct.pack_into('<I', h, AEA_FRAME_COUNT_OFFSET, frame_count)
    h[AEA_CHANNEL_COUNT_OFFSET] = channel_count
    return bytes(h)


def parse_aea_header(header):
    if len(header) != AEA_HEADER_SIZE:
        raise ValueError('Header must be %d bytes' % AEA_HEADER_SIZE)
    if bytes(header[0:4]) != AEA_MAGIC:
        raise ValueError('Invalid AEA file')
    end = bytes(header).find(b'\x00', AEA_TITLE_OFFSET)
    n = AEA_TITLE_SIZE if end < 0 else end - AEA_TITLE_OFFSET
    return {'title': bytes(header[AEA_TITLE_OFFSET:AEA_TITLE_OFFSET + n]).decode('utf-8', 'replace'),
            'frameCount': struct.unpack_from('<I', header, AEA_FRAME_COUNT_OFFSET)[0],
            'channelCount': header[AEA_CHANNEL_COUNT_OFFSET]}


def pinned_empty(shape, dtype=np.float32):
    """numpy array in page-locked host memory (c1_host_alloc).  Batch calls whose host buffers all live in such
    arrays stream the batch over PCIe in overlapping chunks (include/carta1_hip.h).  Freed with the array."""
    import weakref
    dtype = np.dtype(dtype)
    n = int(np.prod(shape))
    ptr = C.c_void_p()
    capi.check(capi.load().c1_host_alloc(max(1, n * dtype.itemsize), C.byref(ptr)))
    buf = (C.c_uint8 * (n * dtype.itemsize)).from_address(ptr.value)
    arr = np.frombuffer(buf, dtype=dtype, count=n).reshape(shape)
    weakref.finalize(buf, capi.load().c1_host_free, ptr)
    return arr


_default_ctx = None


def _state_rows(states, floats, rows):
    """states as a contiguous (rows, floats) float32 array; a ctypes array of capi.EncState / DecState is viewed, not converted"""
    if isinstance(states, (C.Array, C.Structure)):
        st = np.frombuffer(states, dtype=np.float32).copy()
    else:
        st = np.ascontiguousarray(states, dtype=np.float32)
    if st.size != rows * floats:
        raise ValueError('expected %d state(s) of %d floats, got %d floats' % (rows, floats, st.size))
    return st.reshape(rows, floats)


def _field_arrays(fields):
    """the five frame-field arrays of `fields` (Context.FIELD_SHAPES order) as contiguous int32, sizes checked"""
    units = int(np.asarray(fields['nbfu']).size)
    arrs = []
    for k, shape in Context.FIELD_SHAPES:
        a = np.ascontiguousarray(fields[k], dtype=np.int32)
        if a.size != units * int(np.prod(shape, dtype=np.int64)):
            raise ValueError('%s must hold %s entries per frame' % (k, shape or 1))
        arrs.append(a)
    return arrs


def _ragged(rows):
    """a sequence of 1-D arrays -> (float64 values, int64 offsets[len + 1]) as the batched decision entries take them"""
    arrs = [np.ascontiguousarray(r, dtype=np.float64).reshape(-1) for r in rows]
    off = np.zeros(len(arrs) + 1, dtype=np.int64)
    if arrs:
        off[1:] = np.cumsum([a.size for a in arrs])
    vals = np.concatenate(arrs) if arrs and off[-1] else np.zeros(1)
    return np.ascontiguousarray(vals), off


def _check_quantize_args(scale_factor_index, bits_per_sample):
    """quantize / dequantize take int32 arguments; anything else would be truncated silently on its way through ctypes"""
    for name, v in (('scale_factor_index', scale_factor_index), ('bits_per_sample', bits_per_sample)):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or not -2**31 <= int(v) < 2**31:
            raise ValueError('%s must be an int32, got %r' % (name, v))


def _ctx(ctx):
    global _default_ctx
    if ctx is not None:
        return ctx
    if _default_ctx is None:
        _default_ctx = Context(0)
    return _default_ctx


DECODE_EXACT, DECODE_BINARY32_BULK, DECODE_BINARY32 = 0, 1, 2
_PRECISIONS = {'exact': DECODE_EXACT, 'binary32': DECODE_BINARY32}


def check_precision(precision):
    """None (the context's model as it is) | 'exact' | 'binary32' -> the decode model of the call, or None"""
    if precision is None:
        return None
    if not isinstance(precision, str) or precision not in _PRECISIONS:
        raise ValueError("precision must be None, 'exact' or 'binary32', got %r" % (precision,))
    return _PRECISIONS[precision]


class _decode_model:
    """the context's decode model set for the length of a call and put back afterwards, also on error"""

    def __init__(self, ctx, model):
        self.ctx, self.model = ctx, model

    def __enter__(self):
        if self.model is not None:
            self.before = self.ctx.decode_model
            self.ctx.set_decode_model(self.model)
        return self.ctx

    def __exit__(self, *exc):
        if self.model is not None:
            self.ctx.set_decode_model(self.before)
        return False


def _check_channels(channels):
    if (not isinstance(channels, (list, tuple)) or len(channels) not in (1, 2)
            or any(not (isinstance(c, np.ndarray) and c.dtype == np.float32) for c in channels)):
        raise TypeError('ATRAC1 encoding requires one or two Float32 channels')   # processor.js:603


def encode_pcm(channels, options=None, ctx=None):
    """Planar PCM of any length -> units; the final partial frame is zero padded and a shorter channel
    is padded to the longer one (frameBufferToFrames, processor.js:246-279)."""
    _check_channels(channels)
    n = max(len(c) for c in channels)
    frames = (n + 511) // 512
    padded = []
    for c in channels:
        p = np.zeros(frames * 512, dtype=np.float32)
        p[:len(c)] = c
        padded.append(p)
    return _ctx(ctx).encode(padded, options)


def decode_units(units, channels, ctx=None, precision=None):
    """precision: None (the context's decode model) | 'exact' | 'binary32' (Context.set_decode_model's DECODE_BINARY32) for
    this call; the context's model is put back afterwards"""
    model = check_precision(precision)
    with _decode_model(_ctx(ctx), model) as c:
        return c.decode(units, channels)


def encode_aea_pcm(channels, options=None, ctx=None):
    """encodeAeaPcm (processor.js:597-617): 2048-byte header + 212 bytes per unit, L/R interleaved;
    header frameCount counts sound units over both channels (processor.js:320-325)."""
    _check_channels(channels)
    options = dict(options or {})
    title = options.pop('title', 'encoded by carta1')
    units = encode_pcm(channels, EncoderOptions(options), ctx)
    return aea_header(title, units.shape[0], len(channels)) + units.tobytes()


# ---- many items in one call: the pure host part (layout only, no device) ---------------------------------------------
def pad_signal(x):
    """one mono signal as float32, zero padded to whole frames (frameBufferToFrames, processor.js:246-279)"""
    x = np.ascontiguousarray(x, dtype=np.float32).reshape(-1)
    if x.size % 512 == 0:
        return x
    p = np.zeros((x.size + 511) // 512 * 512, dtype=np.float32)
    p[:x.size] = x
    return p


def signals_layout(signals):
    """whole-frame signals -> (the concatenated PCM, int64 frame offsets [n + 1]) as the c1_*_signals* calls take them"""
    for x in signals:
        if x.size % 512:
            raise ValueError('signals must hold whole frames of 512 samples')
    off = np.zeros(len(signals) + 1, dtype=np.int64)
    if signals:
        off[1:] = np.cumsum([x.size // 512 for x in signals])
    pcm = np.concatenate(signals) if signals else np.zeros(0, dtype=np.float32)
    return np.ascontiguousarray(pcm, dtype=np.float32), off


def split_rows(rows, off):
    return [rows[int(off[i]):int(off[i + 1])] for i in range(off.size - 1)]


def items_to_signals(items):
    """items, each [L] or [L, R] -> (signals, channel counts): one padded mono signal per channel in item order, both channels
    of an item padded to the longer one (encode_pcm does the same for one item)"""
    signals, counts = [], []
    for channels in items:
        _check_channels(channels)
        frames = (max(len(c) for c in channels) + 511) // 512
        for c in channels:
            p = np.zeros(frames * 512, dtype=np.float32)
            p[:len(c)] = c
            signals.append(p)
        counts.append(len(channels))
    return signals, counts


def interleave_item_units(signal_units, counts):
    """per-signal units (as items_to_signals ordered the signals) -> per item (frames * channels, 212), interleaved L, R"""
    out, k = [], 0
    for nch in counts:
        chans = signal_units[k:k + nch]
        k += nch
        u = np.zeros((chans[0].shape[0] * nch, 212), dtype=np.uint8)
        for c in range(nch):
            u[c::nch] = chans[c]
        out.append(u)
    return out


def deinterleave_item_units(item_units, counts):
    """the inverse: per item (frames * channels, 212) -> one (frames, 212) array per channel, in item order"""
    out = []
    for u, nch in zip(item_units, counts):
        u = np.asarray(u, dtype=np.uint8).reshape(-1, 212)
        if u.shape[0] % nch:
            raise ValueError('an item of %d channels needs a multiple of %d units' % (nch, nch))
        for c in range(nch):
            out.append(np.ascontiguousarray(u[c::nch]))
    return out


def aea_image_units(data):
    """one AEA image -> (units (n, 212) with the dummy right unit behind a lone trailing left one, channel count):
    decodeAeaPcm's reading of a file (processor.js:628-654, :222-232, :516-521)"""
    if isinstance(data, np.ndarray):
        data = data.tobytes()
    if not isinstance(data, (bytes, bytearray, memoryview)):
        raise TypeError('ATRAC1 decoding requires AEA bytes or a Blob')
    data = bytes(data)
    info = parse_aea_header(data[:AEA_HEADER_SIZE])
    body = data[AEA_HEADER_SIZE:]
    n_units = len(body) // 212            # a trailing partial unit is dropped (processor.js:516-521)
    nch = info['channelCount']
    units = np.frombuffer(body[:n_units * 212], dtype=np.uint8).reshape(-1, 212)
    if nch == 2 and n_units % 2:          # trailing lone L unit gets an all-zero partner (processor.js:222-232)
        dummy = np.zeros((1, 212), dtype=np.uint8)
        dummy[0, 0], dummy[0, 1] = 0xAC, 0x00   # modes 0,0,0; 20 BFUs; every word length 0 == _createDummyFrame
        units = np.concatenate([units, dummy])
    if nch not in (1, 2):
        raise ValueError('Unsupported channel count: %d' % nch)
    return units, nch


def encode_aea_pcm_many(items, options=None, ctx=None, measured_allocation=False, scale_factor_offsets=None, masking=None,
                        measured_mode_candidates=None):
    """encode_aea_pcm for many items in one device call: items is a list of [L] or [L, R]; options.title may be one string
    or one per item.  Every result is byte for byte what encode_aea_pcm returns for that item alone.
    measured_allocation: the units of every item are Context.encode_measured's for that item alone (with scale_factor_offsets
    and masking as there, which need it), through Context.encode_signals_measured.
    measured_mode_candidates (needs measured_allocation; with scale_factor_offsets or without, never with masking): the units
    of every item are Context.encode_measured_modes' for that item alone, through Context.encode_signals_measured_modes."""
    options = dict(options or {})
    title = options.pop('title', 'encoded by carta1')
    titles = [title] * len(items) if isinstance(title, str) else list(title)
    if len(titles) != len(items):
        raise ValueError('title must be one string or one per item')
    if not measured_allocation and (scale_factor_offsets is not None or masking is not None):
        raise ValueError('scale_factor_offsets and masking need measured_allocation')
    if measured_mode_candidates is not None:
        if not measured_allocation:
            raise ValueError('measured_mode_candidates needs measured_allocation')
        if masking is not None:
            raise ValueError('measured_mode_candidates and masking cannot be combined: the mode search has no masking weights')
        cand = mode_candidates(measured_mode_candidates)
        if scale_factor_offsets is not None:
            check_scale_factor_offsets(scale_factor_offsets)
    signals, counts = items_to_signals(items)
    if measured_mode_candidates is not None:
        units = _ctx(ctx).encode_signals_measured_modes(signals, cand, options=EncoderOptions(options),
                                                        scale_factor_offsets=scale_factor_offsets)[0]
    elif measured_allocation:
        units = _ctx(ctx).encode_signals_measured(signals, options=EncoderOptions(options), scale_factor_offsets=scale_factor_offsets,
                                                  masking=masking)[0]
    else:
        units = _ctx(ctx).encode_signals(signals, EncoderOptions(options))
    return [aea_header(t, u.shape[0], nch) + u.tobytes() for t, u, nch in zip(titles, interleave_item_units(units, counts), counts)]


def decode_aea_pcm_many(images, ctx=None, precision=None):
    """decode_aea_pcm for many AEA images in one device call -> per image a list of float32 arrays (one per channel).
    precision: as decode_units"""
    model = check_precision(precision)
    parsed = [aea_image_units(d) for d in images]
    counts = [nch for _, nch in parsed]
    with _decode_model(_ctx(ctx), model) as c:
        pcm = c.decode_signals(deinterleave_item_units([u for u, _ in parsed], counts))
    out, k = [], 0
    for nch in counts:
        out.append(list(pcm[k:k + nch]))
        k += nch
    return out


def decode_aea_pcm(data, ctx=None, precision=None):
    """decodeAeaPcm (processor.js:628-654): bytes / bytearray / ndarray(uint8) -> list of float32 arrays.
    precision: as decode_units"""
    model = check_precision(precision)
    units, nch = aea_image_units(data)
    with _decode_model(_ctx(ctx), model) as c:
        return c.decode(units, nch)


# ---- sound unit <-> fields: codec/io/serialization.js:41-176 (format code, host side) ----------------
def deserialize_frame(unit):
    u = bytes(unit)
    if len(u) != 212:
        raise ValueError('Frame must be 212 bytes')
    bits = int.from_bytes(u, 'big')
    total = 212 * 8

    def get(pos, n):
        avail = max(0, min(n, total - pos))
        return (bits >> (total - pos - avail)) & ((1 << avail) - 1) if avail else 0
    header = get(0, 16)
    modes = [2 - ((header >> 14) & 3), 2 - ((header >> 12) & 3), 3 - ((header >> 10) & 3)]
    n = BFU_AMOUNTS[(header >> 5) & 7]
    wl = [get(16 + 4 * i, 4) for i in range(n)]
    sfi = [get(16 + 4 * n + 6 * i, 6) for i in range(n)]
    pos = 16 + 10 * n
    q = []
    for i in range(n):
        b = WORD_LENGTH_BITS[wl[i]]
        vals = []
        for _ in range(SPECS_PER_BFU[i]):
            v = 0
            if b:
                v = get(pos, b)
                pos += b
                if v >= 1 << (b - 1):
                    v -= 1 << b
            vals.append(v)
        q.append(vals)
    return {'nBfu': n, 'blockModes': modes, 'wordLengthIndices': wl, 'scaleFactorIndices': sfi,
            'quantizedCoefficients': q}


def serialize_frame(f):
    n = f['nBfu']
    header = ((2 - f['blockModes'][0]) << 14) | ((2 - f['blockModes'][1]) << 12) | ((3 - f['blockModes'][2]) << 10) \
        | (BFU_AMOUNTS.index(n) << 5)
    acc, nbits = header & 0xffff, 16
    for i in range(n):
        acc, nbits = (acc << 4) | (f['wordLengthIndices'][i] & 15), nbits + 4
    for i in range(n):
        acc, nbits = (acc << 6) | (f['scaleFactorIndices'][i] & 63), nbits + 6
    for i in range(n):
        b = WORD_LENGTH_BITS[f['wordLengthIndices'][i]]
        if b:
            for v in f['quantizedCoefficients'][i]:
                acc, nbits = (acc << b) | (v & ((1 << b) - 1)), nbits + b
    acc <<= 212 * 8 - nbits
    return acc.to_bytes(212, 'big')
