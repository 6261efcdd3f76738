"""CPU-only: the measured block-mode search for n signals in one call (c1_encode_signals_measured_modes*,
Context.encode_signals_measured_modes, encode_aea_pcm_many(measured_mode_candidates=...)).  The symbols and their prototypes, and
everything the host form and the Python wrappers decide before they need a context or a device: what makes
tests/test_gpu_signals_measured_modes.py's rejections mean something."""
import ctypes as C
import os
import re

import numpy as np
import pytest

C1_ERR_ARG, C1_ERR_NO_DEVICE = 1, 2   # include/carta1_hip.h
I64P = C.POINTER(C.c_int64)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('c1_encode_signals_measured_modes', 'c1_encode_signals_measured_modes_device')
OFFSETS = (0, -1, 1, -2, -3)


def _lib():
    from carta1_amd import build, capi
    build.build_library()
    return capi.load()


def test_the_symbols_are_declared_exported_and_bound_with_equal_prototypes():
    from carta1_amd import capi
    lib = _lib()
    header = open(os.path.join(ROOT, 'include', 'carta1_hip.h')).read()
    assert re.search(r'#define\s+C1_ABI_VERSION\s+3\b', header) and lib.c1_abi_version() == 3
    assert re.search(r'\bC1_ERR_ARG\s*=\s*%d\b' % C1_ERR_ARG, header) and re.search(r'\bC1_ERR_NO_DEVICE\s*=\s*%d\b' % C1_ERR_NO_DEVICE, header)
    stream = capi.SIGNATURES['c1_enc_stream_push_measured_modes'][1]
    signals = capi.SIGNATURES['c1_encode_signals'][1]
    for name in NAMES:
        assert re.search(r'\bint\s+%s\s*\(' % name, header), name + ' is not declared'
        assert hasattr(lib, name), name + ' is not exported'
        res, args = capi.SIGNATURES[name]
        assert res is C.c_int and len(args) == 18
        # c1_encode_signals' leading arguments, the candidates and offsets of the stream push, units, out, the push's outputs
        assert args[:6] == signals[:6]
        assert args[6:10] == stream[3:7]
        assert args[10:12] == signals[6:8]
        assert args[12:] == stream[8:]
    assert capi.SIGNATURES[NAMES[0]] == capi.SIGNATURES[NAMES[1]]
    # the header's two prototypes: the same parameter types in the same order
    protos = []
    for name in NAMES:
        text = re.search(r'\bint\s+%s\s*\((.*?)\)\s*;' % name, header, re.S).group(1)
        text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
        protos.append([re.sub(r'\s+', ' ', re.sub(r'\w+\s*$', '', p.strip())).strip() for p in text.split(',')])
    assert protos[0] == protos[1] and len(protos[0]) == 18


def _outputs(n, signals, n_cand=8):
    return {'units': np.full((n, 212), 0xA5, dtype=np.uint8), 'out': np.full((signals, 483), -1.0, dtype=np.float32),
            'choice': np.full(n, 0xA5, dtype=np.uint8), 'modes_out': np.full(n, 0xA5, dtype=np.uint8),
            'taken': np.full(n, 0xA5, dtype=np.uint8), 'shifts': np.full((n, 52), 0x5A, dtype=np.int8),
            'distortion': np.full((n, n_cand, 2), -1.0), 'energy': np.full((n, n_cand), -1.0)}


ALL = ('units', 'out', 'choice', 'modes_out', 'taken', 'shifts', 'distortion', 'energy')


def test_argument_checks_need_neither_context_nor_device():
    """c1_encode_signals_measured_modes decides what its arguments alone decide before it looks at its context: C1_ERR_ARG with
    the composed calls' messages, with or without a device, and nothing written.  With everything valid only the context (or the
    device) is missing."""
    from carta1_amd import capi
    lib = _lib()
    err = lambda: lib.c1_last_error().decode()
    lengths = [2, 0, 3]
    total, n = sum(lengths), len(lengths)
    good_off = np.array([0, 2, 2, 5], dtype=np.int64)
    pcm = np.zeros(total * 512, dtype=np.float32)
    out = _outputs(total, n)
    opts = capi.EncodeOptions()
    lib.c1_default_encode_options(C.byref(opts))

    def call(off=good_off, cand=(0, 10, 58), n_cand=None, offsets=OFFSETS, n_offsets=None, states=None, ask=ALL):
        c = None if cand is None else np.ascontiguousarray(list(cand) + [0] * 10, dtype=np.uint8)
        o = None if offsets is None else np.ascontiguousarray(list(offsets) + [0] * 9, dtype=np.int8)
        kc = n_cand if n_cand is not None else len(cand)
        ko = n_offsets if n_offsets is not None else (0 if offsets is None else len(offsets))
        data = lambda a: None if a is None else a.ctypes.data
        p = {key: (out[key].ctypes.data if key in ask else None) for key in out}
        return lib.c1_encode_signals_measured_modes(None, n, None if off is None else off.ctypes.data_as(I64P), pcm.ctypes.data, data(states),
                                                    C.byref(opts), data(c), kc, data(o), ko, p['units'], p['out'], p['choice'],
                                                    p['modes_out'], p['taken'], p['shifts'], p['distortion'], p['energy'])

    what = 'c1_encode_signals_measured_modes: '
    # the candidates, as check_mode_candidates words them
    assert call(cand=(), n_cand=0) == C1_ERR_ARG and what + 'n_cand = 0 is outside 1..8' in err(), err()
    assert call(cand=(0, 2, 8, 10, 48, 50, 56, 58, 0), n_cand=9) == C1_ERR_ARG and what + 'n_cand = 9 is outside 1..8' in err(), err()
    assert call(cand=(0, 58, 0)) == C1_ERR_ARG and what + "candidate 2: mode byte 0x00 is candidate 0's" in err(), err()
    assert call(cand=(0, 1)) == C1_ERR_ARG and what + 'candidate 1: low field of mode byte 0x01 is 1, not 0 or 2' in err(), err()
    assert call(cand=(0, 0x10)) == C1_ERR_ARG and what + 'candidate 1: high field of mode byte 0x10 is 1, not 0 or 3' in err(), err()
    assert call(cand=(0x42,)) == C1_ERR_ARG and what + 'candidate 0: bits 6-7 of mode byte 0x42 are set' in err(), err()
    assert call(cand=None, n_cand=2) == C1_ERR_ARG and what + 'cand_modes is NULL' in err(), err()
    # the offsets, as check_sf_offsets words them, and a count without offsets
    assert call(offsets=(-1, 0)) == C1_ERR_ARG and what + 'sf_offsets[0] = -1, not 0' in err(), err()
    assert call(offsets=(0, 9)) == C1_ERR_ARG and what + 'sf_offsets[1] = 9 is outside -8..8' in err(), err()
    assert call(offsets=(0, 1, 1)) == C1_ERR_ARG and what + 'sf_offsets[2] repeats sf_offsets[1] = 1' in err(), err()
    assert call(offsets=(0,), n_offsets=9) == C1_ERR_ARG and what + 'n_offsets = 9 is outside 1..8' in err(), err()
    assert call(offsets=None, n_offsets=5) == C1_ERR_ARG and what + 'n_offsets = 5, but sf_offsets is NULL' in err(), err()
    # frame_offsets
    assert call(off=np.array([1, 2, 2, 5], dtype=np.int64)) == C1_ERR_ARG and what + 'frame_offsets must start at 0, got 1' in err(), err()
    assert call(off=np.array([0, 3, 2, 5], dtype=np.int64)) == C1_ERR_ARG and what + 'frame_offsets decreases at signal 1 (2 after 3)' in err(), err()
    assert call(off=np.array([0, 2, 2, (1 << 22) + 1], dtype=np.int64)) == C1_ERR_ARG and what + '4194305 frames in all, at most 4194304 per call' in err(), err()
    assert call(off=None) == C1_ERR_ARG and what + 'frame_offsets is NULL' in err(), err()
    # a state entry that is not finite, naming signal and field
    states = np.zeros((n, 483), dtype=np.float32)
    states[2, 131 + 5] = np.inf
    assert call(states=states) == C1_ERR_ARG and what in err() and 'signal 2' in err() and 'mdct_overlap' in err(), err()
    states[2, 131 + 5] = 0.0
    states[1, 227] = np.nan
    assert call(states=states) == C1_ERR_ARG and 'signal 1' in err() and 'transient_mags' in err(), err()
    states[1, 227] = 0.0
    # nothing to report
    assert call(ask=()) == C1_ERR_ARG and what + 'units, choice, modes_out, taken, shifts, distortion and energy are all NULL' in err(), err()
    assert call(ask=('out',)) == C1_ERR_ARG and 'are all NULL' in err(), err()
    # the options, as check_measured_opts judges them: an invalid table; threshold and fixed modes are not read
    bad = capi.EncodeOptions()
    C.memmove(C.byref(bad), C.byref(opts), C.sizeof(opts))
    bad.biased_scale_factors[5] = float('nan')
    keep, opts = opts, bad
    assert call() == C1_ERR_ARG and what + 'biased_scale_factors[5] is not a finite non-negative number' in err(), err()
    opts = keep
    odd = capi.EncodeOptions()
    C.memmove(C.byref(odd), C.byref(opts), C.sizeof(opts))
    odd.transient_threshold = float('nan')
    odd.fixed_block_modes[0], odd.fixed_block_modes[1], odd.fixed_block_modes[2] = 1, 7, -3
    opts = odd
    rc = call()
    assert rc != 0 and ('context is NULL' in err() or 'no HIP device available' in err()), err()
    opts = keep
    # valid arguments, with and without offsets and states, one candidate and eight, single outputs: only the context (or the
    # device) is missing
    have_device = C.c_int(0)
    lib.c1_device_count(C.byref(have_device))
    for kw in ({}, {'offsets': None}, {'states': states}, {'cand': (58,)}, {'cand': (0, 2, 8, 10, 48, 50, 56, 58)}, {'ask': ('choice',)},
               {'ask': ('units',)}, {'ask': ('energy', 'out')}):
        rc = call(**kw)
        if have_device.value > 0:
            assert rc == C1_ERR_ARG and 'context is NULL' in err(), (kw, err())
        else:
            assert rc == C1_ERR_NO_DEVICE and what + 'no HIP device available' in err(), (kw, rc, err())
    fill = _outputs(total, n)
    assert all(np.array_equal(out[k].view(np.uint8), fill[k].view(np.uint8)) for k in out)


class _NoSignals:
    """the library without its signals calls"""
    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, name):
        if name.startswith('c1_encode_signals'):
            raise AssertionError('the wrapper reached ' + name)
        return getattr(self._lib, name)


def test_the_wrappers_reject_before_any_library_call(monkeypatch):
    import carta1_amd as c1
    from carta1_amd import capi
    _lib()
    ctx = object.__new__(c1.Context)                                       # no device, no handle: the checks come first
    ctx._h = None
    guarded = _NoSignals(capi.load())
    monkeypatch.setattr(capi, 'load', lambda: guarded)
    sigs = [np.zeros(2 * 512, dtype=np.float32), np.zeros(0, dtype=np.float32), np.zeros(700, dtype=np.float32)]
    enc = ctx.encode_signals_measured_modes
    with pytest.raises(ValueError, match='between 1 and 8 candidate block modes per call, got 0'):
        enc(sigs, [])
    with pytest.raises(ValueError, match='between 1 and 8 candidate block modes per call, got 9'):
        enc(sigs, [0, 2, 8, 10, 48, 50, 56, 58, 0])
    with pytest.raises(ValueError, match='candidate 1: mode byte 0x3a is given twice'):
        enc(sigs, [58, 58])
    with pytest.raises(ValueError, match='candidate 1: low field of mode byte 0x01 is 1, not 0 or 2'):
        enc(sigs, [0, 1])
    with pytest.raises(ValueError, match='candidate 0: bits 6-7'):
        enc(sigs, [0x40])
    with pytest.raises(ValueError, match='a mode byte or a triple'):
        enc(sigs, [[2, 2]])
    with pytest.raises(ValueError, match='outside -8..8'):
        enc(sigs, [0, 58], scale_factor_offsets=(0, 9))
    with pytest.raises(ValueError, match='first scale-factor offset must be 0'):
        enc(sigs, [0, 58], scale_factor_offsets=(1, 0))
    with pytest.raises(ValueError, match='in_place needs states'):
        enc(sigs, [0, 58], in_place=True)
    many = lambda **kw: c1.encode_aea_pcm_many([[sigs[0]], [sigs[2], sigs[2]]], ctx=ctx, **kw)
    with pytest.raises(ValueError, match='measured_mode_candidates needs measured_allocation'):
        many(measured_mode_candidates=[0, 58])
    with pytest.raises(ValueError, match='measured_mode_candidates.*masking|masking.*measured_mode_candidates'):
        many(measured_allocation=True, measured_mode_candidates=[0, 58], masking=True)
    with pytest.raises(ValueError, match='given twice'):
        many(measured_allocation=True, measured_mode_candidates=[0, 0])
    with pytest.raises(ValueError, match='outside -8..8'):
        many(measured_allocation=True, measured_mode_candidates=[0, 58], scale_factor_offsets=(0, -9))
    # everything valid: the one entry point, with offsets and without, triples too
    with pytest.raises(AssertionError, match='the wrapper reached c1_encode_signals_measured_modes$'):
        enc(sigs, [0, (2, 2, 3)], scale_factor_offsets=OFFSETS, return_distortion=True, return_shifts=True, return_states=True)
    with pytest.raises(AssertionError, match='the wrapper reached c1_encode_signals_measured_modes$'):
        enc(sigs, np.array([58], dtype=np.uint8))
    with pytest.raises(AssertionError, match='the wrapper reached c1_encode_signals_measured_modes$'):
        many(measured_allocation=True, measured_mode_candidates=[0, 10, 58], scale_factor_offsets=OFFSETS)
    with pytest.raises(AssertionError, match='the wrapper reached c1_encode_signals_measured_modes_device$'):
        ctx.encode_signals_measured_modes_device([0, 1], 256, [0, 58], units_ptr=512)
    # without the new argument: today's calls
    with pytest.raises(AssertionError, match='the wrapper reached c1_encode_signals_measured$'):
        many(measured_allocation=True, scale_factor_offsets=OFFSETS)
    with pytest.raises(AssertionError, match='the wrapper reached c1_encode_signals$'):
        many()
