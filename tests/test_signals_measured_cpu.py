"""CPU-only: the measured allocation for n signals in one call (c1_encode_signals_measured*, Context.encode_signals_measured).
The symbols and their prototypes, and everything the host form and the Python wrapper decide before they need a context or a
device: what makes tests/test_gpu_signals_measured.py's rejections mean something."""
import ctypes as C

import numpy as np
import pytest

import masked_alloc_lib as MK
import scale_factor_choice_lib as SF

C1_ERR_ARG = 1   # include/carta1_hip.h
I64P = C.POINTER(C.c_int64)


def _lib():
    from carta1_amd import build, capi
    build.build_library()
    return capi.load()


def test_the_symbols_exist_with_their_prototypes():
    from carta1_amd import capi
    lib = _lib()
    stream = capi.SIGNATURES['c1_enc_stream_push_measured'][1]
    signals = capi.SIGNATURES['c1_encode_signals'][1]
    for name in ('c1_encode_signals_measured', 'c1_encode_signals_measured_device'):
        assert hasattr(lib, name), name
        res, args = capi.SIGNATURES[name]
        assert res is C.c_int and len(args) == 18
        # c1_encode_signals' leading arguments, then modes, the measured arguments of the stream push, units, out, its outputs
        assert args[:6] == signals[:6]
        assert args[6:11] == stream[3:8]
        assert args[11:13] == signals[6:8]
        assert args[13:] == stream[9:]


def _outputs(n, signals):
    return {'units': np.full((n, 212), 0xA5, dtype=np.uint8), 'out': np.full((signals, 483), -1.0, dtype=np.float32),
            'taken': np.full(n, 0xA5, dtype=np.uint8), 'shifts': np.full((n, 52), 0x5A, dtype=np.int8),
            'distortion': np.full((n, 2), -1.0), 'energy': np.full(n, -1.0), 'weights': np.full((n, 52), -1.0)}


def test_argument_checks_need_neither_context_nor_device():
    """c1_encode_signals_measured decides what its arguments alone decide before it looks at its context: C1_ERR_ARG with the
    neighbouring calls' messages, with or without a device, and nothing written.  With everything valid only the context (or
    the device) is missing."""
    lib = _lib()
    err = lambda: lib.c1_last_error().decode()
    lengths = [2, 0, 3]
    total, n = sum(lengths), len(lengths)
    good_off = np.array([0, 2, 2, 5], dtype=np.int64)
    pcm = np.zeros(total * 512, dtype=np.float32)
    out = _outputs(total, n)
    good_floor, good_spread = (np.ascontiguousarray(a) for a in MK.packaged())
    from carta1_amd import capi
    opts = capi.EncodeOptions()
    lib.c1_default_encode_options(C.byref(opts))
    GIVEN = object()

    def call(off=good_off, floor=good_floor, spread=good_spread, offsets=SF.OFFSETS, n_offsets=None, weights=GIVEN, modes=None,
             states=None, ask=('units', 'out', 'taken', 'shifts', 'distortion', 'energy', 'weights')):
        o = None if offsets is None else np.ascontiguousarray(list(offsets) + [0] * 9, dtype=np.int8)
        k = n_offsets if n_offsets is not None else (0 if offsets is None else len(offsets))
        f = None if floor is None else np.ascontiguousarray(floor, dtype=np.float64)
        s = None if spread is None else np.ascontiguousarray(spread, dtype=np.float64)
        data = lambda a: None if a is None else a.ctypes.data
        p = {key: (out[key].ctypes.data if key in ask else None) for key in out}
        if weights is not GIVEN:
            p['weights'] = weights
        return lib.c1_encode_signals_measured(None, n, None if off is None else off.ctypes.data_as(I64P), pcm.ctypes.data, data(states),
                                              C.byref(opts), data(modes), data(o), k, data(f), data(s), p['units'], p['out'], p['taken'],
                                              p['shifts'], p['distortion'], p['energy'], p['weights'])

    what = 'c1_encode_signals_measured: '
    # frame_offsets
    assert call(off=np.array([1, 2, 2, 5], dtype=np.int64)) == C1_ERR_ARG and what + 'frame_offsets must start at 0, got 1' in err(), err()
    assert call(off=np.array([0, 3, 2, 5], dtype=np.int64)) == C1_ERR_ARG and what + 'frame_offsets decreases at signal 1 (2 after 3)' in err(), err()
    assert call(off=None) == C1_ERR_ARG and what + 'frame_offsets is NULL' in err(), err()
    # the measured arguments, as c1_enc_stream_push_measured words them
    assert call(floor=None, weights=None) == C1_ERR_ARG and what + 'mask_spread is given without mask_floor' in err(), err()
    assert call(floor=None, spread=None) == C1_ERR_ARG and what + 'weights is given without mask_floor' in err(), err()
    assert call(offsets=None, n_offsets=5) == C1_ERR_ARG and what + 'n_offsets = 5, but sf_offsets is NULL' in err(), err()
    assert call(offsets=(-1, 0)) == C1_ERR_ARG and what + 'sf_offsets[0] = -1, not 0' in err(), err()
    assert call(offsets=(0, 9)) == C1_ERR_ARG and what + 'sf_offsets[1] = 9 is outside -8..8' in err(), err()
    f = good_floor.copy()
    f[17] = 0.0
    assert call(floor=f) == C1_ERR_ARG and what + 'mask_floor[17]' in err(), err()
    # a mode byte outside the domain, naming its frame of the concatenation
    modes = np.zeros(total, dtype=np.uint8)
    modes[3] = 0x42
    assert call(modes=modes) == C1_ERR_ARG and what + 'frame 3: bits 6-7 of mode byte 0x42 are set' in err(), err()
    modes[3] = 0x10
    assert call(modes=modes) == C1_ERR_ARG and what + 'frame 3: high field of mode byte 0x10 is 1, not 0 or 3' in err(), err()
    # nothing to report
    assert call(ask=(), weights=None) == C1_ERR_ARG and 'units, taken, shifts, distortion, energy and weights are all NULL' in err(), err()
    assert call(ask=('out',), weights=None) == C1_ERR_ARG and 'are all NULL' in err(), err()
    # a state entry that is not finite, naming signal and field
    states = np.zeros((n, 483), dtype=np.float32)
    states[2, 131 + 5] = np.inf
    assert call(states=states) == C1_ERR_ARG and 'signal 2' in err() and 'mdct_overlap' in err(), err()
    states[2, 131 + 5] = 0.0
    states[1, 227] = np.nan
    assert call(states=states) == C1_ERR_ARG and 'signal 1' in err() and 'transient_mags' in err(), err()
    # valid arguments of all four kinds, with and without modes and states: only the context is missing
    states[1, 227] = 0.0
    modes[3] = 0x3a
    for kw in ({}, {'offsets': None}, {'spread': None}, {'floor': None, 'spread': None, 'weights': None},
               {'floor': None, 'spread': None, 'weights': None, 'offsets': None}, {'modes': modes}, {'states': states},
               {'ask': ('taken',), 'weights': None}):
        rc = call(**kw)
        assert rc != 0 and ('context is NULL' in err() or 'no HIP device available' in err()), (kw, err())
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


def test_encode_signals_measured_rejects_before_any_library_call(monkeypatch):
    import carta1_amd as c1
    from carta1_amd import capi
    _lib()
    ctx = object.__new__(c1.Context)                                       # no device, no handle: the checks come first
    ctx._h = None
    guarded = _NoSignals(capi.load())
    monkeypatch.setattr(capi, 'load', lambda: guarded)
    sigs = [np.zeros(2 * 512, dtype=np.float32), np.zeros(0, dtype=np.float32), np.zeros(700, dtype=np.float32)]
    with pytest.raises(ValueError, match='return_shifts needs scale_factor_offsets'):
        ctx.encode_signals_measured(sigs, return_shifts=True)
    with pytest.raises(ValueError, match='return_shifts needs'):
        ctx.encode_signals_measured(sigs, masking=True, return_shifts=True)
    with pytest.raises(ValueError, match='return_weights needs masking'):
        ctx.encode_signals_measured(sigs, return_weights=True)
    with pytest.raises(ValueError, match='in_place needs states'):
        ctx.encode_signals_measured(sigs, in_place=True)
    with pytest.raises(ValueError, match='one array of mode bytes per signal'):
        ctx.encode_signals_measured(sigs, modes=[np.zeros(2, dtype=np.uint8)])
    with pytest.raises(ValueError, match='modes must hold'):               # signal 2 has two frames (700 samples padded)
        ctx.encode_signals_measured(sigs, modes=[np.zeros(2, dtype=np.uint8), np.zeros(0, dtype=np.uint8), np.zeros(3, dtype=np.uint8)])
    with pytest.raises(ValueError, match='high field'):
        ctx.encode_signals_measured(sigs, modes=[np.zeros(2, dtype=np.uint8), np.zeros(0, dtype=np.uint8), np.full(2, 0x10, dtype=np.uint8)])
    with pytest.raises(ValueError, match='outside -8..8'):
        ctx.encode_signals_measured(sigs, scale_factor_offsets=(0, 9))
    with pytest.raises(ValueError, match=r'mask_floor\[3\]'):
        ctx.encode_signals_measured(sigs, masking=(np.where(np.arange(52) == 3, 0.0, 1.0), None))
    with pytest.raises(ValueError, match='need measured_allocation'):
        c1.encode_aea_pcm_many([[sigs[0]]], ctx=ctx, masking=True)
    with pytest.raises(AssertionError, match='c1_encode_signals_measured'):  # everything valid: the one entry point, whatever the kind
        ctx.encode_signals_measured(sigs, masking=True, modes=[np.zeros(2, dtype=np.uint8), np.zeros(0, dtype=np.uint8), np.full(2, 0x3a, dtype=np.uint8)])
    with pytest.raises(AssertionError, match='c1_encode_signals_measured'):
        c1.encode_aea_pcm_many([[sigs[0]]], ctx=ctx, measured_allocation=True)
    with pytest.raises(AssertionError, match='the wrapper reached c1_encode_signals$'):   # the default arguments: today's call
        c1.encode_aea_pcm_many([[sigs[0]]], ctx=ctx)
