"""CPU-only: the measured allocation on live streams (c1_enc_stream_push_measured, EncoderStream.push_measured).  What makes
tests/test_gpu_stream_measured.py mean something.  The per-unit function is c1_encode_measured_masked_*'s, so the model is
tests/masked_alloc_lib.py's over the units the reference leaves for the same stream.  For the streams that never change options
those are the shared cases ('detect', 'pink'), (10, 'pink') and (58, 'white'), whose margins tests/test_masked_alloc_cpu.py
asserts as they are; the stream that changes options is asserted here.  Then the checks that the new entry point and the Python
wrapper make before they need a stream or a device."""
import numpy as np
import pytest

import masked_alloc_lib as MK
import measured_alloc_lib as MA
import option_changes_lib as OC
import scale_factor_choice_lib as SF
import stream_measured_lib as SM

C1_ERR_ARG = 1   # include/carta1_hip.h


def test_every_decision_on_the_option_change_stream_has_a_margin():
    """pink, fixedBlockModes [2, 2, 0] for frames 0 .. 39, detection from frame 40 (the switch stayed where it was first put),
    56 stereo frames, the reference's units from the oracle run segment by segment; packaged tables, offsets (0,-1,1,-2,-3).
    Measured here: least decision margin 1.08e-6, least candidate margin 3.62e-6, no exact tie, 112 of 112 units taken.  The
    error sums are known to 1e-12, so the GPU must reproduce every decision."""
    m = SM.option_change_case()
    print('least margin %.3g, least candidate margin %.3g, ties %d, taken %d of %d' % (
        float(m['margin'].min()), float(m['cand_margin']), int(m['ties']), int(m['taken'].sum()), len(m['taken'])))
    assert len(m['taken']) == SM.CHANGE_FRAMES * 2
    assert np.isfinite(m['D']).all() and (m['D'] > 0).all() and np.isfinite(m['P']).all() and (m['P'] > 0).all()
    assert (m['margin'] > MA.MARGIN).all(), float(m['margin'].min())
    assert m['cand_margin'] > 1e-9, float(m['cand_margin'])
    assert m['ties'] == 0
    assert MK.check_valid(m['units'], m['coefs'], m['taken'], m['D'], m['P'], SM.OFFSETS) is None
    # the schedule does what the GPU test needs of it: the frames before the switch carry [2, 2, 0], and detection decides
    # something else on some frame after it
    modes = OC.unit_modes(m['ref'])
    assert modes[:3 * 2 * SM.SWITCH] == '220' * (2 * SM.SWITCH)
    assert set(modes[i:i + 3] for i in range(3 * 2 * SM.SWITCH, len(modes), 3)) - {'220'}
    # before the switch the stream is the one under the constant byte 10: the shared case's rows
    ten = MK.case(10, 'pink')
    for key in ('units', 'taken', 'shifts'):
        assert np.array_equal(m[key][:2 * SM.SWITCH], ten[key][:2 * SM.SWITCH]), key
    assert MK.bitwise(m['D'][:2 * SM.SWITCH], ten['D'][:2 * SM.SWITCH])


def _outputs(n):
    return {'units': np.full((n, 212), 0xA5, dtype=np.uint8), 'taken': np.full(n, 0xA5, dtype=np.uint8),
            'shifts': np.full((n, 52), 0x5A, dtype=np.int8), 'distortion': np.full((n, 2), -1.0), 'energy': np.full(n, -1.0),
            'weights': np.full((n, 52), -1.0)}


def test_argument_checks_need_neither_stream_nor_device():
    """c1_enc_stream_push_measured decides what its arguments alone decide before it looks at its stream: C1_ERR_ARG naming
    the argument, with or without a device, and nothing written.  With everything valid only the stream is missing."""
    from carta1_amd import build, capi
    build.build_library()
    lib = capi.load()
    err = lambda: lib.c1_last_error().decode()
    frames, nch = 4, 2
    chans = [np.zeros(frames * 512, dtype=np.float32) for _ in range(nch)]
    ptrs = capi.ptr_array([c.ctypes.data for c in chans])
    out = _outputs(frames * nch)
    good_floor, good_spread = (np.ascontiguousarray(a) for a in MK.packaged())
    GIVEN = object()

    def call(floor=good_floor, spread=good_spread, offsets=SF.OFFSETS, n_offsets=None, weights=GIVEN):
        off = None if offsets is None else np.ascontiguousarray(list(offsets) + [0] * 9, dtype=np.int8)
        n = n_offsets if n_offsets is not None else (0 if offsets is None else len(offsets))
        f = None if floor is None else np.ascontiguousarray(floor, dtype=np.float64)
        s = None if spread is None else np.ascontiguousarray(spread, dtype=np.float64)
        w = out['weights'].ctypes.data if weights is GIVEN else weights
        return lib.c1_enc_stream_push_measured(None, ptrs, frames, None, None if off is None else off.ctypes.data, n,
                                               None if f is None else f.ctypes.data, None if s is None else s.ctypes.data,
                                               out['units'].ctypes.data, out['taken'].ctypes.data, out['shifts'].ctypes.data,
                                               out['distortion'].ctypes.data, out['energy'].ctypes.data, w)

    assert call(floor=None, weights=None) == C1_ERR_ARG and 'mask_spread is given without mask_floor' in err(), err()
    assert call(floor=None, spread=None) == C1_ERR_ARG and 'weights is given without mask_floor' in err(), err()
    assert call(offsets=None, n_offsets=5) == C1_ERR_ARG and 'n_offsets = 5, but sf_offsets is NULL' in err(), err()
    assert call(floor=None, spread=None, weights=None, offsets=None, n_offsets=1) == C1_ERR_ARG and 'sf_offsets is NULL' in err(), err()
    assert call(offsets=(0, 9)) == C1_ERR_ARG and 'c1_enc_stream_push_measured: sf_offsets[1] = 9 is outside -8..8' in err(), err()
    assert call(offsets=(-1, 0)) == C1_ERR_ARG and 'sf_offsets[0] = -1, not 0' in err(), err()
    assert call(offsets=(0, 1, 1)) == C1_ERR_ARG and 'sf_offsets[2] repeats sf_offsets[1] = 1' in err(), err()
    assert call(offsets=(0,), n_offsets=0) == C1_ERR_ARG and 'n_offsets = 0 is outside 1..8' in err(), err()
    assert call(offsets=(0,), n_offsets=9) == C1_ERR_ARG and 'n_offsets = 9 is outside 1..8' in err(), err()
    for v in (0.0, -1.0, np.nan, np.inf, 1e-61, 1e61):
        f = good_floor.copy()
        f[17] = v
        assert call(floor=f) == C1_ERR_ARG and 'c1_enc_stream_push_measured: mask_floor[17]' in err(), (v, err())
    for v in (-1e-3, np.nan, 1e61):
        s = good_spread.copy()
        s.reshape(-1)[53] = v
        assert call(spread=s) == C1_ERR_ARG and 'c1_enc_stream_push_measured: mask_spread[53]' in err(), (v, err())
    # valid arguments of all four kinds: only the stream is missing
    for kw in ({}, {'offsets': None}, {'spread': None}, {'floor': None, 'spread': None, 'weights': None},
               {'floor': None, 'spread': None, 'weights': None, 'offsets': None}):
        assert call(**kw) == C1_ERR_ARG and 'stream is NULL' in err(), (kw, err())
    fill = _outputs(frames * nch)
    assert all(np.array_equal(out[k].view(np.uint8), fill[k].view(np.uint8)) for k in out)


class _NoPush:
    """the library without its stream pushes"""
    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, name):
        if name.startswith('c1_enc_stream_push'):
            raise AssertionError('the wrapper reached ' + name)
        return getattr(self._lib, name)


def test_push_measured_rejects_before_any_library_call(monkeypatch):
    import carta1_amd as c1
    from carta1_amd import build, capi
    build.build_library()
    assert capi.SIGNATURES['c1_enc_stream_push_measured'][1][3:] == capi.SIGNATURES['c1_encode_measured_masked_batch'][1][6:]
    s = object.__new__(c1.EncoderStream)                                    # no device, no handle: the checks come first
    s._h, s.channels = None, 2
    guarded = _NoPush(capi.load())
    monkeypatch.setattr(capi, 'load', lambda: guarded)
    chans = [np.zeros(4 * 512, dtype=np.float32)] * 2
    with pytest.raises(ValueError, match='expected 2 channels'):
        s.push_measured(chans[:1])
    with pytest.raises(ValueError, match='multiple of 512'):
        s.push_measured([c[:1000] for c in chans])
    with pytest.raises(ValueError, match=r'mask_floor\[3\]'):
        s.push_measured(chans, masking=(np.where(np.arange(52) == 3, 0.0, 1.0), None))
    with pytest.raises(ValueError, match='return_weights needs masking'):
        s.push_measured(chans, return_weights=True)
    with pytest.raises(ValueError, match='return_shifts needs'):
        s.push_measured(chans, masking=True, return_shifts=True)
    with pytest.raises(ValueError, match='outside -8..8'):
        s.push_measured(chans, masking=True, scale_factor_offsets=(0, 9))
    with pytest.raises(ValueError):
        s.push_measured(chans, modes=np.full((4, 2), 0x10, dtype=np.uint8))
    with pytest.raises(AssertionError, match='c1_enc_stream_push_measured'):  # everything valid: the one entry point, whatever the kind
        s.push_measured(chans, masking=True)
    with pytest.raises(AssertionError, match='c1_enc_stream_push_measured'):
        s.push_measured(chans)
