"""CPU-only: the mode search of the measured allocation on live streams (c1_enc_stream_push_measured_modes,
EncoderStream.push_measured_modes).  The entry point is declared, exported and bound; what its arguments alone decide is decided
before it looks at its stream, with or without a device, and nothing is written; the Python wrapper raises its ValueErrors before
any library call.  The model of the pushed units is tests/measured_modes_lib.py's over the whole signal, whose margins
tests/test_measured_modes_cpu.py asserts as they are."""
import os
import re

import numpy as np
import pytest

import measured_modes_lib as MM

C1_ERR_ARG = 1   # include/carta1_hip.h
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
NAME = 'c1_enc_stream_push_measured_modes'


def test_declared_exported_and_bound():
    from carta1_amd import build, capi
    build.build_library()
    with open(os.path.join(ROOT, 'include', 'carta1_hip.h')) as f:
        header = f.read()
    assert re.search(r'\bint %s\(c1_enc_stream \*s, const float \*const \*pcm' % NAME, header)
    assert '#define C1_ABI_VERSION 3' in header
    lib = capi.load()
    assert getattr(lib, NAME) is not None                                   # exported
    restype, argtypes = capi.SIGNATURES[NAME]
    assert restype is capi.SIGNATURES['c1_encode_measured_modes_batch'][0]
    # stream, pcm, frames, then c1_encode_measured_modes_batch's arguments from the candidates on
    assert argtypes[3:] == capi.SIGNATURES['c1_encode_measured_modes_batch'][1][6:]
    assert getattr(lib, NAME).argtypes == argtypes


def _outputs(n, n_cand):
    return {'units': np.full((n, 212), 0xA5, dtype=np.uint8), 'choice': np.full(n, 0xA5, dtype=np.uint8),
            'modes': np.full(n, 0xA5, dtype=np.uint8), 'taken': np.full(n, 0xA5, dtype=np.uint8),
            'shifts': np.full((n, 52), 0x5A, dtype=np.int8), 'distortion': np.full((n, n_cand, 2), -1.0),
            'energy': np.full((n, n_cand), -1.0)}


def test_argument_checks_need_neither_stream_nor_device():
    from carta1_amd import build, capi
    build.build_library()
    lib = capi.load()
    err = lambda: lib.c1_last_error().decode()
    frames, nch = 4, 2
    chans = [np.zeros(frames * 512, dtype=np.float32) for _ in range(nch)]
    ptrs = capi.ptr_array([c.ctypes.data for c in chans])
    out = _outputs(frames * nch, 8)
    order = ('units', 'choice', 'modes', 'taken', 'shifts', 'distortion', 'energy')

    def call(cand=MM.CANDIDATES, n_cand=None, offsets=MM.OFFSETS, n_offsets=None, frames=frames, pcm=ptrs, units=True):
        cb = None if cand is None else np.ascontiguousarray(list(cand) + [0] * 9, dtype=np.uint8)
        off = None if offsets is None else np.ascontiguousarray(list(offsets) + [0] * 9, dtype=np.int8)
        n = n_cand if n_cand is not None else (0 if cand is None else len(cand))
        no = n_offsets if n_offsets is not None else (0 if offsets is None else len(offsets))
        bufs = [out[k].ctypes.data for k in order]
        if not units:
            bufs[0] = None
        return getattr(lib, NAME)(None, pcm, frames, None if cb is None else cb.ctypes.data, n, None if off is None else off.ctypes.data, no,
                                  *bufs)

    assert call(n_cand=0) == C1_ERR_ARG and NAME + ': n_cand = 0 is outside 1..8' in err(), err()
    assert call(n_cand=9) == C1_ERR_ARG and 'n_cand = 9 is outside 1..8' in err(), err()
    assert call(cand=None, n_cand=2) == C1_ERR_ARG and 'cand_modes is NULL' in err(), err()
    assert call(cand=[0, 1]) == C1_ERR_ARG and NAME + ': candidate 1: low field of mode byte 0x01 is 1, not 0 or 2' in err(), err()
    assert call(cand=[0x20]) == C1_ERR_ARG and 'candidate 0: high field of mode byte 0x20 is 2, not 0 or 3' in err(), err()
    assert call(cand=[0, 0x40]) == C1_ERR_ARG and 'bits 6-7 of mode byte 0x40 are set' in err(), err()
    assert call(cand=[10, 58, 10]) == C1_ERR_ARG and "candidate 2: mode byte 0x0a is candidate 0's" in err(), err()
    assert call(offsets=None, n_offsets=5) == C1_ERR_ARG and 'n_offsets = 5, but sf_offsets is NULL' in err(), err()
    assert call(offsets=(0, 9)) == C1_ERR_ARG and NAME + ': sf_offsets[1] = 9 is outside -8..8' in err(), err()
    assert call(offsets=(-1, 0)) == C1_ERR_ARG and 'sf_offsets[0] = -1, not 0' in err(), err()
    assert call(offsets=(0, 1, 1)) == C1_ERR_ARG and 'sf_offsets[2] repeats sf_offsets[1] = 1' in err(), err()
    assert call(offsets=(0,), n_offsets=0) == C1_ERR_ARG and 'n_offsets = 0 is outside 1..8' in err(), err()
    assert call(offsets=(0,), n_offsets=9) == C1_ERR_ARG and 'n_offsets = 9 is outside 1..8' in err(), err()
    assert call(frames=-1) == C1_ERR_ARG and 'frames must be >= 0' in err(), err()
    assert call(frames=(1 << 22) + 1) == C1_ERR_ARG and 'frames per call' in err(), err()
    assert call(pcm=None) == C1_ERR_ARG and 'pcm or units is NULL' in err(), err()
    assert call(units=False) == C1_ERR_ARG and 'pcm or units is NULL' in err(), err()
    # valid arguments, with and without offsets, one candidate and eight: only the stream is missing
    for kw in ({}, {'offsets': None}, {'cand': [58]}, {'cand': [0, 58], 'offsets': (0,)}, {'frames': 0}):
        assert call(**kw) == C1_ERR_ARG and 'stream is NULL' in err(), (kw, err())
    fill = _outputs(frames * nch, 8)
    assert all(np.array_equal(out[k].view(np.uint8), fill[k].view(np.uint8)) for k in out)


class _NoPush:
    """the library without its stream pushes"""
    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, name):
        if name.startswith('c1_enc_stream_push'):
            raise AssertionError('the wrapper reached ' + name)
        return getattr(self._lib, name)


def test_push_measured_modes_rejects_before_any_library_call(monkeypatch):
    import carta1_amd as c1
    from carta1_amd import build, capi
    build.build_library()
    s = object.__new__(c1.EncoderStream)                                    # no device, no handle: the checks come first
    s._h, s.channels = None, 2
    ctx = object.__new__(c1.Context)
    guarded = _NoPush(capi.load())
    monkeypatch.setattr(capi, 'load', lambda: guarded)
    chans = [np.zeros(4 * 512, dtype=np.float32)] * 2
    with pytest.raises(ValueError, match='expected 2 channels'):
        s.push_measured_modes(chans[:1], [0, 58])
    with pytest.raises(ValueError, match='multiple of 512'):
        s.push_measured_modes([c[:1000] for c in chans], [0, 58])
    # the candidates' and the offsets' errors are Context.encode_measured_modes' own, word for word
    for bad in ([], list(range(0, 18, 2)), [0, 1], [10, 10], [(2, 2)], [0x40]):
        with pytest.raises(ValueError) as mine:
            s.push_measured_modes(chans, bad)
        with pytest.raises(ValueError) as theirs:
            ctx.encode_measured_modes(chans, bad)
        assert str(mine.value) == str(theirs.value), bad
    for bad in ((0, 9), (-1, 0), (0, 1, 1), (), tuple(range(9))):
        with pytest.raises(ValueError) as mine:
            s.push_measured_modes(chans, [0, 58], scale_factor_offsets=bad)
        with pytest.raises(ValueError) as theirs:
            ctx.encode_measured_modes(chans, [0, 58], scale_factor_offsets=bad)
        assert str(mine.value) == str(theirs.value), bad
    with pytest.raises(AssertionError, match=NAME):                         # everything valid: the one entry point
        s.push_measured_modes(chans, [0, 58])
    with pytest.raises(AssertionError, match=NAME):
        s.push_measured_modes(chans, MM.CANDIDATES, scale_factor_offsets=MM.OFFSETS, return_distortion=True, return_shifts=True)
