"""CPU-only: the block modes chosen per sound unit from candidates by the error of the measured allocation
(c1_encode_measured_modes_*).  The conditions on the shared test material that make the GPU tests meaningful
(tests/measured_modes_lib.py: the model composed from the per-candidate models), that neither the best-modes choice nor the
two-call sequence gives the joint choice, the new symbols, the checks both entry points make before they need a context or a
device, and the Python wrapper's own."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import best_modes_lib as BMO
import measured_modes_lib as MM

C1_OK, C1_ERR_ARG, C1_ERR_NO_DEVICE = 0, 1, 2   # include/carta1_hip.h
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [('pink', False), ('pink', True), ('white', False), ('white', True)]
# the least aggregate gain of the joint choice over encode_best_modes followed by encode_measured(modes=modes_out), in dB.
# Measured with all eight candidates: 0.41, 0.33, 0.22 and 0.20
LEAST_GAIN_DB = {('pink', False): 0.30, ('pink', True): 0.25, ('white', False): 0.15, ('white', True): 0.15}


@pytest.mark.parametrize('material,sf', CASES)
def test_every_unit_has_one_best_candidate(material, sf):
    """Measured here: the least relative margin of a unit's minimum is 4.8e-5 (pink, plain, eight candidates), 5.0e-4 (pink,
    offsets, the three candidates of measured_modes_lib; 9.1e-5 with all eight, and a subset's is never below the full set's),
    2.0e-4 (white, plain) and 9.7e-4 (white, offsets).  Asserted as more than 1e-9 and as exactly one admissible candidate per
    unit, so the GPU tests excuse no unit."""
    fin = MM.case(material, sf)['final']
    assert np.isfinite(fin).all() and (fin > 0).all()
    margin = MM.unique_margin(fin)
    print(material, sf, 'least margin %.3g' % float(margin.min()))
    assert (margin > MM.UNIQUE_REL).all(), float(margin.min())
    assert (MM.admissible(fin).sum(axis=1) == 1).all()


def test_the_choice_is_not_trivial():
    """On pink at least four candidates win more than 20 units each (measured: 52, 57, 40, 35, 3, 6, 5, 62 of 260 in CANDIDATES
    order), so no constant answer passes the GPU tests."""
    winners = np.bincount(MM.case('pink', False)['choice'], minlength=8)
    print('pink winners', winners.tolist())
    assert (winners > 20).sum() >= 4, winners.tolist()


@pytest.mark.parametrize('material,sf', CASES)
def test_the_best_modes_choice_is_not_the_joint_choice(material, sf):
    """The joint winner differs from the argmin of best_modes_lib's D over the same candidates in more than half of the units
    (measured: 194 of 260 on pink, 182 of 260 with offsets and the three candidates, 104 and 110 of 128 on white): reusing
    k_choose_modes' choice fails the GPU tests."""
    m = MM.case(material, sf)
    seq = MM.sequence_choice(material, m['cand'].tolist())
    differs = int((m['choice'] != seq).sum())
    print(material, sf, differs, 'of', len(seq))
    assert differs > len(seq) // 2, differs


@pytest.mark.parametrize('material,sf', CASES)
def test_gain_over_the_two_call_sequence(material, sf):
    """over all eight candidates, also on pink with offsets (five more scale-factor models, the dearest test of this file): the
    bound is on the full search, and the three candidates the other tests use there give 0.21 dB"""
    gain = MM.gain_over_sequence_db(material, sf, MM.CANDIDATES)
    print(material, sf, 'gain over the sequence %.3f dB' % gain)
    assert gain >= LEAST_GAIN_DB[(material, sf)], gain


def test_model_is_the_per_candidate_models():
    """the composition itself: with one candidate every output is that candidate's model's, and a unit of the joint model is its
    winner's"""
    one = MM.case('white', False, [58])
    per = MM.candidate_case(58, 'white', False)
    assert not one['choice'].any() and (one['modes'] == 58).all()
    assert np.array_equal(one['units'], per['units']) and np.array_equal(one['taken'], per['taken'])
    assert np.array_equal(one['D'][:, 0].view(np.uint64), per['D'].view(np.uint64))
    m = MM.case('white', False)
    for u in (0, 17, 127):
        k = int(m['choice'][u])
        assert np.array_equal(m['units'][u], MM.candidate_case(MM.CANDIDATES[k], 'white', False)['units'][u])


def test_symbols_are_declared_exported_and_bound():
    from carta1_amd import build, capi
    import carta1_amd as c1
    build.build_library()
    lib = capi.load()
    header = open(os.path.join(ROOT, 'include', 'carta1_hip.h')).read()
    for name in ('c1_encode_measured_modes_device', 'c1_encode_measured_modes_batch'):
        assert re.search(r'\bint %s\(c1_ctx \*ctx,' % name, header), name
        assert name in capi.SIGNATURES and getattr(lib, name) is not None
    assert capi.SIGNATURES['c1_encode_measured_modes_batch'] == capi.SIGNATURES['c1_encode_measured_modes_device']
    assert len(capi.SIGNATURES['c1_encode_measured_modes_device'][1]) == 17
    assert callable(c1.Context.encode_measured_modes) and callable(c1.Context.encode_measured_modes_device)
    assert re.search(r'#define C1_ABI_VERSION 3\b', header)


class _NoEncode:
    """the library without its encode entry points"""
    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, name):
        if name.startswith('c1_encode'):
            raise AssertionError('the wrapper reached ' + name)
        return getattr(self._lib, name)


def test_python_wrapper_rejects_before_any_library_call(monkeypatch):
    import carta1_amd as c1
    from carta1_amd import build, capi
    build.build_library()
    ctx = object.__new__(c1.Context)                                        # no device, no handle: the checks come first
    ctx._h = None
    guarded = _NoEncode(capi.load())
    monkeypatch.setattr(capi, 'load', lambda: guarded)
    chans = [np.zeros(4 * 512, dtype=np.float32)] * 2
    for bad, what in (([], 'between 1 and 8'), (list(range(0, 18, 2)), 'between 1 and 8'), ([0, 58, 0], 'given twice'), ([1], 'low field'),
                      ([64], 'bits 6-7')):
        with pytest.raises(ValueError, match=what):
            ctx.encode_measured_modes(chans, bad)
    for bad, what in (([], 'between 1 and 8 scale-factor offsets'), (list(range(9)), 'between 1 and 8 scale-factor offsets'),
                      ([0, 9], 'outside -8..8'), ([0, -1, -1], 'given twice'), ([-1, 0], 'first scale-factor offset must be 0')):
        with pytest.raises(ValueError, match=what):
            ctx.encode_measured_modes(chans, [0, 58], scale_factor_offsets=bad)
    with pytest.raises(ValueError, match='multiple of 512'):
        ctx.encode_measured_modes([np.zeros(100, dtype=np.float32)], [0])


def test_argument_checks_need_neither_context_nor_device():
    """c1_encode_measured_modes_batch validates what its arguments alone decide before it looks at its context: C1_ERR_ARG naming
    the entry, with or without a device, and nothing written.  A valid call without a context is C1_ERR_NO_DEVICE where there is
    no device (and "context is NULL" where there is one).  The device form needs its context first, as its siblings do."""
    from carta1_amd import build, capi, codec
    build.build_library()
    lib = capi.load()
    err = lambda: lib.c1_last_error().decode()
    opts = codec.EncoderOptions().to_c()
    frames, nch = 4, 2
    chans = [np.zeros(frames * 512, dtype=np.float32) for _ in range(nch)]
    ptrs = capi.ptr_array([c.ctypes.data for c in chans])
    bufs = {'units': np.full((frames * nch, 212), 0xA5, dtype=np.uint8), 'choice': np.full(frames * nch, 0xA5, dtype=np.uint8),
            'modes': np.full(frames * nch, 0xA5, dtype=np.uint8), 'taken': np.full(frames * nch, 0xA5, dtype=np.uint8),
            'shifts': np.full((frames * nch, 52), 0x5A, dtype=np.int8), 'distortion': np.full((frames * nch, 8, 2), -1.0),
            'energy': np.full((frames * nch, 8), -1.0)}
    outs = lambda: tuple(a.ctypes.data for a in bufs.values())

    def call(cand, offs=(0,), n=None, n_off=None, o=None, fn=lib.c1_encode_measured_modes_batch, options=opts, channels=nch, halo=0):
        c = np.asarray(cand, dtype=np.uint8)
        f = np.asarray(offs, dtype=np.int8)
        return fn(None, ptrs, channels, frames, halo, C.byref(options) if options is not None else None, c.ctypes.data if c.size else None,
                  len(c) if n is None else n, f.ctypes.data if f.size else None, len(f) if n_off is None else n_off, *(o or outs()))

    all9 = BMO.CANDIDATES + [0]
    assert call(all9, n=0) == C1_ERR_ARG
    assert 'c1_encode_measured_modes_batch' in err() and 'n_cand = 0' in err() and '1..8' in err(), err()
    assert call(all9, n=9) == C1_ERR_ARG and 'n_cand = 9' in err(), err()
    assert call([]) == C1_ERR_ARG and 'n_cand = 0' in err(), err()
    assert call([58, 0, 58]) == C1_ERR_ARG and 'candidate 2' in err() and "0x3a is candidate 0's" in err(), err()
    assert call([0, 1]) == C1_ERR_ARG and 'candidate 1' in err() and 'low field of mode byte 0x01 is 1, not 0 or 2' in err(), err()
    assert call([0, 0x10]) == C1_ERR_ARG and 'candidate 1' in err() and 'high field' in err(), err()
    assert call([64]) == C1_ERR_ARG and 'candidate 0' in err() and 'bits 6-7' in err(), err()
    assert call([0, 58], offs=()) == C1_ERR_ARG and 'c1_encode_measured_modes_batch' in err() and 'n_offsets = 0' in err(), err()
    assert call([0, 58], offs=list(range(9))) == C1_ERR_ARG and 'n_offsets = 9' in err(), err()
    assert call([0, 58], offs=(0, 9)) == C1_ERR_ARG and 'sf_offsets[1] = 9 is outside -8..8' in err(), err()
    assert call([0, 58], offs=(0, -1, -1)) == C1_ERR_ARG and 'sf_offsets[2] repeats sf_offsets[1]' in err(), err()
    assert call([0, 58], offs=(-1, 0)) == C1_ERR_ARG and 'sf_offsets[0] = -1, not 0' in err(), err()
    assert call([0, 58], o=(None,) * 7) == C1_ERR_ARG
    assert 'units, choice, modes_out, taken, shifts, distortion and energy are all NULL' in err(), err()
    assert call([0, 58], options=None) == C1_ERR_ARG and 'options are NULL' in err(), err()
    assert call([0, 58], channels=3) == C1_ERR_ARG and 'channels must be 1 or 2' in err(), err()
    assert call([0, 58], halo=3) == C1_ERR_ARG
    assert call([0, 58], fn=lib.c1_encode_measured_modes_device) == C1_ERR_ARG and 'context is NULL' in err()
    assert call([0, 1], fn=lib.c1_encode_measured_modes_device) == C1_ERR_ARG
    # a valid call: only the context (and, here, the device) is missing
    count = C.c_int(0)
    have_device = lib.c1_device_count(C.byref(count)) == C1_OK and count.value > 0
    only = lambda k: tuple(a.ctypes.data if name == k else None for name, a in bufs.items())
    for cand, offs in (([0], (0,)), ([58, 0], MM.OFFSETS), (BMO.CANDIDATES, MM.OFFSETS)):
        for o in (None, only('choice'), only('units'), only('shifts')):
            rc = call(cand, offs=offs, o=o)
            if have_device:
                assert rc == C1_ERR_ARG and 'context is NULL' in err(), err()
            else:
                assert rc == C1_ERR_NO_DEVICE and 'no HIP device' in err(), err()
    for name, a in bufs.items():
        fill = {'shifts': 0x5A, 'distortion': -1.0, 'energy': -1.0}.get(name, 0xA5)
        assert (a == fill).all(), name
