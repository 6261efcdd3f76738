"""CPU-only: the block modes chosen per sound unit from candidates by least coding error (c1_encode_best_modes_*).  The
conditions on the shared test material that make the GPU tests meaningful (tests/best_modes_lib.py: the model of the weighted D
and E from the oracle alone), the scaling facts the weights rest on, the independence of a unit's candidates from the modes of
the frames before it, the candidate helper of the Python host, and the checks the batch entry point makes before it needs a
context or a device."""
import ctypes as C

import numpy as np
import pytest

import best_modes_lib as BMO
import block_modes_lib as BM

C1_OK, C1_ERR_ARG, C1_ERR_NO_DEVICE = 0, 1, 2   # include/carta1_hip.h
LONG, SHORT = BMO.CANDIDATES.index(0), BMO.CANDIDATES.index(0x3a)


def test_every_unit_has_one_best_candidate():
    """Measured here: the least relative gap between a unit's best and second-best candidate is 6.1e-4 on the pink material
    (260 units) and 3.4e-5 on the white material (128 units); asserted as more than 1e-9, and as exactly one admissible
    candidate per unit, so the GPU test excuses no unit."""
    for kind in ('pink', 'white'):
        D = BMO.case(kind)['D']
        assert np.isfinite(D).all() and (D > 0).all()
        print(kind, 'least margin %.3g' % float(BMO.unique_margin(D).min()))
        assert (BMO.unique_margin(D) > BMO.UNIQUE_REL).all(), float(BMO.unique_margin(D).min())
        assert (BMO.admissible(D).sum(axis=1) == 1).all()


def test_the_choice_is_not_trivial():
    """Measured here, in CANDIDATES order (bytes 0, 48, 8, 56, 2, 50, 10, 58).  Pink: the winners are 1, 0, 1, 0, 77, 9, 103,
    69 of 260 units -- four candidates (2, 50, 10, 58) win more than five units each, and all-long is wrong in 99.6 % of the
    units.  White: 65, 39, 0, 6, 0, 6, 4, 8 of 128 units -- all-long wins more than a third, and five other candidates win
    somewhere.  An implementation that answers any one candidate fails the GPU tests on most units of one material."""
    pink = np.bincount(BMO.case('pink')['D'].argmin(axis=1), minlength=8)
    white = np.bincount(BMO.case('white')['D'].argmin(axis=1), minlength=8)
    print('pink winners', pink.tolist(), 'white winners', white.tolist())
    assert (pink > 5).sum() >= 4, pink.tolist()
    assert pink[LONG] <= 0.1 * pink.sum(), pink.tolist()
    assert white[LONG] >= white.sum() / 3, white.tolist()
    assert (np.delete(white, LONG) > 0).sum() >= 4, white.tolist()


def test_scaling_facts_the_weights_rest_on():
    """Per band, the unweighted coefficient energy of the all-long stream over that of the all-short stream is 0.25, 0.25 and
    0.5 (measured deviation: 5.0e-9 relative at most, asserted within 1e-6), and the weighted E(u, k) of a unit agrees across
    all eight candidates (measured: 2.3e-7 relative at most on pink, 4.1e-8 on white; asserted within 1e-5)."""
    for kind in ('pink', 'white'):
        m = BMO.case(kind)
        cl, cs = m['coefs'][LONG].astype(np.float64), m['coefs'][SHORT].astype(np.float64)
        for band, want in zip(BMO.BANDS, (0.25, 0.25, 0.5)):
            ratio = np.sum(cl[:, band] ** 2) / np.sum(cs[:, band] ** 2)
            print(kind, 'long / short energy %.12g' % ratio)
            assert abs(ratio - want) <= 1e-6 * want, (kind, ratio)
        E = m['E']
        spread = (E.max(axis=1) - E.min(axis=1)) / E.min(axis=1)
        print(kind, 'largest spread of E over the candidates %.3g' % float(spread.max()))
        assert (spread <= 1e-5).all(), float(spread.max())


def test_a_units_candidates_do_not_depend_on_the_modes_before_it():
    """The stream encoded under the per-unit chosen bytes equals, unit for unit, the composition of the eight constant-mode
    streams: applyTailWindowing saves the same tail whatever the band's mode.  Measured: equal on both materials."""
    for kind in ('pink', 'white'):
        m = BMO.case(kind)
        best = m['D'].argmin(axis=1)
        composed = np.stack([m['units'][k][u] for u, k in enumerate(best)])
        assert np.array_equal(BMO.chosen_units(kind, best), composed), kind
        assert np.array_equal(BM.modes_of_units(composed), np.asarray(BMO.CANDIDATES, dtype=np.uint8)[best])


def test_python_candidate_helper():
    from carta1_amd import codec
    assert codec.MAX_MODE_CANDIDATES == 8
    assert codec.mode_candidates([58, 0, (2, 0, 3)]).tolist() == [58, 0, 50]
    assert codec.mode_candidates(BMO.CANDIDATES).tolist() == BMO.CANDIDATES
    with pytest.raises(ValueError, match='between 1 and 8 candidate block modes'):
        codec.mode_candidates([])
    with pytest.raises(ValueError, match='between 1 and 8 candidate block modes'):
        codec.mode_candidates(BMO.CANDIDATES + [0])
    with pytest.raises(ValueError, match='candidate 2: mode byte 0x3a is given twice'):
        codec.mode_candidates([58, 0, (2, 2, 3)])
    with pytest.raises(ValueError, match='candidate 1: low field of mode byte 0x01 is 1, not 0 or 2'):
        codec.mode_candidates([0, 1])
    with pytest.raises(ValueError, match='candidate 0: bits 6-7'):
        codec.mode_candidates([64])
    with pytest.raises(ValueError, match='high field'):
        codec.mode_candidates([(0, 0, 2)])


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
            ctx.encode_best_modes(chans, bad)
    with pytest.raises(ValueError, match='multiple of 512'):
        ctx.encode_best_modes([np.zeros(100, dtype=np.float32)], [0])


def test_batch_argument_checks_need_neither_context_nor_device():
    """c1_encode_best_modes_batch validates what its arguments alone decide before it looks at its context: C1_ERR_ARG naming
    the entry, with or without a device, and nothing written.  A valid call without a context is C1_ERR_NO_DEVICE where there
    is no device (and "context is NULL" where there is one)."""
    from carta1_amd import build, capi, codec
    build.build_library()
    lib = capi.load()
    assert capi.SIGNATURES['c1_encode_best_modes_batch'] == capi.SIGNATURES['c1_encode_best_modes_device']
    err = lambda: lib.c1_last_error().decode()
    opts = codec.EncoderOptions().to_c()
    frames, nch = 4, 2
    chans = [np.zeros(frames * 512, dtype=np.float32) for _ in range(nch)]
    ptrs = capi.ptr_array([c.ctypes.data for c in chans])
    units = np.full((frames * nch, 212), 0xA5, dtype=np.uint8)
    choice = np.full(frames * nch, 0xA5, dtype=np.uint8)
    modes = np.full(frames * nch, 0xA5, dtype=np.uint8)
    dist = np.full((frames * nch, 8), -1.0)
    energy = np.full((frames * nch, 8), -1.0)
    outs = lambda: (units.ctypes.data, choice.ctypes.data, modes.ctypes.data, dist.ctypes.data, energy.ctypes.data)

    def call(cand, n=None, o=None, fn=lib.c1_encode_best_modes_batch):
        c = np.asarray(cand, dtype=np.uint8)
        return fn(None, ptrs, nch, frames, 0, C.byref(opts), c.ctypes.data if c.size else None, len(c) if n is None else n, *(o or outs()))

    all9 = BMO.CANDIDATES + [0]
    assert call(all9, 0) == C1_ERR_ARG
    assert 'c1_encode_best_modes_batch' in err() and 'n_cand = 0' in err() and '1..8' in err(), err()
    assert call(all9, 9) == C1_ERR_ARG
    assert 'n_cand = 9' in err(), err()
    assert call([58, 0, 58]) == C1_ERR_ARG
    assert 'candidate 2' in err() and "0x3a is candidate 0's" in err(), err()
    assert call([0, 1]) == C1_ERR_ARG
    assert 'candidate 1' in err() and 'low field of mode byte 0x01 is 1, not 0 or 2' in err(), err()
    assert call([0, 0x10]) == C1_ERR_ARG
    assert 'candidate 1' in err() and 'high field' in err(), err()
    assert call([64]) == C1_ERR_ARG
    assert 'candidate 0' in err() and 'bits 6-7' in err(), err()
    assert call([0, 58], o=(None,) * 5) == C1_ERR_ARG
    assert 'units, choice, modes_out, distortion and energy are all NULL' in err(), err()
    assert call([0, 58], fn=lib.c1_encode_best_modes_device) == C1_ERR_ARG
    assert 'context is NULL' in err()
    # a valid call: only the context (and, here, the device) is missing
    count = C.c_int(0)
    have_device = lib.c1_device_count(C.byref(count)) == C1_OK and count.value > 0
    for cand in ([0], [58, 0], BMO.CANDIDATES):
        for o in (None, (None, choice.ctypes.data, None, None, None), (units.ctypes.data, None, None, None, None)):
            rc = call(cand, o=o)
            if have_device:
                assert rc == C1_ERR_ARG and 'context is NULL' in err(), err()
            else:
                assert rc == C1_ERR_NO_DEVICE and 'no HIP device' in err(), err()
    assert (units == 0xA5).all() and (choice == 0xA5).all() and (modes == 0xA5).all() and (dist == -1.0).all() and (energy == -1.0).all()
