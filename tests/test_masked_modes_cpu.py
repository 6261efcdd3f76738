"""CPU-only: the measured block-mode search under one masking threshold per unit (c1_encode_measured_modes_masked_*).  Why the
thresholds are shared (a unit's own-mode thresholds are not comparable across candidates), the conditions on the shared test
material that make the GPU tests meaningful (tests/masked_modes_lib.py), that the weighted winner is not the unweighted search's,
the gains over what a masking caller has without this call, the new symbols, the checks the entry points make before they need a
context, a stream or a device, and the Python wrappers' own."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import best_modes_lib as BMO
import masked_alloc_lib as MK
import masked_modes_lib as X
import measured_modes_lib as MM

C1_OK, C1_ERR_ARG, C1_ERR_NO_DEVICE = 0, 1, 2   # include/carta1_hip.h
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# all eight candidates, the packaged tables; the pink five-offset case costs about two minutes here and is shared by four tests
CASES = [('pink', (0,)), ('pink', X.OFFSETS), ('white', (0,)), ('white', X.OFFSETS)]
IDS = ['pink-0', 'pink-5', 'white-0', 'white-5']
# the aggregate weighted error of the masked allocation under the detector's modes over the joint choice's, both judged from the
# bytes under the shared weights, in dB.  Measured: 2.30 (offset 0) and 2.09 (the five offsets); asserted: three quarters of
# that, rounded down to 0.05 dB, the margin the unweighted search's tests gave their gains
LEAST_GAIN_OVER_DETECTOR_DB = {(0,): 1.70, X.OFFSETS: 1.55}


def joint(material, offsets):
    return X.case(material, 'packaged', offsets, X.CANDIDATES)


def test_own_mode_thresholds_are_not_comparable():
    """Under the packaged tables a unit's thresholds under byte 58, formed as c1_encode_measured_masked_* forms them from the
    all-short spectrum, differ from its thresholds under byte 0 by more than 10 dB in some BFU of the pink material (measured:
    19.7 dB).  Weighing candidate 58 with the one and candidate 0 with the other would compare errors in units that differ by a
    factor of up to 90: the definition shares one threshold."""
    with np.errstate(divide='ignore', invalid='ignore'):
        db = np.abs(10.0 * np.log10(X.own_thresholds(58) / X.own_thresholds(0)))
    print('largest difference %.2f dB, median over the units of their largest %.2f dB' % (np.nanmax(db), np.nanmedian(np.nanmax(db, axis=1))))
    assert np.nanmax(db) > 10.0


@pytest.mark.parametrize('material,offsets', CASES, ids=IDS)
def test_every_unit_has_one_best_candidate(material, offsets):
    """Measured here, with all eight candidates: the least relative margin of a unit's minimum weighted T_final is 3.9e-4 (pink,
    offset 0), 2.4e-5 (pink, five offsets), 2.0e-4 and 1.4e-4 (white).  Asserted as more than 1e-9 and as exactly one admissible
    candidate per unit, so the GPU tests excuse no unit (a subset's margin is never below the full set's)."""
    fin = joint(material, offsets)['final']
    assert np.isfinite(fin).all() and (fin > 0).all()
    margin = MM.unique_margin(fin)
    print(material, offsets, 'least margin %.3g' % float(margin.min()))
    assert (margin > X.UNIQUE_REL).all(), float(margin.min())
    assert (MM.admissible(fin).sum(axis=1) == 1).all()


@pytest.mark.parametrize('material,offsets', CASES, ids=IDS)
def test_the_choice_is_not_the_unweighted_searchs(material, offsets):
    """The weighted winner differs from the unweighted search's over the same candidates in at least a quarter of the units
    (measured: 119 and 121 of 260 on pink, 88 and 62 of 128 on white): handing on k_measured_modes' choice fails the GPU tests."""
    m = joint(material, offsets)
    unweighted = MM.case(material, tuple(offsets) != (0,), X.CANDIDATES)
    differs = int((m['choice'] != unweighted['choice']).sum())
    print(material, offsets, differs, 'of', len(m['choice']), 'winners', np.bincount(m['choice'], minlength=8).tolist())
    assert 4 * differs >= len(m['choice']), differs


@pytest.mark.parametrize('offsets', [(0,), X.OFFSETS], ids=['offset0', 'offsets'])
def test_gains_over_what_a_masking_caller_has(offsets):
    """On pink, judged from the bytes with masked_alloc_lib.weighted_errors under the shared weights P.  Against the masked
    allocation under the detector's modes: at least LEAST_GAIN_OVER_DETECTOR_DB.  Against the exact two-call composition (the
    unweighted search for modes_out, then the masked call under those modes with its own-mode weights; measured: 0.29 and 0.19
    dB): not negative."""
    m = joint('pink', offsets)
    ar = np.arange(len(m['choice']))
    ours = X.weighted_total(m['units'], m['coefs'], m['P'])
    reported = m['final'][ar, m['choice']].sum()
    assert abs(ours - reported) <= 1e-9 * reported                                   # the bytes hold what the model reports
    base = X.weighted_total(*X.detector_baseline('pink', 'packaged', offsets), m['P'])
    units, coefs, _ = X.two_call_composition('pink', 'packaged', offsets, X.CANDIDATES)
    composed = X.weighted_total(units, coefs, m['P'])
    print(offsets, 'over the detector\'s modes %.3f dB, over the two-call composition %.3f dB' % (X.gain_db(base, ours), X.gain_db(composed, ours)))
    assert X.gain_db(base, ours) >= LEAST_GAIN_OVER_DETECTOR_DB[tuple(offsets)]
    assert X.gain_db(composed, ours) >= 0.0


def test_model_is_the_existing_models():
    """the composition itself: under flat tables the model is measured_modes_lib's (the unweighted search's); with the single
    candidate 0 it is masked_alloc_lib's under constant modes 0, weights included; weights does not depend on the candidates"""
    flat = X.case('white', 'flat', (0,), X.CANDIDATES)
    unweighted = MM.case('white', False, X.CANDIDATES)
    assert (flat['P'] == 1.0).all()
    for k in ('choice', 'modes', 'taken', 'units'):
        assert np.array_equal(flat[k], unweighted[k]), k
    assert np.array_equal(flat['D'].view(np.uint64), unweighted['D'].view(np.uint64))
    one, own = X.case('white', 'packaged', X.OFFSETS, [0]), MK.case(0, 'white', 'packaged', X.OFFSETS)
    for k in ('taken', 'units', 'shifts'):
        assert np.array_equal(one[k], own[k]), k
    assert MK.bitwise(one['D'][:, 0], own['D']) and MK.bitwise(one['E'][:, 0], own['E']) and MK.bitwise(one['P'], own['P'])
    assert MK.bitwise(X.case('white', 'packaged', X.OFFSETS, [58])['P'], own['P'])
    assert MK.bitwise(joint('white', X.OFFSETS)['D'][:, 0], own['D'])                # the column of byte 0


NAMES = ('c1_encode_measured_modes_masked_device', 'c1_encode_measured_modes_masked_batch', 'c1_enc_stream_push_measured_modes_masked')


def test_symbols_are_declared_exported_and_bound():
    from carta1_amd import build, capi
    import carta1_amd as c1
    import inspect
    build.build_library()
    lib = capi.load()
    header = open(os.path.join(ROOT, 'include', 'carta1_hip.h')).read()
    for name in NAMES:
        assert re.search(r'\bint %s\((c1_ctx \*ctx|c1_enc_stream \*s),' % name, header), name
        assert name in capi.SIGNATURES and getattr(lib, name) is not None
    assert capi.SIGNATURES[NAMES[1]] == capi.SIGNATURES[NAMES[0]]
    assert len(capi.SIGNATURES[NAMES[0]][1]) == 20 == len(capi.SIGNATURES['c1_encode_measured_modes_device'][1]) + 3
    assert len(capi.SIGNATURES[NAMES[2]][1]) == 17 == len(capi.SIGNATURES['c1_enc_stream_push_measured_modes'][1]) + 3
    for fn in (c1.Context.encode_measured_modes, c1.EncoderStream.push_measured_modes):
        p = inspect.signature(fn).parameters
        assert p['masking'].default is None and p['return_weights'].default is False
    p = inspect.signature(c1.Context.encode_measured_modes_device).parameters
    assert p['masking'].default is None and p['weights_ptr'].default is None
    assert re.search(r'#define C1_ABI_VERSION 3\b', header)


class _NoEncode:
    """the library without its encode and push entry points"""
    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, name):
        if name.startswith('c1_encode') or name.startswith('c1_enc_stream_push'):
            raise AssertionError('the wrapper reached ' + name)
        return getattr(self._lib, name)


def test_python_wrappers_reject_before_any_library_call(monkeypatch):
    import carta1_amd as c1
    from carta1_amd import build, capi
    build.build_library()
    ctx = object.__new__(c1.Context)                                        # no device, no handle: the checks come first
    ctx._h = None
    stream = object.__new__(c1.EncoderStream)
    stream._h, stream.channels = None, 2
    guarded = _NoEncode(capi.load())
    monkeypatch.setattr(capi, 'load', lambda: guarded)
    chans = [np.zeros(4 * 512, dtype=np.float32)] * 2
    floor, spread = MK.packaged()
    bad_floor = np.array(floor)
    bad_floor[3] = 0.0
    bad_spread = np.array(spread)
    bad_spread[0, 1] = -1.0
    for call in (lambda **kw: ctx.encode_measured_modes(chans, [0, 58], **kw), lambda **kw: stream.push_measured_modes(chans, [0, 58], **kw)):
        with pytest.raises(ValueError, match='return_weights needs masking'):
            call(return_weights=True)
        with pytest.raises(ValueError, match='masking must be True or a'):
            call(masking=False)
        with pytest.raises(ValueError, match='the floor must hold 52 values'):
            call(masking=(floor[:51], None))
        with pytest.raises(ValueError, match='the spread must hold 52 x 52 values'):
            call(masking=(floor, spread[:51]))
        with pytest.raises(ValueError, match=r'mask_floor\[3\] = 0.0 is outside'):
            call(masking=(bad_floor, spread))
        with pytest.raises(ValueError, match=r'mask_spread\[1\] = -1.0 is outside'):
            call(masking=(floor, bad_spread))
        with pytest.raises(ValueError, match='outside -8..8'):
            call(masking=True, scale_factor_offsets=[0, 9])
    with pytest.raises(ValueError, match='given twice'):
        ctx.encode_measured_modes(chans, [0, 58, 0], masking=True)
    with pytest.raises(ValueError, match='low field'):
        stream.push_measured_modes(chans, [1], masking=True)
    with pytest.raises(ValueError, match='weights_ptr needs masking'):
        ctx.encode_measured_modes_device([0, 0], 4, [0, 58], units_ptr=1, weights_ptr=1)
    # the combinations that stay rejected: a signals form and the many-items form do not exist
    with pytest.raises(ValueError, match='measured_mode_candidates and masking cannot be combined: the mode search has no masking weights'):
        c1.encode_aea_pcm_many([], measured_allocation=True, masking=True, measured_mode_candidates=[0, 58])


def test_argument_checks_need_neither_context_nor_stream_nor_device():
    """c1_encode_measured_modes_masked_batch and c1_enc_stream_push_measured_modes_masked validate what their arguments alone
    decide before they look at their context or stream: C1_ERR_ARG naming the entry, with or without a device, and nothing
    written.  A valid batch call without a context is C1_ERR_NO_DEVICE where there is no device (and "context is NULL" where
    there is one).  The device form needs its context first, as its siblings do."""
    from carta1_amd import build, capi, codec
    build.build_library()
    lib = capi.load()
    err = lambda: lib.c1_last_error().decode()
    opts = codec.EncoderOptions().to_c()
    frames, nch = 4, 2
    chans = [np.zeros(frames * 512, dtype=np.float32) for _ in range(nch)]
    ptrs = capi.ptr_array([c.ctypes.data for c in chans])
    n = frames * nch
    fills = {'units': 0xA5, 'choice': 0xA5, 'modes': 0xA5, 'taken': 0xA5, 'shifts': 0x5A, 'distortion': -1.0, 'energy': -1.0, 'weights': -1.0}
    bufs = {'units': np.full((n, 212), 0xA5, dtype=np.uint8), 'choice': np.full(n, 0xA5, dtype=np.uint8), 'modes': np.full(n, 0xA5, dtype=np.uint8),
            'taken': np.full(n, 0xA5, dtype=np.uint8), 'shifts': np.full((n, 52), 0x5A, dtype=np.int8), 'distortion': np.full((n, 8, 2), -1.0),
            'energy': np.full((n, 8), -1.0), 'weights': np.full((n, 52), -1.0)}
    outs = lambda: tuple(a.ctypes.data for a in bufs.values())
    good_floor, good_spread = (np.ascontiguousarray(a, dtype=np.float64) for a in MK.packaged())

    def entry(a, at, value):
        a = np.array(a, dtype=np.float64)
        a.reshape(-1)[at] = value
        return a

    def call(cand, offs=(0,), n_cand=None, n_off=None, o=None, fn='batch', options=opts, channels=nch, halo=0, floor=good_floor, spread=good_spread):
        c = np.asarray(cand, dtype=np.uint8)
        f = np.asarray(offs, dtype=np.int8)
        tail = (c.ctypes.data if c.size else None, len(c) if n_cand is None else n_cand, f.ctypes.data if f.size else None,
                len(f) if n_off is None else n_off, None if floor is None else floor.ctypes.data, None if spread is None else spread.ctypes.data)
        if fn == 'push':
            return lib.c1_enc_stream_push_measured_modes_masked(None, ptrs, frames, *tail, *(o or outs()))
        fn = lib.c1_encode_measured_modes_masked_batch if fn == 'batch' else lib.c1_encode_measured_modes_masked_device
        return fn(None, ptrs, channels, frames, halo, C.byref(options) if options is not None else None, *tail, *(o or outs()))

    all9 = BMO.CANDIDATES + [0]
    for fn, name in (('batch', NAMES[1]), ('push', NAMES[2])):
        assert call(all9, n_cand=0, fn=fn) == C1_ERR_ARG and name in err() and 'n_cand = 0' in err() and '1..8' in err(), err()
        assert call(all9, n_cand=9, fn=fn) == C1_ERR_ARG and 'n_cand = 9' in err(), err()
        assert call([58, 0, 58], fn=fn) == C1_ERR_ARG and 'candidate 2' in err() and "0x3a is candidate 0's" in err(), err()
        assert call([0, 1], fn=fn) == C1_ERR_ARG and 'candidate 1' in err() and 'low field of mode byte 0x01 is 1, not 0 or 2' in err(), err()
        assert call([64], fn=fn) == C1_ERR_ARG and 'candidate 0' in err() and 'bits 6-7' in err(), err()
        assert call([0, 58], offs=list(range(9)), fn=fn) == C1_ERR_ARG and name in err() and 'n_offsets = 9' in err(), err()
        assert call([0, 58], offs=(0, 9), fn=fn) == C1_ERR_ARG and 'sf_offsets[1] = 9 is outside -8..8' in err(), err()
        assert call([0, 58], offs=(0, -1, -1), fn=fn) == C1_ERR_ARG and 'sf_offsets[2] repeats sf_offsets[1]' in err(), err()
        assert call([0, 58], offs=(-1, 0), fn=fn) == C1_ERR_ARG and 'sf_offsets[0] = -1, not 0' in err(), err()
        # the tables: c1_encode_measured_masked_*'s checks, with its messages
        assert call([0, 58], floor=None, fn=fn) == C1_ERR_ARG and '%s: mask_floor is NULL' % name in err(), err()
        assert call([0, 58], floor=entry(good_floor, 0, 1e-61), fn=fn) == C1_ERR_ARG and '%s: mask_floor[0] = 1e-61 is outside [1e-60, 1e60]' % name in err(), err()
        assert call([0, 58], floor=entry(good_floor, 51, np.nan), fn=fn) == C1_ERR_ARG and 'mask_floor[51] = nan' in err(), err()
        assert call([0, 58], floor=entry(good_floor, 20, np.inf), fn=fn) == C1_ERR_ARG and 'mask_floor[20] = inf' in err(), err()
        assert call([0, 58], spread=entry(good_spread, 52 * 3 + 5, -1e-300), fn=fn) == C1_ERR_ARG
        assert '%s: mask_spread[161] = -1e-300 (masker 5 onto BFU 3) is outside [0, 1e60]' % name in err(), err()
        assert call([0, 58], spread=entry(good_spread, 2703, 1e61), fn=fn) == C1_ERR_ARG and 'mask_spread[2703] = 1e+61 (masker 51 onto BFU 51)' in err(), err()
    assert call([0, 58], offs=()) == C1_ERR_ARG and 'n_offsets = 0' in err(), err()
    assert call([0, 58], offs=(), n_off=3, fn='push') == C1_ERR_ARG and 'n_offsets = 3, but sf_offsets is NULL' in err(), err()
    assert call([0, 58], o=(None,) * 8) == C1_ERR_ARG
    assert 'units, choice, modes_out, taken, shifts, distortion, energy and weights are all NULL' in err(), err()
    assert call([0, 58], o=(None,) * 8, fn='push') == C1_ERR_ARG and 'pcm or units is NULL' in err(), err()
    assert call([0, 58], options=None) == C1_ERR_ARG and 'options are NULL' in err(), err()
    assert call([0, 58], channels=3) == C1_ERR_ARG and 'channels must be 1 or 2' in err(), err()
    assert call([0, 58], halo=3) == C1_ERR_ARG
    assert call([0, 58], fn='device') == C1_ERR_ARG and 'context is NULL' in err()
    assert call([0, 1], fn='device') == C1_ERR_ARG
    # valid calls: only the stream, or the context (and, here, the device), is missing
    assert call([0, 58], offs=MM.OFFSETS, fn='push') == C1_ERR_ARG and '%s: stream is NULL' % NAMES[2] in err(), err()
    assert call([0, 58], offs=(), fn='push', spread=None) == C1_ERR_ARG and 'stream is NULL' in err(), err()
    count = C.c_int(0)
    have_device = lib.c1_device_count(C.byref(count)) == C1_OK and count.value > 0
    only = lambda k: tuple(a.ctypes.data if name == k else None for name, a in bufs.items())
    for cand, offs, spread in (([0], (0,), None), ([58, 0], MM.OFFSETS, good_spread), (BMO.CANDIDATES, MM.OFFSETS, good_spread)):
        for o in (None, only('choice'), only('units'), only('weights')):
            rc = call(cand, offs=offs, o=o, spread=spread)
            if have_device:
                assert rc == C1_ERR_ARG and 'context is NULL' in err(), err()
            else:
                assert rc == C1_ERR_NO_DEVICE and 'no HIP device' in err(), err()
    for name, a in bufs.items():
        assert (a == fills[name]).all(), name
