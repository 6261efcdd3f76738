"""CPU-only: the measured allocation with every BFU's scale-factor index chosen by the same error (c1_encode_measured_sf_*).
What makes the GPU tests mean something, on the model of tests/scale_factor_choice_lib.py (built from the oracle alone): every
decision of the model on the shared material -- greedy steps, totals, the fallback and the choice among the candidates -- is
decided by a margin far above the tolerance of the error sums, its units are ordinary sound units, both branches of the fallback
occur, the gain over the plain measured allocation is the one the feature was proposed for, and one offset of 0 is that
allocation exactly.  Then silence, candidates whose index leaves 1 .. 63, and the checks the batch entry point makes before it
needs a context or a device."""
import ctypes as C

import numpy as np
import pytest

import measured_alloc_lib as MA
import scale_factor_choice_lib as SF

C1_OK, C1_ERR_ARG, C1_ERR_NO_DEVICE = 0, 1, 2   # include/carta1_hip.h
CASES = [('pink', 0), ('pink', 10), ('pink', 'detect'), ('white', 0), ('white', 58)]
# the aggregate gain over the plain measured model's, in dB.  Measured with this model: 1.71 (pink 10), 2.44 (white 58), 1.97 (pink,
# detection), 2.11 (pink 0) and 2.44 (white 0); the bar of 1.2 leaves 0.5 dB under the least of them
EXTRA_DB = 1.2


@pytest.mark.parametrize('material,kind', CASES)
def test_every_decision_of_the_model_has_a_margin(material, kind):
    """Measured here, the least greedy margin / the least candidate margin: pink 0 4.1e-7 / 1.4e-5, pink 10 1.06e-8 / 3.6e-6,
    pink detection 4.1e-7 / 1.4e-5, white 0 4.5e-7 / 1.7e-6, white 58 2.5e-7 / 1.6e-5; no exact tie between candidates at any
    entry with e < e(b, 0).  The error sums are known to 1e-12, so the GPU must reproduce every decision."""
    m = SF.case(kind, material)
    print(material, kind, 'least margin %.3g, least candidate margin %.3g, ties %d' % (float(m['margin'].min()), float(m['cand_margin']), int(m['ties'])))
    assert np.isfinite(m['D']).all() and (m['D'] > 0).all()
    assert (m['margin'] > MA.MARGIN).all(), float(m['margin'].min())
    assert m['cand_margin'] > 1e-9, float(m['cand_margin'])
    assert m['ties'] == 0


@pytest.mark.parametrize('material,kind', CASES)
def test_the_models_units_are_ordinary_sound_units(material, kind):
    m = SF.case(kind, material)
    assert SF.check_valid(m['units'], m['coefs'], m['taken'], m['D']) is None
    assert SF.check_outputs(m, m['units'], m['taken'], m['shifts'], m['D'], m['E']) is None
    final = np.where(m['taken'] != 0, m['D'][:, 1], m['D'][:, 0])
    assert (final <= m['D'][:, 0]).all()
    assert not m['shifts'][m['taken'] == 0].any()
    assert set(np.unique(m['shifts']).tolist()) <= set(SF.OFFSETS)
    assert (m['sfi'][m['s0'] != 0] >= 1).all() and (m['sfi'] <= 63).all()


def test_both_branches_occur():
    """Measured here on pink under byte 10: 253 units taken, 7 kept with the reference's record."""
    m = SF.case(10, 'pink')
    taken = int(m['taken'].sum())
    print('taken', taken, 'kept', len(m['taken']) - taken)
    assert taken >= 200 and len(m['taken']) - taken >= 3
    kept = m['taken'] == 0
    assert np.array_equal(m['units'][kept], m['ref'][kept]) and (m['units'][~kept] != m['ref'][~kept]).any(axis=1).all()


@pytest.mark.parametrize('material,kind', CASES)
def test_the_gain_is_the_one_proposed(material, kind):
    m, plain = SF.case(kind, material), MA.case(kind, material)
    assert np.array_equal(m['D'][:, 0], plain['D'][:, 0])                     # T_ref is the plain model's: the offset-0 table
    gain, before = float(SF.gain_db(m)), float(MA.gain_db(plain))
    shifted = m['shifts'][(m['taken'] != 0)[:, None] & (m['wl'] > 0) & (np.arange(52)[None, :] < m['nbfu'][:, None])]
    print(material, kind, 'gain %.2f dB, plain measured %.2f dB, taken %d of %d, offsets written %r' % (
        gain, before, int(m['taken'].sum()), len(m['taken']), {int(v): int((shifted == v).sum()) for v in SF.OFFSETS}))
    assert gain >= before + EXTRA_DB, (gain, before)
    assert len(set(shifted.tolist())) == len(SF.OFFSETS)                      # every candidate is written somewhere


@pytest.mark.parametrize('material,kind', [('white', 58), ('pink', 'detect')])
def test_offset_zero_alone_is_the_plain_measured_model(material, kind):
    m, plain = SF.case(kind, material, (0,)), MA.case(kind, material)
    for key in ('units', 'taken', 'nbfu', 'wl', 'margin'):
        assert np.array_equal(m[key], plain[key]), key
    for key in ('D', 'E'):
        assert np.array_equal(m[key].view(np.uint64), plain[key].view(np.uint64)), key
    assert not m['shifts'].any() and np.array_equal(m['sfi'], m['s0'])


def test_silence_is_left_to_the_reference():
    import oracle_lib as O
    silence = [np.zeros(8 * 512, dtype=np.float32)] * 2
    ref = O.encode_stream(silence)[0]
    m = SF.model(silence, ref)
    assert not m['taken'].any() and not m['D'].view(np.uint64).any() and not m['E'].view(np.uint64).any()    # +0.0 exactly
    assert np.array_equal(m['units'], ref) and not m['shifts'].any()


def test_candidates_whose_index_leaves_the_table_are_skipped():
    """a hand-built unit: BFUs of tiny coefficients (findScaleFactor 1 and 2), of huge ones (62 and 63), of silence (0) and of
    ordinary ones; offsets that reach below 1 and above 63"""
    offsets = (0, -2, 2, -1, 1, -8, 8)
    slots = np.zeros(512, dtype=np.float32)
    rng = np.random.RandomState(5)
    peak = {0: 5.5e-7, 1: 7e-7, 2: 0.7, 3: 0.9, 5: 0.01, 6: 1e-4}          # BFU -> peak; BFU 4 stays silent
    import pack_model_lib as PM
    for b, p in peak.items():
        first, n = int(PM.FIRST[b]), int(PM.SPECS[b])
        slots[first:first + n] = (rng.uniform(-1, 1, n) * p).astype(np.float32)
        slots[first] = p
    ek, valid, s0 = SF.error_tables(slots, [0, 0, 0], offsets)
    assert s0[:7].tolist() == [1, 2, 62, 63, 0, 44, 24], s0[:7].tolist()
    want = np.array([[s != 0 and 1 <= s + o <= 63 for s in s0] for o in offsets])
    assert np.array_equal(valid, want)
    assert not valid[:, 0][[1, 3, 5]].any() and valid[:, 0][[0, 2, 4, 6]].all()        # index 1: nothing below it
    assert not valid[:, 3][[2, 4, 6]].any() and valid[:, 3][[0, 1, 3, 5]].all()        # index 63: nothing above it
    assert not valid[:, 4].any() and valid[:, 5].all()
    e, pick = SF.least(ek, valid)
    assert np.isfinite(e).all()
    for b in range(7):
        assert valid[pick[b, 1:], b].all() or s0[b] == 0, b
        assert (1 <= s0[b] + np.asarray(offsets)[pick[b, 1:]]).all() or s0[b] == 0
    assert (e[4] == e[4, 0]).all() and not pick[4].any()                                # silence codes nothing
    assert (e[:, 1:] <= ek[0][:, 1:]).all()


def test_batch_argument_checks_need_neither_context_nor_device():
    """c1_encode_measured_sf_batch validates what its arguments alone decide, the offsets among them, before it looks at its
    context: C1_ERR_ARG with or without a device, and nothing written.  A valid call without a context is C1_ERR_NO_DEVICE where
    there is no device (and "context is NULL" where there is one)."""
    from carta1_amd import build, capi, codec
    build.build_library()
    lib = capi.load()
    assert capi.SIGNATURES['c1_encode_measured_sf_batch'] == capi.SIGNATURES['c1_encode_measured_sf_device']
    err = lambda: lib.c1_last_error().decode()
    opts = codec.EncoderOptions().to_c()
    frames, nch = 4, 2
    chans = [np.zeros(frames * 512, dtype=np.float32) for _ in range(nch)]
    ptrs = capi.ptr_array([c.ctypes.data for c in chans])
    units = np.full((frames * nch, 212), 0xA5, dtype=np.uint8)
    taken = np.full(frames * nch, 0xA5, dtype=np.uint8)
    shifts = np.full((frames * nch, 52), 0x5A, dtype=np.int8)
    dist = np.full((frames * nch, 2), -1.0)
    energy = np.full(frames * nch, -1.0)
    outs = lambda: (units.ctypes.data, taken.ctypes.data, shifts.ctypes.data, dist.ctypes.data, energy.ctypes.data)

    def call(offsets=SF.OFFSETS, n=None, o=None, fn=lib.c1_encode_measured_sf_batch, nch_=nch, frames_=frames, halo=0, options=opts, pcm=ptrs,
             modes=None):
        off = np.ascontiguousarray(list(offsets or ()) + [0] * 9, dtype=np.int8)
        m = None if modes is None else np.ascontiguousarray(modes, dtype=np.uint8)
        return fn(None, pcm, nch_, frames_, halo, C.byref(options) if options is not None else None, None if m is None else m.ctypes.data,
                  off.ctypes.data if offsets is not None else None, len(offsets) if n is None else n, *(o or outs()))

    assert call(n=0) == C1_ERR_ARG and 'c1_encode_measured_sf_batch' in err() and 'n_offsets = 0 is outside 1..8' in err(), err()
    assert call(n=9) == C1_ERR_ARG and 'n_offsets = 9 is outside 1..8' in err(), err()
    assert call((0, -1, 2, -1)) == C1_ERR_ARG and 'sf_offsets[3] repeats sf_offsets[1] = -1' in err(), err()
    assert call((0, 9)) == C1_ERR_ARG and 'sf_offsets[1] = 9 is outside -8..8' in err(), err()
    assert call((0, -9)) == C1_ERR_ARG and 'outside -8..8' in err(), err()
    assert call((-1, 0)) == C1_ERR_ARG and 'sf_offsets[0] = -1, not 0' in err(), err()
    assert call(None, n=1) == C1_ERR_ARG and 'sf_offsets is NULL' in err(), err()
    assert call(nch_=3) == C1_ERR_ARG and 'channels must be 1 or 2' in err(), err()
    assert call(frames_=-1) == C1_ERR_ARG and call(halo=3) == C1_ERR_ARG
    assert call(frames_=(1 << 22) + 1) == C1_ERR_ARG and 'at most' in err(), err()
    assert call(options=None) == C1_ERR_ARG and 'options are NULL' in err(), err()
    assert call(o=(None,) * 5) == C1_ERR_ARG
    assert 'c1_encode_measured_sf_batch: units, taken, shifts, distortion and energy are all NULL' in err(), err()
    assert call(pcm=None) == C1_ERR_ARG and 'pcm is NULL' in err(), err()
    bad = np.zeros(frames * nch, dtype=np.uint8)
    bad[5] = 1
    assert call(modes=bad) == C1_ERR_ARG and 'frame 2, channel 1' in err() and 'low field' in err(), err()
    assert call(fn=lib.c1_encode_measured_sf_device) == C1_ERR_ARG and 'context is NULL' in err()
    # a valid call: only the context (and, here, the device) is missing
    count = C.c_int(0)
    have_device = lib.c1_device_count(C.byref(count)) == C1_OK and count.value > 0
    for offsets in ((0,), SF.OFFSETS, (0, 8, -8, 1, -1, 2, -2, 3)):
        for o in (None, (None, None, shifts.ctypes.data, None, None), (units.ctypes.data, None, None, None, None)):
            rc = call(offsets, o=o)
            if have_device:
                assert rc == C1_ERR_ARG and 'context is NULL' in err(), err()
            else:
                assert rc == C1_ERR_NO_DEVICE and 'no HIP device' in err(), err()
    assert (units == 0xA5).all() and (taken == 0xA5).all() and (shifts == 0x5A).all() and (dist == -1.0).all() and (energy == -1.0).all()


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
    assert c1.SCALE_FACTOR_OFFSETS == SF.OFFSETS and c1.MAX_SCALE_FACTOR_OFFSETS == 8
    assert c1.check_scale_factor_offsets(c1.SCALE_FACTOR_OFFSETS).tolist() == [0, -1, 1, -2, -3]
    ctx = object.__new__(c1.Context)                                        # no device, no handle: the checks come first
    ctx._h = None
    guarded = _NoEncode(capi.load())
    monkeypatch.setattr(capi, 'load', lambda: guarded)
    chans = [np.zeros(4 * 512, dtype=np.float32)] * 2
    for bad, what in (((), 'between 1 and 8'), (range(9), 'between 1 and 8'), ((0, 1, 1), 'given twice'), ((0, 9), 'outside -8..8'),
                      ((1, 0), 'first scale-factor offset must be 0'), ((0, 300), 'within -8..8')):
        with pytest.raises(ValueError, match=what):
            ctx.encode_measured(chans, scale_factor_offsets=bad)
    with pytest.raises(ValueError, match='return_shifts needs'):
        ctx.encode_measured(chans, return_shifts=True)
    with pytest.raises(ValueError, match='low field'):
        ctx.encode_measured(chans, modes=np.ones((4, 2), dtype=np.uint8), scale_factor_offsets=(0, -1))
