"""CPU-only: the measured allocation with every BFU's error divided by a masking threshold (c1_encode_measured_masked_*).  What
makes the GPU tests mean something, on the model of tests/masked_alloc_lib.py: every decision of the model on the shared material
is decided by a margin far above the tolerance of the error sums, under the packaged tables and under three explicit ones; both
branches of the fallback occur under non-trivial weights; flat tables are the scale-factor-choice model exactly; scaling both
tables by 4 scales the errors by exactly 1/4 and moves nothing; the weighted error of the model's units lies below that of the
unweighted model's units judged under the same weights.  Then the packaged tables against the tool that documents them, silence,
and the checks the hosts make before they need a context or a device."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import masked_alloc_lib as MK
import measured_alloc_lib as MA
import scale_factor_choice_lib as SF

C1_OK, C1_ERR_ARG, C1_ERR_NO_DEVICE = 0, 1, 2   # include/carta1_hip.h
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [('pink', 0), ('pink', 10), ('pink', 'detect'), ('white', 58)]
EXPLICIT = ['specs', 'ramp', 'self']


@pytest.mark.parametrize('material,kind', CASES)
def test_every_decision_under_the_packaged_tables_has_a_margin(material, kind):
    """Measured here with the packaged tables and the offsets (0,-1,1,-2,-3), the least decision margin / the least candidate
    margin / units taken: pink 0 3.9e-7 / 1.4e-5 / 260 of 260, pink 10 6.5e-7 / 3.6e-6 / 260, pink detection 3.9e-7 / 1.4e-5 /
    260, white 58 1.8e-6 / 1.6e-5 / 128 of 128; no exact tie.  The error sums are known to 1e-12, so the GPU must reproduce
    every decision."""
    m = MK.case(kind, material)
    print(material, kind, 'least margin %.3g, least candidate margin %.3g, ties %d, taken %d of %d' % (
        float(m['margin'].min()), float(m['cand_margin']), int(m['ties']), int(m['taken'].sum()), len(m['taken'])))
    assert np.isfinite(m['D']).all() and (m['D'] > 0).all() and np.isfinite(m['P']).all() and (m['P'] > 0).all()
    assert (m['margin'] > MA.MARGIN).all(), float(m['margin'].min())
    assert m['cand_margin'] > 1e-9, float(m['cand_margin'])
    assert m['ties'] == 0


@pytest.mark.parametrize('name,taken,kept', [('specs', 235, 25), ('ramp', 230, 30), ('self', 260, 0)])
def test_explicit_tables_on_pink_under_byte_10(name, taken, kept):
    """offsets (0,); measured here, the least margin: 9.2e-7 (floor = SPECS_PER_BFU), 2.7e-7 (floor[b] = 10^(b/13 - 2)), 5.8e-8
    (floor 1e-12 under the identity: pure self-masking)"""
    m = MK.case(10, 'pink', name, (0,))
    print(name, 'taken', int(m['taken'].sum()), 'kept', int((m['taken'] == 0).sum()), 'least margin %.3g' % float(m['margin'].min()))
    assert (m['margin'] > MA.MARGIN).all(), float(m['margin'].min())
    assert int(m['taken'].sum()) == taken and int((m['taken'] == 0).sum()) == kept
    assert not m['shifts'].any()


@pytest.mark.parametrize('name', ['specs', 'ramp'])
def test_both_branches_of_the_fallback_occur_under_weights(name):
    m = MK.case(10, 'pink', name, (0,))
    kept = m['taken'] == 0
    assert kept.any() and (~kept).any()
    assert np.array_equal(m['units'][kept], m['ref'][kept]) and (m['units'][~kept] != m['ref'][~kept]).any(axis=1).all()
    assert (m['D'][~kept, 1] < m['D'][~kept, 0]).all() and not (m['D'][kept, 1] < m['D'][kept, 0]).any()
    assert len(np.unique(m['P'])) > 1                                         # the weights are not trivial


@pytest.mark.parametrize('material,kind,offsets', [('white', 58, SF.OFFSETS), ('pink', 10, (0,))])
def test_flat_tables_are_the_scale_factor_choice_model(material, kind, offsets):
    m, parent = MK.case(kind, material, 'flat', offsets), SF.case(kind, material, offsets)
    assert (m['P'] == 1.0).all() and m['at_floor'].all()
    for key in ('units', 'taken', 'nbfu', 'wl', 'shifts', 'sfi', 'margin'):
        assert np.array_equal(m[key], parent[key]), key
    for key in ('D', 'E'):
        assert MK.bitwise(m[key], parent[key]), key
    zeros = np.zeros((52, 52))
    z = MK.model_of(MK.unit_tables(kind, material, offsets), np.ones(52), zeros)   # an all-zero matrix is NULL
    assert np.array_equal(z['units'], m['units']) and MK.bitwise(z['D'], m['D']) and MK.bitwise(z['P'], m['P'])


@pytest.mark.parametrize('material,kind,tables,offsets', [('pink', 10, 'packaged', SF.OFFSETS), ('white', 58, 'packaged', SF.OFFSETS),
                                                          ('pink', 10, 'specs', (0,)), ('pink', 10, 'self', (0,))])
def test_scaling_both_tables_by_four(material, kind, tables, offsets):
    m, q = MK.case(kind, material, tables, offsets), MK.case(kind, material, tables + '*4', offsets)
    for key in ('units', 'taken', 'shifts', 'nbfu', 'wl'):
        assert np.array_equal(m[key], q[key]), key
    for key in ('D', 'E', 'P'):
        assert MK.bitwise(q[key], 0.25 * m[key]), key


@pytest.mark.parametrize('material,kind,tables,offsets', [(mt, k, 'packaged', SF.OFFSETS) for mt, k in CASES] +
                         [('pink', 10, n, (0,)) for n in EXPLICIT])
def test_the_models_units_are_ordinary_sound_units(material, kind, tables, offsets):
    m = MK.case(kind, material, tables, offsets)
    assert MK.check_valid(m['units'], m['coefs'], m['taken'], m['D'], m['P'], offsets) is None
    assert MK.check_outputs(m, m['units'], m['taken'], m['shifts'], m['D'], m['E'], m['P']) is None
    final = np.where(m['taken'] != 0, m['D'][:, 1], m['D'][:, 0])
    assert (final <= m['D'][:, 0]).all()                                      # weighted T_final <= T_ref on every unit
    assert not m['shifts'][m['taken'] == 0].any()


@pytest.mark.parametrize('material,kind,tables,offsets', [(mt, k, 'packaged', SF.OFFSETS) for mt, k in CASES] +
                         [('pink', 10, n, (0,)) for n in EXPLICIT])
def test_the_weighted_error_lies_below_the_unweighted_models(material, kind, tables, offsets):
    """the weighted error of this model's units against the weighted error of the scale-factor-choice model's units (flat tables:
    the same model, shown above), both judged under this model's P.  Measured here: 3.76 (pink 0), 4.27 (pink 10), 3.98 (pink,
    detection) and 3.85 dB (white 58) under the packaged tables; 0.38 (SPECS_PER_BFU), 10.81 (the ramp) and 2.43 dB
    (self-masking) under the explicit ones."""
    t = MK.unit_tables(kind, material, offsets)
    m, flat = MK.case(kind, material, tables, offsets), MK.case(kind, material, 'flat', offsets)
    gain = float(MK.gain_over_db(t, m, flat))
    final = np.where(m['taken'] != 0, m['D'][:, 1], m['D'][:, 0])
    assert np.allclose(MK.error_under(t, m['P'], m), final, rtol=1e-12, atol=0)   # error_under is the model's own total
    print(material, kind, tables, 'gain %.2f dB over the unweighted model\'s units, %.2f dB over T_ref, %d of %d units at another BFU amount, '
          '%.1f %% of the thresholds at the floor' % (gain, float(MK.gain_db(m)), int((m['nbfu'] != flat['nbfu']).sum()), len(m['nbfu']),
                                                     100.0 * float(m['at_floor'].mean())))
    assert gain > 0.0, gain


def test_the_packaged_tables_are_the_tools():
    """the JSON is the authority (libm may differ in the last bits): the tool's formulas, run here, within a relative 1e-12"""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    try:
        import make_masking_tables as MT
    finally:
        sys.path.pop(0)
    import carta1_amd as c1
    floor, spread = MT.tables()
    assert np.allclose(np.array(floor), c1.MASKING_DEFAULT[0], rtol=1e-12, atol=0)
    assert np.allclose(np.array(spread), c1.MASKING_DEFAULT[1], rtol=1e-12, atol=0)
    assert MT.worst_relative_difference() <= 1e-12
    f2, s2 = MT.load()
    assert MK.bitwise(np.array(f2), c1.MASKING_DEFAULT[0]) and MK.bitwise(np.array(s2), c1.MASKING_DEFAULT[1])
    assert c1.check_masking(True)[0].shape == (52,) and c1.check_masking(True)[1].shape == (52, 52)
    assert (c1.MASKING_DEFAULT[0] >= 1e-60).all() and (c1.MASKING_DEFAULT[1] >= 0).all()
    import json
    assert json.load(open(os.path.join(ROOT, 'carta1_amd', 'masking_default.json')))['parameters']['G'] == MT.G


def test_silence_is_left_to_the_reference():
    import oracle_lib as O
    silence = [np.zeros(8 * 512, dtype=np.float32)] * 2
    ref = O.encode_stream(silence)[0]
    floor, spread = MK.packaged()
    m = MK.model_of(MK.tables_of(silence, ref, SF.OFFSETS), floor, spread)
    assert not m['taken'].any() and not m['D'].view(np.uint64).any() and not m['E'].view(np.uint64).any()    # +0.0 exactly
    assert np.array_equal(m['units'], ref) and not m['shifts'].any()
    assert m['at_floor'].all() and MK.bitwise(m['P'], np.broadcast_to(1.0 / floor, m['P'].shape))


BAD_FLOORS = [0.0, -1.0, np.nan, np.inf, 1e-61, 1e61]
BAD_SPREADS = [-1e-3, np.nan, 1e61]


def test_batch_argument_checks_need_neither_context_nor_device():
    """c1_encode_measured_masked_batch validates what its arguments alone decide, the tables among them, before it looks at its
    context: C1_ERR_ARG naming the table and the index, with or without a device, and nothing written."""
    from carta1_amd import build, capi, codec
    build.build_library()
    lib = capi.load()
    assert capi.SIGNATURES['c1_encode_measured_masked_batch'] == capi.SIGNATURES['c1_encode_measured_masked_device']
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
    weights = np.full((frames * nch, 52), -1.0)
    outs = lambda: (units.ctypes.data, taken.ctypes.data, shifts.ctypes.data, dist.ctypes.data, energy.ctypes.data, weights.ctypes.data)
    good_floor, good_spread = (np.ascontiguousarray(a) for a in MK.packaged())

    def call(floor=good_floor, spread=good_spread, offsets=SF.OFFSETS, o=None, fn=lib.c1_encode_measured_masked_batch, nch_=nch,
             frames_=frames):
        off = np.ascontiguousarray(list(offsets) + [0] * 9, dtype=np.int8)
        f = None if floor is None else np.ascontiguousarray(floor, dtype=np.float64)
        s = None if spread is None else np.ascontiguousarray(spread, dtype=np.float64)
        return fn(None, ptrs, nch_, frames_, 0, C.byref(opts), None, off.ctypes.data, len(offsets), None if f is None else f.ctypes.data,
                  None if s is None else s.ctypes.data, *(o or outs()))

    for at in (0, 17, 51):
        for v in BAD_FLOORS:
            f = good_floor.copy()
            f[at] = v
            assert call(floor=f) == C1_ERR_ARG, (at, v)
            assert 'c1_encode_measured_masked_batch: mask_floor[%d]' % at in err() and 'outside [1e-60, 1e60]' in err(), err()
            assert call(floor=f, spread=None) == C1_ERR_ARG and 'mask_floor[%d]' % at in err(), err()
    for at in (0, 53, 52 * 52 - 1):
        for v in BAD_SPREADS:
            s = good_spread.copy()
            s.reshape(-1)[at] = v
            assert call(spread=s) == C1_ERR_ARG, (at, v)
            assert 'c1_encode_measured_masked_batch: mask_spread[%d]' % at in err() and 'outside [0, 1e60]' in err(), err()
    assert call(floor=None) == C1_ERR_ARG and 'mask_floor is NULL' in err(), err()
    assert call(offsets=(0, 9)) == C1_ERR_ARG and 'sf_offsets[1] = 9 is outside -8..8' in err(), err()
    assert call(offsets=(-1, 0)) == C1_ERR_ARG and 'sf_offsets[0] = -1, not 0' in err(), err()
    assert call(nch_=3) == C1_ERR_ARG and 'channels must be 1 or 2' in err(), err()
    assert call(frames_=(1 << 22) + 1) == C1_ERR_ARG and 'at most' in err(), err()
    assert call(o=(None,) * 6) == C1_ERR_ARG
    assert 'c1_encode_measured_masked_batch: units, taken, shifts, distortion, energy and weights are all NULL' in err(), err()
    assert call(fn=lib.c1_encode_measured_masked_device) == C1_ERR_ARG and 'context is NULL' in err()
    # valid calls, the limits of the tables' ranges among them: only the context (and, here, the device) is missing
    count = C.c_int(0)
    have_device = lib.c1_device_count(C.byref(count)) == C1_OK and count.value > 0
    edge = np.full(52 * 52, 1e60)
    edge[::2] = 0.0
    for f, s in ((good_floor, good_spread), (good_floor, None), (np.full(52, 1e-60), edge), (np.full(52, 1e60), None)):
        for o in (None, (None, None, None, None, None, weights.ctypes.data), (units.ctypes.data, None, None, None, None, None)):
            rc = call(floor=f, spread=s, o=o)
            if have_device:
                assert rc == C1_ERR_ARG and 'context is NULL' in err(), err()
            else:
                assert rc == C1_ERR_NO_DEVICE and 'no HIP device' in err(), err()
    assert (units == 0xA5).all() and (taken == 0xA5).all() and (shifts == 0x5A).all() and (dist == -1.0).all() and (energy == -1.0).all()
    assert (weights == -1.0).all()


class _NoEncode:
    """the library without its encode entry points"""
    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, name):
        if name.startswith('c1_encode'):
            raise AssertionError('the wrapper reached ' + name)
        return getattr(self._lib, name)


def test_check_masking_and_the_wrapper_reject_before_any_library_call(monkeypatch):
    import carta1_amd as c1
    from carta1_amd import build, capi
    build.build_library()
    good_floor, good_spread = MK.packaged()
    floor, spread = c1.check_masking((list(good_floor), None))
    assert spread is None and MK.bitwise(floor, good_floor)
    floor, spread = c1.check_masking((good_floor, good_spread.reshape(-1)))
    assert spread.shape == (52, 52) and MK.bitwise(spread, good_spread)
    for at in (0, 51):
        for v in BAD_FLOORS:
            f = np.array(good_floor)
            f[at] = v
            with pytest.raises(ValueError, match=r'mask_floor\[%d\]' % at):
                c1.check_masking((f, good_spread))
    for at in (1, 52 * 52 - 1):
        for v in BAD_SPREADS:
            s = np.array(good_spread)
            s.reshape(-1)[at] = v
            with pytest.raises(ValueError, match=r'mask_spread\[%d\]' % at):
                c1.check_masking((good_floor, s))
    for bad, what in (((good_floor[:51], None), '52 values'), ((good_floor, good_spread[:51]), '52 x 52'), (False, 'pair'),
                      ((good_floor,), 'pair')):
        with pytest.raises(ValueError, match=what):
            c1.check_masking(bad)
    ctx = object.__new__(c1.Context)                                        # no device, no handle: the checks come first
    ctx._h = None
    guarded = _NoEncode(capi.load())
    monkeypatch.setattr(capi, 'load', lambda: guarded)
    chans = [np.zeros(4 * 512, dtype=np.float32)] * 2
    with pytest.raises(ValueError, match=r'mask_floor\[3\]'):
        ctx.encode_measured(chans, masking=(np.where(np.arange(52) == 3, 0.0, 1.0), None))
    with pytest.raises(ValueError, match='return_weights needs masking'):
        ctx.encode_measured(chans, return_weights=True)
    with pytest.raises(ValueError, match='return_shifts needs'):
        ctx.encode_measured(chans, masking=True, return_shifts=True)
    with pytest.raises(ValueError, match='outside -8..8'):
        ctx.encode_measured(chans, masking=True, scale_factor_offsets=(0, 9))
    with pytest.raises(AssertionError, match='c1_encode_measured_masked_batch'):     # masking alone: offsets (0,), the new entry point
        ctx.encode_measured(chans, masking=True)
    with pytest.raises(AssertionError, match='c1_encode_measured_batch'):            # no masking: today's entry point
        ctx.encode_measured(chans)
