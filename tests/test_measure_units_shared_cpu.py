"""No GPU: the coding error of given sound units under the all-long threshold (c1_measure_units_shared_*).  The symbols are
declared, exported and bound; both calls decide what their arguments alone decide without a context or device and write nothing;
the Python wrappers reject before any library call and threshold_from='own' reaches the calls that were there before; the CPU
model of tests/measure_units_shared_lib.py, which reads units back from their bytes, reproduces bit for bit what the model of the
masked block-mode search (tests/masked_modes_lib.py) reports for the units it packs, equals the own-mode meter's model for units
that are all long, and differs from it by more than 6 dB in some BFU's weight otherwise."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import best_modes_lib as BMO
import masked_alloc_lib as MK
import masked_modes_lib as X
import measure_units_lib as MU
import measure_units_shared_lib as MS

C1_OK, C1_ERR_ARG, C1_ERR_NO_DEVICE = 0, 1, 2   # include/carta1_hip.h
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('c1_measure_units_shared_device', 'c1_measure_units_shared_batch')
# material, offsets, candidates, frames (None: the whole material, the case tests/test_masked_modes_cpu.py shares)
CASES = [('white', (0,), [0, 58, 10, 48], 12), ('pink', X.OFFSETS, [0, 58, 10], 16), ('pink', (0,), X.CANDIDATES, None)]


def test_symbols_are_declared_exported_and_bound():
    from carta1_amd import build, capi
    import carta1_amd as c1
    build.build_library()
    header = open(os.path.join(ROOT, 'include', 'carta1_hip.h')).read()
    lib = capi.load()
    for name in NAMES:
        assert re.search(r'^int %s\(' % name, header, re.M), name
        assert name in capi.SIGNATURES and getattr(lib, name).argtypes == capi.SIGNATURES[name][1]
    assert capi.SIGNATURES[NAMES[0]] == capi.SIGNATURES[NAMES[1]] == capi.SIGNATURES['c1_measure_units_batch']
    assert '#define C1_ABI_VERSION 3' in header and lib.c1_abi_version() == 3
    import inspect
    for fn in (c1.Context.measure_units, c1.Context.measure_units_device):
        assert inspect.signature(fn).parameters['threshold_from'].default == 'own'


@pytest.mark.parametrize('name', NAMES)
def test_argument_checks_need_neither_context_nor_device(name):
    """every C1_ERR_ARG the arguments alone decide, in both calls, with a NULL context and the outputs untouched; valid arguments
    then miss only the context (and, in the host call without a device, the device)"""
    from carta1_amd import build, capi
    build.build_library()
    lib = capi.load()
    fn = getattr(lib, name)
    host = name.endswith('_batch')
    err = lambda: lib.c1_last_error().decode()
    frames, nch = 4, 2
    chans = [np.zeros(frames * 512, dtype=np.float32) for _ in range(nch)]
    ptrs = capi.ptr_array([c.ctypes.data for c in chans])     # 16-byte aligned: numpy's allocations of this size are
    assert all(c.ctypes.data % 16 == 0 for c in chans)
    good_units = MU.random_units(5, frames * nch)
    noise, signal, weights = (np.full((frames * nch, 52), -1.0) for _ in range(3))
    totals = np.full((frames * nch, 2), -1.0)
    outs = lambda: (noise.ctypes.data, signal.ctypes.data, totals.ctypes.data, weights.ctypes.data)
    good_floor, good_spread = (np.ascontiguousarray(a) for a in MK.packaged())

    def call(floor=good_floor, spread=good_spread, units=good_units, o=None, nch_=nch, frames_=frames, halo=0, pcm=ptrs):
        f = None if floor is None else np.ascontiguousarray(floor, dtype=np.float64)
        s = None if spread is None else np.ascontiguousarray(spread, dtype=np.float64)
        u = None if units is None else np.ascontiguousarray(units, dtype=np.uint8)
        return fn(None, pcm, nch_, frames_, halo, None if u is None else u.ctypes.data, None if f is None else f.ctypes.data,
                  None if s is None else s.ctypes.data, *(o or outs()))

    for v in (0.0, -1.0, np.nan, np.inf, 1e-61, 1e61):
        f = good_floor.copy()
        f[17] = v
        assert call(floor=f) == C1_ERR_ARG and name + ': mask_floor[17]' in err() and 'outside [1e-60, 1e60]' in err(), err()
    for v in (-1.0, np.nan, 1e61):
        s = good_spread.copy()
        s.reshape(-1)[53] = v
        assert call(spread=s) == C1_ERR_ARG and name + ': mask_spread[53]' in err() and 'outside [0, 1e60]' in err(), err()
    assert call(o=(None,) * 4) == C1_ERR_ARG and 'noise, signal, totals and weights are all NULL' in err(), err()
    assert call(floor=None) == C1_ERR_ARG and 'mask_spread needs mask_floor' in err(), err()
    for o in (None, (None, None, totals.ctypes.data, None)):                       # the floor is required whatever is asked for
        assert call(floor=None, spread=None, o=o) == C1_ERR_ARG and name + ': mask_floor is NULL' in err(), err()
    assert call(units=None) == C1_ERR_ARG and 'units is NULL' in err(), err()
    assert call(pcm=None) == C1_ERR_ARG and 'pcm is NULL' in err(), err()
    assert call(pcm=capi.ptr_array([chans[0].ctypes.data, 0])) == C1_ERR_ARG and 'pcm[1] is NULL' in err(), err()
    assert call(nch_=3) == C1_ERR_ARG and 'channels must be 1 or 2' in err(), err()
    assert call(frames_=-1) == C1_ERR_ARG and call(halo=3) == C1_ERR_ARG and call(halo=-1) == C1_ERR_ARG
    assert call(frames_=(1 << 30) + 1) == C1_ERR_ARG and 'at most' in err(), err()
    if host:
        assert call(frames_=(1 << 22) + 1) == C1_ERR_ARG and 'at most' in err(), err()
        # a unit outside the domain of c1_encode_modes_*: every field, named with its frame and channel
        for at, first, what in ((5, 0x40, 'frame 2, channel 1: low block mode of the unit is 1, not 0 or 2'),
                                (2, 0xC8, 'frame 1, channel 0: low block mode of the unit is -1, not 0 or 2'),
                                (7, 0x9C, 'frame 3, channel 1: mid block mode of the unit is 1, not 0 or 2'),
                                (0, 0xA4, 'frame 0, channel 0: high block mode of the unit is 2, not 0 or 3'),
                                (3, 0xA8, 'frame 1, channel 1: high block mode of the unit is 1, not 0 or 3')):
            u = good_units.copy()
            u[at, 0] = first
            assert call(units=u) == C1_ERR_ARG and err().endswith(what) and name in err(), err()
        u = good_units[::2].copy()
        u[3, 0] = 0x40
        assert call(units=u, nch_=1, pcm=capi.ptr_array([chans[0].ctypes.data])) == C1_ERR_ARG and name + ': frame 3: low' in err(), err()
    else:
        odd = np.zeros(frames * 212 * nch + 4, dtype=np.uint8)
        assert fn(None, ptrs, nch, frames, 0, odd.ctypes.data + 1, good_floor.ctypes.data, None, *outs()) == C1_ERR_ARG and '4-byte aligned' in err(), err()
        assert call(pcm=capi.ptr_array([chans[0].ctypes.data, chans[1].ctypes.data + 4])) == C1_ERR_ARG and '16-byte aligned' in err(), err()
    # valid calls: only the context (and, in the host call without a device, the device) is missing
    count = C.c_int(0)
    have_device = lib.c1_device_count(C.byref(count)) == C1_OK and count.value > 0
    for s, o in ((good_spread, None), (None, None), (None, (None, None, totals.ctypes.data, None)), (None, (None, None, None, weights.ctypes.data))):
        for fr in (frames, 0):
            rc = call(spread=s, o=o, frames_=fr)
            if have_device or not host:
                assert rc == C1_ERR_ARG and 'context is NULL' in err(), err()
            else:
                assert rc == C1_ERR_NO_DEVICE and 'no HIP device' in err(), err()
    assert (noise == -1.0).all() and (signal == -1.0).all() and (totals == -1.0).all() and (weights == -1.0).all()


class _Only:
    """the library with the measuring entry points replaced by a report of which was reached"""
    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, name):
        if name.startswith('c1_measure'):
            raise AssertionError('the wrapper reached ' + name + '.')
        return getattr(self._lib, name)


def test_the_wrappers_reject_before_any_library_call(monkeypatch):
    import carta1_amd as c1
    from carta1_amd import build, capi
    build.build_library()
    ctx = object.__new__(c1.Context)                                        # no device, no handle: the checks come first
    ctx._h = None
    guarded = _Only(capi.load())
    monkeypatch.setattr(capi, 'load', lambda: guarded)
    chans = [np.zeros(4 * 512, dtype=np.float32)] * 2
    units = MU.random_units(5, 8)
    for bad in ('short', 'Long', None, 0, True):
        with pytest.raises(ValueError, match='threshold_from must be'):
            ctx.measure_units(chans, units, masking=True, threshold_from=bad)
        with pytest.raises(ValueError, match='threshold_from must be'):
            ctx.measure_units_device([0x1000, 0x2000], 4, 0x3000, totals_ptr=0x4000, masking=True, threshold_from=bad)
    with pytest.raises(ValueError, match="threshold_from='long' needs masking"):
        ctx.measure_units(chans, units, threshold_from='long')
    with pytest.raises(ValueError, match="threshold_from='long' needs masking"):
        ctx.measure_units_device([0x1000, 0x2000], 4, 0x3000, totals_ptr=0x4000, threshold_from='long')
    # the other checks of measure_units come before the call whatever the threshold
    with pytest.raises(ValueError, match='8 sound units'):
        ctx.measure_units(chans, units[:7], masking=True, threshold_from='long')
    bad = units.copy()
    bad[5, 0] = 0x40
    with pytest.raises(ValueError, match='frame 2, channel 1: low block mode of the unit is 1, not 0 or 2'):
        ctx.measure_units(chans, bad, masking=True, threshold_from='long')
    with pytest.raises(ValueError, match=r'mask_floor\[3\]'):
        ctx.measure_units(chans, units, masking=(np.where(np.arange(52) == 3, 0.0, 1.0), None), threshold_from='long')
    # which symbol every form reaches
    for kw, batch, device in (({}, 'c1_measure_units_batch', 'c1_measure_units_device'),
                              ({'threshold_from': 'own'}, 'c1_measure_units_batch', 'c1_measure_units_device'),
                              ({'threshold_from': 'long'}, 'c1_measure_units_shared_batch', 'c1_measure_units_shared_device')):
        with pytest.raises(AssertionError, match=re.escape(batch + '.')):
            ctx.measure_units(chans, units, masking=True, **kw)
        with pytest.raises(AssertionError, match=re.escape(device + '.')):
            ctx.measure_units_device([0x1000, 0x2000], 4, 0x3000, totals_ptr=0x4000, masking=True, **kw)
    with pytest.raises(AssertionError, match=re.escape('c1_measure_units_batch.')):
        ctx.measure_units(chans, units, threshold_from='own')


def _material(material, frames):
    chans = BMO.material(material)
    return chans if frames is None else [c[:frames * 512] for c in chans]


@pytest.mark.parametrize('material,offsets,cand,frames', CASES, ids=['white-4', 'pink-sf-3', 'pink-8'])
def test_the_model_reads_back_what_the_masked_search_reports(material, offsets, cand, frames):
    """for the units the model of c1_encode_measured_modes_masked_* packs: the weights are its P, totals[:, 0] its D[u, choice,
    taken], totals[:, 1] its E[u, choice] and the bytes its modes, bit for bit; and some BFU's weight lies more than 6 dB from the
    weight the own-mode meter gives it (measured here: 9.6, 15.5 and 13.5 dB)"""
    m = X.case(material, 'packaged', offsets, cand, frames)
    chans = _material(material, frames)
    floor, spread = MK.packaged()
    s = MS.sums(chans, m['units'])
    got = MS.with_tables(s, floor, spread)
    U = m['units'].shape[0]
    ar = np.arange(U)
    assert MS.bitwise(got['weights'], m['P'])
    assert MS.bitwise(got['totals'][:, 0], m['D'][ar, m['choice'], m['taken']])
    assert MS.bitwise(got['totals'][:, 1], m['E'][ar, m['choice']])
    assert np.array_equal(got['bytes'], m['modes']) and len(set(m['modes'].tolist())) > 1
    # the same units rewritten to byte 0: every output is the own-mode meter's
    own = MU.with_tables(s, floor, spread)
    gap = MS.gap_db(got['weights'], own['weights'])
    print('largest gap between the shared and the own-mode weight: %.1f dB' % gap.max())
    assert gap.max() > 6.0
    assert not gap[got['bytes'] == 0].any()


def test_units_that_are_all_long_are_measured_as_before():
    chans = _material('white', 12)
    m = X.case('white', 'packaged', (0,), [0, 58, 10, 48], 12)
    units = MU.with_modes(m['units'], np.zeros(m['units'].shape[0], dtype=np.int64))
    for tables in ('packaged', 'packaged*4', 'flat', 'self'):
        floor, spread = MK.named(tables)
        s = MS.sums(chans, units)
        got, want = MS.with_tables(s, floor, spread), MU.with_tables(s, floor, spread)
        assert (got['bytes'] == 0).all() and all(MS.bitwise(got[k], want[k]) for k in ('noise', 'signal', 'totals', 'weights')), tables
        assert MS.bitwise(s['E0'], s['signal'])
    flat = MS.with_tables(s, np.ones(52), None)
    assert (flat['weights'] == 1.0).all() and MS.bitwise(flat['totals'], MU.with_tables(s)['totals'])
