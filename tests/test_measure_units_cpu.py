"""No GPU: the coding error of given sound units (c1_measure_units_*).  The symbols are declared, exported and bound; the batch
call validates what its arguments alone decide without a context or device and writes nothing; the CPU model of
tests/measure_units_lib.py, which reads units back from their bytes, reproduces bit for bit what the models of the measured
allocation (tests/measured_alloc_lib.py, scale_factor_choice_lib.py, masked_alloc_lib.py) report for the units they pack; the
Python wrapper rejects before any library call."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import best_modes_lib as BMO
import masked_alloc_lib as MK
import measure_units_lib as MU
import measured_alloc_lib as MA
import scale_factor_choice_lib as SF

C1_OK, C1_ERR_ARG, C1_ERR_NO_DEVICE = 0, 1, 2   # include/carta1_hip.h
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('c1_measure_units_device', 'c1_measure_units_batch')


def test_symbols_are_declared_exported_and_bound():
    from carta1_amd import build, capi
    import carta1_amd as c1
    build.build_library()
    header = open(os.path.join(ROOT, 'include', 'carta1_hip.h')).read()
    lib = capi.load()
    for name in NAMES:
        assert re.search(r'^int %s\(' % name, header, re.M), name
        assert name in capi.SIGNATURES and getattr(lib, name).argtypes == capi.SIGNATURES[name][1]
    assert capi.SIGNATURES[NAMES[0]] == capi.SIGNATURES[NAMES[1]]
    assert '#define C1_ABI_VERSION 3' in header and lib.c1_abi_version() == 3
    assert callable(c1.Context.measure_units) and callable(c1.Context.measure_units_device) and callable(c1.check_measured_units)


def test_batch_argument_checks_need_neither_context_nor_device():
    """every C1_ERR_ARG the arguments alone decide, with the outputs untouched; valid arguments then miss only the context (and,
    without one, the device)"""
    from carta1_amd import build, capi
    build.build_library()
    lib = capi.load()
    err = lambda: lib.c1_last_error().decode()
    frames, nch = 4, 2
    chans = [np.zeros(frames * 512, dtype=np.float32) for _ in range(nch)]
    ptrs = capi.ptr_array([c.ctypes.data for c in chans])
    good_units = MU.random_units(5, frames * nch)
    noise, signal, weights = (np.full((frames * nch, 52), -1.0) for _ in range(3))
    totals = np.full((frames * nch, 2), -1.0)
    outs = lambda: (noise.ctypes.data, signal.ctypes.data, totals.ctypes.data, weights.ctypes.data)
    good_floor, good_spread = (np.ascontiguousarray(a) for a in MK.packaged())

    def call(floor=good_floor, spread=good_spread, units=good_units, o=None, fn=lib.c1_measure_units_batch, nch_=nch, frames_=frames,
             halo=0, pcm=ptrs):
        f = None if floor is None else np.ascontiguousarray(floor, dtype=np.float64)
        s = None if spread is None else np.ascontiguousarray(spread, dtype=np.float64)
        u = None if units is None else np.ascontiguousarray(units, dtype=np.uint8)
        return fn(None, pcm, nch_, frames_, halo, None if u is None else u.ctypes.data, None if f is None else f.ctypes.data,
                  None if s is None else s.ctypes.data, *(o or outs()))

    for v in (0.0, -1.0, np.nan, np.inf, 1e-61, 1e61):
        f = good_floor.copy()
        f[17] = v
        assert call(floor=f) == C1_ERR_ARG and 'c1_measure_units_batch: mask_floor[17]' in err() and 'outside [1e-60, 1e60]' in err(), err()
    for v in (-1.0, np.nan, 1e61):
        s = good_spread.copy()
        s.reshape(-1)[53] = v
        assert call(spread=s) == C1_ERR_ARG and 'c1_measure_units_batch: mask_spread[53]' in err() and 'outside [0, 1e60]' in err(), err()
    assert call(o=(None,) * 4) == C1_ERR_ARG and 'noise, signal, totals and weights are all NULL' in err(), err()
    assert call(floor=None) == C1_ERR_ARG and 'mask_spread needs mask_floor' in err(), err()
    assert call(floor=None, spread=None) == C1_ERR_ARG and 'weights needs mask_floor' in err(), err()
    assert call(units=None) == C1_ERR_ARG and 'units is NULL' in err(), err()
    assert call(pcm=None) == C1_ERR_ARG and 'pcm is NULL' in err(), err()
    assert call(pcm=capi.ptr_array([chans[0].ctypes.data, 0])) == C1_ERR_ARG and 'pcm[1] is NULL' in err(), err()
    assert call(nch_=3) == C1_ERR_ARG and 'channels must be 1 or 2' in err(), err()
    assert call(frames_=-1) == C1_ERR_ARG and call(halo=3) == C1_ERR_ARG
    assert call(frames_=(1 << 22) + 1) == C1_ERR_ARG and 'at most' in err(), err()
    # a unit outside the domain of c1_encode_modes_*: every field, named with its frame and channel
    for at, first, what in ((5, 0x40, 'frame 2, channel 1: low block mode of the unit is 1, not 0 or 2'),
                            (2, 0xC8, 'frame 1, channel 0: low block mode of the unit is -1, not 0 or 2'),
                            (7, 0x9C, 'frame 3, channel 1: mid block mode of the unit is 1, not 0 or 2'),
                            (0, 0xA4, 'frame 0, channel 0: high block mode of the unit is 2, not 0 or 3'),
                            (3, 0xA8, 'frame 1, channel 1: high block mode of the unit is 1, not 0 or 3')):
        u = good_units.copy()
        u[at, 0] = first
        assert call(units=u) == C1_ERR_ARG and err().endswith(what), err()
    u = good_units[::2].copy()
    u[3, 0] = 0x40
    assert call(units=u, nch_=1, pcm=capi.ptr_array([chans[0].ctypes.data])) == C1_ERR_ARG and 'c1_measure_units_batch: frame 3: low' in err(), err()
    assert call(fn=lib.c1_measure_units_device) == C1_ERR_ARG and 'context is NULL' in err()
    # valid calls: only the context (and, here, the device) is missing
    count = C.c_int(0)
    have_device = lib.c1_device_count(C.byref(count)) == C1_OK and count.value > 0
    three = (noise.ctypes.data, signal.ctypes.data, totals.ctypes.data, None)
    for f, s, o in ((good_floor, good_spread, None), (good_floor, None, None), (None, None, three), (None, None, (None, None, totals.ctypes.data, None)),
                    (good_floor, None, (None, None, None, weights.ctypes.data))):
        for fr in (frames, 0):
            rc = call(floor=f, spread=s, o=o, frames_=fr)
            if have_device:
                assert rc == C1_ERR_ARG and 'context is NULL' in err(), err()
            else:
                assert rc == C1_ERR_NO_DEVICE and 'no HIP device' in err(), err()
    assert (noise == -1.0).all() and (signal == -1.0).all() and (totals == -1.0).all() and (weights == -1.0).all()


def _chans(material):
    return BMO.material(material)


@pytest.mark.parametrize('material,kind', [('white', 0), ('white', 58), ('pink', 10), ('pink', 'detect')])
def test_the_model_reads_back_what_the_measured_model_reports(material, kind):
    """measured here: 0 mismatches in every column of every case"""
    m = MA.case(kind, material)
    chans = _chans(material)
    ref = MU.model(chans, m['ref'])
    assert MU.bitwise(ref['totals'][:, 0], m['D'][:, 0])
    assert MU.bitwise(ref['totals'][:, 1], m['E'])
    assert (ref['weights'] == 1.0).all()
    taken = m['taken'] != 0
    assert taken.any()
    got = MU.model(chans, m['units'])
    assert MU.bitwise(got['totals'][taken, 0], m['D'][taken, 1])
    assert MU.bitwise(got['totals'][~taken, 0], m['D'][~taken, 0])
    assert MU.bitwise(got['totals'][:, 1], m['E']) and MU.bitwise(got['signal'], ref['signal'])


def test_the_model_reads_back_the_scale_factor_choice_model():
    m = SF.case(10, 'pink')
    chans = _chans('pink')
    got = MU.model(chans, m['units'])
    final = np.where(m['taken'] != 0, m['D'][:, 1], m['D'][:, 0])
    assert MU.bitwise(got['totals'][:, 0], final) and MU.bitwise(got['totals'][:, 1], m['E'])
    assert MU.bitwise(MU.model(chans, m['ref'])['totals'][:, 0], m['D'][:, 0])


def test_the_model_reads_back_the_masked_model_under_the_packaged_tables():
    m = MK.case(10, 'pink', 'packaged', SF.OFFSETS)
    chans = _chans('pink')
    floor, spread = MK.packaged()
    got = MU.model(chans, m['units'], floor, spread)
    final = np.where(m['taken'] != 0, m['D'][:, 1], m['D'][:, 0])
    assert MU.bitwise(got['weights'], m['P'])
    assert MU.bitwise(got['totals'][:, 0], final) and MU.bitwise(got['totals'][:, 1], m['E'])
    assert MU.bitwise(MU.model(chans, m['ref'], floor, spread)['totals'][:, 0], m['D'][:, 0])
    # flat tables: the weights are exactly 1 and the totals are the plain ones
    flat = MU.model(chans, m['units'], np.ones(52), None)
    plain = MU.model(chans, m['units'])
    assert (flat['weights'] == 1.0).all() and MU.bitwise(flat['totals'], plain['totals'])


def test_foreign_bytes_and_the_domain_of_the_model():
    """random bytes are measured like any unit; a mode outside the domain is an error of the host model and is brought into the
    domain by the device model, where negative modes are two's complement"""
    chans = [c[:8 * 512] for c in _chans('white')]
    units = MU.random_units(7, 16)
    m = MU.model(chans, units)
    assert np.isfinite(m['noise']).all() and (m['noise'] >= 0).all() and (m['signal'] > 0).any()
    raw = MU.random_units(8, 16, domain=False)
    with pytest.raises(AssertionError):
        MU.model(chans, raw)
    d = MU.model(chans, raw, device=True)
    assert set(d['bytes'].tolist()) <= set(MU.DOMAIN_BYTES) and len(set(d['bytes'].tolist())) > 2
    assert MU.mode_in_domain(-1) == 0x3a and MU.mode_in_domain(-4) == 0x38 and MU.mode_in_domain(1 | 1 << 2 | 2 << 4) == 0
    again = MU.model(chans, MU.with_modes(raw, d['bytes']))
    assert all(MU.bitwise(again[k], d[k]) for k in ('noise', 'signal', 'totals'))


class _NoMeasure:
    """the library without the entry points of this feature"""
    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, name):
        if name.startswith('c1_measure'):
            raise AssertionError('the wrapper reached ' + name)
        return getattr(self._lib, name)


def test_the_wrapper_rejects_before_any_library_call(monkeypatch):
    import carta1_amd as c1
    from carta1_amd import build, capi
    build.build_library()
    ctx = object.__new__(c1.Context)                                        # no device, no handle: the checks come first
    ctx._h = None
    guarded = _NoMeasure(capi.load())
    monkeypatch.setattr(capi, 'load', lambda: guarded)
    chans = [np.zeros(4 * 512, dtype=np.float32)] * 2
    units = MU.random_units(5, 8)
    with pytest.raises(ValueError, match='multiple of 512'):
        ctx.measure_units([np.zeros(100, dtype=np.float32)], units)
    with pytest.raises(ValueError, match='8 sound units'):
        ctx.measure_units(chans, units[:7])
    with pytest.raises(ValueError, match='uint8'):
        ctx.measure_units(chans, units.astype(np.int32))
    bad = units.copy()
    bad[5, 0] = 0x40
    with pytest.raises(ValueError, match='frame 2, channel 1: low block mode of the unit is 1, not 0 or 2'):
        ctx.measure_units(chans, bad)
    bad[5, 0] = 0xA4
    with pytest.raises(ValueError, match='frame 2, channel 1: high block mode of the unit is 2, not 0 or 3'):
        ctx.measure_units(chans, bad)
    mono = units[:4].copy()
    mono[3, 0] = 0x9C
    with pytest.raises(ValueError, match='^frame 3: mid block mode of the unit is 1, not 0 or 2'):
        ctx.measure_units(chans[:1], mono)
    with pytest.raises(ValueError, match='return_weights needs masking'):
        ctx.measure_units(chans, units, return_weights=True)
    with pytest.raises(ValueError, match=r'mask_floor\[3\]'):
        ctx.measure_units(chans, units, masking=(np.where(np.arange(52) == 3, 0.0, 1.0), None))
    with pytest.raises(AssertionError, match='c1_measure_units_batch'):
        ctx.measure_units(chans, units)
    with pytest.raises(AssertionError, match='c1_measure_units_device'):
        ctx.measure_units_device([0x1000, 0x2000], 4, 0x3000, totals_ptr=0x4000)
