"""CPU-only: the word lengths allocated by the measured coding error (c1_encode_measured_*).  What makes the GPU tests mean
something, on the model of tests/measured_alloc_lib.py (built from the oracle alone): every decision of the model on the shared
material is decided by a margin far above the tolerance of the error sums, its units are ordinary sound units, both branches of
the fallback occur, and the gain is the one the feature was proposed for.  Then silence, and the checks the batch entry point
makes before it needs a context or a device."""
import ctypes as C

import numpy as np
import pytest

import measured_alloc_lib as MA

C1_OK, C1_ERR_ARG, C1_ERR_NO_DEVICE = 0, 1, 2   # include/carta1_hip.h
CASES = [('pink', 0), ('pink', 10), ('pink', 58), ('white', 0), ('white', 58)]
# the aggregate gain of T_final against T_ref, in dB: 0.3 dB under the values measured with this model (2.64, 4.93, 3.13, 1.70, 1.95)
FLOOR_DB = {('pink', 0): 2.3, ('pink', 10): 4.5, ('pink', 58): 2.8, ('white', 0): 1.4, ('white', 58): 1.6}


@pytest.mark.parametrize('material,byte', CASES)
def test_every_decision_of_the_model_has_a_margin(material, byte):
    """Measured here: the least relative margin of any decision of any unit (a greedy step's top gain against the runner-up, the
    least T against the next, T(n*) against T_ref) is 3.1e-7, 2.2e-6 and 2.2e-6 on pink under bytes 0, 10 and 58 and 1.7e-7 and
    6.2e-7 on white under 0 and 58: four orders of magnitude above the 1e-12 the error sums are known to, so the GPU must
    reproduce every decision."""
    m = MA.case(byte, material)
    print(material, byte, 'least margin %.3g' % float(m['margin'].min()))
    assert np.isfinite(m['D']).all() and (m['D'] > 0).all()
    assert (m['margin'] > MA.MARGIN).all(), float(m['margin'].min())


@pytest.mark.parametrize('material,byte', CASES)
def test_the_models_units_are_ordinary_sound_units(material, byte):
    m = MA.case(byte, material)
    assert MA.check_valid(m['units'], m['coefs'], m['taken'], m['D']) is None
    assert MA.check_outputs(m, m['units'], m['taken'], m['D'], m['E']) is None
    final = np.where(m['taken'] != 0, m['D'][:, 1], m['D'][:, 0])
    assert (final <= m['D'][:, 0]).all()


def test_both_branches_occur():
    """Measured here on pink under byte 10: 235 units taken, 25 kept with the reference's record."""
    m = MA.case(10, 'pink')
    taken = int(m['taken'].sum())
    print('taken', taken, 'kept', len(m['taken']) - taken)
    assert taken >= 200 and len(m['taken']) - taken >= 10
    kept = m['taken'] == 0
    assert np.array_equal(m['units'][kept], m['ref'][kept]) and (m['units'][~kept] != m['ref'][~kept]).any(axis=1).all()


@pytest.mark.parametrize('material,byte', CASES)
def test_the_gain_is_the_one_proposed(material, byte):
    m = MA.case(byte, material)
    gain = float(MA.gain_db(m))
    print(material, byte, 'gain %.2f dB, taken %d of %d' % (gain, int(m['taken'].sum()), len(m['taken'])))
    assert gain >= FLOOR_DB[(material, byte)], gain
    if material == 'white' or byte == 0:
        assert m['taken'].all()


def test_energy_is_the_weighted_sum_of_squares():
    """energy[u] equals best_modes_lib's E under the same constant byte (a sum of the same terms in another order)"""
    import best_modes_lib as BMO
    for material, byte in CASES:
        want = BMO.case(material)['E'][:, BMO.CANDIDATES.index(byte)]
        got = MA.case(byte, material)['E']
        assert (np.abs(got - want) <= MA.REL * want).all(), (material, byte)


def test_silence_is_left_to_the_reference():
    import oracle_lib as O
    silence = [np.zeros(8 * 512, dtype=np.float32)] * 2
    ref = O.encode_stream(silence)[0]
    m = MA.model(silence, ref)
    assert not m['taken'].any() and not m['D'].view(np.uint64).any() and not m['E'].view(np.uint64).any()    # +0.0 exactly
    assert np.array_equal(m['units'], ref)


def test_batch_argument_checks_need_neither_context_nor_device():
    """c1_encode_measured_batch validates what its arguments alone decide before it looks at its context: C1_ERR_ARG with or
    without a device, and nothing written.  A valid call without a context is C1_ERR_NO_DEVICE where there is no device (and
    "context is NULL" where there is one)."""
    from carta1_amd import build, capi, codec
    build.build_library()
    lib = capi.load()
    assert capi.SIGNATURES['c1_encode_measured_batch'] == capi.SIGNATURES['c1_encode_measured_device']
    err = lambda: lib.c1_last_error().decode()
    opts = codec.EncoderOptions().to_c()
    frames, nch = 4, 2
    chans = [np.zeros(frames * 512, dtype=np.float32) for _ in range(nch)]
    ptrs = capi.ptr_array([c.ctypes.data for c in chans])
    units = np.full((frames * nch, 212), 0xA5, dtype=np.uint8)
    taken = np.full(frames * nch, 0xA5, dtype=np.uint8)
    dist = np.full((frames * nch, 2), -1.0)
    energy = np.full(frames * nch, -1.0)
    outs = lambda: (units.ctypes.data, taken.ctypes.data, dist.ctypes.data, energy.ctypes.data)
    good = np.zeros(frames * nch, dtype=np.uint8)

    def call(modes=None, o=None, fn=lib.c1_encode_measured_batch, nch_=nch, frames_=frames, halo=0, options=opts, pcm=ptrs):
        m = None if modes is None else np.ascontiguousarray(modes, dtype=np.uint8)
        return fn(None, pcm, nch_, frames_, halo, C.byref(options) if options is not None else None, None if m is None else m.ctypes.data,
                  *(o or outs()))

    assert call(nch_=3) == C1_ERR_ARG and 'channels must be 1 or 2' in err(), err()
    assert call(frames_=-1) == C1_ERR_ARG and call(halo=3) == C1_ERR_ARG
    assert call(frames_=(1 << 22) + 1) == C1_ERR_ARG and 'at most' in err(), err()
    assert call(options=None) == C1_ERR_ARG and 'c1_encode_measured_batch' in err() and 'options are NULL' in err(), err()
    assert call(o=(None,) * 4) == C1_ERR_ARG
    assert 'c1_encode_measured_batch: units, taken, distortion and energy are all NULL' in err(), err()
    assert call(pcm=None) == C1_ERR_ARG and 'pcm is NULL' in err(), err()
    bad = good.copy()
    bad[5] = 1
    assert call(bad) == C1_ERR_ARG
    assert 'c1_encode_measured_batch' in err() and 'frame 2, channel 1' in err() and 'low field of mode byte 0x01 is 1, not 0 or 2' in err(), err()
    bad[5] = 64
    assert call(bad) == C1_ERR_ARG and 'bits 6-7' in err(), err()
    bad_opts = codec.EncoderOptions().to_c()
    bad_opts.biased_scale_factors[3] = float('nan')
    assert call(options=bad_opts) == C1_ERR_ARG and 'c1_encode_measured_batch' in err(), err()
    assert call(good, fn=lib.c1_encode_measured_device) == C1_ERR_ARG
    assert 'context is NULL' in err()
    # a valid call: only the context (and, here, the device) is missing
    count = C.c_int(0)
    have_device = lib.c1_device_count(C.byref(count)) == C1_OK and count.value > 0
    for modes in (None, good, np.full(frames * nch, 0x3a, dtype=np.uint8)):
        for o in (None, (None, taken.ctypes.data, None, None), (units.ctypes.data, None, None, None), (None, None, None, energy.ctypes.data)):
            rc = call(modes, o=o)
            if have_device:
                assert rc == C1_ERR_ARG and 'context is NULL' in err(), err()
            else:
                assert rc == C1_ERR_NO_DEVICE and 'no HIP device' in err(), err()
    assert (units == 0xA5).all() and (taken == 0xA5).all() and (dist == -1.0).all() and (energy == -1.0).all()


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
    with pytest.raises(ValueError, match='low field'):
        ctx.encode_measured(chans, modes=np.ones((4, 2), dtype=np.uint8))
    with pytest.raises(ValueError):
        ctx.encode_measured(chans, modes=np.zeros(3, dtype=np.uint8))
    with pytest.raises(ValueError, match='multiple of 512'):
        ctx.encode_measured([np.zeros(100, dtype=np.float32)])
