"""No GPU: the decoded PCM error of given sound units (c1_measure_pcm_*).  The symbols are declared, exported and bound; both calls
validate what their arguments alone decide without a context or device and write nothing; the Python wrapper rejects before any
library call; and the CPU model of tests/measure_pcm_lib.py is pinned in two ways that do not involve the kernel: its alignment
(the codec delay of 266 samples is unambiguous) and its agreement with the coefficient-domain meter's model."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import measure_pcm_lib as MP
import measure_units_lib as MU
import oracle_lib as O

C1_OK, C1_ERR_ARG, C1_ERR_NO_DEVICE = 0, 1, 2   # include/carta1_hip.h
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('c1_measure_pcm_device', 'c1_measure_pcm_batch')


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
    assert 'input samples 512 f + 32 s - 266' in header
    assert callable(c1.Context.measure_pcm) and callable(c1.Context.measure_pcm_device) and callable(c1.check_pcm_units)
    assert c1.PCM_DELAY == MP.DELAY and c1.PCM_SEGMENTS == MP.SEGMENTS


def test_argument_checks_need_neither_context_nor_device():
    """every C1_ERR_ARG the arguments alone decide, in both calls, with the outputs untouched; valid arguments then miss only the
    context (and, without one, the batch call the device)"""
    from carta1_amd import build, capi
    build.build_library()
    lib = capi.load()
    err = lambda: lib.c1_last_error().decode()
    frames, nch = 4, 2
    chans = [np.zeros(frames * 512, dtype=np.float32) for _ in range(nch)]
    ptrs = capi.ptr_array([c.ctypes.data for c in chans])
    units = MU.random_units(5, frames * nch)
    noise, signal = (np.full((frames * nch, 16), -1.0) for _ in range(2))
    totals = np.full((frames * nch, 2), -1.0)
    outs = (noise.ctypes.data, signal.ctypes.data, totals.ctypes.data)

    for fn in (lib.c1_measure_pcm_batch, lib.c1_measure_pcm_device):
        def call(pcm=ptrs, nch_=nch, frames_=frames, halo=0, u=units.ctypes.data, hu=0, o=outs):
            return fn(None, pcm, nch_, frames_, halo, u, hu, *o)

        assert call(o=(None,) * 3) == C1_ERR_ARG and 'noise, signal and totals are all NULL' in err(), err()
        assert call(u=None) == C1_ERR_ARG and 'units is NULL' in err(), err()
        assert call(pcm=None) == C1_ERR_ARG and 'pcm is NULL' in err(), err()
        assert call(pcm=capi.ptr_array([chans[0].ctypes.data, 0])) == C1_ERR_ARG and 'pcm[1] is NULL' in err(), err()
        for bad in (0, 3, -1):
            assert call(nch_=bad) == C1_ERR_ARG and 'channels must be 1 or 2' in err(), err()
        for bad in (-1, (1 << 22) + 1):
            assert call(frames_=bad) == C1_ERR_ARG and 'frames must be 0 .. 2^22' in err(), err()
        for bad in (-1, 3):
            assert call(halo=bad) == C1_ERR_ARG and 'halo_frames must be 0 .. 2' in err(), err()
        for bad in (-1, 2):
            assert call(hu=bad) == C1_ERR_ARG and 'halo_units must be 0 or 1' in err(), err()
        # valid calls: only the context (and, in the batch call here, the device) is missing
        count = C.c_int(0)
        have_device = lib.c1_device_count(C.byref(count)) == C1_OK and count.value > 0
        for o in (outs, (outs[0], None, None), (None, outs[1], None), (None, None, outs[2]), (outs[0], None, outs[2])):
            for fr, halo, hu in ((frames, 0, 0), (0, 0, 0), (frames - 2, 2, 1), (1 << 22, 0, 0)):
                rc = call(o=o, frames_=fr, halo=halo, hu=hu)
                if have_device or fn is lib.c1_measure_pcm_device:
                    assert rc == C1_ERR_ARG and 'context is NULL' in err(), err()
                else:
                    assert rc == C1_ERR_NO_DEVICE and 'no HIP device' in err(), err()
        # frames == 0 needs neither units nor pcm
        rc = call(frames_=0, u=None, pcm=None)
        assert rc in (C1_ERR_ARG, C1_ERR_NO_DEVICE) and ('context is NULL' in err() or 'no HIP device' in err()), err()
    assert (noise == -1.0).all() and (signal == -1.0).all() and (totals == -1.0).all()


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
        ctx.measure_pcm([np.zeros(100, dtype=np.float32)], units)
    with pytest.raises(ValueError, match='equal length'):
        ctx.measure_pcm([chans[0], chans[0][:512]], units)
    with pytest.raises(ValueError, match='float32'):
        ctx.measure_pcm([c.astype(np.float64) for c in chans], units)
    with pytest.raises(ValueError, match='float32'):
        ctx.measure_pcm([c.reshape(4, 512) for c in chans], units)
    with pytest.raises(ValueError, match='1 or 2'):
        ctx.measure_pcm(chans + chans[:1], units)
    with pytest.raises(ValueError, match='8 sound units'):
        ctx.measure_pcm(chans, units[:7])
    with pytest.raises(ValueError, match='10 sound units'):
        ctx.measure_pcm(chans, units, halo_units=1)
    with pytest.raises(ValueError, match='6 sound units'):
        ctx.measure_pcm(chans, units, halo_frames=1)
    with pytest.raises(ValueError, match='uint8'):
        ctx.measure_pcm(chans, units.astype(np.int32))
    with pytest.raises(ValueError, match='halo_frames'):
        ctx.measure_pcm(chans, units, halo_frames=3)
    with pytest.raises(ValueError, match='halo_frames'):
        ctx.measure_pcm([c[:512] for c in chans], units[:0], halo_frames=2)
    with pytest.raises(ValueError, match='halo_units'):
        ctx.measure_pcm(chans, units, halo_units=2)
    with pytest.raises(AssertionError, match='c1_measure_pcm_batch'):
        ctx.measure_pcm(chans, units)
    with pytest.raises(AssertionError, match='c1_measure_pcm_batch'):
        ctx.measure_pcm(chans, units[:6], halo_frames=1)
    with pytest.raises(AssertionError, match='c1_measure_pcm_device'):
        ctx.measure_pcm_device([0x1000, 0x2000], 4, 0x3000, totals_ptr=0x4000)


# ---- the model itself: mono, seed 1 --------------------------------------------------------------------------------------
MATERIAL = {'pinkT': O.gen_pinkT, 'white': O.gen_white}
_units = {}


def _case(material, modes, frames):
    key = (material, None if modes is None else tuple(modes), frames)
    if key not in _units:
        x = MATERIAL[material](1, frames * 512)
        _units[key] = (x, O.encode_stream([x], fixed_modes=modes)[0])
    return _units[key]


@pytest.mark.parametrize('material,modes', [('pinkT', None), ('white', None), ('pinkT', [0, 0, 0])])
def test_the_delay_of_the_model_is_unambiguous(material, modes):
    """24 frames: the total noise past sample 1024 at delay 266 is less than a quarter of that at every other delay from 262 to
    270.  Measured: a ninth or less (largest ratio: pinkT detection 0.059, white detection 0.113, pinkT [0,0,0] 0.095)"""
    x, units = _case(material, modes, 24)
    y = MP.decoded(units, 1)[0].astype(np.float64)[1024:]
    total = {}
    for d in range(262, 271):
        e = y - MP.delayed(x, 0, d).astype(np.float64)[1024:]
        total[d] = float(np.sum(e * e))
    ratios = {d: total[266] / total[d] for d in total if d != 266}
    print(material, modes, {d: round(r, 4) for d, r in ratios.items()})
    assert all(r < 0.25 for r in ratios.values()), ratios
    # and the model's own sums at the delay are those of this subtraction
    m = MP.model([x], units)
    assert abs(m['totals'][2:, 0].sum() / total[266] - 1.0) < 1e-12


@pytest.mark.parametrize('material,modes', [('pinkT', None), ('white', None), ('pinkT', [0, 0, 0]), ('pinkT', [2, 2, 3])])
def test_the_model_agrees_with_the_coefficient_domain_model(material, modes):
    """frames 2 to 45 of 48: the PCM-domain SNR is within 0.5 dB of measure_units_lib.model's.  Measured: 13.23 against 13.37 dB
    (pinkT, detection), 5.88 against 5.88 (white, detection), 10.84 against 10.90 (pinkT [0,0,0]), 19.28 against 19.35 (pinkT
    [2,2,3]).  The band is for sanity: one sample of misalignment or a wrong W_b moves the figure by many dB"""
    x, units = _case(material, modes, 48)
    pcm_db = MP.snr_db(MP.model([x], units)['totals'], 1, 2, 46)
    coef_db = MP.snr_db(MU.model([x], units)['totals'], 1, 2, 46)
    print(material, modes, 'PCM %.2f dB, coefficients %.2f dB' % (pcm_db, coef_db))
    assert abs(pcm_db - coef_db) < 0.5, (pcm_db, coef_db)


def test_the_model_handles_halos_and_history():
    """the model's own bookkeeping: a tail with its halos equals the rows of the whole; without PCM history the first 266
    samples are compared with zero; without the unit halo the decoder starts fresh"""
    x, units = _case('pinkT', None, 24)
    whole = MP.model([x], units)
    for hf in (1, 2):
        tail = MP.model([x[(10 - hf) * 512:]], units[9:], halo_frames=hf, halo_units=1)
        assert all(MP.bitwise(tail[k], whole[k][10:]) for k in whole)
    bare = MP.model([x[10 * 512:]], units[10:])
    assert not MP.bitwise(bare['noise'][0], whole['noise'][10]) and MP.bitwise(bare['noise'][2:], whole['noise'][12:])
    assert (bare['signal'][0, :8] == 0).all() and bare['signal'][0, 8] > 0 and MP.bitwise(bare['signal'][1:], whole['signal'][11:])
