"""CPU: the encoder's block-selection and quantization stage entry points (c1_select_block_modes, c1_quantize_frames) are
declared, exported and bound, and the reference's stage outputs in tests/golden/encoder_stages.json are reproduced by a second
implementation, the CPU oracle (c1o_qmf_analysis_frame, c1o_block_modes, c1o_mdct_frame, c1o_allocate, c1o_quantize_bfu)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import encoder_stages_golden as EG
import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('c1_select_block_modes', 'c1_quantize_frames')
CASES = EG.cases()
CHAIN = sorted(k for k, v in CASES.items() if v['meta']['kind'] == 'chain')
COEFS = sorted(k for k, v in CASES.items() if v['meta']['kind'] == 'coefs')
SPECS = np.array(O.golden_tables()['specs_per_bfu'])
_fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
_ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))


def test_stage_symbols_declared_exported_and_bound():
    from carta1_amd import build, capi
    build.build_library()
    lib = capi.load()
    header = open(os.path.join(ROOT, 'include', 'carta1_hip.h')).read()
    for name in NAMES:
        assert re.search(r'^int %s\(' % name, header, re.M), name
        assert hasattr(lib, name), name
        assert name in capi.SIGNATURES, name
    import carta1_amd as c1
    for method in ('select_block_modes', 'quantize_frames'):
        assert callable(getattr(c1.Context, method, None)), method


def test_fixture_covers_what_it_claims():
    assert SPECS.sum() == 512 and SPECS.size == 52
    b = CASES['bands']
    x = b['bands'].view(np.uint32)
    assert np.isnan(b['bands']).any() and np.isinf(b['bands']).any() and (x == 0x80000000).any()
    assert ((x & 0x7f800000) == 0).any() and (((x & 0x7fffffff) != 0) & ((x & 0x7f800000) == 0)).any()
    assert (np.abs(b['bands'][np.isfinite(b['bands'])]) > 1e38).any()
    t = b['threshold']
    assert np.isnan(t).any() and (t == 0).any() and (t < 0).any() and (t == 1e300).any()
    assert b['fixed'].any() and not b['fixed'].all()
    assert (b['block_modes'][b['fixed'] == 0] != 0).any()
    c = CASES['coefs_b1']
    w = c['coefficients'].view(np.uint32)
    assert (((w & 0x7fc00000) == 0x7f800000) & ((w & 0x7fffff) != 0)).any()      # signalling NaN patterns
    assert (w == 0x7fc00000).any() and (w == 0x7f800000).any() and (w == 0xff800000).any() and (w == 0x80000000).any()
    assert (np.abs(c['coefficients'][np.isfinite(c['coefficients'])]) > 1).any()
    assert {1, 3, -1, 7} <= set(c['block_modes'].ravel().tolist())
    assert (c['nbfu'] > 0).all() and (c['quantized'] != 0).any()
    for name in COEFS:
        assert CASES[name]['meta']['bias'] in (0.5, 1, 2)


def _options(biased, threshold=1.0, fixed=(-1, -1, -1)):
    o = O.Options()
    o.fixed_modes[:] = list(fixed)
    o.threshold = threshold
    o.biased_sf[:] = [float(v) for v in biased]
    return o


def _fields(coefs, modes, biased):
    """c1o_allocate + c1o_quantize_bfu over the BFUs below nBfu: the layout of c1_quantize_frames"""
    nbfu, wl, sfi = C.c_int(), np.zeros(52, np.int32), np.zeros(52, np.int32)
    coefs = np.ascontiguousarray(coefs, dtype=np.float32)
    m = np.ascontiguousarray(modes, dtype=np.int32)
    bsf = np.ascontiguousarray(biased, dtype=np.float64)
    O.lib().c1o_allocate(_fp(coefs), _ip(m), bsf.ctypes.data_as(C.POINTER(C.c_double)), C.byref(nbfu), _ip(wl), _ip(sfi))
    n = nbfu.value
    q = np.zeros(512, np.int32)
    first = np.concatenate([[0], np.cumsum(SPECS)])
    long_start, short_start = _starts()
    for b in range(n):
        band = 2 if b >= 36 else (1 if b >= 20 else 0)
        start = long_start[b] if m[band] == 0 else short_start[b]
        x = np.ascontiguousarray(coefs[start:start + SPECS[b]])
        out = np.zeros(SPECS[b], np.int32)
        O.lib().c1o_quantize_bfu(_fp(x), int(SPECS[b]), int(sfi[b]), 0 if wl[b] == 0 else int(wl[b]) + 1, _ip(out))
        q[first[b]:first[b] + SPECS[b]] = out
    wl[n:] = 0
    sfi[n:] = 0
    return n, sfi, wl, q


_STARTS = None


def _starts():
    global _STARTS
    if _STARTS is None:
        t = O.golden_tables()
        _STARTS = (np.array(t['bfu_start_long']), np.array(t['bfu_start_short']))
    return _STARTS


def _check_fields(case, f, got):
    n, sfi, wl, q = got
    assert n == case['nbfu'][f], 'frame %d nbfu' % f
    assert np.array_equal(sfi, case['sfi'][f]), 'frame %d sfi' % f
    assert np.array_equal(wl, case['wl'][f]), 'frame %d wl' % f
    assert np.array_equal(q, case['quantized'][f]), 'frame %d quantized' % f


@pytest.mark.parametrize('name', CHAIN)
def test_oracle_reproduces_the_chain(name):
    case = CASES[name]
    meta = case['meta']
    frames = meta['frames']
    pcm = (O.gen_white if meta['signal'] == 'white' else O.gen_pinkT)(meta['seed'], frames * 512)
    fixed = meta['fixed_block_modes'] or [-1, -1, -1]
    o = _options(case['biased'], meta['threshold'], fixed)
    st = O.EncState()
    for f in range(frames):
        bands = np.zeros(512, np.float32)
        O.lib().c1o_qmf_analysis_frame(C.byref(st), _fp(np.ascontiguousarray(pcm[f * 512:(f + 1) * 512])), _fp(bands))
        assert np.array_equal(bands.view(np.uint32), case['bands'][f].view(np.uint32)), 'frame %d bands' % f
        modes = np.zeros(3, np.int32)
        O.lib().c1o_block_modes(C.byref(st), _fp(bands), C.byref(o), _ip(modes))
        assert np.array_equal(modes, case['block_modes'][f]), 'frame %d modes' % f
        coefs = np.zeros(512, np.float32)
        O.lib().c1o_mdct_frame(C.byref(st), _fp(bands), _ip(modes), _fp(coefs))
        assert np.array_equal(coefs.view(np.uint32), case['coefficients'][f].view(np.uint32)), 'frame %d coefficients' % f
        _check_fields(case, f, _fields(coefs, modes, case['biased']))


# Frames of the hand-built bands where the oracle and the reference part: a NaN energy sum (a band of the frame or of the one
# before it has non-finite magnitudes).  The reference's Math.max / Math.min make the score NaN and the band long; the oracle
# (like the encoder's own detector) clamps NaN to 1e-10, 0 and 1 and may call it transient.  The fixture wins; the device
# stage follows the reference there (tests/test_gpu_encoder_stages.py checks every frame).
ORACLE_UNPINNED_BANDS = (19, 39)


def test_oracle_reproduces_the_hand_built_bands():
    case = CASES['bands']
    st = O.EncState()
    for f in range(case['meta']['frames']):
        if case['fixed'][f]:
            continue                                  # fixedBlockModes: the reference leaves transientDetection alone
        if f in ORACLE_UNPINNED_BANDS:
            mags = np.zeros(256, np.float32)
            O.lib().c1o_transient_mags(_fp(np.ascontiguousarray(case['bands'][f])), _fp(mags))
            assert not np.isfinite(np.array(st.prev_mag[:], dtype=np.float32)).all()
            st.prev_mag[:] = mags.tolist()           # the history moves on as in the reference
            continue
        o = _options(np.ones(64), float(case['threshold'][f]))
        modes = np.zeros(3, np.int32)
        O.lib().c1o_block_modes(C.byref(st), _fp(np.ascontiguousarray(case['bands'][f])), C.byref(o), _ip(modes))
        assert np.array_equal(modes, case['block_modes'][f]), 'frame %d' % f


@pytest.mark.parametrize('name', COEFS)
def test_oracle_reproduces_the_hand_built_coefficients(name):
    case = CASES[name]
    for f in range(case['meta']['frames']):
        _check_fields(case, f, _fields(case['coefficients'][f], case['block_modes'][f], case['biased']))
