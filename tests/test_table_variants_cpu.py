"""The CPU oracle under another engine's tables (c1o_set_tables) against the reference run with those tables
(tests/golden/table_variants.json, gen_table_variants.mjs), bit for bit: the KAT streams' units and decoded frames,
quantizationStage on frames whose BFU maxima sit on the scale-factor boundaries, and quantize() at rounding midpoints.
Also the host side of the library: which table shortcuts c1_table_fast_paths grants each variant, and the bias-1 table
EncoderOptions hands the encoder once a variant is installed."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
import table_variants_lib as TV
from test_encoder_stages_cpu import _fields

NAMES = TV.names()


@pytest.fixture
def installed():
    """c1o_set_tables for the test's variant, undone afterwards"""
    def install(v):
        O.set_tables(v['tables'])
        return v
    try:
        yield install
    finally:
        O.set_tables(None)


def test_fixture_covers_what_it_claims():
    fx = TV.fixture()
    assert set(NAMES) == {'ulp', 'inside', 'sfshift', 'sfpow2', 'twiddle'}
    for name in NAMES:
        v = TV.variant(name)
        d = v['differs_from_default']
        # every variant changes its tables and something the reference computes from them
        assert d['tables'] > 0, name
        assert sum(n for k, n in d.items() if k.endswith(('_units', '_pcm8', 'quant_fields', 'quantize_q'))) > 0, name
        assert np.array_equal(v['biased'], v['tables'][:64])
        for case in v['kat'].values():
            assert case['units'].shape == (128, 212) and case['pcm8'].shape == (128, 8)
    # the two scale-factor variants reach a BFU maximum on which the table compare and the log2 boundaries part
    assert fx['variants']['sfshift']['differs_from_default']['quant_fields'] > 0
    assert fx['variants']['sfpow2']['differs_from_default']['quant_fields'] > 0


def test_inputs_are_the_committed_kat_inputs():
    import hashlib
    for case in TV.variant(NAMES[0])['kat'].values():
        got = [hashlib.sha256(c.tobytes()).hexdigest() for c in TV.kat_inputs(case)]
        assert got == case['input_sha256']


def test_default_tables_reproduce_the_kat64_fixtures():
    """under the default tables the four cases are the committed kat64_* streams: the variants' differences are theirs"""
    import os
    for case in TV.variant(NAMES[0])['kat'].values():
        want = np.fromfile(os.path.join(TV.G, 'kat64_%s.units.bin' % case['kat64']), np.uint8).reshape(-1, 212)
        fm, thr = TV.kat_options(case)
        got, _ = O.encode_stream(TV.kat_inputs(case), fixed_modes=fm, threshold=thr)
        assert np.array_equal(got, want), case['kat64']


@pytest.mark.parametrize('name', NAMES)
def test_oracle_reproduces_the_kat_streams(name, installed):
    v = installed(TV.variant(name))
    for cname, case in v['kat'].items():
        fm, thr = TV.kat_options(case)
        units, _ = O.encode_stream(TV.kat_inputs(case), fixed_modes=fm, threshold=thr, biased=v['biased'])
        bad = np.nonzero((units != case['units']).any(axis=1))[0]
        assert bad.size == 0, '%s %s: %d units differ, first %d' % (name, cname, bad.size, bad[0])
        pcm, _ = O.decode_stream(case['units'], 2)
        dig = TV.frame_digests(pcm)
        bad = np.nonzero((dig != case['pcm8']).any(axis=1))[0]
        assert bad.size == 0, '%s %s: %d decoded frames differ, first %d' % (name, cname, bad.size, bad[0])


@pytest.mark.parametrize('name', NAMES)
def test_oracle_reproduces_quantization_on_the_boundaries(name, installed):
    v = installed(TV.variant(name))
    q = v['quant']
    for f in range(q['coefs'].shape[0]):
        n, sfi, wl, quant = _fields(q['coefs'][f], q['modes'][f], v['biased'])
        assert n == q['nbfu'][f], (name, f)
        assert np.array_equal(sfi, q['sfi'][f]), (name, f, np.nonzero(sfi != q['sfi'][f]))
        assert np.array_equal(wl, q['wl'][f]), (name, f)
        assert np.array_equal(quant, q['quantized'][f]), (name, f)


@pytest.mark.parametrize('name', NAMES)
def test_oracle_reproduces_quantize_at_the_midpoints(name, installed):
    v = installed(TV.variant(name))
    p = v['points']
    got = np.zeros_like(p['q'])
    out = np.zeros(1, np.int32)
    for i in range(p['x'].size):
        x = np.ascontiguousarray(p['x'][i:i + 1])
        O.lib().c1o_quantize_bfu(x.ctypes.data_as(C.POINTER(C.c_float)), 1, int(p['sfi'][i]), int(p['bits'][i]),
                                 out.ctypes.data_as(C.POINTER(C.c_int)))
        got[i] = out[0]
    assert np.array_equal(got, p['q']), (name, np.nonzero(got != p['q'])[0][:8])


def test_oracle_tables_reset():
    v = TV.variant('inside')
    case = v['kat']['pinkT_detect']
    fm, thr = TV.kat_options(case)
    O.set_tables(v['tables'])
    O.set_tables(None)
    units, _ = O.encode_stream(TV.kat_inputs(case), fixed_modes=fm, threshold=thr)
    import os
    want = np.fromfile(os.path.join(TV.G, 'kat64_pinkT_detect.units.bin'), np.uint8).reshape(-1, 212)
    assert np.array_equal(units, want)


@pytest.mark.parametrize('name', NAMES)
def test_fast_path_gates_and_bias1_table_follow_the_installed_tables(name):
    """c1_table_fast_paths grants the bit-pattern findScaleFactor form exactly to the variants built for it, and
    EncoderOptions at bias 1 hands the encoder the installed SCALE_FACTORS (bitallocation.js:51-53), not the packaged
    default table.  Host only: no device needed."""
    import carta1_amd as c1
    from carta1_amd import capi
    lib = capi.load()
    v = TV.variant(name)
    a, b = C.c_int(-1), C.c_int(-1)
    t = TV.c_tables(v['tables'])
    try:
        assert lib.c1_set_tables(C.byref(t)) == 0
        assert lib.c1_table_fast_paths(C.byref(a), C.byref(b)) == 0
        assert a.value == v['gates']['sf_fast'], (name, a.value)
        o = c1.EncoderOptions().to_c()
        assert np.array_equal(np.array(o.biased_scale_factors[:]), v['biased'])
        o = c1.EncoderOptions({'allocationBias': 1}).to_c()
        assert np.array_equal(np.array(o.biased_scale_factors[:]), v['biased'])
    finally:
        lib.c1_set_tables(None)
    o = c1.EncoderOptions().to_c()
    assert np.array_equal(np.array(o.biased_scale_factors[:]), c1.codec.packaged_biased_table(1.0))


@pytest.mark.parametrize('name', NAMES)
def test_oracle_reproduces_the_stage_functions(name, installed):
    """performFFT's magnitudes (the detector's FFT), qmfAnalysisStage -> mdctStage, and the decoder's stages over the
    hand-built frame fields of decoder_stages_fields.bin (their PCM), under the variant's tables"""
    import decoder_stages_golden as DG
    v = installed(TV.variant(name))
    st = v['stages']
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    p = O.gen_pinkT(3, 8 * 512)
    es = O.EncState()
    for f in range(8):
        bands, mags = np.zeros(512, np.float32), np.zeros(256, np.float32)
        O.lib().c1o_qmf_analysis_frame(C.byref(es), fp(p[f * 512:(f + 1) * 512].copy()), fp(bands))
        O.lib().c1o_transient_mags(fp(bands), fp(mags))
        assert np.array_equal(mags.view(np.uint32), st['mags'][f].view(np.uint32)), (name, 'mags', f)
    for m, modes in enumerate(st['mdct_modes']):
        x = O.gen_white(51, 4 * 512)
        es = O.EncState()
        md = np.array(modes, np.int32)
        for f in range(4):
            bands, coefs = np.zeros(512, np.float32), np.zeros(512, np.float32)
            O.lib().c1o_qmf_analysis_frame(C.byref(es), fp(x[f * 512:(f + 1) * 512].copy()), fp(bands))
            O.lib().c1o_mdct_frame(C.byref(es), fp(bands), ip(md), fp(coefs))
            assert np.array_equal(coefs.view(np.uint32), st['mdct'][m, f].view(np.uint32)), (name, 'mdct', modes, f)
    case = DG.cases()['fields']
    ds = O.DecState()
    for f in range(case['nbfu'].shape[0]):
        fl = O.Fields()
        fl.nbfu = int(case['nbfu'][f])
        fl.modes[:] = [int(x) for x in case['block_modes'][f]]
        fl.wl[:] = [int(x) for x in case['wl'][f]]
        fl.sfi[:] = [int(x) for x in case['sfi'][f]]
        fl.q[:] = [int(x) for x in case['quantized'][f]]
        pcm = np.zeros(512, np.float32)
        O.lib().c1o_decode_frame(C.byref(ds), C.byref(fl), fp(pcm))
        assert np.array_equal(TV.d8(pcm), st['decoder_d8'][f, 2]), (name, 'decoded frame', f)


def test_fixture_fft_is_the_transform_with_the_variant_w():
    """the recorded FFT.fft outputs are that transform of the recorded inputs (to binary32 rounding), and under
    `twiddle` they differ from the default w's: the GPU test compares c1_fft with the variant w against them bit for bit"""
    for name in NAMES:
        for c in TV.variant(name)['stages']['fft']:
            z = O.gen_white(c['seed'], c['n']).astype(np.float64) + 1j * O.gen_white(c['seed'] + 100, c['n'])
            want = np.fft.fft(z)
            got = c['real'].astype(np.float64) + 1j * c['imag']
            assert np.abs(got - want).max() < 1e-5 * np.sqrt(c['n']), (name, c['n'])
    assert TV.fixture()['variants']['twiddle']['differs_from_default']['stage_fft'] > 0
    assert TV.fixture()['variants']['twiddle']['differs_from_default']['stage_mags'] > 0
