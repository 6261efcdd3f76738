"""GPU: the library under tables another engine builds (c1_set_tables), against the reference run with those tables
(tests/golden/table_variants.json, gen_table_variants.mjs) and against the CPU oracle under the same tables.

Per variant, on contexts created after the variant is installed: the table shortcuts and speculative paths it is built to
open or close; the KAT streams encoded in speculation modes 0, 1 and 2, whole and as a tail from its halo, unit for unit;
proof (ulp, inside) that those units went through the speculative analysis and detector; the exact decode frame for frame
and the binary32 decode within test_gpu_decode32's bounds; quantize_frames on BFU maxima at the scale-factor boundaries and
quantize at rounding midpoints; the detector's FFT, c1_fft with the variant's w, mdct and the decoder's stages against the
reference's stage outputs; dequantize, mdct and select_block_modes against the oracle; and a sweep of patchwork streams
against the oracle.  Last: a context keeps the tables it was created with, and c1_set_tables(NULL) restores the defaults."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle_lib as O
import option_domain_lib as OD
import table_variants_lib as TV

pytestmark = pytest.mark.gpu
NAMES = TV.names()
CUT, HALO = 29, 2


def _lib():
    from carta1_amd import capi
    return capi.load()


@pytest.fixture(scope='module', params=NAMES)
def env(request):
    """(variant, a context created under it); the oracle runs under the same tables meanwhile"""
    import carta1_amd as c1
    v = TV.variant(request.param)
    lib = _lib()
    t = TV.c_tables(v['tables'])
    ctx = None
    try:
        assert lib.c1_set_tables(C.byref(t)) == 0
        O.set_tables(v['tables'])
        ctx = c1.Context(0)
        yield v, ctx
    finally:
        if ctx is not None:
            ctx.close()
        lib.c1_set_tables(None)
        O.set_tables(None)


def options(v, case=None, table=True):
    import carta1_amd as c1
    opts = dict(case['options']) if case else {}
    return c1.EncoderOptions(opts, biased_table=[float(x) for x in v['biased']] if table else None)


def test_gates(env):
    """c1_table_fast_paths and the speculative entry points: open or closed as the variant was built to make them"""
    import torch
    import carta1_amd as c1
    from carta1_amd import capi
    v, ctx = env
    a, b = C.c_int(-1), C.c_int(-1)
    assert _lib().c1_table_fast_paths(C.byref(a), C.byref(b)) == 0
    assert a.value == v['gates']['sf_fast'], a.value
    frames = 4
    pcm = [torch.from_numpy(O.gen_white(5, frames * 512)).cuda()]
    coefs = torch.zeros(frames * 512, dtype=torch.float32, device='cuda')
    eps = torch.zeros(frames * 4, dtype=torch.float32, device='cuda')
    side = torch.zeros(frames * 64, dtype=torch.uint8, device='cuda')
    sc = torch.zeros(frames * 6, dtype=torch.float64, device='cuda')
    modes = torch.zeros(frames, dtype=torch.uint8, device='cuda')
    opened = torch.zeros(1, dtype=torch.int32, device='cuda')
    torch.cuda.synchronize()
    calls = [(lambda: ctx.spec_stages_device([p.data_ptr() for p in pcm], frames, coefs.data_ptr(), eps.data_ptr(), side.data_ptr(),
                                              c1.EncoderOptions({'fixedBlockModes': [0, 0, 0]})), 4),
             (lambda: ctx.detect_scores_device([p.data_ptr() for p in pcm], frames, sc.data_ptr(), modes.data_ptr(), opened.data_ptr(),
                                                c1.EncoderOptions(), speculative=True), 1)]
    for call, closed_code in calls:
        if v['gates']['spec_ok']:
            call()
            ctx.synchronize()
        else:
            with pytest.raises(capi.Carta1Error) as e:
                call()
            assert e.value.code == closed_code


@pytest.mark.parametrize('mode', [0, 1, 2])
def test_kat_streams_encode_to_the_reference_units(env, mode):
    v, ctx = env
    ctx.set_speculation(mode)
    try:
        for name, case in v['kat'].items():
            xs = TV.kat_inputs(case)
            for eo in (options(v, case), options(v, case, table=False)):     # the explicit table; bias 1 as installed
                units = ctx.encode(xs, eo)
                bad = np.nonzero((units != case['units']).any(axis=1))[0]
                assert bad.size == 0, (name, mode, '%d units differ, first %d' % (bad.size, bad[0]))
            tail = ctx.encode([x[(CUT - HALO) * 512:] for x in xs], options(v, case), halo_frames=HALO)
            assert np.array_equal(tail, case['units'][CUT * 2:]), (name, mode, 'tail')
    finally:
        ctx.set_speculation(1)


def test_speculative_paths_carry_the_open_variants(env):
    """in speculation mode 2 the KAT units came through the binary32 analysis and detector when the variant opens them, and
    through the exact kernels alone when it closes them"""
    v, ctx = env
    ctx.set_speculation(2)
    try:
        ctx.speculation_stats(reset=True)
        case = v['kat']['white_m000']
        assert np.array_equal(ctx.encode(TV.kat_inputs(case), options(v, case)), case['units'])
        units, redone = ctx.speculation_stats()
        d0 = ctx.detection_stats()
        case = v['kat']['pinkT_detect']
        assert np.array_equal(ctx.encode(TV.kat_inputs(case), options(v, case)), case['units'])
        d1 = ctx.detection_stats()
        if v['gates']['spec_ok']:
            assert units >= 128 and redone < units, (units, redone)
            assert d1[0] - d0[0] >= 128 and d1[1] - d0[1] < d1[0] - d0[0], (d0, d1)
        else:                                       # closed: every unit on the exact kernels, even when forced
            assert units == 0 and d1[0] == d0[0], (units, d0, d1)
    finally:
        ctx.set_speculation(1)


def test_kat_streams_decode_to_the_reference_pcm(env):
    v, ctx = env
    for name, case in v['kat'].items():
        pcm = ctx.decode(case['units'], 2)
        dig = TV.frame_digests([pcm[0], pcm[1]])
        bad = np.nonzero((dig != case['pcm8']).any(axis=1))[0]
        assert bad.size == 0, (name, '%d frames differ, first %d' % (bad.size, bad[0]))
        ctx.set_decode_precision(True)
        try:
            got = ctx.decode(case['units'], 2)
        finally:
            ctx.set_decode_precision(False)
        for c in range(2):
            d = got[c].astype(np.float64) - pcm[c]
            assert np.sqrt(np.mean(d * d)) < 1e-6 and np.abs(d).max() < 1e-5, (name, c)


def test_quantization_stages_against_the_reference(env):
    v, ctx = env
    q = v['quant']
    got = ctx.quantize_frames(q['coefs'], q['modes'], options(v))
    for k in ('nbfu', 'sfi', 'wl', 'quantized'):
        bad = np.nonzero((np.asarray(got[k]) != q[k]).reshape(q['coefs'].shape[0], -1).any(axis=1))[0]
        assert bad.size == 0, (k, 'frames', bad)
    p = v['points']
    for s in range(1, 64):
        for bits in np.unique(p['bits']):
            sel = (p['sfi'] == s) & (p['bits'] == bits)
            assert np.array_equal(ctx.quantize(p['x'][sel], s, int(bits)), p['q'][sel]), (s, bits)
            want = np.zeros(int(sel.sum()), np.float32)
            qv = np.ascontiguousarray(p['q'][sel])
            O.lib().c1o_dequantize_bfu(qv.ctypes.data_as(C.POINTER(C.c_int)), qv.size, s, int(bits), want.ctypes.data_as(C.POINTER(C.c_float)))
            assert np.array_equal(ctx.dequantize(qv, s, int(bits)).view(np.uint32), want.view(np.uint32)), (s, bits)


def test_transform_stages_against_the_oracle(env):
    """qmf_analysis -> select_block_modes and mdct (the variant's window and MDCT tables) on the pinkT KAT input"""
    v, ctx = env
    x = TV.kat_inputs(v['kat']['pinkT_detect'])[0][:24 * 512]
    bands = ctx.qmf_analysis(x)
    st = O.EncState()
    want_modes, want_coefs = np.zeros((24, 3), np.int32), np.zeros((24, 512), np.float32)
    o = O.make_options(threshold=0.3)
    for f in range(24):
        b = bands[f].copy()                 # c1o_mdct_frame windows the bands in place
        O.lib().c1o_block_modes(C.byref(st), b.ctypes.data_as(C.POINTER(C.c_float)), C.byref(o), want_modes[f].ctypes.data_as(C.POINTER(C.c_int)))
        O.lib().c1o_mdct_frame(C.byref(st), b.ctypes.data_as(C.POINTER(C.c_float)), want_modes[f].ctypes.data_as(C.POINTER(C.c_int)),
                               want_coefs[f].ctypes.data_as(C.POINTER(C.c_float)))
    assert np.array_equal(ctx.select_block_modes(bands, threshold=0.3), want_modes)
    assert len({tuple(m) for m in want_modes}) > 1
    coefs, _ = ctx.mdct(bands, want_modes)
    assert np.array_equal(coefs.view(np.uint32), want_coefs.view(np.uint32))


def test_stage_functions_against_the_reference(env):
    """the detector's FFT magnitudes, c1_fft with the variant's w, qmf_analysis -> mdct, and dequantize_frames -> imdct ->
    qmf_synthesis over the hand-built fields of decoder_stages_fields.bin, against the reference's own stage outputs"""
    import torch
    import carta1_amd as c1
    import decoder_stages_golden as DG
    v, ctx = env
    st = v['stages']
    d_pcm = torch.from_numpy(O.gen_pinkT(3, 8 * 512)).cuda()
    mags = torch.zeros(8 * 256, dtype=torch.float32, device='cuda')
    modes = torch.zeros(8, dtype=torch.uint8, device='cuda')
    torch.cuda.synchronize()
    ctx.detect_stages_device([d_pcm.data_ptr()], 8, mags.data_ptr(), modes.data_ptr(), c1.EncoderOptions({}))
    ctx.synchronize()
    got = mags.cpu().numpy().reshape(8, 256)
    assert np.array_equal(got.view(np.uint32), st['mags'].view(np.uint32)), ('mags', np.nonzero((got != st['mags']).any(axis=1))[0])
    for c in st['fft']:
        re, im = O.gen_white(c['seed'], c['n']), O.gen_white(c['seed'] + 100, c['n'])
        ctx.fft(re, im, TV.fft_w(v['tables'], c['n']))
        assert np.array_equal(re.view(np.uint32), c['real'].view(np.uint32)) and np.array_equal(im.view(np.uint32), c['imag'].view(np.uint32)), ('fft', c['n'])
    bands = ctx.qmf_analysis(O.gen_white(51, 4 * 512))
    for m, md in enumerate(st['mdct_modes']):
        coefs, _ = ctx.mdct(bands, np.tile(np.array(md, np.int32), (4, 1)))
        assert np.array_equal(coefs.view(np.uint32), st['mdct'][m].view(np.uint32)), ('mdct', md)
    fields = DG.fields_of(DG.cases()['fields'])
    coefs = ctx.dequantize_frames(fields)
    bands = ctx.imdct(coefs, fields['block_modes'])
    pcm = ctx.qmf_synthesis(bands)
    for f in range(coefs.shape[0]):
        for k, a in enumerate((coefs, bands, pcm)):
            assert np.array_equal(TV.d8(a[f]), st['decoder_d8'][f, k]), ('decoder stage', ('coefficients', 'bands', 'pcm')[k], 'frame', f)


SWEEP = [(i, 3 + (i * 97) % 418, 1 + i % 2) for i in range(20)]
SWEEP_OPTIONS = [{}, {'transientThresholdLow': 0.3}, {'fixedBlockModes': [0, 0, 0]}, {'fixedBlockModes': [2, 2, 3]},
                 {'fixedBlockModes': [0, 2, 0]}, {'transientThresholdLow': 0.05}]


def test_patchwork_sweep_against_the_oracle(env):
    v, ctx = env
    for i, frames, nch in SWEEP:
        xs = [OD.material({'kind': 'patch'}, 900 + i + 7919 * c, 0, frames * 512) for c in range(nch)]
        opts = SWEEP_OPTIONS[i % len(SWEEP_OPTIONS)]
        fm = opts.get('fixedBlockModes')
        want, _ = O.encode_stream(xs, fixed_modes=fm, threshold=float(opts.get('transientThresholdLow', 1.0)), biased=v['biased'])
        import carta1_amd as c1
        got = ctx.encode(xs, c1.EncoderOptions(opts))
        bad = np.nonzero((got != want).any(axis=1))[0]
        assert bad.size == 0, (i, frames, nch, opts, '%d units differ, first %d' % (bad.size, bad[0]))
        pw, _ = O.decode_stream(want, nch)
        pg = ctx.decode(got, nch)
        for c in range(nch):
            assert np.array_equal(np.asarray(pg[c]).view(np.uint32), pw[c].view(np.uint32)), (i, c)


def test_contexts_keep_their_tables_and_the_reset_restores_the_defaults():
    import carta1_amd as c1
    lib = _lib()
    # the module-scoped `env` keeps its last variant installed until the module ends: start from the defaults
    assert lib.c1_set_tables(None) == 0
    O.set_tables(None)
    v = TV.variant('inside')
    case = v['kat']['pinkT_detect']
    xs = TV.kat_inputs(case)
    default = np.fromfile(os.path.join(TV.G, 'kat64_%s.units.bin' % case['kat64']), np.uint8).reshape(-1, 212)
    assert not np.array_equal(default, case['units'])
    before = c1.Context(0)
    t = TV.c_tables(v['tables'])
    try:
        assert lib.c1_set_tables(C.byref(t)) == 0
        assert np.array_equal(before.encode(xs, c1.EncoderOptions(case['options'], biased_table=list(default_sf()))), default)
        fresh = c1.Context(0)
        try:
            assert np.array_equal(fresh.encode(xs, c1.EncoderOptions(case['options'])), case['units'])
        finally:
            fresh.close()
    finally:
        lib.c1_set_tables(None)
        before.close()
    after = c1.Context(0)
    try:
        assert np.array_equal(after.encode(xs, c1.EncoderOptions(case['options'])), default)
        for name in ('white_m000_b1', 'white_m223_b1', 'pinkT_detect_thr0.3'):
            c = next(k for k in v['kat'].values() if k['kat64'] == name)
            want = np.fromfile(os.path.join(TV.G, 'kat64_%s.units.bin' % name), np.uint8).reshape(-1, 212)
            assert np.array_equal(after.encode(TV.kat_inputs(c), c1.EncoderOptions(c['options'])), want), name
    finally:
        after.close()


def default_sf():
    from carta1_amd import capi
    t = capi.Tables()
    assert _lib().c1_get_default_tables(C.byref(t)) == 0
    return [float(x) for x in t.scale_factors]
