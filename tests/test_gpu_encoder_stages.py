"""GPU: the encoder's block-selection and quantization stages through the C ABI -- c1_select_block_modes (blockSelectorStage)
and c1_quantize_frames (quantizationStage) -- against the reference's own stage outputs (tests/golden/encoder_stages.json),
composed with c1_qmf_analysis_batch and c1_mdct_batch against the committed KAT units, against the encoder's own detector,
split against whole, and on random inputs against the CPU oracle.  Every comparison is bit for bit on int32 / uint32 views."""
import ctypes as C
import glob
import json
import os

import numpy as np
import pytest

import encoder_stages_golden as EG
import oracle_lib as O
import option_domain_lib as OD

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
CASES = EG.cases()
KAT = json.load(open(os.path.join(G, 'kat_index.json')))
KAT_FILES = sorted(glob.glob(os.path.join(G, 'kat64_*.units.bin')))
SPECS = np.array(O.golden_tables()['specs_per_bfu'])
FIRST = np.concatenate([[0], np.cumsum(SPECS)])
_fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
_ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))


@pytest.fixture(scope='module')
def ctx():
    import carta1_amd as c1
    c = c1.Context(0)
    yield c
    c.close()


def options(bias=1.0, biased=None, **kw):
    import carta1_amd as c1
    vals = dict(kw)
    vals['allocationBias'] = bias
    return c1.EncoderOptions(vals, biased_table=None if biased is None else [float(x) for x in biased])


def assert_fields(got, want, what=''):
    for k in EG.FIELDS:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w.shape, (what, k, g.shape, w.shape)
        bad = np.nonzero((g != w).reshape(g.shape[0], -1).any(axis=1))[0]
        assert bad.size == 0, '%s %s: first differing frame %d of %d' % (what, k, bad[0], bad.size)


# ---- the fixture ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', sorted(k for k, v in CASES.items() if v['meta']['kind'] in ('chain', 'coefs')))
def test_quantize_frames_against_reference(ctx, name):
    case = CASES[name]
    got = ctx.quantize_frames(case['coefficients'], case['block_modes'], options(case['meta']['bias'], case['biased']))
    assert_fields(got, EG.fields_of(case), name)


@pytest.mark.parametrize('name', sorted(k for k, v in CASES.items() if v['meta']['kind'] == 'chain'))
def test_chain_stages_against_reference(ctx, name):
    case = CASES[name]
    meta = case['meta']
    pcm = (O.gen_white if meta['signal'] == 'white' else O.gen_pinkT)(meta['seed'], meta['frames'] * 512)
    bands = ctx.qmf_analysis(pcm)
    assert np.array_equal(bands.view(np.uint32), case['bands'].view(np.uint32))
    if meta['fixed_block_modes'] is None:
        assert np.array_equal(ctx.select_block_modes(bands, meta['threshold']), case['block_modes'])
    coefs, _ = ctx.mdct(bands, case['block_modes'])
    assert np.array_equal(coefs.view(np.uint32), case['coefficients'].view(np.uint32))


def test_select_block_modes_against_reference_hand_built(ctx):
    """one pool: a frame with fixedBlockModes leaves the history alone, so each detection frame decides against the last
    frame detection ran on -- passed as the halo"""
    case = CASES['bands']
    last = None
    for f in range(case['meta']['frames']):
        if case['fixed'][f]:
            continue
        rows = case['bands'][f:f + 1] if last is None else np.stack([case['bands'][last], case['bands'][f]])
        got = ctx.select_block_modes(rows, float(case['threshold'][f]), halo_frames=0 if last is None else 1)
        assert np.array_equal(got[0], case['block_modes'][f]), 'frame %d' % f
        last = f


# ---- composition --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('path', KAT_FILES, ids=[os.path.basename(p) for p in KAT_FILES])
def test_chain_equals_committed_units(ctx, path):
    name = os.path.basename(path)[len('kat64_'):-len('.units.bin')]
    meta = KAT[name]
    opts = dict(meta['options'])
    units = np.fromfile(path, dtype=np.uint8).reshape(-1, 2, 212)
    frames = units.shape[0]
    gen = O.gen_white if meta['signal'] == 'white' else O.gen_pinkT
    o = options(opts.get('allocationBias', 1.0), **{k: v for k, v in opts.items() if k != 'allocationBias'})
    for c in range(2):
        bands = ctx.qmf_analysis(gen(meta['seeds'][c], frames * 512))
        fixed = opts.get('fixedBlockModes')
        modes = np.tile(np.array(fixed, np.int32), (frames, 1)) if fixed else \
            ctx.select_block_modes(bands, opts.get('transientThresholdLow', 1.0))
        coefs, _ = ctx.mdct(bands, modes)
        got = ctx.quantize_frames(coefs, modes, o)
        assert_fields(got, ctx.unpack_units(np.ascontiguousarray(units[:, c])), '%s channel %d' % (name, c))


@pytest.mark.parametrize('signal,threshold', [('white', 1.0), ('pinkT', 1.0), ('pinkT', 0.3), ('white', 0.3)])
def test_select_block_modes_equals_encoder_detector(ctx, signal, threshold):
    import torch
    import carta1_amd as c1
    frames = 3000
    pcm = (O.gen_white(21, frames * 512) if signal == 'white' else O.gen_pinkT(23, frames * 512))
    got = ctx.select_block_modes(ctx.qmf_analysis(pcm), threshold)
    d_pcm = torch.from_numpy(pcm).cuda()
    mags = torch.zeros(frames * 256, dtype=torch.float32, device='cuda')
    modes = torch.zeros(frames, dtype=torch.uint8, device='cuda')
    torch.cuda.synchronize()
    ctx.detect_stages_device([d_pcm.data_ptr()], frames, mags.data_ptr(), modes.data_ptr(),
                             c1.EncoderOptions({'transientThresholdLow': threshold}))
    ctx.synchronize()
    m = modes.cpu().numpy().astype(np.int32)
    want = np.stack([(m >> (2 * b)) & 3 for b in range(3)], axis=1)
    assert (want != 0).any()
    assert np.array_equal(got, want)


def _band_mixture(frames, seed):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((frames, 512)) * rng.choice([1e-3, 0.1, 1.0, 1e20], (frames, 1))).astype(np.float32)
    burst = rng.random(frames) < 0.3
    x[burst, :256] *= 40
    w = x.view(np.uint32)
    special = rng.random((frames, 512)) < rng.choice([0, 0, 0, 0.002, 0.05], (frames, 1))
    w[special] = rng.choice(np.array([0x7fc00000, 0x7f800001, 0x7f800000, 0xff800000, 0x80000000, 0x00000001, 0x7f7fffff],
                                     dtype=np.uint32), int(special.sum()))
    x[rng.random(frames) < 0.05] = 0
    return x


def test_split_with_halo_equals_one_call(ctx):
    bands = np.concatenate([CASES['pinkT_detect']['bands'], _band_mixture(200, 5), CASES['white_detect']['bands']])
    whole = ctx.select_block_modes(bands, 0.3)
    n = bands.shape[0]
    for k in (1, 2, 7, 24, 63, 64, 65, 130, n - 1):
        split = np.concatenate([ctx.select_block_modes(bands[:k], 0.3), ctx.select_block_modes(bands[k - 1:], 0.3, halo_frames=1)])
        assert np.array_equal(split, whole), 'split at %d' % k
    zero_halo = np.concatenate([np.zeros((1, 512), np.float32), bands])
    assert np.array_equal(ctx.select_block_modes(zero_halo, 0.3, halo_frames=1), whole)


def test_random_bands_against_oracle(ctx):
    frames = 20_000
    bands = _band_mixture(frames, 11)
    thresholds = (1.0, 0.3, 0.0)
    got = {t: ctx.select_block_modes(bands, t) for t in thresholds}
    lib = O.lib()
    mags = np.zeros((frames, 256), np.float32)
    for f in range(frames):
        lib.c1o_transient_mags(_fp(bands[f]), _fp(mags[f]))
    finite = np.isfinite(mags).all(axis=1)
    pinned = finite & np.concatenate([[True], finite[:-1]])    # the oracle is pinned where no energy sum is NaN
    assert pinned.mean() > 0.5
    for t in thresholds:
        st = O.EncState()
        o = O.Options()
        o.fixed_modes[:] = [-1, -1, -1]
        o.threshold = t
        want = np.zeros((frames, 3), np.int32)
        for f in range(frames):
            lib.c1o_block_modes(C.byref(st), _fp(bands[f]), C.byref(o), _ip(want[f]))
        bad = np.nonzero((got[t] != want).any(axis=1) & pinned)[0]
        assert bad.size == 0, 'threshold %g: first differing frame %d of %d' % (t, bad[0], bad.size)
        assert (want[pinned] != 0).any()


def _coef_mixture(frames, seed):
    rng = np.random.default_rng(seed)
    scale = rng.choice([1e-6, 1e-3, 0.05, 0.5, 1.0, 4.0], (frames, 1))
    x = (rng.standard_normal((frames, 512)) * scale * np.exp2(-np.arange(512) / 96.0)).astype(np.float32)
    w = x.view(np.uint32)
    sf = np.array([O.h2d(h) for h in O.golden_tables()['scale_factors_f64']], dtype=np.float32).view(np.uint32)
    near = rng.random((frames, 512)) < 0.05
    w[near] = (sf[rng.integers(0, 64, int(near.sum()))].astype(np.int64) + rng.integers(-1, 2, int(near.sum()))).astype(np.uint32) \
        | (rng.integers(0, 2, int(near.sum())).astype(np.uint32) << 31)
    special = rng.random((frames, 512)) < rng.choice([0, 0, 0.001, 0.02], (frames, 1))
    w[special] = rng.choice(np.array([0x7fc00000, 0xffc00000, 0x7f800001, 0x7fa00000, 0xff800001, 0x7f800000, 0xff800000,
                                      0x80000000, 0x00000001, 0x807fffff], dtype=np.uint32), int(special.sum()))
    x[rng.random(frames) < 0.02] = 0
    modes = rng.choice(np.array([0, 0, 0, 0, 1, 2, 3, -1, 7], dtype=np.int32), (frames, 3))
    return x, modes


def _oracle_fields(coefs, modes, biased):
    frames = coefs.shape[0]
    lib = O.lib()
    t = O.golden_tables()
    start_long, start_short = np.array(t['bfu_start_long']), np.array(t['bfu_start_short'])
    band = np.where(np.arange(52) >= 36, 2, np.where(np.arange(52) >= 20, 1, 0))
    bsf = np.ascontiguousarray(biased, dtype=np.float64)
    nbfu = np.zeros(frames, np.int32)
    wl = np.zeros((frames, 52), np.int32)
    sfi = np.zeros((frames, 52), np.int32)
    n = C.c_int()
    for f in range(frames):
        lib.c1o_allocate(_fp(coefs[f]), _ip(modes[f]), bsf.ctypes.data_as(C.POINTER(C.c_double)), C.byref(n), _ip(wl[f]), _ip(sfi[f]))
        nbfu[f] = n.value
    live = np.arange(52)[None, :] < nbfu[:, None]
    wl[~live] = 0
    sfi[~live] = 0
    # c1o_quantize_bfu once per (scale factor, bits) over every coefficient of the BFUs that use them
    q = np.zeros((frames, 512), np.int32)
    starts = np.where(modes[:, band] == 0, start_long[None, :], start_short[None, :])        # [frames, 52]
    bits = np.where(wl == 0, 0, wl + 1)
    for s, b in set(zip(sfi[live].tolist(), bits[live].tolist())):
        if s == 0 or b == 0:
            continue
        fr, bf = np.nonzero(live & (sfi == s) & (bits == b))
        src = np.concatenate([coefs[i, starts[i, j]:starts[i, j] + SPECS[j]] for i, j in zip(fr, bf)])
        out = np.zeros(src.size, np.int32)
        src = np.ascontiguousarray(src)
        lib.c1o_quantize_bfu(_fp(src), src.size, s, b, _ip(out))
        at = 0
        for i, j in zip(fr, bf):
            q[i, FIRST[j]:FIRST[j] + SPECS[j]] = out[at:at + SPECS[j]]
            at += SPECS[j]
    return {'nbfu': nbfu, 'block_modes': modes, 'sfi': sfi, 'wl': wl, 'quantized': q}


@pytest.mark.parametrize('bias', [0.5, 1.0, 2.0] + [float(b) for b in OD.fixture()['biases'] if float(b) not in (0.5, 1.0, 2.0)])
def test_random_coefficients_against_oracle(ctx, bias):
    frames = 40_000                                             # 440 k frames over the eleven biases
    coefs, modes = _coef_mixture(frames, int(bias * 10))
    biased = CASES['coefs_b%g' % bias]['biased'] if bias in (0.5, 1.0, 2.0) else OD.biased(bias)
    got = ctx.quantize_frames(coefs, modes, options(bias, biased))
    assert_fields(got, _oracle_fields(coefs, modes, biased), 'bias %g' % bias)


def test_quantize_frames_round_trips_through_dequantize(ctx):
    case = CASES['white_detect']
    fields = ctx.quantize_frames(case['coefficients'], case['block_modes'])
    assert np.array_equal(fields['block_modes'], case['block_modes'])
    coefs = ctx.dequantize_frames(fields)
    assert coefs.shape == (case['meta']['frames'], 512) and np.isfinite(coefs).all()


# ---- arguments ----------------------------------------------------------------------------------------------------------

def test_bad_arguments_and_empty_calls(ctx):
    from carta1_amd import capi
    lib, h = capi.load(), ctx._h
    bands = np.zeros((2, 512), np.float32)

    def code(fn):
        with pytest.raises(capi.Carta1Error) as e:
            fn()
        return e.value.code

    for halo in (-1, 2):
        assert code(lambda: ctx.select_block_modes(bands, halo_frames=halo)) == 1
    p = bands.ctypes.data
    big = (1 << 20) + 1
    o = options().to_c()
    assert code(lambda: capi.check(lib.c1_select_block_modes(h, p, big, 0, 1.0, p))) == 1
    assert code(lambda: capi.check(lib.c1_select_block_modes(h, p, -1, 0, 1.0, p))) == 1
    assert code(lambda: capi.check(lib.c1_select_block_modes(h, None, 1, 0, 1.0, p))) == 1
    assert code(lambda: capi.check(lib.c1_select_block_modes(h, p, 1, 0, 1.0, None))) == 1
    assert code(lambda: capi.check(lib.c1_quantize_frames(h, p, big, p, C.byref(o), p, p, p, p))) == 1
    assert code(lambda: capi.check(lib.c1_quantize_frames(h, p, 1, p, None, p, p, p, p))) == 1
    assert code(lambda: capi.check(lib.c1_quantize_frames(h, None, 1, p, C.byref(o), p, p, p, p))) == 1
    assert code(lambda: capi.check(lib.c1_quantize_frames(h, p, 1, None, C.byref(o), p, p, p, p))) == 1
    assert code(lambda: capi.check(lib.c1_quantize_frames(h, p, 1, p, C.byref(o), p, p, p, None))) == 1
    # frames == 0: nothing is read or written
    sentinel = np.full(8, 7, np.int32)
    capi.check(lib.c1_select_block_modes(h, None, 0, 0, 1.0, sentinel.ctypes.data))
    capi.check(lib.c1_quantize_frames(h, None, 0, None, C.byref(o), sentinel.ctypes.data, None, None, None))
    assert (sentinel == 7).all()
    assert ctx.select_block_modes(np.zeros((0, 512), np.float32)).shape == (0, 3)
    assert ctx.quantize_frames(np.zeros((0, 512), np.float32), np.zeros((0, 3), np.int32))['quantized'].shape == (0, 512)
    # the threshold and the fixed modes of the options are not read by the quantization stage
    case = CASES['coefs_b1']
    a = ctx.quantize_frames(case['coefficients'], case['block_modes'], options(1.0, case['biased']))
    b = ctx.quantize_frames(case['coefficients'], case['block_modes'],
                            options(1.0, case['biased'], transientThresholdLow=0.5, fixedBlockModes=[2, 2, 3]))
    assert_fields(a, b, 'options')
