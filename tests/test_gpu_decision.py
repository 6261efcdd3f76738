"""GPU: the batched decision entries (c1_perform_fft, c1_detect_transients, c1_find_scale_factors, c1_allocate_bits and the
Math.log2 tap) against every record of the reference's own functions (tests/golden/decision.json), against the CPU model
(tests/model/decision_model.c) on 100 k random problems per function, and composed: groupIntoBFUs + allocate_bits against
quantize_frames, performFFT + detectTransient per band against select_block_modes."""
import numpy as np
import pytest
import torch

import decision_lib as D
import encoder_stages_golden as EG

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ctx():
    import carta1_amd as c1
    c = c1.Context(0)
    yield c
    c.close()


def test_log2_tap_matches_v8(ctx):
    index, words = D.fixture()
    pairs = D.span(words, index['log2']).reshape(-1, 2)
    x = torch.tensor(pairs[:, 0], dtype=torch.float64, device='cuda')
    y = torch.empty_like(x)
    ctx.libm_device(4, x.data_ptr(), y.data_ptr(), x.numel())
    torch.cuda.synchronize()
    assert D.same(y.cpu().numpy(), pairs[:, 1])


def test_perform_fft_records(ctx):
    index, words = D.fixture()
    for r in index['fft']:
        got = ctx.perform_fft([D.span(words, r['x'])], r['n'], w=D.span(words, r['w']))
        assert got.shape == (1, r['n'] // 2)
        assert D.same(got[0], D.span(words, r['y'])), (r['name'], r['n'])


def test_detect_transient_records(ctx):
    index, words = D.fixture()
    recs = index['detect']
    flags, scores = ctx.detect_transient([D.span(words, r['c']) for r in recs],
                                         [None if r['p'] is None else D.span(words, r['p']) for r in recs],
                                         [words[r['t']] for r in recs])
    assert list(flags) == [r['r'] for r in recs]
    assert D.same(scores, [words[r['s']] for r in recs])


def test_find_scale_factor_records(ctx):
    index, words = D.fixture()
    recs = index['sf']
    got = ctx.find_scale_factor([D.span(words, r['x']) for r in recs], [r['len'] for r in recs])
    assert list(got) == [r['r'] for r in recs]


def test_allocate_bits_records(ctx):
    index, words = D.fixture()
    for r in index['alloc']:
        bfus, sizes, mb, table = D.alloc_record(index, words, r)
        s = np.zeros((1, 52), np.int32)
        s[0, :len(sizes)] = sizes
        res = ctx.allocate_bits([bfus], s, mb, biased_table=table)
        count, fb = int(res['bfu_count'][0]), bool(res['fallback'][0])
        assert count == r['count'], r['name']
        assert list(res['allocation'][0, :count]) == r['wl'], r['name']
        assert list(res['scale_factor_indices'][0, :len(r['sfi'])]) == r['sfi'], r['name']
        assert len(r['sfi']) == (52 if fb else mb) and not res['allocation'][0, count:].any(), r['name']


def _values(rng, n, shape):
    """random doubles with a share of edge values: zeros of both signs, tiny, huge, NaN, +-Inf, binary32 and binary64"""
    x = rng.standard_normal(shape) * np.exp2(rng.integers(-30, 10, size=shape))
    edge = np.array([0.0, -0.0, 1e-11, -1e-12, 5e-324, np.nan, np.inf, -np.inf, 1e300, 3.4e38])
    pick = rng.random(shape) < 0.03
    x[pick] = edge[rng.integers(0, edge.size, size=int(pick.sum()))]
    f32 = rng.random(shape[0] if len(shape) > 1 else 1) < 0.5
    if len(shape) > 1:
        with np.errstate(over='ignore'):                        # binary32 rounding overflows to +-Inf, as Math.fround does
            x[f32] = x[f32].astype(np.float32).astype(np.float64)
    return x


def test_find_scale_factor_random_against_model(ctx):
    rng = np.random.default_rng(11)
    n = 100_000
    x = _values(rng, n, (n, 6))
    lengths = rng.integers(-2, 9, size=n)
    got = ctx.find_scale_factor(list(x), lengths)
    want = [D.find_scale_factor(x[p], lengths[p]) for p in range(n)]
    assert np.array_equal(got, want)


def test_detect_transient_random_against_model(ctx):
    rng = np.random.default_rng(12)
    n = 100_000
    lens_c = rng.choice([0, 1, 3, 8, 17, 32], size=n)
    lens_p = np.where(rng.random(n) < 0.7, lens_c, rng.integers(0, 40, size=n))
    cur = [np.abs(v) if k % 2 else v for k, v in enumerate(_values(rng, n, (n, 40)))]
    cur = [cur[p][:lens_c[p]] for p in range(n)]
    prev = [None if rng.random() < 0.02 else v[:lens_p[p]] for p, v in enumerate(_values(rng, n, (n, 40)))]
    thr = rng.choice([0.1, 0.3, 1.0, np.nan, -np.inf], size=n)
    flags, scores = ctx.detect_transient(cur, prev, thr)
    want = [D.detect(cur[p], prev[p], thr[p]) for p in range(n)]
    assert list(flags) == [w[0] for w in want]
    assert D.same(scores, [w[1] for w in want])


def test_perform_fft_random_against_model(ctx):
    rng = np.random.default_rng(13)
    index, words = D.fixture()
    w_of = {r['n']: D.span(words, r['w']) for r in index['fft']}
    total = 0
    for n, count in ((2, 30_000), (8, 30_000), (64, 30_000), (256, 10_000), (4096, 200)):
        lens = rng.integers(0, 2 * n, size=count)
        x = _values(rng, count, (count, 2 * n))
        rows = [x[p, :lens[p]] for p in range(count)]
        got = ctx.perform_fft(rows, n, w=w_of[n])
        for p in range(count):
            assert D.same(got[p], D.perform_fft(rows[p], n, w_of[n])), (n, p)
        total += count
    assert total >= 100_000


def test_allocate_bits_random_against_model(ctx):
    rng = np.random.default_rng(14)
    index, words = D.fixture()
    n = 100_000
    for bias, part in zip((0, 1, 2, 3, 4, 5), np.array_split(np.arange(n), 6)):
        m = part.size
        data = _values(rng, m, (m, 52, 20)) * np.exp2(rng.integers(-12, 4, size=(m, 52, 1)))
        sizes = np.where(rng.random((m, 52)) < 0.85, D.SPECS[None, :], rng.choice([0, -5, 1, 20, 25, 60], size=(m, 52)))
        mb = np.where(rng.random(m) < 0.7, 52, rng.integers(0, 53, size=m)).astype(np.int32)
        table = D.table(index, words, bias)
        res = ctx.allocate_bits(data, sizes, mb, biased_table=table)
        for p in range(m):
            count, wl, sfi, fb = D.allocate(list(data[p]), sizes[p], mb[p], table)
            assert res['bfu_count'][p] == count and res['fallback'][p] == fb, (bias, p)
            assert np.array_equal(res['allocation'][p], wl) and np.array_equal(res['scale_factor_indices'][p], sfi), (bias, p)


def test_allocate_bits_composes_to_quantize_frames(ctx):
    import carta1_amd as c1
    checked = 0
    for name, case in EG.cases().items():
        if 'coefficients' not in case or 'nbfu' not in case or 'biased' not in case:
            continue
        coefs, modes = case['coefficients'], case['block_modes']
        bias = case['meta'].get('bias', 1.0)
        fields = ctx.quantize_frames(coefs, modes, c1.EncoderOptions(biased_table=case['biased']))
        frames = coefs.shape[0]
        res = ctx.allocate_bits([D.group_into_bfus(coefs[f], modes[f]) for f in range(frames)], np.tile(D.SPECS, (frames, 1)), 52,
                                biased_table=case['biased'])
        assert np.array_equal(res['bfu_count'], fields['nbfu']) and np.array_equal(fields['nbfu'], case['nbfu']), name
        for f in range(frames):
            k = int(fields['nbfu'][f])
            assert np.array_equal(res['allocation'][f, :k], fields['wl'][f, :k]), (name, f)
            assert np.array_equal(fields['wl'][f, :k], case['wl'][f, :k]), (name, f)
            assert np.array_equal(res['scale_factor_indices'][f, :k], fields['sfi'][f, :k]), (name, f, bias)
        checked += frames
    assert checked > 0


def test_detect_transient_composes_to_select_block_modes(ctx):
    index, words = D.fixture()
    w = {r['n']: D.span(words, r['w']) for r in index['fft']}
    checked = 0
    for name, case in EG.cases().items():
        if case['meta']['kind'] != 'chain' or case['meta']['fixed_block_modes'] is not None:
            continue
        bands = case['bands']
        thr = case['meta']['threshold']
        want = ctx.select_block_modes(bands, thr)
        assert np.array_equal(want, case['block_modes']), name
        prev = [np.zeros(64), np.zeros(64), np.zeros(128)]           # a fresh BufferPool's transientDetection (buffers.js:38-42)
        for f in range(bands.shape[0]):
            spans = ((0, 128), (128, 256), (256, 512))
            mags = [ctx.perform_fft([bands[f, a:b]], b - a, w=w[b - a])[0] for a, b in spans]
            flags, _ = ctx.detect_transient(mags, prev, thr)
            got = [(max(2, b + 1) if flags[b] else 0) for b in range(3)]    # encoder.js:143
            assert got == list(want[f]), (name, f)
            prev = mags
            checked += 1
    assert checked > 0


def test_argument_errors(ctx):
    from carta1_amd import capi
    with pytest.raises(ValueError):
        ctx.perform_fft([np.zeros(4)], 6)
    with pytest.raises(capi.Carta1Error):
        ctx.allocate_bits([[np.zeros(4)]], np.zeros((1, 52)), 53)
