"""GPU: the single-stage exports -- c1_quantize, c1_dequantize, c1_fft, c1_qmf_analysis_batch, c1_mdct_batch -- against the
reference's own outputs over the whole domain the C entry points accept (tests/golden/export_domain.json + .bin, made by
tests/golden/gen/gen_export_domain.mjs), bit for bit, NaN for NaN:
- quantize / dequantize at every word length 0..32 and at -2^31, -1, 33, 48, 2^31 - 1 (the reference takes the shift count
  of (1 << (bits - 1)) - 1 mod 32: 32 gives the range -2147483649 and crossed clamps), with specials, half-way points and
  products past 2^31 and 2^32;
- FFT.fft at every n = 2^0 .. 2^12 and hashed at 2^14 .. 2^22, with V8's twiddles for every stride, all -0, Inf and NaN;
- qmfAnalysisStage -> mdctStage in all 8 long/short combinations over 64 frames of four streams (white, -0 then white,
  beyond full scale, subnormal), whole and split at frame boundaries with halo frames."""
import hashlib
import time

import numpy as np
import pytest

import export_domain_golden as X

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ctx():
    import carta1_amd as c1
    c = c1.Context(0)
    yield c
    c.close()


@pytest.fixture(scope='module')
def golden():
    return X.load()


def test_quantize_and_dequantize_over_the_domain(ctx, golden):
    index, bin_ = golden
    bad = []
    for sfi, bits, x, q, m, d in X.quantize_cases(index, bin_):
        got = ctx.quantize(x, sfi, bits)
        if not np.array_equal(got, q):
            bad.append(('quantize', sfi, bits, x[got != q][:3], got[got != q][:3], q[got != q][:3]))
        dg = ctx.dequantize(m, sfi, bits)
        ok = X.same_f32(dg, d)
        if not ok.all():
            bad.append(('dequantize', sfi, bits, m[~ok][:3], dg[~ok][:3], d[~ok][:3]))
    assert not bad, (len(bad), bad[:6])


def test_fft_over_every_size(ctx, golden):
    index, bin_ = golden
    seconds = {}
    for v in index['fft']:
        n = v['n']
        re, im = X.hash_noise(v['seed_real'], n, v['amp']), X.hash_noise(v['seed_imag'], n, v['amp'])
        t0 = time.perf_counter()
        ctx.fft(re, im, X.twiddles(index, n))
        seconds[n] = time.perf_counter() - t0
        if 'sha256' in v:
            assert hashlib.sha256(re.astype('<f4').tobytes() + im.astype('<f4').tobytes()).hexdigest() == v['sha256'], n
        else:
            assert X.same_f32(re, X.words(bin_, v['real'], n, np.float32)).all(), n
            assert X.same_f32(im, X.words(bin_, v['imag'], n, np.float32)).all(), n
    assert sorted(seconds) == [1 << k for k in range(13)] + [1 << k for k in range(14, 23, 2)]
    print('c1_fft seconds by n:', {n: round(s, 4) for n, s in seconds.items() if n >= 1 << 14})


def test_fft_of_signed_zeros_and_non_finite_input(ctx, golden):
    index, bin_ = golden
    for v in index['fft_special']:
        n = v['n']
        if v['input'] == 'all -0':
            re, im = np.full(n, -0.0, np.float32), np.full(n, -0.0, np.float32)
        else:
            re, im = X.words(bin_, v['in_real'], n, np.float32), X.words(bin_, v['in_imag'], n, np.float32)
            assert np.isinf(re).any() and np.isnan(im).any()
        ctx.fft(re, im, X.twiddles(index, n))
        assert X.same_f32(re, X.words(bin_, v['real'], n, np.float32)).all(), v['input']
        assert X.same_f32(im, X.words(bin_, v['imag'], n, np.float32)).all(), v['input']


def _modes(run, frames):
    return np.tile(np.array(run['modes'], dtype=np.int32), (frames, 1))


@pytest.mark.parametrize('stream', range(4))
def test_qmf_and_mdct_stages_over_every_mode_combination(ctx, golden, stream):
    index, _ = golden
    s = index['stages'][stream]
    frames = s['frames']
    bands = ctx.qmf_analysis(X.stage_pcm(s))
    assert [X.h16(b) for b in bands] == s['bands_raw'], s['name']
    assert len(s['runs']) == 8
    for run in s['runs']:
        co, bw = ctx.mdct(bands, _modes(run, frames))
        assert [X.h16(c) for c in co] == run['coefficients'], (s['name'], run['modes'])
        assert [X.h16(b) for b in bw] == run['bands_after'], (s['name'], run['modes'])


@pytest.mark.parametrize('stream', range(4))
def test_qmf_and_mdct_split_at_frame_boundaries_equal_the_whole_stream(ctx, golden, stream):
    index, _ = golden
    s = index['stages'][stream]
    frames = s['frames']
    pcm = X.stage_pcm(s)
    bands = ctx.qmf_analysis(pcm)
    for cut in (1, 2, 4, 5, 33, frames - 1):
        for halo in (1, 2):
            h = min(halo, cut)
            tail = ctx.qmf_analysis(pcm[(cut - h) * 512:], halo_frames=h)
            assert np.array_equal(np.concatenate([ctx.qmf_analysis(pcm[:cut * 512]), tail]).view(np.uint32),
                                  bands.view(np.uint32)), (s['name'], cut, halo)
    for run in s['runs'][::3]:
        modes = _modes(run, frames)
        co, bw = ctx.mdct(bands, modes)
        for cut in (1, 4, 5, 33, frames - 1):
            c0, b0 = ctx.mdct(bands[:cut], modes[:cut])
            c1, b1 = ctx.mdct(bands[cut - 1:], modes[cut:], halo_frames=1)
            assert np.array_equal(np.concatenate([c0, c1]).view(np.uint32), co.view(np.uint32)), (s['name'], run['modes'], cut)
            assert np.array_equal(np.concatenate([b0, b1]).view(np.uint32), bw.view(np.uint32)), (s['name'], run['modes'], cut)


def test_quantize_argument_domain(ctx):
    """every int32 bits_per_sample is accepted with the reference's meaning; scale_factor_index outside 0..63 is refused
    (the reference would read SCALE_FACTORS[sfi] as undefined), as is anything that is not an int32"""
    import carta1_amd as c1
    x = np.array([0.5, -0.25, 3.0], dtype=np.float32)
    q = np.array([1, -1, 7], dtype=np.int32)
    for bits in (-2**31, -1, 33, 48, 2**31 - 1):
        ctx.quantize(x, 5, bits)
        ctx.dequantize(q, 5, bits)
    # 33 and 1 share a range of 0 (the shift count is taken mod 32), -1 and 31 one of 2^30 - 1
    assert np.array_equal(ctx.quantize(x, 40, 33), ctx.quantize(x, 40, 1))
    assert np.array_equal(ctx.quantize(x, 40, -1), ctx.quantize(x, 40, 31))
    assert ctx.quantize(x, 40, 32).tolist() == [2147483647] * 3
    for sfi in (-1, 64, 2**31 - 1, -2**31):
        for fn, arg in ((ctx.quantize, x), (ctx.dequantize, q)):
            with pytest.raises(c1.Carta1Error) as e:
                fn(arg, sfi, 8)
            assert e.value.code == 1 and 'scaleFactorIndex' in str(e.value)                  # C1_ERR_ARG
    for sfi, bits in ((5, 2**31), (5, -2**31 - 1), (2**32, 8), (5, 8.0), (5.0, 8), (True, 8), (5, None)):
        for fn, arg in ((ctx.quantize, x), (ctx.dequantize, q)):
            with pytest.raises(ValueError):
                fn(arg, sfi, bits)
    assert ctx.quantize(x, np.int32(40), np.int64(8)).tolist() == ctx.quantize(x, 40, 8).tolist()
