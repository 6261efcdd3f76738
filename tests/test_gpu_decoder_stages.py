"""GPU: the decoder's pipeline stages through the C ABI -- c1_unpack_units (deserializeFrame), c1_dequantize_frames
(dequantizationStage), c1_imdct_batch (imdctStage), c1_qmf_synthesis_batch (qmfSynthesisStage) -- against the reference's
own stage outputs (tests/golden/decoder_stages.json), composed against c1_decode_batch, split against whole, and on random
frame fields no encoder writes against the CPU oracle.  Every comparison is bit for bit on the uint32 views."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

import decoder_stages_golden as DG
import oracle_lib as O

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
CASES = DG.cases()
KAT_FILES = sorted(glob.glob(os.path.join(G, 'kat64_*.units.bin')))


@pytest.fixture(scope='module')
def ctx():
    import carta1_amd as c1
    c = c1.Context(0)
    yield c
    c.close()


def same(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def chain(ctx, units):
    fields = ctx.unpack_units(units)
    coefs = ctx.dequantize_frames(fields)
    bands = ctx.imdct(coefs, fields['block_modes'])
    return ctx.qmf_synthesis(bands)


@pytest.mark.parametrize('name', ['pinkT_detect', 'white_m000_b1'])
def test_unpack_units_against_reference(ctx, name):
    case = CASES[name]
    got = ctx.unpack_units(case['units'])
    for k in DG.FIELDS:
        assert np.array_equal(got[k], case[k]), k


@pytest.mark.parametrize('name', sorted(CASES))
def test_each_stage_against_reference(ctx, name):
    case = CASES[name]
    coefs = ctx.dequantize_frames(DG.fields_of(case))
    assert same(coefs, case['coefficients'])
    bands = ctx.imdct(case['coefficients'], case['block_modes'])
    assert same(bands, case['bands'])
    pcm = ctx.qmf_synthesis(case['bands'])
    assert same(pcm, case['pcm'])


@pytest.mark.parametrize('path', KAT_FILES, ids=[os.path.basename(p) for p in KAT_FILES])
def test_chain_equals_decode_batch(ctx, path):
    units = np.fromfile(path, dtype=np.uint8).reshape(-1, 2, 212)
    stereo = ctx.decode(np.ascontiguousarray(units.reshape(-1, 212)), 2)
    for c in range(2):
        mono_units = np.ascontiguousarray(units[:, c])
        pcm = chain(ctx, mono_units).reshape(-1)
        assert same(pcm, stereo[c]), 'channel %d vs stereo decode' % c
        assert same(pcm, ctx.decode(mono_units, 1)[0]), 'channel %d vs mono decode' % c


def _mixed_stream(ctx):
    # 64 frames with short and long bands mixed from frame to frame, then the hand-built fields
    units = np.fromfile(os.path.join(G, 'kat64_pinkT_detect_thr0.3.units.bin'), dtype=np.uint8).reshape(-1, 2, 212)
    f = ctx.unpack_units(np.ascontiguousarray(units[:, 0]))
    g = DG.fields_of(CASES['fields'])
    return {k: np.concatenate([f[k], g[k]]) for k in DG.FIELDS}


def test_split_with_halo_equals_one_call(ctx):
    fields = _mixed_stream(ctx)
    coefs = ctx.dequantize_frames(fields)
    modes = fields['block_modes']
    bands = ctx.imdct(coefs, modes)
    pcm = ctx.qmf_synthesis(bands)
    n = coefs.shape[0]
    for k in (1, 2, 5, 31, 64, 65, n - 1):
        b2 = np.concatenate([ctx.imdct(coefs[:k], modes[:k]), ctx.imdct(coefs[k - 1:], modes[k - 1:], halo_frames=1)])
        assert same(b2, bands), 'imdct split at %d' % k
        p2 = np.concatenate([ctx.qmf_synthesis(bands[:k]), ctx.qmf_synthesis(bands[k - 1:], halo_frames=1)])
        assert same(p2, pcm), 'synthesis split at %d' % k


def _random_fields(frames, seed):
    rng = np.random.default_rng(seed)
    nbfu = rng.integers(0, 53, frames).astype(np.int32)
    modes = rng.choice(np.array([0, 0, 0, 1, 2, 3, -1, 7], dtype=np.int32), (frames, 3))
    wl = rng.integers(0, 16, (frames, 52)).astype(np.int32)
    wl[rng.random((frames, 52)) < 0.25] = 0
    sfi = rng.integers(0, 64, (frames, 52)).astype(np.int32)
    unread = np.arange(52)[None, :] >= nbfu[:, None]            # entries at or above nBfu are not read
    wl[unread] = 99
    sfi[unread] = -5
    q = rng.integers(-(1 << 31), 1 << 31, (frames, 512), dtype=np.int64)
    small = rng.random((frames, 512)) < 0.6
    q[small] = rng.integers(-40000, 40000, int(small.sum()))
    return {'nbfu': nbfu, 'block_modes': modes, 'sfi': sfi, 'wl': wl, 'quantized': q.astype(np.int32)}


def test_random_noncanonical_fields_against_oracle(ctx):
    frames = 100_000
    fields = _random_fields(frames, 7)
    pcm = ctx.qmf_synthesis(ctx.imdct(ctx.dequantize_frames(fields), fields['block_modes']))
    # c1o_fields is nbfu, modes[3], wl[52], sfi[52], q[512]: 620 ints
    packed = np.concatenate([fields['nbfu'][:, None], fields['block_modes'], fields['wl'], fields['sfi'], fields['quantized']],
                            axis=1).astype(np.int32)
    assert packed.shape[1] * 4 == C.sizeof(O.Fields)
    packed = np.ascontiguousarray(packed)
    ref = np.zeros((frames, 512), dtype=np.float32)
    st = O.DecState()
    lib, base, out = O.lib(), packed.ctypes.data, ref.ctypes.data
    for f in range(frames):
        lib.c1o_decode_frame(C.byref(st), C.cast(base + f * 2480, C.POINTER(O.Fields)), C.cast(out + f * 2048, C.POINTER(C.c_float)))
    bad = np.nonzero((pcm.view(np.uint32) != ref.view(np.uint32)).any(axis=1))[0]
    assert bad.size == 0, 'first differing frame %d of %d' % (bad[0], bad.size)


def test_bad_arguments(ctx):
    from carta1_amd import capi
    lib, h = capi.load(), ctx._h
    coefs = np.zeros((2, 512), dtype=np.float32)
    modes = np.zeros((2, 3), dtype=np.int32)
    out = np.zeros((2, 512), dtype=np.float32)

    def code(fn):
        with pytest.raises(capi.Carta1Error) as e:
            fn()
        return e.value.code

    for halo in (-1, 2):
        assert code(lambda: ctx.imdct(coefs, modes, halo_frames=halo)) == 1
        assert code(lambda: ctx.qmf_synthesis(coefs, halo_frames=halo)) == 1
    good = DG.fields_of(CASES['fields'], 2, 3)
    for key, value in (('wl', 16), ('sfi', 64), ('wl', -1), ('sfi', -1)):
        f = {k: v.copy() for k, v in good.items()}
        b = int(np.nonzero(np.arange(52) < f['nbfu'][0])[0][-1])
        f[key][0, b] = value
        assert code(lambda: ctx.dequantize_frames(f)) == 1, key
    for n in (-1, 53):
        f = {k: v.copy() for k, v in good.items()}
        f['nbfu'][0] = n
        assert code(lambda: ctx.dequantize_frames(f)) == 1
    big = (1 << 20) + 1
    p = out.ctypes.data
    assert code(lambda: capi.check(lib.c1_unpack_units(h, p, big, p, p, p, p, p))) == 1
    assert code(lambda: capi.check(lib.c1_dequantize_frames(h, big, p, p, p, p, p, p))) == 1
    assert code(lambda: capi.check(lib.c1_imdct_batch(h, p, big, 0, p, p))) == 1
    assert code(lambda: capi.check(lib.c1_qmf_synthesis_batch(h, p, big, 0, p))) == 1
    assert code(lambda: capi.check(lib.c1_unpack_units(h, None, 1, p, p, p, p, p))) == 1
    assert code(lambda: capi.check(lib.c1_unpack_units(h, p, 1, p, p, p, p, None))) == 1
    assert code(lambda: capi.check(lib.c1_dequantize_frames(h, 1, p, None, p, p, p, p))) == 1
    assert code(lambda: capi.check(lib.c1_imdct_batch(h, p, 1, 0, None, p))) == 1
    assert code(lambda: capi.check(lib.c1_imdct_batch(h, p, 1, 0, p, None))) == 1
    assert code(lambda: capi.check(lib.c1_qmf_synthesis_batch(h, None, 1, 0, p))) == 1
    assert code(lambda: capi.check(lib.c1_qmf_synthesis_batch(h, p, 1, 0, None))) == 1
