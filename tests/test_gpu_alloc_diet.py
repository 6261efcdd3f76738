"""GPU: the bit-allocation kernels against the oracle's allocateBits (c1o_allocate) on more than 200 000 scale-factor
index vectors, bit for bit -- BFU count, scale-factor indices and all 52 word lengths through Context.quantize_frames, the
chosen candidate through alloc_bounds_device -- at three biases, under a biased table without an integer rank form
(the kernels then look ranks up) and under one whose distortion terms the host cannot tabulate (the kernels then form
them in the reference's order of operations).  c1_alloc_tables says which path a table takes; both fallbacks and the
fast path must be seen.

An index vector is realised as a coefficient frame with one value per BFU just below SCALE_FACTORS[s] (nothing for
s = 0): findScaleFactor (bitallocation.js:290-299) then returns s, which the oracle's own indices confirm."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
from test_alloc_tables_cpu import host_tables

pytestmark = pytest.mark.gpu

SPECS = [8] * 4 + [4] * 4 + [8] * 4 + [6] * 12 + [7] * 4 + [9] * 4 + [10] * 4 + [12] * 8 + [20] * 8
START = np.concatenate([[0], np.cumsum(SPECS)[:-1]])
AMOUNTS = [20, 28, 32, 36, 40, 44, 48, 52]


@pytest.fixture(scope='module')
def ctx():
    import carta1_amd as c1
    c = c1.Context(0)
    yield c
    c.close()


def _below_scale_factor():
    """float32 [64]: the largest binary32 below 2^(s/3 - 21); 0 for s = 0"""
    sf = np.array([O.h2d(h) for h in O.golden_tables()['scale_factors_f64']])
    v = np.nextafter(sf.astype(np.float32), np.float32(0))
    v[0] = 0
    return v


def _vectors(rng, random_units):
    out = [rng.randint(0, 64, size=(random_units, 52))]                                       # anything
    out.append(np.repeat(np.arange(64)[:, None], 52, axis=1))                                 # all equal: all 0 .. all 63
    one = np.zeros((52 * 63, 52), int)
    for b in range(52):
        one[b * 63:(b + 1) * 63, b] = np.arange(1, 64)
    out.append(one)                                                                           # one live BFU
    alt = np.zeros((4, 52), int)
    alt[0, 0::2] = 63; alt[1, 1::2] = 63; alt[2, 0::2] = 63; alt[2, 1::2] = 1; alt[3, 0::4] = 63
    out.append(alt)                                                                           # alternating 0 / 63
    n = random_units // 4
    out.append(np.clip(rng.randint(1, 12, size=(n, 1)) + 3 * rng.randint(0, 18, size=(n, 52)), 0, 63))   # three apart: priorities tie
    out.append(np.clip(rng.randint(20, 50, size=(n, 1)) + rng.randint(-2, 3, size=(n, 52)), 0, 63))      # flat spectra
    tilt = -rng.uniform(0.2, 1.5, size=(n, 1)) * np.arange(52)[None, :]
    out.append(np.clip(rng.randint(40, 63, size=(n, 1)) + tilt + rng.randint(-3, 4, size=(n, 52)), 0, 63).astype(int))   # falling
    out.append(rng.randint(1, 64, size=(n, 52)) * (rng.uniform(size=(n, 52)) < rng.uniform(0.05, 0.9, size=(n, 1))))  # sparse
    out.append(np.clip(60 + rng.randint(0, 4, size=(n, 52)), 0, 63))                          # clipping level
    return np.concatenate(out).astype(np.int32)


def _coefs(vectors):
    c = np.zeros((vectors.shape[0], 512), np.float32)
    c[:, START] = _below_scale_factor()[vectors]
    return c


def _oracle(coefs, table):
    """c1o_allocate per frame: nbfu [n], wl [n, 52], sfi [n, 52]"""
    lib = O.lib()
    n = coefs.shape[0]
    ip = C.POINTER(C.c_int)
    nb, wl, sfi = np.zeros(n, np.int32), np.zeros((n, 52), np.int32), np.zeros((n, 52), np.int32)
    modes = np.zeros(3, np.int32)
    bsf = np.ascontiguousarray(table, np.float64)
    pb, pm = bsf.ctypes.data_as(C.POINTER(C.c_double)), O._ip(modes)
    fp = C.POINTER(C.c_float)
    for f in range(n):
        lib.c1o_allocate(C.cast(coefs.ctypes.data + f * 2048, fp), pm, pb, C.cast(nb.ctypes.data + 4 * f, ip),
                         C.cast(wl.ctypes.data + 208 * f, ip), C.cast(sfi.ctypes.data + 208 * f, ip))
    return nb, wl, sfi


def _check(ctx, coefs, table, what, vectors=None):
    """quantize_frames and the candidate choice of alloc_bounds_device against the oracle on these coefficient frames"""
    import torch
    import carta1_amd as c1
    n = coefs.shape[0]
    nb, wl, sfi = _oracle(coefs, table)
    if vectors is not None:
        assert np.array_equal(sfi, vectors), what                    # the frames realise the index vectors
    opts = c1.EncoderOptions({'fixedBlockModes': [0, 0, 0]}, biased_table=[float(x) for x in table])
    modes = np.zeros((n, 3), np.int32)
    for at in range(0, n, 16384):
        got = ctx.quantize_frames(coefs[at:at + 16384], modes[at:at + 16384], opts)
        for k, want in (('nbfu', nb), ('sfi', sfi), ('wl', wl)):
            w = want[at:at + 16384]
            g = got[k]
            if k != 'nbfu':                                          # entries at or above nBfu are not part of the result
                live = np.arange(52)[None, :] < nb[at:at + 16384, None]
                g, w = np.where(live, g, 0), np.where(live, w, 0)
            bad = np.nonzero((g != w).reshape(len(w), -1).any(axis=1))[0]
            assert bad.size == 0, (what, k, at + bad[:5], g[bad[0]], w[bad[0]])
    side = np.zeros((n, 64), np.uint8)
    side[:, :52] = sfi
    d_side = torch.from_numpy(side).cuda()
    d_out = torch.zeros((n, 16), dtype=torch.float64, device='cuda')
    ctx.alloc_bounds_device(d_side.data_ptr(), n, d_out.data_ptr(), opts)
    ctx.synchronize()
    out = d_out.cpu().numpy()
    tot, choice = out[:, :8], out[:, 15]
    want_choice = np.array([AMOUNTS.index(int(x)) for x in nb])
    bad = np.nonzero(choice != want_choice)[0]
    assert bad.size == 0, (what, 'choice', bad[:5], choice[bad[:5]], want_choice[bad[:5]], tot[bad[0]])
    assert np.array_equal(np.argmin(tot, axis=1), want_choice), what   # and every candidate's total puts it there
    return n


def _defeating_tables():
    rng = np.random.RandomState(5)
    shuffled = np.concatenate([[2.0 ** -21], rng.permutation(2.0 ** (np.arange(1, 64) / 3.0 - 21))])
    tiny = O.biased_table(1.0).copy()
    tiny[1:4] = [2.0 ** -1012, 2.0 ** -1011, 2.0 ** -1010]             # coded terms of these indices are subnormal
    return shuffled, tiny


def test_index_vectors_at_three_biases_and_under_both_fallbacks(ctx):
    rng = np.random.RandomState(20251)
    vectors = _vectors(rng, 36000)
    coefs = _coefs(vectors)
    seen = set()
    total = 0
    for bias in (0.5, 1.0, 2.0):
        table = O.biased_table(bias)
        t = host_tables(table)
        seen.add((t['affine'], t['dist_ok']))
        total += _check(ctx, coefs, table, 'bias %s' % bias, vectors)
    assert (1, 1) in seen                                               # the usual tables take both shortcuts
    shuffled, tiny = _defeating_tables()
    sub = np.concatenate([vectors[:12000], vectors[36000:]])[::2]
    low = sub.copy()
    low[::2] = np.minimum(low[::2], rng.randint(0, 6, size=low[::2].shape))   # many BFUs at the indices whose terms are not tabulated
    for table, name, flags, v in ((shuffled, 'no integer rank form', (0, 1), sub), (tiny, 'terms not tabulated', None, low)):
        t = host_tables(table)
        if flags is not None:
            assert (t['affine'], t['dist_ok']) == flags, name
        else:
            assert t['dist_ok'] == 0, name
        seen.add((t['affine'], t['dist_ok']))
        total += _check(ctx, _coefs(v), table, name, v)
    assert any(a == 0 for a, _ in seen) and any(d == 0 for _, d in seen)   # both fallbacks ran
    assert total >= 200000, total


def test_units_of_real_signals(ctx):
    """white, pink with bursts and stationary partials through the device's own analysis: what encode chose, and
    quantize_frames on the same coefficients, against the oracle's allocateBits"""
    import torch
    import carta1_amd as c1
    frames = 2048
    t = np.arange(frames * 512, dtype=np.float64)
    tone = sum(a * np.sin(2 * np.pi * f * t / 44100 + p) for a, f, p in ((0.3, 220, 0), (0.2, 440, 1), (0.1, 660, 2), (0.05, 1320, .5), (0.02, 3300, .1), (0.01, 7040, .3)))
    shuffled, tiny = _defeating_tables()
    for x in (O.gen_white(1, frames * 512), O.gen_pinkT(3, frames * 512), tone.astype(np.float32)):
        for table in (O.biased_table(0.5), O.biased_table(1.0), O.biased_table(2.0), shuffled, tiny):
            opts = c1.EncoderOptions({'fixedBlockModes': [0, 0, 0]}, biased_table=[float(v) for v in table])
            d_pcm = torch.from_numpy(np.ascontiguousarray(x)).cuda()
            d_coefs = torch.zeros(frames * 512, dtype=torch.float32, device='cuda')
            d_side = torch.zeros(frames * 64, dtype=torch.uint8, device='cuda')
            d_alloc = torch.zeros(frames * 32, dtype=torch.uint8, device='cuda')
            ctx.encode_stages_device([d_pcm.data_ptr()], frames, 0, d_coefs.data_ptr(), d_side.data_ptr(), d_alloc.data_ptr(), opts)
            ctx.synchronize()
            coefs = d_coefs.cpu().numpy().reshape(frames, 512)
            _check(ctx, coefs, table, 'signal')
            nb, wl, _ = _oracle(coefs, table)
            alloc = d_alloc.cpu().numpy().reshape(frames, 32)
            amount = (alloc.view(np.uint32)[:, 7] >> 28) & 7
            assert np.array_equal(np.array(AMOUNTS)[amount], nb)
            nib = np.stack([alloc & 15, alloc >> 4], axis=2).reshape(frames, 64)[:, :52].astype(np.int32)
            live = np.arange(52)[None, :] < nb[:, None]
            assert np.array_equal(np.where(live, nib, 0), np.where(live, wl, 0))
