"""GPU: c1_pack_units (serializeFrame) through Context.pack_units against the reference's own units
(tests/golden/pack_units.json), at the end of the encoder's stage chain against the committed KAT units, as the inverse of
c1_unpack_units both ways, against the NumPy model on random frames from the whole int32 domain, split against whole, and
its argument errors.  Every comparison is byte for byte."""
import ctypes as C
import glob
import json
import os

import numpy as np
import pytest

import oracle_lib as O
import pack_units_model as M

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
CASES = M.cases()
KAT = json.load(open(os.path.join(G, 'kat_index.json')))
KAT_FILES = sorted(glob.glob(os.path.join(G, 'kat64_*.units.bin')))


@pytest.fixture(scope='module')
def ctx():
    import carta1_amd as c1
    c = c1.Context(0)
    yield c
    c.close()


def assert_units(got, want, what=''):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.uint8 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, '%s: first differing frame %d of %d (byte %d)' % (
        what, bad[0], bad.size, np.nonzero(got[bad[0]] != want[bad[0]])[0][0])


def assert_fields(got, want, what=''):
    for k in M.FIELDS:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w.shape, (what, k, g.shape, w.shape)
        bad = np.nonzero((g != w).reshape(g.shape[0], -1).any(axis=1))[0]
        assert bad.size == 0, '%s %s: first differing frame %d of %d' % (what, k, bad[0], bad.size)


def kat_units():
    return np.concatenate([np.fromfile(p, dtype=np.uint8).reshape(-1, 212) for p in KAT_FILES])


# ---- the fixture --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', sorted(CASES))
def test_pack_units_against_reference(ctx, name):
    case = CASES[name]
    assert_units(ctx.pack_units(M.fields_of(case)), case['units'], name)


# ---- composition --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('path', KAT_FILES, ids=[os.path.basename(p) for p in KAT_FILES])
def test_encoder_stage_chain_packs_the_committed_units(ctx, path):
    import carta1_amd as c1
    name = os.path.basename(path)[len('kat64_'):-len('.units.bin')]
    meta = KAT[name]
    opts = dict(meta['options'])
    units = np.fromfile(path, dtype=np.uint8).reshape(-1, 2, 212)
    frames = units.shape[0]
    gen = O.gen_white if meta['signal'] == 'white' else O.gen_pinkT
    o = c1.EncoderOptions(opts)
    for c in range(2):
        bands = ctx.qmf_analysis(gen(meta['seeds'][c], frames * 512))
        fixed = opts.get('fixedBlockModes')
        modes = np.tile(np.array(fixed, np.int32), (frames, 1)) if fixed else \
            ctx.select_block_modes(bands, opts.get('transientThresholdLow', 1.0))
        coefs, _ = ctx.mdct(bands, modes)
        fields = ctx.quantize_frames(coefs, modes, o)
        got = ctx.pack_units(fields)
        assert_units(got, units[:, c], '%s channel %d' % (name, c))
        assert_fields(ctx.unpack_units(got), fields, '%s channel %d round trip' % (name, c))


def test_pack_of_unpack_is_the_canonical_unit(ctx):
    r = np.random.default_rng(5)
    rand = r.integers(0, 256, size=(24000, 212), dtype=np.uint8)
    # every BFU amount and every header bit pattern among them; short streams (word lengths 0) too
    rand[:256, 0] = np.arange(256)
    rand[256:512, 1] = np.arange(256)
    rand[512:2000, 2:30] &= 0x11
    for units, what in ((kat_units(), 'KAT units'), (rand, 'random units')):
        want = units & M.canonical_mask(units)
        assert_units(ctx.pack_units(ctx.unpack_units(units)), want, what)
    assert np.array_equal(kat_units() & M.canonical_mask(kat_units()), kat_units())


@pytest.mark.parametrize('name', sorted(k for k, v in CASES.items() if v['meta']['kind'] == 'canonical'))
def test_unpack_of_pack_is_the_fields(ctx, name):
    f = M.fields_of(CASES[name])
    assert_fields(ctx.unpack_units(ctx.pack_units(f)), f, name)


# ---- the whole int32 domain ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize('seed', [1, 2])
def test_random_fields_against_model(ctx, seed):
    f = M.random_fields(12000, seed)
    if seed == 1:                                  # edge values in every field of the first frames
        e = M.EDGES.astype(np.int32)
        for i in range(e.size):
            f['block_modes'][i] = [e[i], e[(i + 5) % e.size], e[(i + 11) % e.size]]
            f['wl'][e.size + i] = e[i]
            f['sfi'][2 * e.size + i] = e[i]
            f['quantized'][3 * e.size + i] = e[i]
        f['nbfu'][e.size:4 * e.size] = 52
    assert_units(ctx.pack_units(f), M.pack(f), 'seed %d' % seed)


def test_split_equals_whole(ctx):
    f = M.random_fields(3000, 9)
    whole = ctx.pack_units(f)
    for cuts in ([1], [63, 64, 65], [1000, 1001, 2999], [7, 500, 1500, 2500]):
        parts, at = [], 0
        for b in cuts + [3000]:
            parts.append(ctx.pack_units({k: v[at:b] for k, v in f.items()}))
            at = b
        assert_units(np.concatenate(parts), whole, 'cuts %s' % cuts)


# ---- arguments ----------------------------------------------------------------------------------------------------------

def test_bad_arguments_and_empty_calls(ctx):
    from carta1_amd import capi
    lib, h = capi.load(), ctx._h

    def code(fn):
        with pytest.raises(capi.Carta1Error) as e:
            fn()
        return e.value.code

    f = M.fields_of(CASES['kat_pinkT_detect'], 0, 2)
    for bad in (53, -1, -2 ** 31):
        g = {k: v.copy() for k, v in f.items()}
        g['nbfu'][1] = bad
        with pytest.raises(capi.Carta1Error) as e:
            ctx.pack_units(g)
        assert e.value.code == 1 and 'nBfu %d' % bad in str(e.value), str(e.value)
    p = [f[k].ctypes.data for k in M.FIELDS]
    out = np.zeros((2, 212), np.uint8)
    for frames in (-1, (1 << 20) + 1):
        assert code(lambda: capi.check(lib.c1_pack_units(h, frames, *p, out.ctypes.data))) == 1
    for i in range(6):
        args = p + [out.ctypes.data]
        args[i] = None
        assert code(lambda: capi.check(lib.c1_pack_units(h, 2, *args))) == 1
    # frames == 0: nothing is read or written
    sentinel = np.full(212, 7, np.uint8)
    capi.check(lib.c1_pack_units(h, 0, None, None, None, None, None, sentinel.ctypes.data))
    assert (sentinel == 7).all()
    assert ctx.pack_units({k: np.zeros((0,) + s, np.int32) for k, s in ctx.FIELD_SHAPES}).shape == (0, 212)
    with pytest.raises(ValueError):
        ctx.pack_units({**f, 'wl': f['wl'][:, :51]})
