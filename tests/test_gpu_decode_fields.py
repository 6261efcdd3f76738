"""GPU: decode() from frame fields in one launch -- c1_decode_fields_batch / _device (k_decode_fields) and
c1_dec_stream_push_fields -- against the reference's decode() PCM (tests/golden/decoder_stages.json), the CPU oracle on random
fields no encoder writes, the three-stage chain, the unit decoder on every KAT file, itself split at run and call seams, and
streams that mix unit and field pushes.  Every comparison is bit for bit on the uint32 views."""
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
PER = {'nbfu': 1, 'block_modes': 3, 'sfi': 52, 'wl': 52, 'quantized': 512}


@pytest.fixture(scope='module')
def ctx():
    import carta1_amd as c1
    c = c1.Context(0)
    yield c
    c.close()


def same(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def cat(*parts):
    return {k: np.concatenate([np.asarray(p[k]).reshape(-1, PER[k]) for p in parts]).reshape((-1,) + (() if PER[k] == 1 else (PER[k],)))
            for k in DG.FIELDS}


def sub(fields, start, stop):
    return {k: np.ascontiguousarray(np.asarray(v)[start:stop]) for k, v in fields.items()}


def random_fields(frames, seed):
    # as tests/test_gpu_decoder_stages.py draws them: any nBfu 0..52, modes beyond the short codes, wide and extreme
    # mantissas, junk above nBfu
    rng = np.random.default_rng(seed)
    nbfu = rng.integers(0, 53, frames).astype(np.int32)
    modes = rng.choice(np.array([0, 0, 0, 1, 2, 3, -1, 7], dtype=np.int32), (frames, 3))
    wl = rng.integers(0, 16, (frames, 52)).astype(np.int32)
    wl[rng.random((frames, 52)) < 0.25] = 0
    sfi = rng.integers(0, 64, (frames, 52)).astype(np.int32)
    unread = np.arange(52)[None, :] >= nbfu[:, None]
    wl[unread] = 99
    sfi[unread] = -5
    q = rng.integers(-(1 << 31), 1 << 31, (frames, 512), dtype=np.int64)
    small = rng.random((frames, 512)) < 0.6
    q[small] = rng.integers(-40000, 40000, int(small.sum()))
    return {'nbfu': nbfu, 'block_modes': modes, 'sfi': sfi, 'wl': wl, 'quantized': q.astype(np.int32)}


def oracle_decode(fields):
    frames = fields['nbfu'].size
    packed = np.ascontiguousarray(np.concatenate([fields['nbfu'][:, None], fields['block_modes'], fields['wl'], fields['sfi'],
                                                  fields['quantized']], axis=1).astype(np.int32))
    assert packed.shape[1] * 4 == C.sizeof(O.Fields)
    ref = np.zeros((frames, 512), dtype=np.float32)
    st = O.DecState()
    lib, base, out = O.lib(), packed.ctypes.data, ref.ctypes.data
    for f in range(frames):
        lib.c1o_decode_frame(C.byref(st), C.cast(base + f * 2480, C.POINTER(O.Fields)), C.cast(out + f * 2048, C.POINTER(C.c_float)))
    return ref


def kat_units(path):
    return np.fromfile(path, dtype=np.uint8).reshape(-1, 2, 212)


def mixed_stream(ctx):
    # 64 frames with short and long bands mixed from frame to frame, then the hand-built fields: 76 frames, several runs
    units = kat_units(os.path.join(G, 'kat64_pinkT_detect_thr0.3.units.bin'))
    return cat(ctx.unpack_units(np.ascontiguousarray(units[:, 0])), DG.fields_of(CASES['fields']))


@pytest.mark.parametrize('name', sorted(CASES))
def test_cases_against_reference(ctx, name):
    case = CASES[name]
    pcm = ctx.decode_fields(DG.fields_of(case))
    assert len(pcm) == 1
    assert same(pcm[0].reshape(-1, 512), case['pcm'])


def test_random_noncanonical_fields_against_oracle_and_chain(ctx):
    fields = random_fields(100_000, 11)
    pcm = ctx.decode_fields(fields)[0].reshape(-1, 512)
    chain = ctx.qmf_synthesis(ctx.imdct(ctx.dequantize_frames(fields), fields['block_modes']))
    assert same(pcm, chain)
    ref = oracle_decode(fields)
    bad = np.nonzero((pcm.view(np.uint32) != ref.view(np.uint32)).any(axis=1))[0]
    assert bad.size == 0, 'first differing frame %d of %d' % (bad[0], bad.size)


@pytest.mark.parametrize('path', KAT_FILES, ids=[os.path.basename(p) for p in KAT_FILES])
def test_unpacked_units_equal_unit_decode(ctx, path):
    units = kat_units(path)
    inter = np.ascontiguousarray(units.reshape(-1, 212))
    stereo = ctx.decode(inter, 2)
    got = ctx.decode_fields(ctx.unpack_units(inter), channels=2)
    for c in range(2):
        assert same(got[c], stereo[c]), 'stereo channel %d' % c
        mono_units = np.ascontiguousarray(units[:, c])
        assert same(ctx.decode_fields(ctx.unpack_units(mono_units))[0], ctx.decode(mono_units, 1)[0]), 'mono channel %d' % c


def test_split_with_halo_equals_one_call(ctx):
    fields = mixed_stream(ctx)
    n = fields['nbfu'].size
    assert n > 64
    whole = ctx.decode_fields(fields)[0]
    for k in (1, 2, 5, 31, 64, 65, n - 1):
        a = ctx.decode_fields(sub(fields, 0, k))[0]
        b = ctx.decode_fields(sub(fields, k - 1, n), halo_frames=1)[0]
        assert same(np.concatenate([a, b]), whole), 'split at %d' % k
    # stereo: the mixed stream and its reverse interleaved, split with a halo of one frame per channel
    other = {k: np.ascontiguousarray(v[::-1]) for k, v in fields.items()}
    inter = {k: np.ascontiguousarray(np.stack([fields[k], other[k]], axis=1).reshape((2 * n,) + fields[k].shape[1:])) for k in fields}
    st = ctx.decode_fields(inter, channels=2)
    assert same(st[0], whole) and same(st[1], ctx.decode_fields(other)[0])
    for k in (1, 33, n - 1):
        a = ctx.decode_fields(sub(inter, 0, 2 * k), channels=2)
        b = ctx.decode_fields(sub(inter, 2 * (k - 1), 2 * n), channels=2, halo_frames=1)
        for c in range(2):
            assert same(np.concatenate([a[c], b[c]]), st[c]), 'stereo split at %d, channel %d' % (k, c)


def _unit_pool(ctx):
    units = np.concatenate([kat_units(p).reshape(-1, 212) for p in KAT_FILES])      # canonical units, 1 408 of them
    return units, ctx.unpack_units(units)


@pytest.mark.parametrize('channels', [1, 2])
@pytest.mark.parametrize('kinds,sizes', [('UFUFU', (1, 3, 64, 1, 200)), ('FUFUF', (1, 3, 64, 1, 200)),
                                         ('UUFFUUF', (5, 7, 3, 70, 2, 1, 9)), ('FFFU', (2, 130, 1, 4))])
def test_stream_mixing_unit_and_field_pushes(ctx, channels, kinds, sizes):
    import carta1_amd as c1
    units, unit_fields = _unit_pool(ctx)
    rnd = random_fields(2 * sum(sizes), 5 + len(kinds))
    s = c1.DecoderStream(ctx, channels)
    parts, outs, u_at, r_at = [], [], 0, 0
    for kind, n in zip(kinds, sizes):
        m = n * channels
        if kind == 'U':
            parts.append(sub(unit_fields, u_at, u_at + m))
            outs.append(s.push(units[u_at:u_at + m]))
            u_at += m
        else:
            f = sub(rnd, r_at, r_at + m)
            parts.append(f)
            outs.append(s.push_fields(f))
            r_at += m
    s.close()
    want = ctx.decode_fields(cat(*parts), channels=channels)
    for c in range(channels):
        assert same(np.concatenate([o[c] for o in outs]), want[c]), 'channel %d' % c


def test_decode_precision_does_not_apply(ctx):
    import carta1_amd as c1
    fields = cat(mixed_stream(ctx), random_fields(3000, 3))
    want = ctx.decode_fields(fields)[0]
    c32 = c1.Context(0)
    try:
        c32.set_decode_precision(1)
        assert same(c32.decode_fields(fields)[0], want)
        s = c1.DecoderStream(c32, 1)
        got = np.concatenate([s.push_fields(sub(fields, 0, 100))[0], s.push_fields(sub(fields, 100, fields['nbfu'].size))[0]])
        s.close()
        assert same(got, want)
    finally:
        c32.close()


@pytest.mark.parametrize('channels,halo', [(1, 0), (1, 1), (2, 0), (2, 1)])
def test_device_entry_equals_batch(ctx, channels, halo):
    import torch
    fields = cat(mixed_stream(ctx), random_fields(500, 17 + channels))
    units = fields['nbfu'].size // channels * channels
    fields = sub(fields, 0, units)
    frames = units // channels - halo
    want = ctx.decode_fields(fields, channels=channels, halo_frames=halo)
    dev = {k: torch.from_numpy(np.ascontiguousarray(fields[k])).to('cuda:0') for k in DG.FIELDS}
    pcm = [torch.empty(frames * 512, dtype=torch.float32, device='cuda:0') for _ in range(channels)]
    ptrs = [dev[k].data_ptr() + 4 * PER[k] * halo * channels for k in DG.FIELDS]
    ctx.decode_fields_device(ptrs, channels, frames, [p.data_ptr() for p in pcm], halo_frames=halo)
    ctx.synchronize()
    for c in range(channels):
        assert same(pcm[c].cpu().numpy(), want[c]), 'channel %d' % c


def test_kernel_time_is_reported(ctx):
    ctx.set_profiling(True)
    try:
        ctx.decode_fields(random_fields(64, 1))
        ms, launches = ctx.kernel_ms('decode_fields')
    finally:
        ctx.set_profiling(False)
    assert launches == 1 and ms > 0


def test_bad_arguments(ctx):
    import carta1_amd as c1
    from carta1_amd import capi
    lib, h = capi.load(), ctx._h

    def code(fn):
        with pytest.raises(capi.Carta1Error) as e:
            fn()
        return e.value.code, str(e.value)

    good = DG.fields_of(CASES['fields'], 2, 5)           # nBfu 52, 7, 21
    b = int(good['nbfu'][1]) - 1
    for key, value, word in (('wl', 16, 'word length index 16 outside 0..15'), ('sfi', 64, 'scale factor index 64 outside 0..63'),
                             ('wl', -1, 'word length index -1'), ('sfi', -1, 'scale factor index -1')):
        f = {k: v.copy() for k, v in good.items()}
        f[key][1, b] = value
        rc, msg = code(lambda: ctx.decode_fields(f))
        assert rc == 1 and ('frame 1 BFU %d: %s' % (b, word)) in msg, msg
        s = c1.DecoderStream(ctx, 1)
        rc, msg2 = code(lambda: s.push_fields(f))
        s.close()
        assert rc == 1 and ('frame 1 BFU %d: %s' % (b, word)) in msg2, msg2
    for n in (-1, 53):
        f = {k: v.copy() for k, v in good.items()}
        f['nbfu'][2] = n
        rc, msg = code(lambda: ctx.decode_fields(f))
        assert rc == 1 and 'frame 2: nBfu %d outside 0..52' % n in msg, msg
    # the halo is validated too, and named frame -1; stereo names the channel
    f = {k: v.copy() for k, v in good.items()}
    f['wl'][0, 0] = 16
    assert 'frame -1 BFU 0' in code(lambda: ctx.decode_fields(f, halo_frames=1))[1]
    two = {k: v.copy() for k, v in DG.fields_of(CASES['fields'], 2, 6).items()}
    two['sfi'][3, 0] = 64
    assert 'frame 1 channel 1 BFU 0' in code(lambda: ctx.decode_fields(two, channels=2))[1]
    # junk at and above nBfu is accepted and ignored
    f = {k: v.copy() for k, v in good.items()}
    want = ctx.decode_fields(f)[0]
    above = np.arange(52)[None, :] >= f['nbfu'][:, None]
    f['wl'][above] = 99
    f['sfi'][above] = -7
    assert same(ctx.decode_fields(f)[0], want)
    # halo, channels, frames and NULL pointers
    ok = [v.ctypes.data for v in (good[k] for k in DG.FIELDS)]
    out = np.zeros(3 * 512, dtype=np.float32)
    pcm = capi.ptr_array([out.ctypes.data])
    for halo in (-1, 2):
        assert code(lambda: capi.check(lib.c1_decode_fields_batch(h, 1, 1, halo, *ok, pcm)))[0] == 1
        assert code(lambda: capi.check(lib.c1_decode_fields_device(h, 1, 1, halo, *ok, pcm)))[0] == 1
    assert code(lambda: capi.check(lib.c1_decode_fields_batch(h, 3, 1, 0, *ok, pcm)))[0] == 1
    assert code(lambda: capi.check(lib.c1_decode_fields_batch(h, 1, (1 << 20) + 1, 0, *ok, pcm)))[0] == 1
    assert code(lambda: capi.check(lib.c1_decode_fields_batch(h, 1, -1, 0, *ok, pcm)))[0] == 1
    for i in range(5):
        args = list(ok)
        args[i] = None
        assert code(lambda: capi.check(lib.c1_decode_fields_batch(h, 1, 3, 0, *args, pcm)))[0] == 1
        assert code(lambda: capi.check(lib.c1_decode_fields_device(h, 1, 3, 0, *args, pcm)))[0] == 1
    assert code(lambda: capi.check(lib.c1_decode_fields_batch(h, 1, 3, 0, *ok, None)))[0] == 1
    assert code(lambda: capi.check(lib.c1_decode_fields_batch(h, 1, 3, 0, *ok, capi.ptr_array([0]))))[0] == 1
    assert code(lambda: capi.check(lib.c1_dec_stream_push_fields(None, 3, *ok, pcm)))[0] == 1
    # frames == 0 writes nothing and succeeds
    capi.check(lib.c1_decode_fields_batch(h, 1, 0, 0, *ok, pcm))
