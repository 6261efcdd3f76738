"""GPU: encode with the allocation bias supplied per frame and channel from a palette (c1_encode_biases_device / _batch,
c1_enc_stream_push_biases).  The reference's own bias schedule; random per-unit schedules over the eight packaged biases
against the CPU oracle, with given modes, under detection and under fixed modes; palettes that mix the table forms of the
allocation kernels; degenerate palettes; the geometry of the unit lists, up to one longer than the bounded grid of list-mode
allocation; independence of chunking, pipeline, speculation and halo; one stream through every schedule of
tests/golden/option_changes.json with the bias given through the pushes alone; what the entry points reject; index bytes
outside the palette on the device entry point; and the order on a caller's stream.
The random schedules run on pink noise with transients: tests/test_bias_palette_cpu.py shows that every pair of the packaged
biases differs there in at least three quarters of the units, so a unit allocated under a wrong entry fails these tests."""
import ctypes as C
import os

import numpy as np
import pytest

import carta1_amd as c1
from carta1_amd import capi, codec
import bias_palette_lib as BP
import block_modes_lib as BM
import oracle_lib as O
import option_changes_lib as OC
import option_domain_lib as L
import stream_state_lib as SL
from test_alloc_tables_cpu import host_tables

pytestmark = pytest.mark.gpu

C1_OK, C1_ERR_ARG = 0, 1   # include/carta1_hip.h
FIX = OC.fixture()
CASES = [(name, sig) for name, s in FIX['schedules'].items() for sig in s['results']]
R_FRAMES = 130
COUNTS = (1, 2, 3, 63, 64, 65, 130, 257)          # one wave of the sorting kernel, its seams, more than one 256-unit block
BIASES = list(BP.PACKAGED_BIASES)


def opts(v=None, table=None):
    return c1.EncoderOptions(v or {}, biased_table=None if table is None else [float(x) for x in table])


@pytest.fixture(scope='module')
def ctx():
    c = c1.Context(0)
    yield c
    c.close()


def _context(stream=None, **env_vars):
    old = {k: os.environ.get(k) for k in env_vars}
    os.environ.update({k: str(v) for k, v in env_vars.items()})
    try:
        return c1.Context(0, stream=stream)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


@pytest.fixture(scope='module')
def random_case():
    """stereo pink noise with transients, 130 frames, the eight packaged biases, each channel on its own index schedule;
    the oracle's units with random modes over the whole domain, under detection and under fixed modes [2,0,3]: computed once,
    shared, never written"""
    chans = [O.gen_pinkT(3, (R_FRAMES + 2) * 512), O.gen_pinkT(4, (R_FRAMES + 2) * 512)]
    body = [c[2 * 512:] for c in chans]
    index = BP.random_index(20261018, R_FRAMES, 2, 8)
    assert set(index.reshape(-1).tolist()) == set(range(8)) and (index[:, 0] != index[:, 1]).any()
    modes = BM.random_modes(20261019, R_FRAMES, 2)
    assert set(modes.reshape(-1).tolist()) == set(BM.DOMAIN_BYTES)
    fixed = {'fixedBlockModes': [2, 0, 3]}
    want = {'modes': BP.oracle_encode_schedule(body, BIASES, index, modes)[0],
            'detect': BP.oracle_encode_schedule(body, BIASES, index, None, {})[0],
            'fixed': BP.oracle_encode_schedule(body, BIASES, index, None, fixed)[0]}
    assert BP.differing_units(want['modes'], want['detect']) and BP.differing_units(want['fixed'], want['detect'])
    return {'with_halo': chans, 'chans': body, 'index': index, 'biases': np.array(BIASES)[index], 'modes': modes, 'fixed': fixed, 'want': want}


def dev_encode_biases(ctx, dev, frames, palette_options, index, modes=None, halo=0):
    """c1_encode_biases_device on torch buffers: dev = per-channel tensors that start `halo` frames before frame 0"""
    import torch
    nch = len(dev)
    up = lambda a: a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8).reshape(-1).copy()).cuda()
    d_index = up(index)
    d_modes = None if modes is None else up(modes)
    units = torch.zeros(frames * nch * 212, dtype=torch.uint8, device='cuda')
    torch.cuda.synchronize()
    ctx.encode_biases_device([d.data_ptr() + halo * 2048 for d in dev], frames, palette_options, d_index.data_ptr(), units.data_ptr(),
                             None if d_modes is None else d_modes.data_ptr(), halo_frames=halo)
    ctx.synchronize()
    return units.cpu().numpy().reshape(-1, 212)


def first_bad(got, want):
    return np.flatnonzero((got != want).any(axis=1))[:4]


# ---- 1. the reference's own bias schedule ----
@pytest.mark.parametrize('sig', list(FIX['schedules']['bias_fixed000']['results']))
def test_reference_bias_schedule(ctx, sig):
    import torch
    s = FIX['schedules']['bias_fixed000']
    frames = FIX['frames']
    chans = OC.signal(FIX['signals'][sig], frames)
    nch = len(chans)
    per_frame = OC.options_at(s['initial'], s['changes'], frames)
    biases = np.array([v['allocationBias'] for v in per_frame])
    assert sorted(set(biases.tolist())) == [0.5, 1.0, 2.0]
    got = ctx.encode_biases(chans, biases, options=opts({'fixedBlockModes': [0, 0, 0]}))
    assert OC.check_against(s['results'][sig], got, nch) is None
    got = ctx.encode_biases(chans, biases, modes=np.zeros((frames, nch), dtype=np.uint8))
    assert OC.check_against(s['results'][sig], got, nch) is None
    values, index = BP.palette_of(np.repeat(biases[:, None], nch, axis=1))
    dev = [torch.from_numpy(c).cuda() for c in chans]
    got = dev_encode_biases(ctx, dev, frames, [opts({'allocationBias': b, 'fixedBlockModes': [0, 0, 0]}) for b in values], index)
    assert OC.check_against(s['results'][sig], got, nch) is None


# ---- 2. random per-unit schedules over the eight packaged biases against the oracle ----
@pytest.mark.parametrize('kind', ['modes', 'detect', 'fixed'])
def test_random_schedule_matches_oracle(ctx, random_case, kind):
    r = random_case
    got = ctx.encode_biases(r['chans'], r['biases'], modes=r['modes'] if kind == 'modes' else None,
                            options=opts(r['fixed']) if kind == 'fixed' else None)
    assert np.array_equal(got, r['want'][kind]), first_bad(got, r['want'][kind])
    if kind == 'modes':     # threshold and fixed modes of the entries are not read, and need not agree
        import torch
        pal = [opts({'allocationBias': b, 'transientThresholdLow': 0.3 + 0.1 * k, 'fixedBlockModes': [2, 0, 3] if k & 1 else None}) for k, b in enumerate(BIASES)]
        dev = [torch.from_numpy(c).cuda() for c in r['chans']]
        assert np.array_equal(dev_encode_biases(ctx, dev, R_FRAMES, pal, r['index'], r['modes']), got)


# ---- 3. both forms of the rank and distortion tables in one call ----
def test_palette_mixing_table_forms(ctx, random_case):
    r = random_case
    rng = np.random.RandomState(5)
    shuffled = np.concatenate([[2.0 ** -21], rng.permutation(2.0 ** (np.arange(1, 64) / 3.0 - 21))])   # no order in sfi: no integer form
    tiny = L.biased('1') * 2.0 ** -1010                                                                # subnormal coded terms: no tabled distortion
    tables = [O.biased_table(2), shuffled, tiny, O.biased_table(0.5)]
    forms = [(host_tables(t)['affine'], host_tables(t)['dist_ok']) for t in tables]
    assert forms[0] == (1, 1) and forms[1] == (0, 1) and forms[2][1] == 0 and forms[3] == (1, 1), forms
    index = r['index'] % 4
    assert set(index.reshape(-1).tolist()) == {0, 1, 2, 3}
    import torch
    dev = [torch.from_numpy(c).cuda() for c in r['chans']]
    for modes in (r['modes'], None):
        want = BP.oracle_encode_schedule(r['chans'], tables, index, modes, {})[0]
        got = dev_encode_biases(ctx, dev, R_FRAMES, [opts(table=t) for t in tables], index, modes)
        assert np.array_equal(got, want), first_bad(got, want)


# ---- 4. degenerate palettes ----
def test_degenerate_palettes(ctx, random_case):
    import torch
    r = random_case
    dev = [torch.from_numpy(c).cuda() for c in r['chans']]
    zeros = np.zeros(R_FRAMES * 2, dtype=np.uint8)
    for o in (opts({'allocationBias': 0.5}), opts({'allocationBias': 2, 'fixedBlockModes': [2, 0, 3]}), opts({'allocationBias': 3.3, 'transientThresholdLow': 0.3})):
        # one entry: c1_encode_device with that entry's options; with modes, c1_encode_modes_device
        assert np.array_equal(dev_encode_biases(ctx, dev, R_FRAMES, [o], zeros), ctx.encode(r['chans'], o))
        assert np.array_equal(dev_encode_biases(ctx, dev, R_FRAMES, [o], zeros, r['modes']), ctx.encode_modes(r['chans'], r['modes'], o))
    o = opts({'allocationBias': 1.5})
    want = ctx.encode(r['chans'], o)
    assert np.array_equal(dev_encode_biases(ctx, dev, R_FRAMES, [o, o], r['index'] % 2), want)            # the same table twice, any index
    two = [opts({'allocationBias': 0.25}), opts({'allocationBias': 5})]
    base = dev_encode_biases(ctx, dev, R_FRAMES, two, r['index'] % 2)
    assert BP.differing_units(base, ctx.encode(r['chans'], two[0])) and BP.differing_units(base, ctx.encode(r['chans'], two[1]))
    for extra in ([opts({'allocationBias': 1})], [opts({'allocationBias': 1}), opts({'allocationBias': 2})] * 3):
        assert np.array_equal(dev_encode_biases(ctx, dev, R_FRAMES, two + extra, r['index'] % 2), base)   # entries no unit uses


# ---- 5. the geometry of the unit lists ----
@pytest.mark.parametrize('nch', [1, 2])
def test_list_geometry(ctx, random_case, nch):
    import torch
    chans = random_case['chans'][:nch]
    biases = (0.5, 1, 2)
    pal = [opts({'allocationBias': b}) for b in biases]
    full = [torch.from_numpy(np.concatenate([c, c])).cuda() for c in chans]        # 260 frames
    for frames in COUNTS:
        host = [np.concatenate([c, c])[:frames * 512] for c in chans]
        const = [ctx.encode(host, o) for o in pal]
        for kind in ('cycle', 'last', 'single'):
            index = BP.pattern_index(kind, frames * nch, 3)
            got = dev_encode_biases(ctx, full, frames, pal, index)
            want = BP.compose(index, const)
            assert np.array_equal(got, want), (frames, kind, first_bad(got, want))


# ---- 6. a list longer than the bounded grid of list-mode allocation (256 * 12 blocks of 64 units) ----
def test_list_longer_than_the_bounded_grid(ctx):
    import torch
    frames = 1 << 18
    assert frames > 256 * 12 * 64
    pcm = torch.zeros(frames * 512, dtype=torch.float32, device='cuda')
    const = [torch.zeros(frames * 212, dtype=torch.uint8, device='cuda') for _ in range(2)]
    got = torch.zeros(frames * 212, dtype=torch.uint8, device='cuda')
    pal = [opts({'allocationBias': 1}), opts({'allocationBias': 2})]
    ones = torch.ones(frames, dtype=torch.uint8, device='cuda')
    odd = (torch.arange(frames, device='cuda') & 1).to(torch.uint8)
    torch.cuda.synchronize()
    ctx.generate_device(c1.SIGNAL_PINK_BURSTS, 7, frames, pcm.data_ptr())
    for k in range(2):
        ctx.encode_device([pcm.data_ptr()], frames, const[k].data_ptr(), pal[k])
    ctx.encode_biases_device([pcm.data_ptr()], frames, pal, ones.data_ptr(), got.data_ptr())
    ctx.synchronize()
    assert torch.equal(got, const[1])
    differ = (const[0].view(frames, 212) != const[1].view(frames, 212)).any(dim=1)
    assert int(differ[0::2].sum()) > frames // 8 and int(differ[1::2].sum()) > frames // 8    # the two biases are told apart on both halves
    ctx.encode_biases_device([pcm.data_ptr()], frames, pal, odd.data_ptr(), got.data_ptr())
    ctx.synchronize()
    want = torch.where(odd.bool()[:, None], const[1].view(frames, 212), const[0].view(frames, 212))
    assert torch.equal(got.view(frames, 212), want)


# ---- 7. chunk seams, pipeline, speculation, halo ----
@pytest.mark.parametrize('env', [{'C1_CHUNK_FRAMES': 16}, {'C1_CHUNK_FRAMES': 33}, {'C1_CHUNK_FRAMES': 16, 'C1_PIPELINE': 1, 'C1_OVERLAP': 1}],
                         ids=['chunk16', 'chunk33', 'chunk16-piped'])
def test_bytes_do_not_depend_on_chunks_or_speculation(random_case, env):
    r = random_case
    c = _context(**env)
    try:
        for mode in (0, 1, 2):
            c.set_speculation(mode)
            assert np.array_equal(c.encode_biases(r['chans'], r['biases'], modes=r['modes']), r['want']['modes']), (env, mode)
            assert np.array_equal(c.encode_biases(r['chans'], r['biases']), r['want']['detect']), (env, mode)
            assert np.array_equal(c.encode_biases(r['chans'], r['biases'], options=opts(r['fixed'])), r['want']['fixed']), (env, mode)
        c.set_profiling(True)
        c.encode_biases(r['chans'], r['biases'], modes=r['modes'])
        ms, launches = c.kernel_ms('allocate')
        assert launches == -(-R_FRAMES // env['C1_CHUNK_FRAMES']) > 1 and ms > 0      # the sorting and all chains of a chunk: one entry
    finally:
        c.close()


def test_bytes_do_not_depend_on_speculation(ctx, random_case):
    r = random_case
    try:
        for mode in (0, 1, 2):
            ctx.set_speculation(mode)
            assert np.array_equal(ctx.encode_biases(r['chans'], r['biases'], modes=r['modes']), r['want']['modes']), mode
            assert np.array_equal(ctx.encode_biases(r['chans'], r['biases']), r['want']['detect']), mode
            assert np.array_equal(ctx.encode_biases(r['chans'], r['biases'], options=opts({'fixedBlockModes': [0, 0, 0]})),
                                  BP.oracle_encode_schedule(r['chans'], BIASES, r['index'], None, {'fixedBlockModes': [0, 0, 0]})[0]), mode
    finally:
        ctx.set_speculation(1)


@pytest.mark.parametrize('halo', [0, 1, 2])
def test_halo_against_the_slice_of_a_longer_encode(ctx, random_case, halo):
    """frames 2.. of the longer signal, with `halo` frames of it in front: for halo 2 the slice of the encode of everything; for
    less, the oracle started that many frames early"""
    r = random_case
    long_index = np.concatenate([np.zeros((2, 2), dtype=np.uint8), r['index']])
    long_modes = np.concatenate([np.zeros((2, 2), dtype=np.uint8), r['modes']])
    part = [c[(2 - halo) * 512:] for c in r['with_halo']]
    for modes, base in ((r['modes'], None), (None, {})):
        got = ctx.encode_biases(part, r['biases'], modes=modes, halo_frames=halo)
        lead = 2 - halo
        want = BP.oracle_encode_schedule(part, BIASES, long_index[lead:], None if modes is None else long_modes[lead:], base)[0][halo * 2:]
        assert np.array_equal(got, want), (halo, modes is None, first_bad(got, want))
        if halo == 2:
            whole = ctx.encode_biases(r['with_halo'], np.array(BIASES)[long_index], modes=None if modes is None else long_modes)
            assert np.array_equal(got, whole[4:])


# ---- 8. one stream through the reference's option schedules, the bias through the pushes alone ----
@pytest.mark.parametrize('name,sig', CASES, ids=['%s-%s' % c for c in CASES])
def test_stream_follows_reference_schedule(ctx, name, sig):
    s = FIX['schedules'][name]
    frames = FIX['frames']
    chans = OC.signal(FIX['signals'][sig], frames)
    per_frame = OC.options_at(s['initial'], s['changes'], frames)
    for split in (None, 1, 5):
        steps = BP.plan(per_frame, len(chans), split)
        stream = c1.EncoderStream(ctx, len(chans), opts(steps[0][1]))
        try:
            units = BP.run_plan_on_stream(stream, opts, chans, steps)
            state = stream.get_state()
        finally:
            stream.close()
        err = OC.check_against(s['results'][sig], units, len(chans))
        assert err is None, (err, split)
        if split is None:
            want_state = BP.run_plan_on_oracle(chans, steps)[1]
            assert np.array_equal(SL.bits(state), SL.bits(want_state)), [k for k, (o, n) in SL.ENC_FIELDS.items() if not np.array_equal(SL.bits(state[:, o:o + n]), SL.bits(want_state[:, o:o + n]))]


@pytest.mark.parametrize('detect', [True, False], ids=['detect', 'modes'])
def test_stream_push_right_after_set_state(ctx, random_case, detect):
    """the first two frames after a restore are encoded from the explicit state, one allocation per frame and channel: each
    under its own unit's entry; the third takes the usual path"""
    r = random_case
    seg = lambda x, y: [ch[x * 512:y * 512] for ch in r['chans']]
    a, b = 20, 31
    modes = None if detect else r['modes']
    u0, st = SL.oracle_encode(seg(0, a), {})
    want, st_after = BP.oracle_encode_schedule(seg(a, b), BIASES, r['index'][a:b], None if detect else modes[a:b], {}, st)
    s1, s2 = c1.EncoderStream(ctx, 2, opts()), c1.EncoderStream(ctx, 2, opts())
    try:
        assert np.array_equal(s1.push(seg(0, a)), u0)
        state = s1.get_state()
        assert np.array_equal(SL.bits(state), SL.bits(st))
        for pieces in ((a, b), (a, a + 1, a + 2, a + 3, b)):
            s2.set_state(state)
            got = [s2.push(seg(x, y), modes=None if detect else modes[x:y], biases=r['biases'][x:y]) for x, y in zip(pieces, pieces[1:])]
            assert np.array_equal(np.concatenate(got), want), (pieces, first_bad(np.concatenate(got), want))
            assert np.array_equal(SL.bits(s2.get_state()), SL.bits(st_after))
    finally:
        s1.close()
        s2.close()


# ---- 9. what the entry points reject ----
def test_rejections(ctx, random_case):
    lib = capi.load()
    r = random_case
    chans, nch, frames = r['chans'], 2, R_FRAMES
    ptrs = capi.ptr_array([c.ctypes.data for c in chans])
    pal8 = codec.palette_array([opts({'allocationBias': b}).to_c() for b in BIASES] + [opts().to_c()])
    units = np.full((frames * nch, 212), 0xA5, dtype=np.uint8)
    s = c1.EncoderStream(ctx, nch, opts())
    batch = lambda pal, n, idx, modes=None: lib.c1_encode_biases_batch(ctx._h, ptrs, nch, frames, 0, pal, n, idx.ctypes.data, None if modes is None else modes.ctypes.data, units.ctypes.data)
    push = lambda pal, n, idx, modes=None: lib.c1_enc_stream_push_biases(s._h, ptrs, frames, pal, n, idx.ctypes.data, None if modes is None else modes.ctypes.data, units.ctypes.data)
    err = lambda: lib.c1_last_error().decode()
    try:
        head = s.push([c[:512 * 7] for c in chans])
        good = (r['index'] % 3).reshape(-1).copy()
        for call in (batch, push):
            for n, bad in ((3, 3), (3, 0xFF), (8, 8)):                 # index n, 0xFF
                for at in (0, frames * nch - 1):
                    idx = good.copy()
                    idx[at] = bad
                    assert call(pal8, n, idx) == C1_ERR_ARG
                    assert 'frame %d, channel %d' % (at // 2, at % 2) in err() and 'bias index %d' % bad in err(), err()
            for n in (0, 9):                                           # the size of the palette
                assert call(pal8, n, good) == C1_ERR_ARG
                assert 'n_palette = %d' % n in err(), err()
            broken = codec.palette_array([pal8[k] for k in range(4)])
            broken[2].biased_scale_factors[5] = -1.0                   # a bad table in entry 2
            assert call(broken, 4, good) == C1_ERR_ARG
            assert 'palette entry 2' in err() and 'biased_scale_factors[5]' in err(), err()
            bad_mode = r['modes'].reshape(-1).copy()
            bad_mode[11] = 0x01
            assert call(pal8, 3, good, bad_mode) == C1_ERR_ARG
            assert 'frame 5, channel 1' in err() and 'low field' in err(), err()
            assert (units == 0xA5).all()
        # entries that disagree on threshold or modes, and no modes given: the batch and device calls refuse, naming the entry
        for key, value, word in (('transientThresholdLow', 0.5, 'transient_threshold'), ('fixedBlockModes', [0, 0, 0], 'fixed_block_modes')):
            mixed = codec.palette_array([opts({'allocationBias': 1}).to_c(), opts({'allocationBias': 2}).to_c(), opts({'allocationBias': 0.5, key: value}).to_c()])
            assert batch(mixed, 3, good) == C1_ERR_ARG
            assert 'palette entry 2' in err() and word in err(), err()
            assert lib.c1_encode_biases_device(ctx._h, ptrs, nch, frames, 0, mixed, 3, good.ctypes.data, None, units.ctypes.data) == C1_ERR_ARG
            assert 'palette entry 2' in err() and word in err(), err()
            assert batch(mixed, 2, good % 2) == C1_OK                 # the entry that differs is not part of this palette
            units[:] = 0xA5
            assert batch(mixed, 3, good, r['modes'].reshape(-1)) == C1_OK     # with modes given the fields are not read
            units[:] = 0xA5
        mono = np.zeros(5, dtype=np.uint8)
        mono[3] = 2
        assert lib.c1_encode_biases_batch(ctx._h, ptrs, 1, 5, 0, pal8, 2, mono.ctypes.data, None, units.ctypes.data) == C1_ERR_ARG
        assert 'frame 3' in err() and 'channel' not in err(), err()
        with pytest.raises(ValueError, match='at most 8 distinct'):
            ctx.encode_biases(chans, np.arange(frames) % 9 * 0.5)
        assert (units == 0xA5).all()
        # the stream continues as if the calls had not been made
        rest = s.push([c[512 * 7:] for c in chans])
        assert np.array_equal(np.concatenate([head, rest]), ctx.encode(chans, opts()))
        # frames = 0 writes nothing
        assert lib.c1_encode_biases_batch(ctx._h, ptrs, nch, 0, 0, pal8, 8, None, None, units.ctypes.data) == C1_OK
        assert lib.c1_enc_stream_push_biases(s._h, ptrs, 0, pal8, 8, None, None, units.ctypes.data) == C1_OK
        assert lib.c1_encode_biases_device(ctx._h, ptrs, nch, 0, 0, pal8, 8, None, None, None) == C1_OK
        assert (units == 0xA5).all()
        assert ctx.encode_biases([c[:0] for c in chans], np.zeros(0)).shape == (0, 212)
    finally:
        s.close()


# ---- 10. the device entry point on index bytes outside the palette ----
def test_device_entry_point_stays_in_bounds_for_any_index_byte(ctx, random_case):
    import torch
    r = random_case
    units_n = R_FRAMES * 2
    index = r['index'].reshape(-1).copy()
    at = np.random.RandomState(3).permutation(units_n)[:256]
    index[at] = np.arange(256, dtype=np.uint8)                      # every byte value, at scattered units
    inside = index < 8
    assert inside.sum() == units_n - 248
    want = BP.oracle_encode_schedule(r['chans'], BIASES, np.where(inside, index, 0), r['modes'])[0]
    G = 4096                                                         # guard bytes on either side
    buf_units = torch.full((G + units_n * 212 + G,), 0xA5, dtype=torch.uint8, device='cuda')
    buf_index = torch.full((G + units_n + G,), 0xFF, dtype=torch.uint8, device='cuda')
    buf_index[G:G + units_n] = torch.from_numpy(index).cuda()
    dev = [torch.from_numpy(c).cuda() for c in r['chans']]
    d_modes = torch.from_numpy(r['modes'].reshape(-1).copy()).cuda()
    pal = [opts({'allocationBias': b}) for b in BIASES]
    torch.cuda.synchronize()
    for modes_ptr, expect in ((d_modes.data_ptr(), want), (None, None)):
        ctx.encode_biases_device([d.data_ptr() for d in dev], R_FRAMES, pal, buf_index.data_ptr() + G, buf_units.data_ptr() + G, modes_ptr)
        ctx.synchronize()
        u = buf_units.cpu().numpy()
        i = buf_index.cpu().numpy()
        assert (u[:G] == 0xA5).all() and (u[-G:] == 0xA5).all()
        assert (i[:G] == 0xFF).all() and (i[-G:] == 0xFF).all() and np.array_equal(i[G:-G], index)
        got = u[G:-G].reshape(-1, 212)
        if expect is None:
            expect = BP.oracle_encode_schedule(r['chans'], BIASES, np.where(inside, index, 0), None, {})[0]
        assert np.array_equal(got[inside], expect[inside]), first_bad(got[inside], expect[inside])


# ---- 11. on a caller's stream ----
def test_on_a_callers_stream(random_case):
    """PCM, index and modes are written by work queued just before the call and the units are read by work queued just after,
    with no host synchronisation in between; then inputs and output are overwritten behind it"""
    import torch
    r = random_case
    S = torch.cuda.Stream()
    c = _context(stream=S.cuda_stream)
    try:
        src = [torch.from_numpy(x).cuda() for x in r['chans']]
        src_modes = torch.from_numpy(r['modes'].reshape(-1).copy()).cuda()
        src_index = torch.from_numpy(r['index'].reshape(-1).copy()).cuda()
        pcm = [torch.zeros_like(x) for x in src]
        modes = torch.full_like(src_modes, 0x3a)
        index = torch.full_like(src_index, 7)
        units = torch.zeros(R_FRAMES * 2 * 212, dtype=torch.uint8, device='cuda')
        busy = torch.ones(1 << 26, dtype=torch.float32, device='cuda')
        torch.cuda.synchronize()
        pal = [opts({'allocationBias': b}) for b in BIASES]
        call = lambda: c.encode_biases_device([p.data_ptr() for p in pcm], R_FRAMES, pal, index.data_ptr(), units.data_ptr(), modes.data_ptr())
        with torch.cuda.stream(S):
            call()                                   # warm: options and palette on the device, workspace grown (these drain the stream)
            S.synchronize()
            for _ in range(200):
                busy.mul_(-1.0)
            for p, x in zip(pcm, src):
                p.copy_(x)
            modes.copy_(src_modes)
            index.copy_(src_index)
            call()
            snapshot = units.clone()
            for p in pcm:
                p.zero_()
            modes.zero_()
            index.zero_()
            units.fill_(0xA5)
            queued_behind_busy_stream = not S.query()
            S.synchronize()
        assert queued_behind_busy_stream
        assert np.array_equal(snapshot.cpu().numpy().reshape(-1, 212), r['want']['modes'])
    finally:
        c.close()
