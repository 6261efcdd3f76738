"""GPU: the allocation bias of every sound unit chosen from a palette by least coding error (c1_encode_best_bias_device /
_batch, k_choose_bias).  Distortion, energy, choice and bytes against the CPU model of tests/best_bias_lib.py (built from the
oracle alone) with given modes over the whole domain, under detection and under fixed modes; the geometry of the new kernel
(one wave per unit, four waves per workgroup, a grid bounded at 2 048 workgroups: 8 192 units per sweep); ties, silence and
repeatability; independence of chunking, pipeline, speculation, halo and of which outputs are asked for; the device entry
point on a caller's stream and on mode bytes outside the domain.
tests/test_best_bias_cpu.py shows that on this material every unit has exactly one admissible entry, that five or six
different entries win, and that "always bias 1" is wrong in at least 85 % of the units."""
import os

import numpy as np
import pytest

import carta1_amd as c1
from carta1_amd import capi, codec
import best_bias_lib as BB
import bias_palette_lib as BP
import oracle_lib as O

pytestmark = pytest.mark.gpu

C1_OK, C1_ERR_ARG = 0, 1   # include/carta1_hip.h
FRAMES = BB.FRAMES
BIASES = BB.BIASES
# frames per call, mono and stereo: one wave of k_choose_bias (1 unit), a partly filled workgroup of four waves and its seam (2 .. 5),
# the counts of the issue (63, 64, 65, 130, 257: many workgroups), and the seam of the bounded grid, 2 048 workgroups * 4 waves =
# 8 192 units, past which the waves stride (mono 8 191 .. 8 193 units, stereo 8 190 .. 8 194)
COUNTS = {1: (1, 2, 3, 4, 5, 63, 64, 65, 130, 257, 8191, 8192, 8193), 2: (1, 2, 3, 4, 5, 63, 64, 65, 130, 257, 4095, 4096, 4097)}
LARGE = {1: 8400, 2: 4200}


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
def mat():
    with_halo, body = BB.material()
    return {'with_halo': with_halo, 'body': body, 'modes': BB.given_modes()}


def batch(ctx, chans, palette_options, modes=None, halo=0, ask=('units', 'choice', 'distortion', 'energy')):
    """c1_encode_best_bias_batch with any subset of the outputs; the others are passed as NULL -> dict of the ones asked for"""
    chans = [np.ascontiguousarray(c, dtype=np.float32) for c in chans]
    nch, frames, n = len(chans), len(chans[0]) // 512 - halo, len(palette_options)
    pal = codec.palette_array([o.to_c() for o in palette_options])
    out = {'units': np.full((frames * nch, 212), 0xA5, dtype=np.uint8), 'choice': np.full(frames * nch, 0xA5, dtype=np.uint8),
           'distortion': np.full((frames * nch, n), -1.0), 'energy': np.full(frames * nch, -1.0)}
    m = None if modes is None else np.ascontiguousarray(modes, dtype=np.uint8).reshape(-1)
    ptrs = capi.ptr_array([c.ctypes.data + halo * 2048 for c in chans])
    capi.check(capi.load().c1_encode_best_bias_batch(ctx._h, ptrs, nch, frames, halo, pal, n, None if m is None else m.ctypes.data,
                                                     *[out[k].ctypes.data if k in ask else None for k in ('units', 'choice', 'distortion', 'energy')]))
    return {k: out[k] for k in ask}


def same(a, b):
    """bitwise equality of two output dicts (doubles compared as bit patterns)"""
    return a.keys() == b.keys() and all(np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) for k in a)


def rows(out, a, b, nch):
    return {k: v[a * nch:b * nch] for k, v in out.items()}


PAL8 = [opts({'allocationBias': b}) for b in BIASES]


# ---- 1. against the model ----
@pytest.mark.parametrize('kind', ['modes', 'detect', 'fixed'])
def test_against_the_model(ctx, mat, kind):
    modes = mat['modes'] if kind == 'modes' else None
    o = opts(BB.FIXED) if kind == 'fixed' else None
    units, choice, dist, energy = ctx.encode_best_bias(mat['body'], BIASES, modes=modes, options=o, return_distortion=True)
    m = BB.case(kind)
    print('largest relative error of D %.3g, of E %.3g' % (np.max(np.abs(dist - m['D']) / m['D']), np.max(np.abs(energy - m['E']) / m['E'])))
    assert BB.check_outputs(kind, units, choice, dist, energy) is None
    assert np.array_equal(units, ctx.encode_biases(mat['body'], np.array(BIASES)[choice].reshape(FRAMES, 2), modes=modes, options=o))
    u2, c2 = ctx.encode_best_bias(mat['body'], BIASES, modes=modes, options=o)
    assert np.array_equal(u2, units) and np.array_equal(c2, choice)


# ---- 2. geometry ----
@pytest.mark.parametrize('nch', [1, 2])
@pytest.mark.parametrize('n', [1, 2, 8])
def test_geometry(ctx, mat, nch, n):
    reps = -(-LARGE[nch] // FRAMES)
    chans = [np.tile(c, reps)[:LARGE[nch] * 512] for c in mat['body'][:nch]]
    modes = np.tile(mat['modes'][:, :nch], (reps, 1))[:LARGE[nch]]
    pal = {1: [PAL8[4]], 2: [PAL8[3], PAL8[5]], 8: PAL8}[n]
    large = batch(ctx, chans, pal, modes)
    assert (large['choice'] < n).all()
    if n == 8:
        assert len(set(large['choice'][-2 * FRAMES:].tolist())) >= 3
    # the bytes of the whole call, the second sweep of the grid included: the palette path fed the choice
    biases = np.array([float(o.allocationBias) for o in pal])[large['choice']].reshape(-1, nch)
    assert np.array_equal(large['units'], ctx.encode_biases(chans, biases, modes=modes))
    for frames in COUNTS[nch]:
        got = batch(ctx, [c[:frames * 512] for c in chans], pal, modes[:frames])
        assert same(got, rows(large, 0, frames, nch)), (frames, nch, n)
    # the last frames of the call, past the first sweep, from two frames of halo
    a = LARGE[nch] - FRAMES
    got = batch(ctx, [c[(a - 2) * 512:] for c in chans], pal, modes[a:], halo=2)
    assert same(got, rows(large, a, LARGE[nch], nch))
    if n == 1:
        assert not large['choice'].any()
        assert np.array_equal(large['units'], ctx.encode_modes(chans, modes, pal[0]))
        plain = batch(ctx, chans, pal)
        assert not plain['choice'].any() and np.array_equal(plain['units'], ctx.encode(chans, pal[0]))


# ---- 3. ties and degenerate input ----
def test_ties_silence_and_repeatability(ctx, mat):
    t1, t2 = O.biased_table(1), O.biased_table(2)
    pal = [opts(table=t1), opts(table=t1), opts(table=t2), opts(table=t1)]
    for modes in (mat['modes'], None):
        got = batch(ctx, mat['body'], pal, modes)
        assert set(got['choice'].tolist()) == {0, 2}
        d = got['distortion'].view(np.uint64)
        assert np.array_equal(d[:, 0], d[:, 1]) and np.array_equal(d[:, 0], d[:, 3]) and not np.array_equal(d[:, 0], d[:, 2])
        assert same(got, batch(ctx, mat['body'], pal, modes))                        # run to run
    silence = [np.zeros(FRAMES * 512, dtype=np.float32)] * 2
    got = batch(ctx, silence, PAL8)
    assert not got['choice'].any()
    assert not got['distortion'].view(np.uint64).any() and not got['energy'].view(np.uint64).any()    # +0.0 exactly
    assert np.array_equal(got['units'], O.encode_stream(silence)[0])
    got = batch(ctx, silence, PAL8, mat['modes'])
    assert not got['choice'].any() and not got['distortion'].view(np.uint64).any()
    assert np.array_equal(got['units'], BP.oracle_encode_schedule(silence, [1], np.zeros((FRAMES, 2), dtype=np.uint8), mat['modes'])[0])


# ---- 4. independence ----
@pytest.fixture(scope='module')
def baseline(ctx, mat):
    out = {'modes': batch(ctx, mat['body'], PAL8, mat['modes']), 'detect': batch(ctx, mat['body'], PAL8),
           'fixed': batch(ctx, mat['body'], [opts(dict(BB.FIXED, allocationBias=b)) for b in BIASES])}
    for v in out.values():
        for a in v.values():
            a.setflags(write=False)
    return out


def three_kinds(c, mat):
    return {'modes': batch(c, mat['body'], PAL8, mat['modes']), 'detect': batch(c, mat['body'], PAL8),
            'fixed': batch(c, mat['body'], [opts(dict(BB.FIXED, allocationBias=b)) for b in BIASES])}


@pytest.mark.parametrize('env', [{'C1_CHUNK_FRAMES': 16}, {'C1_CHUNK_FRAMES': 16, 'C1_PIPELINE': 0}, {'C1_PIPELINE': 0}, {'C1_PIPELINE': 1},
                                 {'C1_CHUNK_FRAMES': 33, 'C1_PIPELINE': 1, 'C1_OVERLAP': 1}],
                         ids=['chunk16', 'chunk16-unpiped', 'unpiped', 'piped', 'chunk33-piped-overlap'])
def test_outputs_do_not_depend_on_chunks_pipeline_or_speculation(mat, baseline, env):
    c = _context(**env)
    try:
        for mode in (0, 1, 2):
            c.set_speculation(mode)
            got = three_kinds(c, mat)
            for kind in got:
                assert same(got[kind], baseline[kind]), (env, mode, kind)
        c.set_profiling(True)
        batch(c, mat['body'], PAL8, mat['modes'])
        chunks = -(-FRAMES // env['C1_CHUNK_FRAMES']) if 'C1_CHUNK_FRAMES' in env else 1
        ms, launches = c.kernel_ms('choose')
        assert launches == chunks and ms > 0
        ms, launches = c.kernel_ms('allocate')
        assert launches == chunks and ms > 0                                         # the eight chains of a chunk: one entry
        batch(c, mat['body'], PAL8, mat['modes'], ask=('choice',))
        assert c.kernel_ms('pack')[1] == 0 and c.kernel_ms('choose')[1] == chunks    # units NULL: no packing runs
    finally:
        c.close()


def test_outputs_do_not_depend_on_speculation(ctx, mat, baseline):
    try:
        for mode in (0, 1, 2):
            ctx.set_speculation(mode)
            got = three_kinds(ctx, mat)
            for kind in got:
                assert same(got[kind], baseline[kind]), (mode, kind)
            long_pal = [opts({'allocationBias': b, 'fixedBlockModes': [0, 0, 0]}) for b in BIASES]     # the all-long kernels
            got = batch(ctx, mat['body'], long_pal)
            assert same(got, batch(ctx, mat['body'], PAL8, np.zeros((FRAMES, 2), dtype=np.uint8))), mode
    finally:
        ctx.set_speculation(1)


@pytest.mark.parametrize('halo', [0, 1, 2])
def test_halo_with_the_same_real_history(ctx, mat, halo):
    """frames `halo`.. of a signal, given its first `halo` frames as halo, against the rows of the call on the whole signal"""
    modes = np.concatenate([np.zeros((2, 2), dtype=np.uint8), mat['modes']])
    part = [c[(2 - halo) * 512:] for c in mat['with_halo']]
    for m in (modes[2 - halo:], None):
        whole = batch(ctx, part, PAL8, m)
        got = batch(ctx, part, PAL8, None if m is None else m[halo:], halo=halo)
        assert same(got, rows(whole, halo, halo + FRAMES, 2)), (halo, m is None)
    if halo == 2:       # two frames are all the history there is to carry
        longer = [np.concatenate([np.full(3 * 512, 0.25, dtype=np.float32), c]) for c in mat['with_halo']]
        whole = batch(ctx, longer, PAL8)
        got = batch(ctx, [c[3 * 512:] for c in longer], PAL8, halo=2)
        assert same(got, rows(whole, 5, 5 + FRAMES, 2))


def test_outputs_do_not_depend_on_which_are_asked_for(ctx, mat, baseline):
    for kind, modes in (('modes', mat['modes']), ('detect', None)):
        full = baseline[kind]
        for ask in (('choice', 'distortion'), ('units',), ('choice',), ('distortion',), ('energy',), ('units', 'energy')):
            got = batch(ctx, mat['body'], PAL8, modes, ask=ask)
            assert same(got, {k: full[k] for k in ask}), (kind, ask)


# ---- 5. the device entry point ----
def test_on_a_callers_stream(mat, baseline):
    """PCM and modes are written by work queued just before the call and the outputs are read by work queued just after, with
    no host synchronisation in between; then inputs and outputs are overwritten behind it"""
    import torch
    S = torch.cuda.Stream()
    c = _context(stream=S.cuda_stream)
    try:
        src = [torch.from_numpy(x).cuda() for x in mat['body']]
        src_modes = torch.from_numpy(mat['modes'].reshape(-1).copy()).cuda()
        pcm = [torch.zeros_like(x) for x in src]
        modes = torch.full_like(src_modes, 0x3a)
        units = torch.zeros(FRAMES * 2 * 212, dtype=torch.uint8, device='cuda')
        choice = torch.zeros(FRAMES * 2, dtype=torch.uint8, device='cuda')
        dist = torch.zeros(FRAMES * 2 * 8, dtype=torch.float64, device='cuda')
        energy = torch.zeros(FRAMES * 2, dtype=torch.float64, device='cuda')
        busy = torch.ones(1 << 26, dtype=torch.float32, device='cuda')
        torch.cuda.synchronize()
        call = lambda: c.encode_best_bias_device([p.data_ptr() for p in pcm], FRAMES, PAL8, units.data_ptr(), choice.data_ptr(),
                                                 dist.data_ptr(), energy.data_ptr(), modes.data_ptr())
        with torch.cuda.stream(S):
            call()                                   # warm: options and palette on the device, workspace grown (these drain the stream)
            S.synchronize()
            for _ in range(200):
                busy.mul_(-1.0)
            for p, x in zip(pcm, src):
                p.copy_(x)
            modes.copy_(src_modes)
            call()
            snap = [t.clone() for t in (units, choice, dist, energy)]
            for p in pcm:
                p.zero_()
            modes.zero_()
            units.fill_(0xA5)
            choice.fill_(0xA5)
            dist.fill_(-1.0)
            energy.fill_(-1.0)
            queued_behind_busy_stream = not S.query()
            S.synchronize()
        assert queued_behind_busy_stream
        got = {'units': snap[0].cpu().numpy().reshape(-1, 212), 'choice': snap[1].cpu().numpy(),
               'distortion': snap[2].cpu().numpy().reshape(-1, 8), 'energy': snap[3].cpu().numpy()}
        assert same(got, dict(baseline['modes']))
    finally:
        c.close()


def test_device_entry_point_stays_in_bounds_for_any_mode_byte(ctx, mat, baseline):
    import torch
    units_n = FRAMES * 2
    modes = mat['modes'].reshape(-1).copy()
    at = np.random.RandomState(3).permutation(units_n)[:256]
    modes[at] = np.arange(256, dtype=np.uint8)                      # every byte value, at scattered units
    clean = np.ones(units_n, dtype=bool)
    clean[at] = False
    G = 4096                                                         # guard bytes on either side of every output
    buf = {'units': (torch.uint8, units_n * 212, 0xA5), 'choice': (torch.uint8, units_n, 0xA5),
           'distortion': (torch.float64, units_n * 8, -1.0), 'energy': (torch.float64, units_n, -1.0)}
    size = {torch.uint8: 1, torch.float64: 8}
    t = {k: torch.full((2 * G // size[d] + n,), fill, dtype=d, device='cuda') for k, (d, n, fill) in buf.items()}
    dev = [torch.from_numpy(c).cuda() for c in mat['body']]
    d_modes = torch.from_numpy(modes).cuda()
    torch.cuda.synchronize()
    ctx.encode_best_bias_device([d.data_ptr() for d in dev], FRAMES, PAL8, *[t[k].data_ptr() + G for k in ('units', 'choice', 'distortion', 'energy')],
                                modes_ptr=d_modes.data_ptr())
    ctx.synchronize()
    assert np.array_equal(d_modes.cpu().numpy(), modes)
    for k, (d, n, fill) in buf.items():
        g = G // size[d]
        a = t[k].cpu().numpy()
        assert (a[:g] == fill).all() and (a[-g:] == fill).all(), k
        got = a[g:-g].reshape(units_n, -1)
        want = baseline['modes'][k].reshape(units_n, -1)
        assert np.array_equal(got[clean].view(np.uint8), want[clean].view(np.uint8)), k     # a unit's frame reads no other unit's mode byte


def test_device_entry_point_rejections(ctx, mat):
    lib = capi.load()
    pal = codec.palette_array([o.to_c() for o in PAL8])
    ptrs = capi.ptr_array([c.ctypes.data for c in mat['body']])
    assert lib.c1_encode_best_bias_device(ctx._h, ptrs, 2, FRAMES, 0, pal, 8, None, None, None, None, None) == C1_ERR_ARG
    assert 'all NULL' in lib.c1_last_error().decode()
    assert lib.c1_encode_best_bias_device(ctx._h, ptrs, 2, FRAMES, 0, pal, 9, None, None, ptrs, None, None) == C1_ERR_ARG
    assert 'n_palette = 9' in lib.c1_last_error().decode()
    assert lib.c1_encode_best_bias_device(ctx._h, ptrs, 2, 0, 0, pal, 8, None, None, ptrs, None, None) == C1_OK      # frames = 0 writes nothing
