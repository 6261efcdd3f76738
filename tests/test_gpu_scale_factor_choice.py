"""GPU: the measured allocation with every BFU's scale-factor index chosen by the same error (c1_encode_measured_sf_device /
_batch, k_measured_sf).  distortion, energy, taken, nBfu, word lengths, written scale-factor indices, shifts and bytes against the
CPU model of tests/scale_factor_choice_lib.py (built from the oracle alone) under constant mode bytes on two materials, given
modes over the whole domain, detection and fixed modes; the validity of the units from their bytes alone; one offset of 0 against
c1_encode_measured_device bit for bit; the geometry of the new kernel (one wave per unit, four waves per workgroup, a grid
bounded at 2 048 workgroups: 8 192 units per sweep); silence and repeatability; independence of chunking, pipeline, overlap,
speculation, halo and of which outputs are asked for; eight offsets reaching +-8; the device entry point on a caller's stream,
on mode bytes outside the domain, and the rejections.
tests/test_scale_factor_choice_cpu.py shows that every decision of the model on this material has a margin above 1e-9."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

import carta1_amd as c1
from carta1_amd import capi
import best_bias_lib as BB
import best_modes_lib as BMO
import measured_alloc_lib as MA
import oracle_lib as O
import scale_factor_choice_lib as SF

pytestmark = pytest.mark.gpu

C1_OK, C1_ERR_ARG = 0, 1   # include/carta1_hip.h
FRAMES = BB.FRAMES
OUTPUTS = ('units', 'taken', 'shifts', 'distortion', 'energy')
EIGHT = (0, 8, -8, -1, 1, -2, -3, 2)
# frames per call, mono and stereo: one wave (1 unit), a partly filled workgroup of four waves (2), the counts of the issue (63,
# 64, 65, 257: many workgroups), and the seam of the bounded grid, 2 048 workgroups * 4 waves = 8 192 units, past which the waves
# stride (mono 8 191 .. 8 194 units, stereo 8 190 .. 8 194)
COUNTS = {1: (1, 2, 63, 64, 65, 257, 8191, 8192, 8193, 8194), 2: (1, 2, 63, 64, 65, 257, 4095, 4096, 4097)}
LARGE = {1: 8400, 2: 4200}
SHORT = 48                                       # frames of the model under given modes and fixed modes


def opts(v=None):
    return c1.EncoderOptions(v or {})


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


def batch(ctx, chans, options=None, modes=None, halo=0, ask=OUTPUTS, offsets=SF.OFFSETS):
    """c1_encode_measured_sf_batch with any subset of the outputs; the others are passed as NULL -> dict of the ones asked for"""
    chans = [np.ascontiguousarray(c, dtype=np.float32) for c in chans]
    nch, frames = len(chans), len(chans[0]) // 512 - halo
    o = (options or opts()).to_c()
    out = {'units': np.full((frames * nch, 212), 0xA5, dtype=np.uint8), 'taken': np.full(frames * nch, 0xA5, dtype=np.uint8),
           'shifts': np.full((frames * nch, 52), 0x5A, dtype=np.int8), 'distortion': np.full((frames * nch, 2), -1.0),
           'energy': np.full(frames * nch, -1.0)}
    m = None if modes is None else np.ascontiguousarray(modes, dtype=np.uint8).reshape(-1)
    off = np.ascontiguousarray(offsets, dtype=np.int8)
    ptrs = capi.ptr_array([c.ctypes.data + halo * 2048 for c in chans])
    capi.check(capi.load().c1_encode_measured_sf_batch(ctx._h, ptrs, nch, frames, halo, C.byref(o), None if m is None else m.ctypes.data,
                                                       off.ctypes.data, len(off), *[out[k].ctypes.data if k in ask else None for k in OUTPUTS]))
    return {k: out[k] for k in ask}


def plain_batch(ctx, chans, options=None, modes=None):
    """c1_encode_measured_batch, all four outputs"""
    units, taken, dist, energy = ctx.encode_measured(chans, modes=modes, options=options, return_distortion=True)
    return {'units': units, 'taken': taken, 'distortion': dist, 'energy': energy}


def same(a, b):
    """bitwise equality of two output dicts (doubles compared as bit patterns)"""
    return a.keys() == b.keys() and all(np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) for k in a)


def rows(out, a, b, nch):
    return {k: v[a * nch:b * nch] for k, v in out.items()}


def call_of(kind, mat, material='pink', frames=None):
    """(channels, options, modes) of the shared case `kind`"""
    chans = BMO.material(material)
    n = len(chans[0]) // 512 if frames is None else frames
    chans = [c[:n * 512] for c in chans]
    if kind == 'detect':
        return chans, None, None
    if kind == 'fixed':
        return chans, opts({'fixedBlockModes': MA.FIXED}), None
    if kind == 'modes':
        return chans, None, mat['modes'][:n]
    return chans, None, np.full((n, 2), kind, dtype=np.uint8)


# ---- 1. against the model ----
@pytest.mark.parametrize('material,kind,frames', [('pink', 10, None), ('white', 58, None), ('pink', 'detect', None), ('pink', 'modes', SHORT),
                                                  ('pink', 'fixed', SHORT)])
def test_against_the_model(ctx, mat, material, kind, frames):
    """distortion and energy within 1e-12 of the model (exact zeros zero; seen on an MI355X: equal bit for bit); taken, nBfu and,
    where taken, every word length, every written scale-factor index and shifts equal to the model's; units the model's bytes,
    those not taken the plain encode's; T_final <= T_ref; and from the bytes alone (scale_factor_choice_lib.check_valid): nBfu of
    BFU_AMOUNTS, the mantissa bits within the budget, every written index findScaleFactor's plus one of the offsets within 1 ..
    63 and findScaleFactor's own where nothing is coded, every mantissa c1o_quantize_bfu's at the written index,
    c1o_pack_unit of the fields the same bytes, the weighted error of the dequantized unit the reported one, the decoded
    stream finite."""
    chans, o, modes = call_of(kind, mat, material, frames)
    units, taken, shifts, dist, energy = ctx.encode_measured(chans, modes=modes, options=o, return_distortion=True,
                                                             scale_factor_offsets=c1.SCALE_FACTOR_OFFSETS, return_shifts=True)
    m = SF.case(kind, material, frames=frames)
    print('taken %d of %d; bit-equal: T_ref %s, T(n*) %s, E %s' % (
        int(taken.sum()), len(taken), np.array_equal(dist[:, 0], m['D'][:, 0]), np.array_equal(dist[:, 1], m['D'][:, 1]),
        np.array_equal(energy, m['E'])))
    assert SF.check_outputs(m, units, taken, shifts, dist, energy) is None
    assert SF.check_valid(units, m['coefs'], taken, dist) is None
    final = np.where(taken != 0, dist[:, 1], dist[:, 0])
    assert (final <= dist[:, 0]).all()
    plain = ctx.encode(chans, o) if modes is None else ctx.encode_modes(chans, modes, o)
    assert np.array_equal(plain, m['ref'])
    assert np.array_equal(units[taken == 0], plain[taken == 0])
    u2, t2 = ctx.encode_measured(chans, modes=modes, options=o, scale_factor_offsets=c1.SCALE_FACTOR_OFFSETS)
    assert np.array_equal(u2, units) and np.array_equal(t2, taken)


# ---- 2. one offset of 0 is today's call ----
def test_offset_zero_alone_is_the_plain_measured_call(ctx, mat):
    for o, modes in ((None, mat['modes']), (None, None), (opts({'fixedBlockModes': MA.FIXED}), None), (opts({'fixedBlockModes': [0, 0, 0]}), None)):
        got = batch(ctx, mat['body'], o, modes, offsets=(0,))
        assert not got.pop('shifts').any()
        assert same(got, plain_batch(ctx, mat['body'], o, modes))


# ---- 3. geometry ----
@pytest.mark.parametrize('nch', [1, 2])
def test_geometry(ctx, mat, nch):
    reps = -(-LARGE[nch] // FRAMES)
    chans = [np.tile(c, reps)[:LARGE[nch] * 512] for c in mat['body'][:nch]]
    modes = np.tile(mat['modes'][:, :nch], (reps, 1))[:LARGE[nch]]
    large = batch(ctx, chans, None, modes)
    assert set(large['taken'].tolist()) <= {0, 1} and large['taken'].any()
    final = np.where(large['taken'] != 0, large['distortion'][:, 1], large['distortion'][:, 0])
    assert (final <= large['distortion'][:, 0]).all()
    # the bytes of the whole call, the second sweep of the grid included: the plain encode where not taken, other bytes where taken
    plain = ctx.encode_modes(chans, modes)
    kept = large['taken'] == 0
    assert np.array_equal(large['units'][kept], plain[kept])
    assert (large['units'][~kept] != plain[~kept]).any(axis=1).all()
    assert not large['shifts'][kept].any() and set(np.unique(large['shifts']).tolist()) <= set(SF.OFFSETS)
    assert all(np.isfinite(p).all() for p in O.decode_stream(large['units'], nch)[0])
    for frames in COUNTS[nch]:
        got = batch(ctx, [c[:frames * 512] for c in chans], None, modes[:frames])
        assert same(got, rows(large, 0, frames, nch)), (frames, nch)
    # the last frames of the call, past the first sweep, from two frames of halo
    a = LARGE[nch] - FRAMES
    got = batch(ctx, [c[(a - 2) * 512:] for c in chans], None, modes[a:], halo=2)
    assert same(got, rows(large, a, LARGE[nch], nch))
    # under detection: the rows of the larger call
    plain = batch(ctx, [c[:257 * 512] for c in chans])
    for frames in (1, 2, 64, 65):
        assert same(batch(ctx, [c[:frames * 512] for c in chans]), rows(plain, 0, frames, nch)), (frames, nch)


# ---- 4. degenerate input, repeatability, eight offsets ----
def test_silence_and_repeatability(ctx, mat):
    silence = [np.zeros(FRAMES * 512, dtype=np.float32)] * 2
    for modes in (None, mat['modes']):
        got = batch(ctx, silence, None, modes)
        assert not got['taken'].any() and not got['shifts'].any()
        assert not got['distortion'].view(np.uint64).any() and not got['energy'].view(np.uint64).any()    # +0.0 exactly
        want = O.encode_stream(silence)[0] if modes is None else ctx.encode_modes(silence, modes)
        assert np.array_equal(got['units'], want)
        first = batch(ctx, mat['body'], None, modes)
        assert same(first, batch(ctx, mat['body'], None, modes))                      # run to run


def test_eight_offsets_reaching_both_ends(ctx):
    """eight candidates with +-8 against the model on 24 frames of the white material as it is (findScaleFactor 35 .. 52), scaled
    by 2^-11 (2 .. 19: offset -8 leaves the table below for the quiet BFUs) and by 4 (41 .. 58: offset +8 leaves it above for the
    loud ones).  With +-8 among the candidates two table entries have two candidates of exactly equal error: the first in the
    order given wins in the model and on the device, which relies on the sums being equal bit for bit."""
    import block_modes_lib as BM
    frames = 24
    chans = [c[:frames * 512] for c in BMO.material('white')]
    modes = np.full((frames, 2), 58, dtype=np.uint8)
    for scale, reaches in ((1.0, None), (2.0 ** -11, -8), (4.0, 8)):
        scaled = [np.ascontiguousarray(c * np.float32(scale)) for c in chans]
        m = SF.model(scaled, BM.oracle_encode_modes(scaled, modes, 1.0)[0], EIGHT)
        assert (m['margin'] > MA.MARGIN).all()
        coded = m['s0'][m['s0'] != 0]
        if reaches is not None:
            assert ((coded + reaches < 1) | (coded + reaches > 63)).any() and ((coded + reaches >= 1) & (coded + reaches <= 63)).any()
        got = batch(ctx, scaled, None, modes, offsets=EIGHT)
        assert SF.check_outputs(m, got['units'], got['taken'], got['shifts'], got['distortion'], got['energy']) is None, scale
        assert SF.check_valid(got['units'], m['coefs'], got['taken'], got['distortion'], EIGHT) is None, scale
        assert got['taken'].any()


# ---- 5. independence ----
def three_kinds(c, mat):
    return {'modes': batch(c, mat['body'], None, mat['modes']), 'detect': batch(c, mat['body']),
            'fixed': batch(c, mat['body'], opts({'fixedBlockModes': MA.FIXED}))}


@pytest.fixture(scope='module')
def baseline(ctx, mat):
    out = three_kinds(ctx, mat)
    for v in out.values():
        for a in v.values():
            a.setflags(write=False)
    return out


@pytest.mark.parametrize('env', [{'C1_CHUNK_FRAMES': 7}, {'C1_CHUNK_FRAMES': 64}, {'C1_PIPELINE': 0}, {'C1_PIPELINE': 1},
                                 {'C1_CHUNK_FRAMES': 64, 'C1_PIPELINE': 1, 'C1_OVERLAP': 1}],
                         ids=['chunk7', 'chunk64', 'unpiped', 'piped', 'chunk64-piped-overlap'])
def test_outputs_do_not_depend_on_chunks_pipeline_or_speculation(mat, baseline, env):
    c = _context(**env)
    try:
        for mode in (0, 1, 2):
            c.set_speculation(mode)
            got = three_kinds(c, mat)
            for kind in got:
                assert same(got[kind], baseline[kind]), (env, mode, kind)
        c.set_profiling(True)
        batch(c, mat['body'], None, mat['modes'])
        chunks = -(-FRAMES // max(env['C1_CHUNK_FRAMES'], 16)) if 'C1_CHUNK_FRAMES' in env else 1   # a context's chunk is at least 16 frames
        ms, launches = c.kernel_ms('measure')
        assert launches == chunks and ms > 0
        assert c.kernel_ms('allocate')[1] == chunks and c.kernel_ms('choose')[1] == 0
        batch(c, mat['body'], None, mat['modes'], ask=('shifts',))
        assert c.kernel_ms('pack')[1] == 0 and c.kernel_ms('measure')[1] == chunks   # units NULL: no packing runs
    finally:
        c.close()


def test_outputs_do_not_depend_on_speculation(ctx, mat, baseline):
    try:
        for mode in (0, 1, 2):
            ctx.set_speculation(mode)
            got = three_kinds(ctx, mat)
            for kind in got:
                assert same(got[kind], baseline[kind]), (mode, kind)
            got = batch(ctx, mat['body'], opts({'fixedBlockModes': [0, 0, 0]}))                     # the all-long kernels
            assert same(got, batch(ctx, mat['body'], None, np.zeros((FRAMES, 2), dtype=np.uint8))), mode
    finally:
        ctx.set_speculation(1)


@pytest.mark.parametrize('halo', [1, 2])
def test_halo_with_the_same_real_history(ctx, mat, halo):
    """frames `halo`.. of a signal, given its first `halo` frames as halo, against the rows of the call on the whole signal"""
    modes = np.concatenate([np.zeros((2, 2), dtype=np.uint8), mat['modes']])
    part = [c[(2 - halo) * 512:] for c in mat['with_halo']]
    for m in (modes[2 - halo:], None):
        whole = batch(ctx, part, None, m)
        got = batch(ctx, part, None, None if m is None else m[halo:], halo=halo)
        assert same(got, rows(whole, halo, halo + FRAMES, 2)), (halo, m is None)


def test_outputs_do_not_depend_on_which_are_asked_for(ctx, mat, baseline):
    """every single output and every set of all but one; a measure-only call leaves the units it was not given unwritten and the
    records of the context alone: the next plain encode gives the reference's bytes"""
    subsets = [s for k in (1, 4) for s in itertools.combinations(OUTPUTS, k)]
    for kind, modes in (('modes', mat['modes']), ('detect', None)):
        full = baseline[kind]
        for ask in subsets:
            got = batch(ctx, mat['body'], None, modes, ask=ask)
            assert same(got, {k: full[k] for k in ask}), (kind, ask)
    batch(ctx, mat['body'], None, mat['modes'], ask=('taken', 'shifts', 'distortion', 'energy'))
    assert np.array_equal(ctx.encode_modes(mat['body'], mat['modes']), MA.case('modes')['ref'])
    batch(ctx, mat['body'], None, mat['modes'])                                       # and after a call that rewrote its records
    assert np.array_equal(ctx.encode_modes(mat['body'], mat['modes']), MA.case('modes')['ref'])


# ---- 6. the device entry point ----
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
        taken = torch.zeros(FRAMES * 2, dtype=torch.uint8, device='cuda')
        shifts = torch.zeros(FRAMES * 2 * 52, dtype=torch.int8, device='cuda')
        dist = torch.zeros(FRAMES * 2 * 2, dtype=torch.float64, device='cuda')
        energy = torch.zeros(FRAMES * 2, dtype=torch.float64, device='cuda')
        busy = torch.ones(1 << 26, dtype=torch.float32, device='cuda')
        torch.cuda.synchronize()
        call = lambda: c.encode_measured_device([p.data_ptr() for p in pcm], FRAMES, units.data_ptr(), taken.data_ptr(),
                                                dist.data_ptr(), energy.data_ptr(), modes_ptr=modes.data_ptr(),
                                                scale_factor_offsets=SF.OFFSETS, shifts_ptr=shifts.data_ptr())
        with torch.cuda.stream(S):
            call()                                   # warm: options on the device, workspace grown (these drain the stream)
            S.synchronize()
            for _ in range(200):
                busy.mul_(-1.0)
            for p, x in zip(pcm, src):
                p.copy_(x)
            modes.copy_(src_modes)
            call()
            snap = [t.clone() for t in (units, taken, shifts, dist, energy)]
            for p in pcm:
                p.zero_()
            modes.zero_()
            units.fill_(0xA5)
            taken.fill_(0xA5)
            shifts.fill_(0x5A)
            dist.fill_(-1.0)
            energy.fill_(-1.0)
            queued_behind_busy_stream = not S.query()
            S.synchronize()
        assert queued_behind_busy_stream
        got = {'units': snap[0].cpu().numpy().reshape(-1, 212), 'taken': snap[1].cpu().numpy(), 'shifts': snap[2].cpu().numpy().reshape(-1, 52),
               'distortion': snap[3].cpu().numpy().reshape(-1, 2), 'energy': snap[4].cpu().numpy()}
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
    buf = {'units': (torch.uint8, units_n * 212, 0xA5), 'taken': (torch.uint8, units_n, 0xA5), 'shifts': (torch.int8, units_n * 52, 0x5A),
           'distortion': (torch.float64, units_n * 2, -1.0), 'energy': (torch.float64, units_n, -1.0)}
    size = {torch.uint8: 1, torch.int8: 1, torch.float64: 8}
    t = {k: torch.full((2 * G // size[d] + n,), fill, dtype=d, device='cuda') for k, (d, n, fill) in buf.items()}
    dev = [torch.from_numpy(c).cuda() for c in mat['body']]
    d_modes = torch.from_numpy(modes).cuda()
    torch.cuda.synchronize()
    p = {k: t[k].data_ptr() + G for k in OUTPUTS}
    ctx.encode_measured_device([d.data_ptr() for d in dev], FRAMES, p['units'], p['taken'], p['distortion'], p['energy'],
                               modes_ptr=d_modes.data_ptr(), scale_factor_offsets=EIGHT, shifts_ptr=p['shifts'])
    ctx.synchronize()
    assert np.array_equal(d_modes.cpu().numpy(), modes)
    want_all = batch(ctx, mat['body'], None, mat['modes'], offsets=EIGHT)
    for k, (d, n, fill) in buf.items():
        g = G // size[d]
        a = t[k].cpu().numpy()
        assert (a[:g] == fill).all() and (a[-g:] == fill).all(), k
        got = a[g:-g].reshape(units_n, -1)
        want = want_all[k].reshape(units_n, -1)
        assert np.array_equal(got[clean].view(np.uint8), want[clean].view(np.uint8)), k     # a unit's frame reads no other unit's mode byte
    got_taken = t['taken'].cpu().numpy()[G:-G]
    assert set(got_taken.tolist()) <= {0, 1}
    got_shifts = t['shifts'].cpu().numpy()[G:-G]
    assert set(np.unique(got_shifts).tolist()) <= set(EIGHT)


def test_rejections_leave_the_outputs_untouched(ctx, mat):
    lib = capi.load()
    o = opts().to_c()
    ptrs = capi.ptr_array([c.ctypes.data for c in mat['body']])
    off = np.array(SF.OFFSETS, dtype=np.int8)
    dev = lambda *a: lib.c1_encode_measured_sf_device(ctx._h, ptrs, *a)
    assert dev(2, FRAMES, 0, C.byref(o), None, off.ctypes.data, 5, None, None, None, None, None) == C1_ERR_ARG
    assert 'all NULL' in lib.c1_last_error().decode()
    assert dev(2, FRAMES, 3, C.byref(o), None, off.ctypes.data, 5, None, ptrs, None, None, None) == C1_ERR_ARG
    assert dev(3, FRAMES, 0, C.byref(o), None, off.ctypes.data, 5, None, ptrs, None, None, None) == C1_ERR_ARG
    assert dev(2, FRAMES, 0, None, None, off.ctypes.data, 5, None, ptrs, None, None, None) == C1_ERR_ARG
    assert dev(2, FRAMES, 0, C.byref(o), None, None, 5, None, ptrs, None, None, None) == C1_ERR_ARG
    assert dev(2, 0, 0, C.byref(o), None, off.ctypes.data, 5, None, ptrs, None, None, None) == C1_OK      # frames = 0 writes nothing
    units = np.full((FRAMES * 2, 212), 0xA5, dtype=np.uint8)
    taken = np.full(FRAMES * 2, 0xA5, dtype=np.uint8)
    shifts = np.full((FRAMES * 2, 52), 0x5A, dtype=np.int8)
    dist = np.full((FRAMES * 2, 2), -1.0)
    energy = np.full(FRAMES * 2, -1.0)
    outs = (units.ctypes.data, taken.ctypes.data, shifts.ctypes.data, dist.ctypes.data, energy.ctypes.data)
    host = lambda modes, offsets, n: lib.c1_encode_measured_sf_batch(
        ctx._h, ptrs, 2, FRAMES, 0, C.byref(o), None if modes is None else modes.ctypes.data,
        np.ascontiguousarray(list(offsets) + [0] * 9, dtype=np.int8).ctypes.data, n, *outs)
    for offsets, n, what in (((0,), 0, 'n_offsets = 0'), ((0,), 9, 'n_offsets = 9'), ((0, 1, 1), 3, 'repeats'), ((0, 9), 2, 'outside -8..8'),
                             ((0, -9), 2, 'outside -8..8'), ((1, 0), 2, 'not 0')):
        assert host(None, offsets, n) == C1_ERR_ARG and what in lib.c1_last_error().decode(), (offsets, lib.c1_last_error().decode())
    bad = mat['modes'].reshape(-1).copy()
    bad[77] = 0x10
    assert host(bad, SF.OFFSETS, 5) == C1_ERR_ARG
    assert 'frame 38, channel 1' in lib.c1_last_error().decode() and 'high field' in lib.c1_last_error().decode()
    assert (units == 0xA5).all() and (taken == 0xA5).all() and (shifts == 0x5A).all() and (dist == -1.0).all() and (energy == -1.0).all()
    with pytest.raises(ValueError, match='high field'):
        ctx.encode_measured(mat['body'], modes=bad, scale_factor_offsets=SF.OFFSETS)
    with pytest.raises(ValueError, match='given twice'):
        ctx.encode_measured(mat['body'], scale_factor_offsets=(0, 2, 2))
