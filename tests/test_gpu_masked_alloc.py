"""GPU: the measured allocation with every BFU's error divided by a masking threshold (c1_encode_measured_masked_device / _batch,
k_measured_masked).  weights, distortion, energy, taken, nBfu, word lengths, written scale-factor indices, shifts and bytes
against the CPU model of tests/masked_alloc_lib.py under the packaged tables and under floor = SPECS_PER_BFU; the validity of the
units from their bytes alone; flat tables against c1_encode_measured_sf_* bit for bit; both tables times 4; the geometry of the
new kernel (one wave per unit, four per workgroup, a grid bounded at 2 048 workgroups: 8 192 units per sweep); independence of
chunking, pipeline, overlap, speculation, halo and of which outputs are asked for; that no later call sees the uploaded tables or
a rewritten record; two calls with different tables back to back; a caller's stream; repeatability; the rejections.
tests/test_masked_alloc_cpu.py shows that every decision of the model on this material has a margin above 1e-9."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

import carta1_amd as c1
from carta1_amd import capi
import best_bias_lib as BB
import best_modes_lib as BMO
import masked_alloc_lib as MK
import measured_alloc_lib as MA
import oracle_lib as O
import scale_factor_choice_lib as SF

pytestmark = pytest.mark.gpu

C1_OK, C1_ERR_ARG = 0, 1   # include/carta1_hip.h
FRAMES = BB.FRAMES
OUTPUTS = ('units', 'taken', 'shifts', 'distortion', 'energy', 'weights')
FILL = {'units': 0xA5, 'taken': 0xA5, 'shifts': 0x5A, 'distortion': -1.0, 'energy': -1.0, 'weights': -1.0}
# frames per call, mono and stereo: one wave (1 unit), a partly filled workgroup of four waves (2), many workgroups (63, 64, 65,
# 130, 257) and the seam of the bounded grid, 2 048 workgroups * 4 waves = 8 192 units, past which the waves stride
COUNTS = {1: (1, 2, 63, 64, 65, 130, 257, 8191, 8192, 8193, 8194), 2: (1, 2, 63, 64, 65, 130, 257, 4095, 4096, 4097)}
LARGE = {1: 8400, 2: 4200}
SHORT = 48                                       # frames of the model under given modes, detection and fixed modes


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


def batch(ctx, chans, options=None, modes=None, halo=0, ask=OUTPUTS, offsets=SF.OFFSETS, tables='packaged'):
    """c1_encode_measured_masked_batch with any subset of the outputs; the others are passed as NULL -> dict of the ones asked for"""
    chans = [np.ascontiguousarray(c, dtype=np.float32) for c in chans]
    nch, frames = len(chans), len(chans[0]) // 512 - halo
    n = frames * nch
    o = (options or opts()).to_c()
    shape = {'units': ((n, 212), np.uint8), 'taken': ((n,), np.uint8), 'shifts': ((n, 52), np.int8), 'distortion': ((n, 2), np.float64),
             'energy': ((n,), np.float64), 'weights': ((n, 52), np.float64)}
    out = {k: np.full(s, FILL[k], dtype=d) for k, (s, d) in shape.items()}
    m = None if modes is None else np.ascontiguousarray(modes, dtype=np.uint8).reshape(-1)
    off = np.ascontiguousarray(offsets, dtype=np.int8)
    floor, spread = MK.named(tables) if isinstance(tables, str) else tables
    floor = np.ascontiguousarray(floor, dtype=np.float64)
    spread = None if spread is None else np.ascontiguousarray(spread, dtype=np.float64)
    ptrs = capi.ptr_array([c.ctypes.data + halo * 2048 for c in chans])
    capi.check(capi.load().c1_encode_measured_masked_batch(
        ctx._h, ptrs, nch, frames, halo, C.byref(o), None if m is None else m.ctypes.data, off.ctypes.data, len(off), floor.ctypes.data,
        None if spread is None else spread.ctypes.data, *[out[k].ctypes.data if k in ask else None for k in OUTPUTS]))
    return {k: out[k] for k in ask}


def sf_batch(ctx, chans, options=None, modes=None, offsets=SF.OFFSETS):
    """c1_encode_measured_sf_batch, all five outputs"""
    units, taken, shifts, dist, energy = ctx.encode_measured(chans, modes=modes, options=options, return_distortion=True,
                                                             scale_factor_offsets=offsets, return_shifts=True)
    return {'units': units, 'taken': taken, 'shifts': shifts, 'distortion': dist, 'energy': energy}


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


def against(m, got, offsets):
    print('taken %d of %d; bit-equal: weights %s, T_ref %s, T(n*) %s, E %s' % (
        int(got['taken'].sum()), len(got['taken']), MK.bitwise(got['weights'], m['P']), MK.bitwise(got['distortion'][:, 0], m['D'][:, 0]),
        MK.bitwise(got['distortion'][:, 1], m['D'][:, 1]), MK.bitwise(got['energy'], m['E'])))
    assert MK.check_outputs(m, got['units'], got['taken'], got['shifts'], got['distortion'], got['energy'], got['weights']) is None
    assert MK.check_valid(got['units'], m['coefs'], got['taken'], got['distortion'], got['weights'], offsets) is None
    final = np.where(got['taken'] != 0, got['distortion'][:, 1], got['distortion'][:, 0])
    assert (final <= got['distortion'][:, 0]).all()


# ---- 1. against the model ----
@pytest.mark.parametrize('material,kind,frames,tables,offsets', [
    ('pink', 10, None, 'packaged', SF.OFFSETS), ('white', 58, None, 'packaged', SF.OFFSETS), ('pink', 'detect', SHORT, 'packaged', SF.OFFSETS),
    ('pink', 'modes', SHORT, 'packaged', SF.OFFSETS), ('pink', 'fixed', SHORT, 'packaged', SF.OFFSETS),
    ('pink', 10, None, 'specs', (0,)), ('pink', 'modes', SHORT, 'specs', SF.OFFSETS), ('pink', 10, 65, 'self', (0,))])
def test_against_the_model(ctx, mat, material, kind, frames, tables, offsets):
    """weights, distortion and energy within 1e-12 of the model (exact zeros zero; bit-for-bit equality is expected and printed;
    seen on an MI355X: all four equal bit for bit in every case); taken, nBfu and, where taken, every word length, every written
    scale-factor index and shifts equal to the model's; units the model's bytes, those not taken the plain encode's; weighted
    T_final <= T_ref; and from the bytes alone what scale_factor_choice_lib.check_valid asks, with the reported error the one the
    bytes give under the reported weights.  Under floor = SPECS_PER_BFU both branches of the fallback occur."""
    chans, o, modes = call_of(kind, mat, material, frames)
    m = MK.case(kind, material, tables, offsets, frames)
    got = batch(ctx, chans, o, modes, offsets=offsets, tables=tables)
    against(m, got, offsets)
    if tables == 'specs' and frames is None:
        assert got['taken'].any() and not got['taken'].all()
    plain = ctx.encode(chans, o) if modes is None else ctx.encode_modes(chans, modes, o)
    assert np.array_equal(plain, m['ref'])
    assert np.array_equal(got['units'][got['taken'] == 0], plain[got['taken'] == 0])
    # the Python host: the same call
    res = ctx.encode_measured(chans, modes=modes, options=o, return_distortion=True, scale_factor_offsets=offsets, return_shifts=True,
                              masking=True if tables == 'packaged' else MK.named(tables), return_weights=True)
    assert same(dict(zip(OUTPUTS, res)), got)


def test_masking_alone_means_the_offset_zero(ctx, mat):
    units, taken = ctx.encode_measured(mat['body'], modes=mat['modes'], masking=True)
    got = batch(ctx, mat['body'], None, mat['modes'], offsets=(0,))
    assert np.array_equal(units, got['units']) and np.array_equal(taken, got['taken']) and not got['shifts'].any()


# ---- 2. flat tables are the parent's call; both tables times 4 ----
def test_flat_tables_are_the_scale_factor_choice_call(ctx, mat):
    zeros = np.zeros((52, 52))
    for o, modes in ((None, mat['modes']), (None, None), (opts({'fixedBlockModes': MA.FIXED}), None), (opts({'fixedBlockModes': [0, 0, 0]}), None)):
        want = sf_batch(ctx, mat['body'], o, modes)
        for tables in ('flat', (np.ones(52), zeros)):
            got = batch(ctx, mat['body'], o, modes, tables=tables)
            assert (got.pop('weights') == 1.0).all()
            assert same(got, want)
    got = batch(ctx, mat['body'], None, mat['modes'], offsets=(0,), tables='flat')
    got.pop('weights')
    assert same(got, sf_batch(ctx, mat['body'], None, mat['modes'], offsets=(0,)))


@pytest.mark.parametrize('tables', ['packaged', 'specs', 'self'])
def test_scaling_both_tables_by_four(ctx, mat, tables):
    for modes in (mat['modes'], None):
        a, q = batch(ctx, mat['body'], None, modes, tables=tables), batch(ctx, mat['body'], None, modes, tables=tables + '*4')
        for k in ('units', 'taken', 'shifts'):
            assert np.array_equal(a[k], q[k]), k
        for k in ('distortion', 'energy', 'weights'):
            assert MK.bitwise(q[k], 0.25 * a[k]), k


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
    assert np.isfinite(large['weights']).all() and (large['weights'] > 0).all()
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


# ---- 4. degenerate input, repeatability ----
def test_silence_and_repeatability(ctx, mat):
    silence = [np.zeros(FRAMES * 512, dtype=np.float32)] * 2
    floor = MK.packaged()[0]
    for modes in (None, mat['modes']):
        got = batch(ctx, silence, None, modes)
        assert not got['taken'].any() and not got['shifts'].any()
        assert not got['distortion'].view(np.uint64).any() and not got['energy'].view(np.uint64).any()    # +0.0 exactly
        assert MK.bitwise(got['weights'], np.broadcast_to(1.0 / floor, got['weights'].shape))             # every threshold the floor
        want = O.encode_stream(silence)[0] if modes is None else ctx.encode_modes(silence, modes)
        assert np.array_equal(got['units'], want)
        first = batch(ctx, mat['body'], None, modes)
        assert same(first, batch(ctx, mat['body'], None, modes))                      # run to run


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
        batch(c, mat['body'], None, mat['modes'], ask=('weights',))
        assert c.kernel_ms('pack')[1] == 0 and c.kernel_ms('measure')[1] == chunks   # units NULL: measure only, no packing runs
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
    """every single output and every set of all but one"""
    subsets = [s for k in (1, 5) for s in itertools.combinations(OUTPUTS, k)]
    for kind, modes in (('modes', mat['modes']), ('detect', None)):
        full = baseline[kind]
        for ask in subsets:
            got = batch(ctx, mat['body'], None, modes, ask=ask)
            assert same(got, {k: full[k] for k in ask}), (kind, ask)


def test_later_calls_see_neither_the_tables_nor_a_rewritten_record(ctx, mat, baseline):
    """a measure-only call leaves the records of the context alone, a packing call rewrites them: after either a plain encode gives
    the reference's bytes and c1_encode_measured_sf_* its own outputs"""
    ref = MA.case('modes')['ref']
    sf_before = sf_batch(ctx, mat['body'], None, mat['modes'])
    batch(ctx, mat['body'], None, mat['modes'], ask=('taken', 'shifts', 'distortion', 'energy', 'weights'))
    assert np.array_equal(ctx.encode_modes(mat['body'], mat['modes']), ref)
    assert same(batch(ctx, mat['body'], None, mat['modes']), dict(baseline['modes']))
    assert np.array_equal(ctx.encode_modes(mat['body'], mat['modes']), ref)
    batch(ctx, mat['body'], None, mat['modes'], tables='ramp')
    assert same(sf_batch(ctx, mat['body'], None, mat['modes']), sf_before)
    batch(ctx, mat['body'])
    assert np.array_equal(ctx.encode(mat['body']), MA.case('detect')['ref'])


# ---- 6. the device entry point ----
def _device_buffers(torch, n):
    kinds = {'units': (torch.uint8, n * 212), 'taken': (torch.uint8, n), 'shifts': (torch.int8, n * 52), 'distortion': (torch.float64, n * 2),
             'energy': (torch.float64, n), 'weights': (torch.float64, n * 52)}
    return {k: torch.full((size,), FILL[k], dtype=d, device='cuda') for k, (d, size) in kinds.items()}


def _to_host(t):
    shape = {'units': (-1, 212), 'taken': (-1,), 'shifts': (-1, 52), 'distortion': (-1, 2), 'energy': (-1,), 'weights': (-1, 52)}
    return {k: v.cpu().numpy().reshape(shape[k]) for k, v in t.items()}


def _device_call(c, pcm, modes, t, tables, offsets=SF.OFFSETS):
    c.encode_measured_device([p.data_ptr() for p in pcm], FRAMES, t['units'].data_ptr(), t['taken'].data_ptr(), t['distortion'].data_ptr(),
                             t['energy'].data_ptr(), modes_ptr=modes.data_ptr(), scale_factor_offsets=offsets,
                             shifts_ptr=t['shifts'].data_ptr(), masking=tables, weights_ptr=t['weights'].data_ptr())


def test_two_calls_with_different_tables_back_to_back(ctx, mat, baseline):
    """two device calls queued one behind the other with no host synchronisation between them, each with tables of its own that
    the host overwrites as soon as its call returns: each equals its own model.  This pins the order of the upload on the stream."""
    import torch
    pcm = [torch.from_numpy(x).cuda() for x in mat['body']]
    modes = torch.from_numpy(mat['modes'].reshape(-1).copy()).cuda()
    first, second = _device_buffers(torch, FRAMES * 2), _device_buffers(torch, FRAMES * 2)
    _device_call(ctx, pcm, modes, first, MK.FLAT)                            # warm: workspace, options, the tables' buffer
    ctx.synchronize()
    floor_a, spread_a = (np.array(a) for a in MK.packaged())
    floor_b, spread_b = np.array(MK.explicit('self')[0]), np.array(MK.explicit('self')[1])
    _device_call(ctx, pcm, modes, first, (floor_a, spread_a))
    floor_a[:] = 1.0
    spread_a[:] = 0.0
    _device_call(ctx, pcm, modes, second, (floor_b, spread_b), offsets=(0,))
    floor_b[:] = 1.0
    spread_b[:] = 0.0
    ctx.synchronize()
    assert same(_to_host(first), dict(baseline['modes']))
    # the encoder is causal: the first frames of either call against the model of those frames
    against(MK.case('modes', 'pink', 'packaged', SF.OFFSETS, SHORT), rows(_to_host(first), 0, SHORT, 2), SF.OFFSETS)
    against(MK.case('modes', 'pink', 'self', (0,), SHORT), rows(_to_host(second), 0, SHORT, 2), (0,))


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
        t = _device_buffers(torch, FRAMES * 2)
        busy = torch.ones(1 << 26, dtype=torch.float32, device='cuda')
        torch.cuda.synchronize()
        with torch.cuda.stream(S):
            _device_call(c, pcm, modes, t, MK.FLAT)  # warm: options on the device, workspace grown (these drain the stream)
            S.synchronize()
            for _ in range(200):
                busy.mul_(-1.0)
            for p, x in zip(pcm, src):
                p.copy_(x)
            modes.copy_(src_modes)
            _device_call(c, pcm, modes, t, True)
            snap = {k: v.clone() for k, v in t.items()}
            for p in pcm:
                p.zero_()
            modes.zero_()
            for k, v in t.items():
                v.fill_(FILL[k])
            queued_behind_busy_stream = not S.query()
            S.synchronize()
        assert queued_behind_busy_stream
        assert same(_to_host(snap), dict(baseline['modes']))
    finally:
        c.close()


def test_device_entry_point_stays_in_bounds_for_any_mode_byte(ctx, mat):
    import torch
    units_n = FRAMES * 2
    modes = mat['modes'].reshape(-1).copy()
    at = np.random.RandomState(3).permutation(units_n)[:256]
    modes[at] = np.arange(256, dtype=np.uint8)                      # every byte value, at scattered units
    clean = np.ones(units_n, dtype=bool)
    clean[at] = False
    G = 4096                                                         # guard bytes on either side of every output
    buf = {'units': (torch.uint8, units_n * 212), 'taken': (torch.uint8, units_n), 'shifts': (torch.int8, units_n * 52),
           'distortion': (torch.float64, units_n * 2), 'energy': (torch.float64, units_n), 'weights': (torch.float64, units_n * 52)}
    size = {torch.uint8: 1, torch.int8: 1, torch.float64: 8}
    t = {k: torch.full((2 * G // size[d] + n,), FILL[k], dtype=d, device='cuda') for k, (d, n) in buf.items()}
    dev = [torch.from_numpy(c).cuda() for c in mat['body']]
    d_modes = torch.from_numpy(modes).cuda()
    torch.cuda.synchronize()
    p = {k: t[k].data_ptr() + G for k in OUTPUTS}
    ctx.encode_measured_device([d.data_ptr() for d in dev], FRAMES, p['units'], p['taken'], p['distortion'], p['energy'],
                               modes_ptr=d_modes.data_ptr(), scale_factor_offsets=SF.OFFSETS, shifts_ptr=p['shifts'], masking=True,
                               weights_ptr=p['weights'])
    ctx.synchronize()
    assert np.array_equal(d_modes.cpu().numpy(), modes)
    want_all = batch(ctx, mat['body'], None, mat['modes'])
    for k, (d, n) in buf.items():
        g = G // size[d]
        a = t[k].cpu().numpy()
        assert (a[:g] == FILL[k]).all() and (a[-g:] == FILL[k]).all(), k
        got = a[g:-g].reshape(units_n, -1)
        want = want_all[k].reshape(units_n, -1)
        assert np.array_equal(got[clean].view(np.uint8), want[clean].view(np.uint8)), k     # a unit's frame reads no other unit's mode byte
    assert set(t['taken'].cpu().numpy()[G:-G].tolist()) <= {0, 1}
    assert set(np.unique(t['shifts'].cpu().numpy()[G:-G]).tolist()) <= set(SF.OFFSETS)


def test_rejections_leave_the_outputs_untouched(ctx, mat):
    lib = capi.load()
    o = opts().to_c()
    ptrs = capi.ptr_array([c.ctypes.data for c in mat['body']])
    off = np.array(SF.OFFSETS, dtype=np.int8)
    floor, spread = (np.ascontiguousarray(a) for a in MK.packaged())
    dev = lambda *a: lib.c1_encode_measured_masked_device(ctx._h, ptrs, *a)
    tab = (floor.ctypes.data, spread.ctypes.data)
    assert dev(2, FRAMES, 0, C.byref(o), None, off.ctypes.data, 5, *tab, None, None, None, None, None, None) == C1_ERR_ARG
    assert 'all NULL' in lib.c1_last_error().decode()
    assert dev(2, FRAMES, 3, C.byref(o), None, off.ctypes.data, 5, *tab, None, ptrs, None, None, None, None) == C1_ERR_ARG
    assert dev(3, FRAMES, 0, C.byref(o), None, off.ctypes.data, 5, *tab, None, ptrs, None, None, None, None) == C1_ERR_ARG
    assert dev(2, FRAMES, 0, None, None, off.ctypes.data, 5, *tab, None, ptrs, None, None, None, None) == C1_ERR_ARG
    assert dev(2, FRAMES, 0, C.byref(o), None, None, 5, *tab, None, ptrs, None, None, None, None) == C1_ERR_ARG
    assert dev(2, FRAMES, 0, C.byref(o), None, off.ctypes.data, 5, None, None, None, ptrs, None, None, None, None) == C1_ERR_ARG
    assert 'mask_floor is NULL' in lib.c1_last_error().decode()
    assert dev(2, 0, 0, C.byref(o), None, off.ctypes.data, 5, *tab, None, ptrs, None, None, None, None) == C1_OK      # frames = 0 writes nothing
    n = FRAMES * 2
    out = {'units': np.full((n, 212), 0xA5, dtype=np.uint8), 'taken': np.full(n, 0xA5, dtype=np.uint8), 'shifts': np.full((n, 52), 0x5A, dtype=np.int8),
           'distortion': np.full((n, 2), -1.0), 'energy': np.full(n, -1.0), 'weights': np.full((n, 52), -1.0)}
    outs = [out[k].ctypes.data for k in OUTPUTS]

    def host(f=floor, s=spread, offsets=SF.OFFSETS, modes=None, fn=lib.c1_encode_measured_masked_batch, p=ptrs):
        f, s = np.ascontiguousarray(f), None if s is None else np.ascontiguousarray(s)
        return fn(ctx._h, p, 2, FRAMES, 0, C.byref(o), None if modes is None else modes.ctypes.data,
                  np.ascontiguousarray(list(offsets) + [0] * 9, dtype=np.int8).ctypes.data, len(offsets), f.ctypes.data,
                  None if s is None else s.ctypes.data, *outs)

    dptr = capi.ptr_array([0x1000, 0x2000])        # the device call decides on the tables before it touches a pointer
    for fn, p in ((lib.c1_encode_measured_masked_batch, ptrs), (lib.c1_encode_measured_masked_device, dptr)):
        for v in (0.0, -1.0, np.nan, np.inf, 1e-61, 1e61):
            f = floor.copy()
            f[7] = v
            assert host(f=f, fn=fn, p=p) == C1_ERR_ARG and 'mask_floor[7]' in lib.c1_last_error().decode(), (v, lib.c1_last_error().decode())
        for v in (-1.0, np.nan, 1e61):
            s = spread.copy()
            s[3, 9] = v
            assert host(s=s, fn=fn, p=p) == C1_ERR_ARG and 'mask_spread[165]' in lib.c1_last_error().decode(), (v, lib.c1_last_error().decode())
    assert host(offsets=(0, 9)) == C1_ERR_ARG and 'outside -8..8' in lib.c1_last_error().decode()
    bad = mat['modes'].reshape(-1).copy()
    bad[77] = 0x10
    assert host(modes=bad) == C1_ERR_ARG
    assert 'frame 38, channel 1' in lib.c1_last_error().decode() and 'high field' in lib.c1_last_error().decode()
    assert all((out[k] == FILL[k]).all() for k in OUTPUTS)
    with pytest.raises(ValueError, match=r'mask_spread\[165\]'):
        ctx.encode_measured(mat['body'], masking=(floor, np.where(np.arange(52 * 52).reshape(52, 52) == 165, -1.0, spread)))
    with pytest.raises(c1.Carta1Error, match=r'mask_floor\[0\]'):
        ctx.encode_measured_device([0x1000, 0x2000], FRAMES, units_ptr=0x3000, masking=(np.zeros(52), None))
