"""GPU: the coding error of given sound units against their PCM (c1_measure_units_device / _batch, k_measure_units).  noise,
signal, totals and weights against the CPU model of tests/measure_units_lib.py for the units of plain encodes, flat and under the
packaged tables; totals and weights against what c1_encode_measured_*, _sf_ and _masked_ report for the units they pack, bit for
bit; foreign bytes through the device entry point between guard words; a corrupted stream; the geometry of the kernel (one wave
per unit, four per workgroup, a grid bounded at 2 048 workgroups); independence of chunking, pipeline, overlap, speculation, halo
and of which outputs are asked for; a caller's stream; two calls with different tables back to back; the rejections; the timing
kind.  tests/test_measure_units_cpu.py shows the model to agree bit for bit with the models of the measured allocation."""
import itertools
import os

import numpy as np
import pytest

import carta1_amd as c1
from carta1_amd import capi
import best_bias_lib as BB
import best_modes_lib as BMO
import masked_alloc_lib as MK
import measure_units_lib as MU
import measured_alloc_lib as MA
import scale_factor_choice_lib as SF

pytestmark = pytest.mark.gpu

C1_OK, C1_ERR_ARG = 0, 1   # include/carta1_hip.h
FRAMES = BB.FRAMES
OUTPUTS = ('noise', 'signal', 'totals', 'weights')
WIDTH = {'noise': 52, 'signal': 52, 'totals': 2, 'weights': 52}
FILL = -1.0
SHORT = 48                                       # frames of the model where the whole material is not needed
COUNTS = (1, 2, 3, 4, 5, 63, 64, 65, 130)


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


class _env:
    """an environment variable the library reads at every launch"""
    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        os.environ.update({k: str(v) for k, v in self.kv.items()})

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def tables_of(name):
    return (None, None) if name is None else MK.named(name)


def measure(ctx, chans, units, tables=None, halo=0, ask=OUTPUTS):
    """c1_measure_units_batch with any subset of the outputs; the others are passed as NULL -> dict of the ones asked for.
    tables: None, a name of masked_alloc_lib.named, or a (floor, spread) pair"""
    chans = [np.ascontiguousarray(c, dtype=np.float32) for c in chans]
    nch, frames = len(chans), len(chans[0]) // 512 - halo
    n = frames * nch
    u = np.ascontiguousarray(units, dtype=np.uint8).reshape(-1, 212)
    assert u.shape[0] == n
    if tables is None:
        ask = tuple(k for k in ask if k != 'weights')
    floor, spread = tables_of(tables) if tables is None or isinstance(tables, str) else tables
    floor = None if floor is None else np.ascontiguousarray(floor, dtype=np.float64)
    spread = None if spread is None else np.ascontiguousarray(spread, dtype=np.float64)
    out = {k: np.full((n, WIDTH[k]), FILL) for k in OUTPUTS}
    ptrs = capi.ptr_array([c.ctypes.data + halo * 2048 for c in chans])
    capi.check(capi.load().c1_measure_units_batch(
        ctx._h, ptrs, nch, frames, halo, u.ctypes.data, None if floor is None else floor.ctypes.data,
        None if spread is None else spread.ctypes.data, *[out[k].ctypes.data if k in ask else None for k in OUTPUTS]))
    assert all((out[k] == FILL).all() for k in OUTPUTS if k not in ask)
    return {k: out[k] for k in ask}


def same(a, b):
    """bitwise equality of two output dicts (doubles compared as bit patterns)"""
    return a.keys() == b.keys() and all(np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) for k in a)


def rows(out, a, b, nch):
    return {k: v[a * nch:b * nch] for k, v in out.items()}


@pytest.fixture(scope='module')
def mat(ctx):
    with_halo, body = BB.material()
    modes = BB.given_modes()
    m = {'with_halo': with_halo, 'body': body, 'modes': modes, 'white': BMO.material('white')}
    m['units'] = ctx.encode_modes(body, modes)                 # plain units over the whole domain of the modes
    m['units_halo'] = ctx.encode_modes(with_halo, np.concatenate([np.zeros((2, 2), dtype=np.uint8), modes]))
    m['units'].setflags(write=False)
    return m


_models = {}


def model_of(key, chans, units, tables=None):
    """the model of these units, its sums computed once per key and shared by every table set"""
    if key not in _models:
        _models[key] = MU.model(chans, units)
    return MU.with_tables(_models[key], *tables_of(tables))


def against(m, got):
    print('bit-equal: ' + ', '.join('%s %s' % (k, MU.bitwise(got[k], m[k])) for k in got))
    assert MU.check_outputs(m, got) is None


# ---- 1. against the model ----
@pytest.mark.parametrize('kind', ['detect', 'fixed', 0, 10, 58, 'modes'])
def test_plain_units_against_the_model(ctx, mat, kind):
    """noise, signal, totals and weights within 1e-12 of the model, exact zeros zero, flat and under the packaged tables;
    bit-for-bit equality is expected and printed (seen on an MI355X: equal in every case)"""
    n = FRAMES if kind == 10 else SHORT
    chans = [c[:n * 512] for c in mat['body']]
    if kind == 'detect':
        units = ctx.encode(chans)
    elif kind == 'fixed':
        units = ctx.encode(chans, opts({'fixedBlockModes': MA.FIXED}))
    elif kind == 'modes':
        units = mat['units'][:n * 2]
    else:
        units = ctx.encode_modes(chans, np.full((n, 2), kind, dtype=np.uint8))
    for tables in (None, 'packaged'):
        got = measure(ctx, chans, units, tables)
        against(model_of(('plain', kind), chans, units, tables), got)
        assert (got['signal'] > 0).any() and (got['noise'] > 0).any()
        # the Python host: the same call
        res = ctx.measure_units(chans, units, masking=None if tables is None else True, return_weights=tables is not None)
        assert same(dict(zip(OUTPUTS, res)), got)
    if kind == 'modes':
        white = [c[:SHORT * 512] for c in mat['white']]
        units = ctx.encode(white, opts({'allocationBias': 2.0}))
        against(model_of(('white', 'bias2'), white, units, 'packaged'), measure(ctx, white, units, 'packaged'))


# ---- 2. against the library's own reports, bit for bit ----
@pytest.mark.parametrize('offsets,tables', [(None, None), (SF.OFFSETS, None), (SF.OFFSETS, 'packaged'), ((0,), 'specs')])
@pytest.mark.parametrize('given', [True, False])
def test_the_measured_calls_report_what_their_units_hold(ctx, mat, offsets, tables, given):
    """totals[:, 0] == distortion[u, taken[u]], totals[:, 1] == energy and weights equal for the units c1_encode_measured_*,
    _sf_ and _masked_ pack; for the plain units totals[:, 0] == distortion[:, 0]"""
    modes = mat['modes'] if given else None
    masking = None if tables is None else (True if tables == 'packaged' else MK.named(tables))
    res = ctx.encode_measured(mat['body'], modes=modes, return_distortion=True, scale_factor_offsets=offsets, masking=masking,
                              return_weights=masking is not None)
    units, taken, dist, energy = res[0], res[1], res[2], res[3]
    assert taken.any()
    got = measure(ctx, mat['body'], units, tables)
    final = np.where(taken != 0, dist[:, 1], dist[:, 0])
    print('bit-equal: T %s, E %s' % (MU.bitwise(got['totals'][:, 0], final), MU.bitwise(got['totals'][:, 1], energy)))
    assert MU.bitwise(got['totals'][:, 0], final)
    assert MU.bitwise(got['totals'][:, 1], energy)
    if masking is not None:
        assert MU.bitwise(got['weights'], res[4])
    plain = ctx.encode_modes(mat['body'], modes) if given else ctx.encode(mat['body'])
    ref = measure(ctx, mat['body'], plain, tables)
    assert MU.bitwise(ref['totals'][:, 0], dist[:, 0]) and MU.bitwise(ref['totals'][:, 1], energy)
    assert MU.bitwise(ref['signal'], got['signal'])


def test_one_candidate_of_best_modes_within_rounding(ctx, mat):
    for byte in (0, 10, 58):
        units, choice, modes, D, E = ctx.encode_best_modes(mat['body'], [byte], return_distortion=True)
        got = measure(ctx, mat['body'], units)
        assert MU.close(D[:, 0], got['totals'][:, 0]) and MU.close(E[:, 0], got['totals'][:, 1]), byte


# ---- 3. foreign bytes, a corrupted stream ----
def _device_buffers(torch, n, guard):
    g = guard // 8
    return {k: torch.full((2 * g + n * WIDTH[k],), FILL, dtype=torch.float64, device='cuda') for k in OUTPUTS}


def _device_call(c, pcm, frames, units, t, tables, guard=0):
    p = {k: t[k].data_ptr() + guard for k in OUTPUTS}
    c.measure_units_device([x.data_ptr() for x in pcm], frames, units.data_ptr(), p['noise'], p['signal'], p['totals'], p['weights'],
                           masking=tables)


def _to_host(t, n, guard=0):
    g = guard // 8
    out = {}
    for k, v in t.items():
        a = v.cpu().numpy()
        assert (a[:g] == FILL).all() and (a[len(a) - g:] == FILL).all(), k          # the words around the output are untouched
        out[k] = a[g:len(a) - g].reshape(n, WIDTH[k])
    return out


@pytest.mark.parametrize('domain', [True, False])
def test_foreign_bytes_through_the_device_entry_point(ctx, mat, domain):
    """512 units of random bytes (domain: the mode bits rewritten to a random byte of the domain; else raw, mode bits included):
    every unit is measured, the outputs are the model's (under mode_in_domain for the raw bytes), and the 4 096 bytes on either
    side of every output keep their fill.  The host call agrees where it accepts the units and names the first it rejects"""
    import torch
    frames, G = 256, 4096
    chans = [np.tile(c, 2)[:frames * 512] for c in mat['body']]
    units = MU.random_units(20261019 + int(domain), frames * 2, domain)
    m = MU.with_tables(MU.model(chans, units, device=not domain), *MK.packaged())
    assert len(set(m['bytes'].tolist())) == 8
    pcm = [torch.from_numpy(x).cuda() for x in chans]
    d_units = torch.from_numpy(units).cuda()
    t = _device_buffers(torch, frames * 2, G)
    _device_call(ctx, pcm, frames, d_units, t, True, G)
    ctx.synchronize()
    assert np.array_equal(d_units.cpu().numpy(), units)
    got = _to_host(t, frames * 2, G)
    against(m, got)
    assert np.isfinite(got['noise']).all() and (got['noise'] > 0).all(axis=1).any()
    if domain:
        assert same(measure(ctx, chans, units, 'packaged'), got)
    else:
        with pytest.raises(c1.Carta1Error, match='block mode of the unit'):
            measure(ctx, chans, units, 'packaged')


def test_a_corrupted_stream(ctx, mat):
    """one bit flipped in ten units of a measured stream (behind the mode bits): only those units' rows change"""
    units, taken = ctx.encode_measured(mat['body'], modes=mat['modes'], scale_factor_offsets=SF.OFFSETS, masking=True)
    clean = measure(ctx, mat['body'], units, 'packaged')
    rs = np.random.RandomState(9)
    hit = np.sort(rs.permutation(units.shape[0])[:10])
    bad = units.copy()
    for u in hit:
        bit = int(rs.randint(16, 600))                           # amount, word lengths, scale factors, the first mantissas
        bad[u, bit >> 3] ^= 0x80 >> (bit & 7)
    got = measure(ctx, mat['body'], bad, 'packaged')
    changed = np.flatnonzero((got['noise'] != clean['noise']).any(axis=1) | (got['totals'] != clean['totals']).any(axis=1))
    assert set(changed.tolist()) <= set(hit.tolist()) and len(changed) >= 1
    keep = np.ones(units.shape[0], dtype=bool)
    keep[hit] = False
    assert same({k: v[keep] for k, v in got.items()}, {k: v[keep] for k, v in clean.items()})
    assert MU.bitwise(got['signal'], clean['signal']) and MU.bitwise(got['weights'], clean['weights'])   # the PCM's alone
    # the frames up to the second corrupted unit against the model of the corrupted bytes
    frames = int(hit[1]) // 2 + 1
    m = MU.with_tables(MU.model([c[:frames * 512] for c in mat['body']], bad[:frames * 2]), *MK.packaged())
    against(m, rows(got, 0, frames, 2))


# ---- 4. geometry ----
@pytest.fixture(scope='module')
def baseline(ctx, mat):
    out = {t: measure(ctx, mat['body'], mat['units'], t) for t in (None, 'packaged')}
    for v in out.values():
        for a in v.values():
            a.setflags(write=False)
    return out


@pytest.mark.parametrize('nch', [1, 2])
def test_frame_counts_and_the_stride_of_the_grid(ctx, mat, baseline, nch):
    """the rows of the whole call (the encoder is causal) for every count, also when the grid is bounded at 1 or 3 workgroups, so
    that the waves stride over the units with and without a remainder"""
    chans = mat['body'][:nch]
    units = np.ascontiguousarray(mat['units'].reshape(FRAMES, 2, 212)[:, :nch]).reshape(-1, 212)
    whole = measure(ctx, chans, units, 'packaged')
    if nch == 2:
        assert same(whole, dict(baseline['packaged']))
    else:
        assert same(whole, {k: v[0::2] for k, v in baseline['packaged'].items()})
    for blocks in (None, 1, 3):
        with _env(**({} if blocks is None else {'C1_METER_BLOCKS': blocks})):
            for frames in COUNTS:
                got = measure(ctx, [c[:frames * 512] for c in chans], units[:frames * nch], 'packaged')
                assert same(got, rows(whole, 0, frames, nch)), (blocks, frames, nch)


def test_the_seam_of_the_bounded_grid(ctx, mat):
    """2 048 workgroups of four waves: 8 192 units per sweep.  One unit either side of the seam, against a grid that never strides"""
    n = 8193
    reps = -(-n // FRAMES)
    chan = np.tile(mat['body'][0], reps)[:n * 512]
    units = np.tile(mat['units'][0::2], (reps, 1))[:n]
    with _env(C1_METER_BLOCKS=4096):
        want = measure(ctx, [chan], units, 'packaged')
    for frames in (8191, 8192, 8193):
        got = measure(ctx, [chan[:frames * 512]], units[:frames], 'packaged')
        assert same(got, rows(want, 0, frames, 1)), frames
    assert (want['noise'][8192] > 0).any()


@pytest.mark.parametrize('halo', [1, 2])
def test_halo_with_the_same_real_history(ctx, mat, halo):
    part = [c[(2 - halo) * 512:] for c in mat['with_halo']]
    units = mat['units_halo'][(2 - halo) * 2:]
    whole = measure(ctx, part, units, 'packaged')
    got = measure(ctx, part, units[halo * 2:], 'packaged', halo=halo)
    assert same(got, rows(whole, halo, halo + FRAMES, 2))


@pytest.mark.parametrize('env', [{'C1_CHUNK_FRAMES': 7}, {'C1_CHUNK_FRAMES': 64}, {'C1_PIPELINE': 0}, {'C1_PIPELINE': 1},
                                 {'C1_CHUNK_FRAMES': 64, 'C1_PIPELINE': 1, 'C1_OVERLAP': 1}],
                         ids=['chunk7', 'chunk64', 'unpiped', 'piped', 'chunk64-piped-overlap'])
def test_outputs_do_not_depend_on_chunks_pipeline_or_speculation(mat, baseline, env):
    c = _context(**env)
    try:
        for mode in (0, 1, 2):
            c.set_speculation(mode)
            for t in (None, 'packaged'):
                assert same(measure(c, mat['body'], mat['units'], t), dict(baseline[t])), (env, mode, t)
        # the timing kind: one launch of the meter per chunk, the analysis beside it, nothing else
        c.set_profiling(True)
        measure(c, mat['body'], mat['units'], 'packaged')
        chunks = -(-FRAMES // max(env['C1_CHUNK_FRAMES'], 16)) if 'C1_CHUNK_FRAMES' in env else 1   # a context's chunk is at least 16 frames
        ms, launches = c.kernel_ms('meter')
        assert launches == chunks and ms > 0
        assert c.kernel_ms('analysis')[1] == chunks
        assert all(c.kernel_ms(k)[1] == 0 for k in ('allocate', 'pack', 'measure', 'choose'))
    finally:
        c.close()


# ---- 5. outputs ----
def test_outputs_do_not_depend_on_which_are_asked_for(ctx, mat, baseline):
    """every single output and every set of all but one; the call twice"""
    for ask in [s for k in (1, 3) for s in itertools.combinations(OUTPUTS, k)]:
        assert same(measure(ctx, mat['body'], mat['units'], 'packaged', ask=ask), {k: baseline['packaged'][k] for k in ask}), ask
    for ask in [s for k in (1, 2) for s in itertools.combinations(OUTPUTS[:3], k)]:
        assert same(measure(ctx, mat['body'], mat['units'], None, ask=ask), {k: baseline[None][k] for k in ask}), ask
    assert same(measure(ctx, mat['body'], mat['units'], 'packaged'), dict(baseline['packaged']))
    assert same(measure(ctx, mat['body'], mat['units'], None), dict(baseline[None]))
    # flat tables: weights exactly 1 and the plain totals
    flat = measure(ctx, mat['body'], mat['units'], 'flat')
    assert (flat.pop('weights') == 1.0).all() and same(flat, dict(baseline[None]))


def test_silence_gives_zeros(ctx, mat):
    silence = [np.zeros(FRAMES * 512, dtype=np.float32)] * 2
    units = ctx.encode(silence)
    got = measure(ctx, silence, units, 'packaged')
    for k in ('noise', 'signal', 'totals'):
        assert not got[k].view(np.uint64).any(), k                                   # +0.0 exactly
    assert MU.bitwise(got['weights'], np.broadcast_to(1.0 / MK.packaged()[0], got['weights'].shape))
    # the units of a signal against silence: the noise is what the units decode to, the signal nothing
    got = measure(ctx, silence, mat['units'])
    assert not got['signal'].view(np.uint64).any() and (got['noise'] > 0).any() and MU.bitwise(got['totals'][:, 1], np.zeros(FRAMES * 2))


def test_non_finite_pcm_gives_non_finite_outputs(ctx, mat):
    chans = [np.array(c[:8 * 512]) for c in mat['body']]
    chans[1][3 * 512 + 17] = np.nan
    got = measure(ctx, chans, mat['units'][:16], 'packaged')
    assert np.isnan(got['totals'][7]).all() and np.isfinite(got['totals'][0:6]).all() and np.isfinite(got['totals'][0::2]).all()
    assert np.isfinite(got['weights']).all()


# ---- 6. the caller's stream, tables back to back ----
def test_two_calls_with_different_tables_back_to_back(ctx, mat, baseline):
    """two device calls queued one behind the other with no host synchronisation between them, each with tables of its own that
    the host overwrites as soon as its call returns: each equals its own model.  This pins the order of the upload on the stream."""
    import torch
    pcm = [torch.from_numpy(x).cuda() for x in mat['body']]
    units = torch.from_numpy(np.array(mat['units'])).cuda()
    n = FRAMES * 2
    first, second = _device_buffers(torch, n, 0), _device_buffers(torch, n, 0)
    _device_call(ctx, pcm, FRAMES, units, first, MK.FLAT)                    # warm: workspace, the tables' buffer
    ctx.synchronize()
    floor_a, spread_a = (np.array(a) for a in MK.packaged())
    floor_b, spread_b = np.array(MK.explicit('self')[0]), np.array(MK.explicit('self')[1])
    _device_call(ctx, pcm, FRAMES, units, first, (floor_a, spread_a))
    floor_a[:] = 1.0
    spread_a[:] = 0.0
    _device_call(ctx, pcm, FRAMES, units, second, (floor_b, spread_b))
    floor_b[:] = 1.0
    spread_b[:] = 0.0
    ctx.synchronize()
    assert same(_to_host(first, n), dict(baseline['packaged']))
    key = ('plain', 'modes')
    short = [c[:SHORT * 512] for c in mat['body']]
    against(model_of(key, short, mat['units'][:SHORT * 2], 'packaged'), rows(_to_host(first, n), 0, SHORT, 2))
    against(model_of(key, short, mat['units'][:SHORT * 2], 'self'), rows(_to_host(second, n), 0, SHORT, 2))


def test_on_a_callers_stream(mat, baseline):
    """PCM and units are written by work queued just before the call and the outputs are read by work queued just after, with
    no host synchronisation in between; then inputs and outputs are overwritten behind it"""
    import torch
    S = torch.cuda.Stream()
    c = _context(stream=S.cuda_stream)
    try:
        src = [torch.from_numpy(x).cuda() for x in mat['body']]
        src_units = torch.from_numpy(np.array(mat['units'])).cuda()
        pcm = [torch.zeros_like(x) for x in src]
        units = torch.zeros_like(src_units)
        n = FRAMES * 2
        t = _device_buffers(torch, n, 0)
        busy = torch.ones(1 << 26, dtype=torch.float32, device='cuda')
        torch.cuda.synchronize()
        with torch.cuda.stream(S):
            _device_call(c, pcm, FRAMES, units, t, MK.FLAT)   # warm: workspace grown (this drains the stream)
            S.synchronize()
            for _ in range(200):
                busy.mul_(-1.0)
            for p, x in zip(pcm, src):
                p.copy_(x)
            units.copy_(src_units)
            _device_call(c, pcm, FRAMES, units, t, True)
            snap = {k: v.clone() for k, v in t.items()}
            for p in pcm:
                p.zero_()
            units.zero_()
            for v in t.values():
                v.fill_(FILL)
            queued_behind_busy_stream = not S.query()
            S.synchronize()
        assert queued_behind_busy_stream
        assert same(_to_host(snap, n), dict(baseline['packaged']))
    finally:
        c.close()


# ---- 7. the rejections ----
def test_rejections_leave_the_outputs_untouched(ctx, mat, baseline):
    lib = capi.load()
    err = lambda: lib.c1_last_error().decode()
    ptrs = capi.ptr_array([c.ctypes.data for c in mat['body']])
    floor, spread = (np.ascontiguousarray(a) for a in MK.packaged())
    n = FRAMES * 2
    out = {k: np.full((n, WIDTH[k]), FILL) for k in OUTPUTS}
    outs = [out[k].ctypes.data for k in OUTPUTS]
    units = np.array(mat['units'])
    dptr = capi.ptr_array([0x1000, 0x2000])        # the device call decides on its arguments before it touches a pointer

    def call(fn, p, f=floor, s=spread, u=units, o=outs, nch=2, frames=FRAMES, halo=0):
        f = None if f is None else np.ascontiguousarray(f)
        s = None if s is None else np.ascontiguousarray(s)
        return fn(ctx._h, p, nch, frames, halo, u if isinstance(u, int) or u is None else u.ctypes.data, None if f is None else f.ctypes.data,
                  None if s is None else s.ctypes.data, *o)

    for fn, p, u in ((lib.c1_measure_units_batch, ptrs, units), (lib.c1_measure_units_device, dptr, 0x3000)):
        bad = floor.copy()
        bad[7] = 0.0
        assert call(fn, p, f=bad, u=u) == C1_ERR_ARG and 'mask_floor[7]' in err(), err()
        bad = spread.copy()
        bad[3, 9] = -1.0
        assert call(fn, p, s=bad, u=u) == C1_ERR_ARG and 'mask_spread[165]' in err(), err()
        assert call(fn, p, u=u, o=[None] * 4) == C1_ERR_ARG and 'all NULL' in err(), err()
        assert call(fn, p, f=None, u=u) == C1_ERR_ARG and 'mask_spread needs mask_floor' in err(), err()
        assert call(fn, p, f=None, s=None, u=u) == C1_ERR_ARG and 'weights needs mask_floor' in err(), err()
        assert call(fn, p, u=None) == C1_ERR_ARG and 'units is NULL' in err(), err()
        assert call(fn, p, u=u, nch=3) == C1_ERR_ARG and call(fn, p, u=u, halo=3) == C1_ERR_ARG and call(fn, p, u=u, frames=-1) == C1_ERR_ARG
        assert call(fn, None, u=u) == C1_ERR_ARG and 'pcm is NULL' in err(), err()
    assert call(lib.c1_measure_units_device, dptr, u=0x3001) == C1_ERR_ARG and '4-byte aligned' in err(), err()
    assert call(lib.c1_measure_units_device, capi.ptr_array([0x1000, 0x2004]), u=0x3000) == C1_ERR_ARG and '16-byte aligned' in err(), err()
    assert call(lib.c1_measure_units_batch, ptrs, frames=(1 << 22) + 1) == C1_ERR_ARG and 'at most' in err(), err()
    bad = units.copy()
    bad[77, 0] = (bad[77, 0] & 0xF3) | 0x04                     # high field 1: block mode 2
    assert call(lib.c1_measure_units_batch, ptrs, u=bad) == C1_ERR_ARG
    assert 'frame 38, channel 1: high block mode of the unit is 2, not 0 or 3' in err(), err()
    assert call(lib.c1_measure_units_batch, ptrs, frames=0) == C1_OK and call(lib.c1_measure_units_device, dptr, u=0x3000, frames=0) == C1_OK
    assert all((out[k] == FILL).all() for k in OUTPUTS)
    with pytest.raises(ValueError, match='high block mode'):
        ctx.measure_units(mat['body'], bad)
    with pytest.raises(c1.Carta1Error, match=r'mask_floor\[0\]'):
        ctx.measure_units_device([0x1000, 0x2000], FRAMES, 0x3000, totals_ptr=0x4000, masking=(np.zeros(52), None))
    # the next call is unharmed
    assert same(measure(ctx, mat['body'], mat['units'], 'packaged'), dict(baseline['packaged']))
    assert np.array_equal(ctx.encode_modes(mat['body'], mat['modes']), mat['units'])
