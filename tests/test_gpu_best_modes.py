"""GPU: the block modes of every sound unit chosen from candidates by least coding error (c1_encode_best_modes_device / _batch,
k_choose_modes).  The five outputs against the CPU model of tests/best_modes_lib.py (built from the oracle alone) on both
materials; candidate subsets and orders; the all-long candidate against k_choose_bias; the geometry of the measuring kernel (one
wave per unit, four waves per workgroup, a grid bounded at 2 048 workgroups: 8 192 units per sweep; the composing kernels have
one lane per item and no bound); independence of chunking, pipeline, speculation, halo and of which outputs are asked for;
repeatability and silence; the device entry point on a caller's stream and on bad candidates.
tests/test_best_modes_cpu.py shows that on this material every unit has exactly one admissible candidate, that four candidates
win often on the pink material, that all-long is wrong in 99.6 % of its units and right in half of the white material's."""
import ctypes as C
import os

import numpy as np
import pytest

import carta1_amd as c1
from carta1_amd import capi, codec
import best_bias_lib as BB
import best_modes_lib as BMO
import block_modes_lib as BM

pytestmark = pytest.mark.gpu

C1_OK, C1_ERR_ARG = 0, 1   # include/carta1_hip.h
FRAMES = BB.FRAMES
CAND8 = BMO.CANDIDATES
OUTPUTS = ('units', 'choice', 'modes', 'distortion', 'energy')
# frames per call, mono and stereo: one wave of k_choose_modes (1 unit), a partly filled workgroup of four waves and its seam
# (2 .. 5), the counts of the issue (63, 64, 65, 130, 257: many workgroups), and the seam of the bounded grid, 2 048 workgroups *
# 4 waves = 8 192 units, past which the waves stride (mono 8 191 .. 8 193 units, stereo 8 190 .. 8 194)
COUNTS = {1: (1, 2, 3, 4, 5, 63, 64, 65, 130, 257, 8191, 8192, 8193), 2: (1, 2, 3, 4, 5, 63, 64, 65, 130, 257, 4095, 4096, 4097)}
LARGE = {1: 8400, 2: 4200}


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
    return {'with_halo': with_halo, 'body': body, 'white': BMO.material('white')}


def batch(ctx, chans, cand, halo=0, ask=OUTPUTS, options=None):
    """c1_encode_best_modes_batch with any subset of the outputs; the others are passed as NULL -> dict of the ones asked for"""
    chans = [np.ascontiguousarray(c, dtype=np.float32) for c in chans]
    nch, frames, n = len(chans), len(chans[0]) // 512 - halo, len(cand)
    out = {'units': np.full((frames * nch, 212), 0xA5, dtype=np.uint8), 'choice': np.full(frames * nch, 0xA5, dtype=np.uint8),
           'modes': np.full(frames * nch, 0xA5, dtype=np.uint8), 'distortion': np.full((frames * nch, n), -1.0),
           'energy': np.full((frames * nch, n), -1.0)}
    cb = np.asarray(cand, dtype=np.uint8)
    opts = (options or c1.EncoderOptions()).to_c()
    ptrs = capi.ptr_array([c.ctypes.data + halo * 2048 for c in chans])
    capi.check(capi.load().c1_encode_best_modes_batch(ctx._h, ptrs, nch, frames, halo, C.byref(opts), cb.ctypes.data, n,
                                                      *[out[k].ctypes.data if k in ask else None for k in OUTPUTS]))
    return {k: out[k] for k in ask}


def same(a, b):
    """bitwise equality of two output dicts (doubles compared as bit patterns)"""
    return a.keys() == b.keys() and all(np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) for k in a)


def rows(out, a, b, nch):
    return {k: v[a * nch:b * nch] for k, v in out.items()}


# ---- 1. against the model ----
@pytest.mark.parametrize('kind', ['pink', 'white'])
def test_against_the_model(ctx, mat, kind):
    chans = mat['body'] if kind == 'pink' else mat['white']
    units, choice, modes, dist, energy = ctx.encode_best_modes(chans, CAND8, return_distortion=True)
    m = BMO.case(kind)
    print('largest relative error of D %.3g, of E %.3g' % (np.max(np.abs(dist - m['D']) / m['D']), np.max(np.abs(energy - m['E']) / m['E'])))
    print('winners', np.bincount(choice, minlength=8).tolist())
    assert BMO.check_outputs(kind, units, choice, modes, dist, energy) is None
    assert np.array_equal(units, ctx.encode_modes(chans, modes.reshape(-1, 2)))
    u2, c2, m2 = ctx.encode_best_modes(chans, [BM.triple_of(b) for b in CAND8])      # triples, and without the report
    assert np.array_equal(u2, units) and np.array_equal(c2, choice) and np.array_equal(m2, modes)


# ---- 2. candidate subsets ----
def test_candidate_subsets_and_order(ctx, mat):
    body = mat['body']
    for byte in (0, 58, 10):
        got = batch(ctx, body, [byte])
        assert not got['choice'].any() and (got['modes'] == byte).all()
        assert np.array_equal(got['units'], ctx.encode_modes(body, np.full((FRAMES, 2), byte, dtype=np.uint8))), byte
        assert BMO.check_outputs('pink', got['units'], got['choice'], got['modes'], got['distortion'], got['energy'], [CAND8.index(byte)]) is None
    a, b = batch(ctx, body, [58, 0]), batch(ctx, body, [0, 58])
    assert BMO.check_outputs('pink', *[a[k] for k in OUTPUTS], columns=[CAND8.index(58), CAND8.index(0)]) is None
    assert np.array_equal(a['modes'], b['modes']) and np.array_equal(a['units'], b['units']) and np.array_equal(a['choice'], 1 - b['choice'])
    for k in ('distortion', 'energy'):
        assert np.array_equal(a[k].view(np.uint64), b[k][:, ::-1].view(np.uint64)), k


def test_all_long_candidate_against_the_best_bias_kernel(ctx, mat):
    """W = 1 everywhere under byte 0: the distortion is k_choose_bias's with one entry and modes all zero (its sum is over the
    same terms; the trees differ by nothing here, but only the bound of both kernels' tests is asserted)"""
    got = batch(ctx, mat['body'], [0])
    units, choice, dist, energy = ctx.encode_best_bias(mat['body'], [1.0], modes=np.zeros((FRAMES, 2), dtype=np.uint8), return_distortion=True)
    assert (np.abs(got['distortion'][:, 0] - dist[:, 0]) <= 1e-12 * dist[:, 0]).all()
    assert (np.abs(got['energy'][:, 0] - energy) <= 1e-12 * energy).all()
    assert np.array_equal(got['units'], units)


# ---- 3. geometry ----
@pytest.mark.parametrize('nch', [1, 2])
@pytest.mark.parametrize('n', [1, 2, 8])
def test_geometry(ctx, mat, nch, n):
    reps = -(-(LARGE[nch] + 2) // (FRAMES + 2))
    full = [np.tile(c, reps)[:(LARGE[nch] + 2) * 512] for c in mat['with_halo'][:nch]]
    chans = [c[2 * 512:] for c in full]
    cand = {1: [50], 2: [10, 58], 8: CAND8}[n]
    large = batch(ctx, chans, cand)
    assert (large['choice'] < n).all() and np.array_equal(large['modes'], np.asarray(cand, dtype=np.uint8)[large['choice']])
    if n > 1:
        assert (np.bincount(large['choice'][-2 * FRAMES:], minlength=n) > 0).sum() >= 2
    # the bytes of the whole call, the second sweep of the grid included: the given-modes path fed the choice
    assert np.array_equal(large['units'], ctx.encode_modes(chans, large['modes'].reshape(-1, nch)))
    for frames in COUNTS[nch]:
        got = batch(ctx, [c[:frames * 512] for c in chans], cand)
        assert same(got, rows(large, 0, frames, nch)), (frames, nch, n)
    # the last frames of the call, past the first sweep, from two frames of halo
    a = LARGE[nch] - FRAMES
    got = batch(ctx, [c[(a - 2) * 512:] for c in chans], cand, halo=2)
    assert same(got, rows(large, a, LARGE[nch], nch))


# ---- 4. independence ----
@pytest.fixture(scope='module')
def baseline(ctx, mat):
    out = {'pink': batch(ctx, mat['body'], CAND8), 'pair': batch(ctx, mat['body'], [58, 0]), 'short': batch(ctx, mat['body'], [58])}
    for v in out.values():
        for a in v.values():
            a.setflags(write=False)
    return out


def three_calls(c, mat):
    return {'pink': batch(c, mat['body'], CAND8), 'pair': batch(c, mat['body'], [58, 0]), 'short': batch(c, mat['body'], [58])}


@pytest.mark.parametrize('env', [{'C1_CHUNK_FRAMES': 7}, {'C1_CHUNK_FRAMES': 64}, {'C1_CHUNK_FRAMES': 64, 'C1_PIPELINE': 0},
                                 {'C1_PIPELINE': 1}, {'C1_CHUNK_FRAMES': 33, 'C1_PIPELINE': 1, 'C1_OVERLAP': 1}],
                         ids=['chunk7', 'chunk64', 'chunk64-unpiped', 'piped', 'chunk33-piped-overlap'])
def test_outputs_do_not_depend_on_chunks_pipeline_or_speculation(mat, baseline, env):
    c = _context(**env)
    try:
        for mode in (0, 1, 2):
            c.set_speculation(mode)
            got = three_calls(c, mat)
            for kind in got:
                assert same(got[kind], baseline[kind]), (env, mode, kind)
        c.set_profiling(True)
        batch(c, mat['body'], CAND8)
        chunks = -(-FRAMES // max(16, env['C1_CHUNK_FRAMES'])) if 'C1_CHUNK_FRAMES' in env else 1     # a context's chunk is at least 16 frames
        ms, launches = c.kernel_ms('choose')
        assert launches == chunks and ms > 0
        assert c.kernel_ms('allocate')[1] == 8 * chunks                              # one chain per candidate
        assert c.kernel_ms('analysis')[1] == 9 * chunks                              # the two analyses, and one composing per candidate
        assert c.kernel_ms('pack')[1] == chunks
        batch(c, mat['body'], CAND8, ask=('choice',))
        assert c.kernel_ms('pack')[1] == 0 and c.kernel_ms('choose')[1] == chunks    # units NULL: no packing runs
    finally:
        c.close()


def test_outputs_do_not_depend_on_speculation(ctx, mat, baseline):
    try:
        for mode in (0, 1):
            ctx.set_speculation(mode)
            got = three_calls(ctx, mat)
            for kind in got:
                assert same(got[kind], baseline[kind]), (mode, kind)
    finally:
        ctx.set_speculation(1)


def test_halo(ctx, mat, baseline):
    """halo 0 is leading silence: the body behind two frames of zeros given as halo; and frames 2.. of a signal, given its first
    two frames as halo, against the rows of the call on the whole signal"""
    padded = [np.concatenate([np.zeros(2 * 512, dtype=np.float32), c]) for c in mat['body']]
    assert same(batch(ctx, padded, CAND8, halo=2), baseline['pink'])
    whole = batch(ctx, mat['with_halo'], CAND8)
    for halo in (1, 2):
        got = batch(ctx, [c[(2 - halo) * 512:] for c in mat['with_halo']], CAND8, halo=halo)
        assert same(got, rows(whole, 2, 2 + FRAMES, 2)), halo


def test_outputs_do_not_depend_on_which_are_asked_for(ctx, mat, baseline):
    full = baseline['pink']
    asks = [(k,) for k in OUTPUTS] + [tuple(x for x in OUTPUTS if x != k) for k in OUTPUTS]
    for ask in asks:
        got = batch(ctx, mat['body'], CAND8, ask=ask)
        assert same(got, {k: full[k] for k in ask}), ask


def test_options_reach_the_allocation_only(ctx, mat, baseline):
    """of the options only the biased scale factors are read: threshold and fixed modes change nothing, the bias does"""
    o = c1.EncoderOptions({'transientThresholdLow': 0.5, 'fixedBlockModes': [2, 0, 3]})
    assert same(batch(ctx, mat['body'], CAND8, options=o), baseline['pink'])
    got = batch(ctx, mat['body'], CAND8, options=c1.EncoderOptions({'allocationBias': 2.0}))
    assert not np.array_equal(got['units'], baseline['pink']['units'])
    want = BM.oracle_encode_modes(mat['body'], got['modes'].reshape(-1, 2), 2.0)[0]
    assert np.array_equal(got['units'], want)
    assert np.array_equal(got['energy'].view(np.uint64), baseline['pink']['energy'].view(np.uint64))


# ---- 5. repeatability and silence ----
def test_repeatability_and_silence(ctx, mat, baseline):
    assert same(batch(ctx, mat['body'], CAND8), baseline['pink'])
    assert same(batch(ctx, mat['white'], CAND8), batch(ctx, mat['white'], CAND8))
    silence = [np.zeros(8 * 512, dtype=np.float32)] * 2
    for cand in (CAND8, [58, 0]):
        got = batch(ctx, silence, cand)
        assert not got['choice'].any() and (got['modes'] == cand[0]).all()
        assert not got['distortion'].view(np.uint64).any() and not got['energy'].view(np.uint64).any()    # +0.0 exactly
        assert np.array_equal(got['units'], BM.oracle_encode_modes(silence, np.full((8, 2), cand[0], dtype=np.uint8))[0])


# ---- 6. the device entry point ----
def test_on_a_callers_stream(mat, baseline):
    """PCM is written by work queued just before the call and the outputs are read by work queued just after, with no host
    synchronisation in between; then inputs and outputs are overwritten behind it"""
    import torch
    S = torch.cuda.Stream()
    c = _context(stream=S.cuda_stream)
    try:
        src = [torch.from_numpy(x).cuda() for x in mat['body']]
        pcm = [torch.zeros_like(x) for x in src]
        units = torch.zeros(FRAMES * 2 * 212, dtype=torch.uint8, device='cuda')
        choice = torch.zeros(FRAMES * 2, dtype=torch.uint8, device='cuda')
        modes = torch.zeros(FRAMES * 2, dtype=torch.uint8, device='cuda')
        dist = torch.zeros(FRAMES * 2 * 8, dtype=torch.float64, device='cuda')
        energy = torch.zeros(FRAMES * 2 * 8, dtype=torch.float64, device='cuda')
        busy = torch.ones(1 << 26, dtype=torch.float32, device='cuda')
        torch.cuda.synchronize()
        call = lambda: c.encode_best_modes_device([p.data_ptr() for p in pcm], FRAMES, CAND8, units.data_ptr(), choice.data_ptr(),
                                                  modes.data_ptr(), dist.data_ptr(), energy.data_ptr())
        with torch.cuda.stream(S):
            call()                                   # warm: options on the device, workspace grown (these drain the stream)
            S.synchronize()
            for _ in range(200):
                busy.mul_(-1.0)
            for p, x in zip(pcm, src):
                p.copy_(x)
            call()
            snap = [t.clone() for t in (units, choice, modes, dist, energy)]
            for p in pcm:
                p.zero_()
            units.fill_(0xA5)
            choice.fill_(0xA5)
            modes.fill_(0xA5)
            dist.fill_(-1.0)
            energy.fill_(-1.0)
            queued_behind_busy_stream = not S.query()
            S.synchronize()
        assert queued_behind_busy_stream
        got = {'units': snap[0].cpu().numpy().reshape(-1, 212), 'choice': snap[1].cpu().numpy(), 'modes': snap[2].cpu().numpy(),
               'distortion': snap[3].cpu().numpy().reshape(-1, 8), 'energy': snap[4].cpu().numpy().reshape(-1, 8)}
        assert same(got, dict(baseline['pink']))
    finally:
        c.close()


def test_device_entry_point_rejections_leave_the_outputs_untouched(ctx, mat):
    import torch
    lib = capi.load()
    units_n = FRAMES * 2
    buf = {'units': (torch.uint8, units_n * 212, 0xA5), 'choice': (torch.uint8, units_n, 0xA5), 'modes': (torch.uint8, units_n, 0xA5),
           'distortion': (torch.float64, units_n * 8, -1.0), 'energy': (torch.float64, units_n * 8, -1.0)}
    t = {k: torch.full((n,), fill, dtype=d, device='cuda') for k, (d, n, fill) in buf.items()}
    dev = [torch.from_numpy(c).cuda() for c in mat['body']]
    torch.cuda.synchronize()
    ptrs = capi.ptr_array([d.data_ptr() for d in dev])
    opts = c1.EncoderOptions().to_c()
    outs = [C.c_void_p(t[k].data_ptr()) for k in OUTPUTS]

    def call(cand, n=None, o=outs, frames=FRAMES):
        cb = np.asarray(cand, dtype=np.uint8)
        return lib.c1_encode_best_modes_device(ctx._h, ptrs, 2, frames, 0, C.byref(opts), cb.ctypes.data, len(cb) if n is None else n, *o)

    err = lambda: lib.c1_last_error().decode()
    assert call([0, 58, 0]) == C1_ERR_ARG and 'candidate 2' in err(), err()
    assert call([0, 1]) == C1_ERR_ARG and 'candidate 1' in err() and 'low field' in err(), err()
    assert call([0, 64]) == C1_ERR_ARG and 'bits 6-7' in err(), err()
    assert call([0, 0x20]) == C1_ERR_ARG and 'high field' in err(), err()
    assert call(CAND8 + [0], 9) == C1_ERR_ARG and 'n_cand = 9' in err(), err()
    assert call(CAND8, 0) == C1_ERR_ARG and 'n_cand = 0' in err(), err()
    assert call(CAND8, o=[None] * 5) == C1_ERR_ARG and 'all NULL' in err(), err()
    assert call(CAND8, frames=0) == C1_OK                                            # frames = 0 writes nothing
    ctx.synchronize()
    for k, (d, n, fill) in buf.items():
        assert (t[k].cpu().numpy() == fill).all(), k
