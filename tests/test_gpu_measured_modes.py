"""GPU: the block modes of every sound unit chosen from candidates by the error of the measured allocation
(c1_encode_measured_modes_device / _batch, k_measured_modes).  Per (unit, candidate) the figures bit for bit those of the
measure-only measured calls under that constant byte and within 1e-12 of the CPU model of tests/measured_modes_lib.py; the
choice the model's; units, taken and shifts bit for bit those of encode_measured under the chosen modes; candidate subsets and
orders; the geometry of the new kernel (one wave per unit, four waves per workgroup, a grid bounded at 2 048 workgroups: 8 192
units per sweep); independence of chunking, pipeline, overlap, speculation, halo and of which outputs are asked for; silence and
repeatability; the device entry point on a caller's stream and its rejections.
tests/test_measured_modes_cpu.py shows that on this material every unit has exactly one admissible candidate, that four
candidates win often on pink, and that the best-modes choice is another in most units."""
import ctypes as C
import os

import numpy as np
import pytest

import carta1_amd as c1
from carta1_amd import capi
import best_bias_lib as BB
import block_modes_lib as BM
import measured_modes_lib as MM
import scale_factor_choice_lib as SF

pytestmark = pytest.mark.gpu

C1_OK, C1_ERR_ARG = 0, 1   # include/carta1_hip.h
FRAMES = BB.FRAMES
CAND8 = MM.CANDIDATES
OFFSETS = MM.OFFSETS
OUTPUTS = ('units', 'choice', 'modes', 'taken', 'shifts', 'distortion', 'energy')
# frames per call: one wave (1 unit), a partly filled workgroup and its seam (2, 3), many workgroups (63, 64, 65, 257), and the
# seam of the bounded grid, 2 048 workgroups * 4 waves = 8 192 units, past which the waves stride (8 191 .. 8 194 units mono;
# 8 190, 8 192 and 8 194 stereo)
COUNTS = {1: (1, 2, 3, 63, 64, 65, 257, 8191, 8192, 8193, 8194), 2: (1, 2, 3, 63, 64, 65, 257, 4095, 4096, 4097)}
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
    return {'with_halo': with_halo, 'body': body, 'pink': body, 'white': MM.BMO.material('white')}


def batch(ctx, chans, cand, offsets=OFFSETS, halo=0, ask=OUTPUTS, options=None):
    """c1_encode_measured_modes_batch with any subset of the outputs; the others are passed as NULL -> dict of the ones asked for"""
    chans = [np.ascontiguousarray(c, dtype=np.float32) for c in chans]
    nch, frames, n = len(chans), len(chans[0]) // 512 - halo, len(cand)
    total = frames * nch
    out = {'units': np.full((total, 212), 0xA5, dtype=np.uint8), 'choice': np.full(total, 0xA5, dtype=np.uint8),
           'modes': np.full(total, 0xA5, dtype=np.uint8), 'taken': np.full(total, 0xA5, dtype=np.uint8),
           'shifts': np.full((total, 52), 0x5A, dtype=np.int8), 'distortion': np.full((total, n, 2), -1.0), 'energy': np.full((total, n), -1.0)}
    cb, ob = np.asarray(cand, dtype=np.uint8), np.asarray(offsets, dtype=np.int8)
    opts = (options or c1.EncoderOptions()).to_c()
    ptrs = capi.ptr_array([c.ctypes.data + halo * 2048 for c in chans])
    capi.check(capi.load().c1_encode_measured_modes_batch(ctx._h, ptrs, nch, frames, halo, C.byref(opts), cb.ctypes.data, n, ob.ctypes.data, len(ob),
                                                          *[out[k].ctypes.data if k in ask else None for k in OUTPUTS]))
    return {k: out[k] for k in ask}


def measure_only(ctx, chans, byte, offsets):
    """the measure-only sibling under a constant byte: c1_encode_measured_sf_batch, or c1_encode_measured_batch when offsets is
    None, with units NULL -> (distortion [U, 2], energy [U])"""
    chans = [np.ascontiguousarray(c, dtype=np.float32) for c in chans]
    nch, frames = len(chans), len(chans[0]) // 512
    dist, energy = np.full((frames * nch, 2), -1.0), np.full(frames * nch, -1.0)
    modes = np.full(frames * nch, byte, dtype=np.uint8)
    opts = c1.EncoderOptions().to_c()
    ptrs = capi.ptr_array([c.ctypes.data for c in chans])
    lib = capi.load()
    if offsets is None:
        capi.check(lib.c1_encode_measured_batch(ctx._h, ptrs, nch, frames, 0, C.byref(opts), modes.ctypes.data, None, None, dist.ctypes.data,
                                                energy.ctypes.data))
    else:
        ob = np.asarray(offsets, dtype=np.int8)
        capi.check(lib.c1_encode_measured_sf_batch(ctx._h, ptrs, nch, frames, 0, C.byref(opts), modes.ctypes.data, ob.ctypes.data, len(ob), None,
                                                   None, None, dist.ctypes.data, energy.ctypes.data))
    return dist, energy


def sibling_under(ctx, chans, modes, offsets, options=None):
    """encode_measured under the chosen modes -> the three outputs the new call shares with it"""
    nch = len(chans)
    if offsets is None:
        units, taken = ctx.encode_measured(chans, modes=modes.reshape(-1, nch), options=options)
        return {'units': units, 'taken': taken, 'shifts': np.zeros((len(taken), 52), dtype=np.int8)}
    units, taken, shifts = ctx.encode_measured(chans, modes=modes.reshape(-1, nch), options=options, scale_factor_offsets=offsets, return_shifts=True)
    return {'units': units, 'taken': taken, 'shifts': shifts}


def same(a, b):
    """bitwise equality of two output dicts (doubles compared as bit patterns)"""
    return a.keys() == b.keys() and all(a[k].shape == b[k].shape and np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) for k in a)


def rows(out, a, b, nch):
    return {k: v[a * nch:b * nch] for k, v in out.items()}


def composed(ctx, chans, got, cand, offsets):
    """None, or which output of the call is not bit for bit what the existing calls compose to"""
    for k, byte in enumerate(cand):
        dist, energy = measure_only(ctx, chans, byte, offsets)
        if not np.array_equal(got['distortion'][:, k].view(np.uint64), dist.view(np.uint64)):
            return 'distortion of candidate %d' % k
        if not np.array_equal(got['energy'][:, k].view(np.uint64), energy.view(np.uint64)):
            return 'energy of candidate %d' % k
    fin = np.where(got['distortion'][:, :, 1] < got['distortion'][:, :, 0], got['distortion'][:, :, 1], got['distortion'][:, :, 0])
    if not np.array_equal(got['choice'], fin.argmin(axis=1)):
        return 'choice is not the first least T_final of the values reported'
    if not np.array_equal(got['modes'], np.asarray(cand, dtype=np.uint8)[got['choice']]):
        return 'modes_out is not cand_modes[choice]'
    want = sibling_under(ctx, chans, got['modes'], offsets)
    for k in want:
        if not np.array_equal(got[k], want[k]):
            return '%s under the chosen modes' % k
    return None


# ---- 1. against the existing calls and the model ----
@pytest.mark.parametrize('material,sf', [('pink', False), ('pink', True), ('white', False), ('white', True)])
def test_against_the_siblings_and_the_model(ctx, mat, material, sf):
    chans, cand = mat[material], MM.candidates_of(material, sf)
    offsets = OFFSETS if sf else (0,)
    got = batch(ctx, chans, cand, offsets)
    m = MM.case(material, sf)
    print('winners', np.bincount(got['choice'], minlength=len(cand)).tolist(), 'taken', int(got['taken'].sum()), 'of', len(got['taken']),
          'largest relative error of T %.3g, of E %.3g' % (np.max(np.abs(got['distortion'] - m['D']) / m['D']),
                                                            np.max(np.abs(got['energy'] - m['E']) / m['E'])))
    assert composed(ctx, chans, got, cand, offsets if sf else None) is None
    assert MM.check_outputs(material, sf, got) is None
    ar = np.arange(len(got['choice']))
    assert SF.check_valid(got['units'], m['coefs'], got['taken'], got['distortion'][ar, got['choice']], offsets) is None
    # the Python wrapper: the same outputs, with and without the reports, candidates as triples
    wrapped = ctx.encode_measured_modes(chans, [BM.triple_of(b) for b in cand], scale_factor_offsets=OFFSETS if sf else None,
                                        return_distortion=True, return_shifts=True)
    assert same(dict(zip(OUTPUTS, wrapped)), got)
    assert same(dict(zip(OUTPUTS[:4], ctx.encode_measured_modes(chans, cand, scale_factor_offsets=OFFSETS if sf else None))),
                {k: got[k] for k in OUTPUTS[:4]})


def test_offsets_of_zero_alone_are_the_plain_measured_allocation(ctx, mat):
    got = batch(ctx, mat['white'], CAND8, (0,))
    assert not got['shifts'].any()
    assert composed(ctx, mat['white'], got, CAND8, None) is None                      # c1_encode_measured_*'s figures and bytes
    assert composed(ctx, mat['white'], got, CAND8, (0,)) is None                      # and c1_encode_measured_sf_*'s under {0}


# ---- 2. candidate subsets ----
def test_candidate_subsets_and_order(ctx, mat):
    body = mat['body']
    for byte in (0, 58, 10):
        got = batch(ctx, body, [byte])
        assert not got['choice'].any() and (got['modes'] == byte).all()
        assert composed(ctx, body, got, [byte], OFFSETS) is None
        assert MM.check_outputs('pink', True, got, [MM.PINK_SF_CANDIDATES.index(byte)]) is None
    a, b = batch(ctx, body, [58, 0]), batch(ctx, body, [0, 58])
    assert MM.check_outputs('pink', True, a, [MM.PINK_SF_CANDIDATES.index(58), MM.PINK_SF_CANDIDATES.index(0)]) is None
    assert set(a['choice'].tolist()) == {0, 1} and np.array_equal(a['choice'], 1 - b['choice'])
    for k in ('units', 'modes', 'taken', 'shifts'):
        assert np.array_equal(a[k], b[k]), k
    for k in ('distortion', 'energy'):
        assert np.array_equal(a[k].view(np.uint64), b[k][:, ::-1].view(np.uint64)), k


# ---- 3. geometry ----
@pytest.mark.parametrize('nch', [1, 2])
@pytest.mark.parametrize('n', [1, 2, 8])
def test_geometry(ctx, mat, nch, n):
    reps = -(-(LARGE[nch] + 2) // (FRAMES + 2))
    full = [np.tile(c, reps)[:(LARGE[nch] + 2) * 512] for c in mat['with_halo'][:nch]]
    chans = [c[2 * 512:] for c in full]
    cand = {1: [50], 2: [10, 58], 8: CAND8}[n]
    offsets = (0,) if n == 2 else OFFSETS
    large = batch(ctx, chans, cand, offsets)
    assert (large['choice'] < n).all() and np.array_equal(large['modes'], np.asarray(cand, dtype=np.uint8)[large['choice']])
    if n > 1:
        assert (np.bincount(large['choice'][-2 * FRAMES:], minlength=n) > 0).sum() >= 2
    # the bytes of the whole call, the second sweep of the grid included: the measured call under the chosen modes
    want = sibling_under(ctx, chans, large['modes'], None if n == 2 else offsets)
    for k in want:
        assert np.array_equal(large[k], want[k]), k
    for frames in COUNTS[nch]:
        got = batch(ctx, [c[:frames * 512] for c in chans], cand, offsets)
        assert same(got, rows(large, 0, frames, nch)), (frames, nch, n)
    # the last frames of the call, past the first sweep, from two frames of halo
    a = LARGE[nch] - FRAMES
    got = batch(ctx, [c[(a - 2) * 512:] for c in chans], cand, offsets, halo=2)
    assert same(got, rows(large, a, LARGE[nch], nch))


# ---- 4. independence ----
def three_calls(c, mat):
    return {'pink': batch(c, mat['body'], CAND8), 'pair': batch(c, mat['body'], [58, 0], (0,)), 'short': batch(c, mat['body'], [58])}


@pytest.fixture(scope='module')
def baseline(ctx, mat):
    out = three_calls(ctx, mat)
    for v in out.values():
        for a in v.values():
            a.setflags(write=False)
    return out


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
        ms, launches = c.kernel_ms('measure')
        assert launches == chunks and ms > 0 and c.kernel_ms('choose')[1] == 0
        assert c.kernel_ms('allocate')[1] == 8 * chunks                              # one chain per candidate
        assert c.kernel_ms('analysis')[1] == 9 * chunks                              # the two analyses, and one composing per candidate
        assert c.kernel_ms('pack')[1] == chunks
        batch(c, mat['body'], CAND8, ask=('choice',))
        assert c.kernel_ms('pack')[1] == 0 and c.kernel_ms('measure')[1] == chunks   # units NULL: no packing runs
    finally:
        c.close()


def test_outputs_do_not_depend_on_speculation(ctx, mat, baseline):
    try:
        for mode in (0, 2):
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


def test_a_measure_only_call_touches_no_record(ctx, mat, baseline):
    """units NULL: the winner is not handed on, so a packing call of another kind behind it sees its own records only"""
    batch(ctx, mat['body'], CAND8, ask=('choice', 'taken'))
    plain = ctx.encode_modes(mat['body'], np.full((FRAMES, 2), 58, dtype=np.uint8))
    assert np.array_equal(plain, BM.oracle_encode_modes(mat['body'], np.full((FRAMES, 2), 58, dtype=np.uint8))[0])
    assert same(batch(ctx, mat['body'], CAND8), baseline['pink'])


def test_options_reach_the_allocation_only(ctx, mat, baseline):
    """of the options only the biased scale factors are read: threshold and fixed modes change nothing, the bias does"""
    o = c1.EncoderOptions({'transientThresholdLow': 0.5, 'fixedBlockModes': [2, 0, 3]})
    assert same(batch(ctx, mat['body'], CAND8, options=o), baseline['pink'])
    o2 = c1.EncoderOptions({'allocationBias': 2.0})
    got = batch(ctx, mat['body'], CAND8, options=o2)
    assert not np.array_equal(got['distortion'][:, :, 0], baseline['pink']['distortion'][:, :, 0])           # T_ref follows the bias
    assert np.array_equal(got['energy'].view(np.uint64), baseline['pink']['energy'].view(np.uint64))
    want = sibling_under(ctx, mat['body'], got['modes'], OFFSETS, options=o2)
    for k in want:
        assert np.array_equal(got[k], want[k]), k


# ---- 5. repeatability and silence ----
def test_repeatability_and_silence(ctx, mat, baseline):
    assert same(batch(ctx, mat['body'], CAND8), baseline['pink'])
    assert same(batch(ctx, mat['white'], CAND8), batch(ctx, mat['white'], CAND8))
    silence = [np.zeros(8 * 512, dtype=np.float32)] * 2
    for cand in (CAND8, [58, 0]):
        got = batch(ctx, silence, cand)
        assert not got['choice'].any() and (got['modes'] == cand[0]).all() and not got['taken'].any() and not got['shifts'].any()
        assert not got['distortion'].view(np.uint64).any() and not got['energy'].view(np.uint64).any()    # +0.0 exactly
        assert np.array_equal(got['units'], BM.oracle_encode_modes(silence, np.full((8, 2), cand[0], dtype=np.uint8))[0])


# ---- 6. the device entry point ----
def test_on_a_callers_stream(mat, baseline):
    """PCM is written by work queued just before the call and the outputs are read by work queued just after, with no host
    synchronisation in between; then inputs and outputs are overwritten behind it.  The device form against the batch form"""
    import torch
    S = torch.cuda.Stream()
    c = _context(stream=S.cuda_stream)
    try:
        n = FRAMES * 2
        src = [torch.from_numpy(x).cuda() for x in mat['body']]
        pcm = [torch.zeros_like(x) for x in src]
        shapes = {'units': (torch.uint8, n * 212), 'choice': (torch.uint8, n), 'modes': (torch.uint8, n), 'taken': (torch.uint8, n),
                  'shifts': (torch.int8, n * 52), 'distortion': (torch.float64, n * 16), 'energy': (torch.float64, n * 8)}
        t = {k: torch.zeros(size, dtype=d, device='cuda') for k, (d, size) in shapes.items()}
        busy = torch.ones(1 << 26, dtype=torch.float32, device='cuda')
        torch.cuda.synchronize()
        call = lambda: c.encode_measured_modes_device([p.data_ptr() for p in pcm], FRAMES, CAND8, t['units'].data_ptr(), t['choice'].data_ptr(),
                                                      t['modes'].data_ptr(), t['taken'].data_ptr(), t['shifts'].data_ptr(),
                                                      t['distortion'].data_ptr(), t['energy'].data_ptr(), scale_factor_offsets=OFFSETS)
        with torch.cuda.stream(S):
            call()                                   # warm: options on the device, workspace grown (these drain the stream)
            S.synchronize()
            for _ in range(200):
                busy.mul_(-1.0)
            for p, x in zip(pcm, src):
                p.copy_(x)
            call()
            snap = {k: v.clone() for k, v in t.items()}
            for p in pcm:
                p.zero_()
            for k, v in t.items():
                v.fill_(-1.0 if v.dtype == torch.float64 else 0x5A)
            queued_behind_busy_stream = not S.query()
            S.synchronize()
        assert queued_behind_busy_stream
        got = {k: v.cpu().numpy() for k, v in snap.items()}
        got['units'] = got['units'].reshape(-1, 212)
        got['shifts'] = got['shifts'].reshape(-1, 52)
        got['distortion'] = got['distortion'].reshape(-1, 8, 2)
        got['energy'] = got['energy'].reshape(-1, 8)
        assert same(got, dict(baseline['pink']))
    finally:
        c.close()


def test_rejections_leave_the_outputs_untouched_and_the_next_call_unharmed(ctx, mat, baseline):
    import torch
    lib = capi.load()
    n = FRAMES * 2
    buf = {'units': (torch.uint8, n * 212, 0xA5), 'choice': (torch.uint8, n, 0xA5), 'modes': (torch.uint8, n, 0xA5), 'taken': (torch.uint8, n, 0xA5),
           'shifts': (torch.int8, n * 52, 0x5A), 'distortion': (torch.float64, n * 16, -1.0), 'energy': (torch.float64, n * 8, -1.0)}
    t = {k: torch.full((size,), fill, dtype=d, device='cuda') for k, (d, size, fill) in buf.items()}
    dev = [torch.from_numpy(c).cuda() for c in mat['body']]
    torch.cuda.synchronize()
    ptrs = capi.ptr_array([d.data_ptr() for d in dev])
    opts = c1.EncoderOptions().to_c()
    outs = [C.c_void_p(t[k].data_ptr()) for k in OUTPUTS]

    def call(cand, offs=OFFSETS, n_cand=None, n_off=None, o=outs, frames=FRAMES, halo=0, channels=2):
        cb, ob = np.asarray(cand, dtype=np.uint8), np.asarray(offs, dtype=np.int8)
        return lib.c1_encode_measured_modes_device(ctx._h, ptrs, channels, frames, halo, C.byref(opts), cb.ctypes.data,
                                                   len(cb) if n_cand is None else n_cand, ob.ctypes.data if ob.size else None,
                                                   len(ob) if n_off is None else n_off, *o)

    err = lambda: lib.c1_last_error().decode()
    assert call([0, 58, 0]) == C1_ERR_ARG and 'c1_encode_measured_modes_device' in err() and 'candidate 2' in err(), err()
    assert call([0, 1]) == C1_ERR_ARG and 'candidate 1' in err() and 'low field' in err(), err()
    assert call([0, 64]) == C1_ERR_ARG and 'bits 6-7' in err(), err()
    assert call([0, 0x20]) == C1_ERR_ARG and 'high field' in err(), err()
    assert call(CAND8 + [0], n_cand=9) == C1_ERR_ARG and 'n_cand = 9' in err(), err()
    assert call(CAND8, n_cand=0) == C1_ERR_ARG and 'n_cand = 0' in err(), err()
    assert call(CAND8, offs=()) == C1_ERR_ARG and 'n_offsets = 0' in err(), err()
    assert call(CAND8, offs=list(range(9))) == C1_ERR_ARG and 'n_offsets = 9' in err(), err()
    assert call(CAND8, offs=(0, 9)) == C1_ERR_ARG and 'outside -8..8' in err(), err()
    assert call(CAND8, offs=(0, 1, 1)) == C1_ERR_ARG and 'repeats' in err(), err()
    assert call(CAND8, offs=(1, 0)) == C1_ERR_ARG and 'not 0' in err(), err()
    assert call(CAND8, o=[None] * 7) == C1_ERR_ARG and 'all NULL' in err(), err()
    assert call(CAND8, halo=3) == C1_ERR_ARG
    assert call(CAND8, channels=3) == C1_ERR_ARG
    assert call(CAND8, frames=-1) == C1_ERR_ARG
    assert call(CAND8, frames=0) == C1_OK                                            # frames = 0 writes nothing
    ctx.synchronize()
    for k, (d, size, fill) in buf.items():
        assert (t[k].cpu().numpy() == fill).all(), k
    assert same(batch(ctx, mat['body'], CAND8), baseline['pink'])
