"""GPU: the measured block-mode search under one masking threshold per unit (c1_encode_measured_modes_masked_device / _batch,
k_measured_modes_masked and k_measured_modes_masked_wide).  The consequences of the definition in include/carta1_hip.h, each
against a call that existed before this one: flat tables give the unweighted search bit for bit; the single candidate 0 gives the
masked allocation under constant modes 0; the column of byte 0 is that call's in every candidate set; weights does not depend on
the candidates or the offsets; scaling both tables by 4.0; the candidate order; independence of the run.  Then the CPU model of
tests/masked_modes_lib.py, the wave-per-unit kernel against the workgroup-per-unit one on two contexts, the seams of the dispatch
and of the bounded grid, the hard material of tests/hard_material_lib.py, NaN and +Inf in the PCM, and the housekeeping of every
measured call.  tests/test_masked_modes_cpu.py shows that on this material every unit has exactly one admissible candidate and
that the winner is not the unweighted search's in a quarter of the units and more."""
import ctypes as C

import numpy as np
import pytest

import carta1_amd as c1
from carta1_amd import capi
import best_bias_lib as BB
import block_modes_lib as BM
import hard_material_lib as H
import masked_alloc_lib as MK
import masked_modes_lib as X
import measured_modes_lib as MM
import scale_factor_choice_lib as SF
import test_gpu_measured_modes as TM

pytestmark = pytest.mark.gpu

C1_OK, C1_ERR_ARG = 0, 1   # include/carta1_hip.h
FRAMES = BB.FRAMES
CAND8 = X.CANDIDATES
OFFSETS = X.OFFSETS
OUTPUTS = TM.OUTPUTS + ('weights',)
KINDS = ('narrow', 'wide')
CAND_SETS = ([0], [58], [10], [0, 58], [58, 0], CAND8)      # the long plane alone, the short plane alone, both
OFFSET_SETS = ((0,), OFFSETS)
COUNTS = (1, 2, 3, 63, 130)
TABLES = ('packaged', 'specs', 'self', 'flat', 'packaged*4')
same = TM.same


@pytest.fixture(scope='module')
def ctx():
    c = c1.Context(0)
    yield c
    c.close()


@pytest.fixture(scope='module')
def two():
    ctxs = {'narrow': TM._context(C1_MEASURED_WIDE=0), 'wide': TM._context(C1_MEASURED_WIDE=1)}
    yield ctxs
    for c in ctxs.values():
        c.close()


@pytest.fixture(scope='module')
def mat():
    body = BB.material()[1]
    return {'pink': body, 'white': MM.BMO.material('white'), 'silence': [np.zeros(FRAMES * 512, dtype=np.float32)] * 2}


def cut(chans, frames, nch):
    return [c[:frames * 512] for c in chans[:nch]]


def batch(ctx, chans, cand, offsets=OFFSETS, tables='packaged', halo=0, ask=OUTPUTS, options=None):
    """c1_encode_measured_modes_masked_batch with any subset of the outputs; the others are passed as NULL -> dict of the ones
    asked for.  tables: a name of masked_alloc_lib.named, or a (floor, spread | None) pair"""
    chans = [np.ascontiguousarray(c, dtype=np.float32) for c in chans]
    nch, frames, n = len(chans), len(chans[0]) // 512 - halo, len(cand)
    total = frames * nch
    out = {'units': np.full((total, 212), 0xA5, dtype=np.uint8), 'choice': np.full(total, 0xA5, dtype=np.uint8),
           'modes': np.full(total, 0xA5, dtype=np.uint8), 'taken': np.full(total, 0xA5, dtype=np.uint8),
           'shifts': np.full((total, 52), 0x5A, dtype=np.int8), 'distortion': np.full((total, n, 2), -1.0), 'energy': np.full((total, n), -1.0),
           'weights': np.full((total, 52), -1.0)}
    floor, spread = MK.named(tables) if isinstance(tables, str) else tables
    floor = np.ascontiguousarray(floor, dtype=np.float64)
    spread = None if spread is None else np.ascontiguousarray(spread, dtype=np.float64)
    cb, ob = np.asarray(cand, dtype=np.uint8), np.asarray(offsets, dtype=np.int8)
    opts = (options or c1.EncoderOptions()).to_c()
    ptrs = capi.ptr_array([c.ctypes.data + halo * 2048 for c in chans])
    capi.check(capi.load().c1_encode_measured_modes_masked_batch(
        ctx._h, ptrs, nch, frames, halo, C.byref(opts), cb.ctypes.data, n, ob.ctypes.data, len(ob), floor.ctypes.data,
        None if spread is None else spread.ctypes.data, *[out[k].ctypes.data if k in ask else None for k in OUTPUTS]))
    return {k: out[k] for k in ask}


def masked_under_zero(ctx, chans, offsets, tables, units=True):
    """c1_encode_measured_masked_batch under constant modes 0 -> units, taken, shifts, distortion [U, 2], energy [U], weights"""
    nch, frames = len(chans), len(chans[0]) // 512
    got = ctx.encode_measured(chans, modes=np.zeros((frames, nch), dtype=np.uint8), scale_factor_offsets=offsets, return_shifts=True,
                              return_distortion=True, masking=MK.named(tables), return_weights=True)
    return dict(zip(('units', 'taken', 'shifts', 'distortion', 'energy', 'weights'), got))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


@pytest.fixture(scope='module')
def baseline(ctx, mat):
    out = {'pink': batch(ctx, mat['pink'], CAND8), 'pair': batch(ctx, mat['pink'], [58, 0], (0,)), 'short': batch(ctx, mat['pink'], [58]),
           'white': batch(ctx, mat['white'], CAND8, (0,), 'self')}
    for v in out.values():
        for a in v.values():
            a.setflags(write=False)
    return out


def four_calls(c, mat):
    return {'pink': batch(c, mat['pink'], CAND8), 'pair': batch(c, mat['pink'], [58, 0], (0,)), 'short': batch(c, mat['pink'], [58]),
            'white': batch(c, mat['white'], CAND8, (0,), 'self')}


# ---- consequence 1: flat tables ----
@pytest.mark.parametrize('nch', [1, 2])
@pytest.mark.parametrize('material', ['pink', 'white', 'silence'])
def test_flat_tables_are_the_unweighted_search(ctx, mat, material, nch):
    zeros = np.zeros((52, 52))
    for frames in COUNTS:
        chans = cut(mat[material], min(frames, len(mat[material][0]) // 512), nch)
        for cand in CAND_SETS:
            for offsets in OFFSET_SETS:
                want = TM.batch(ctx, chans, cand, offsets)
                for spread in (None, zeros) if frames in (3, 130) else (None,):
                    got = batch(ctx, chans, cand, offsets, (np.ones(52), spread))
                    assert (got.pop('weights') == 1.0).all()
                    assert same(got, want), (frames, cand, offsets, spread is None)


# ---- consequences 2 and 3: the single candidate 0, and the column of byte 0 ----
@pytest.mark.parametrize('tables', TABLES)
def test_candidate_zero_is_the_masked_allocation_under_long_modes(ctx, mat, tables):
    for material, nch, frames in (('pink', 2, 130), ('pink', 1, 63), ('white', 2, 3), ('white', 1, 1), ('pink', 2, 2), ('silence', 2, 3)):
        chans = cut(mat[material], frames, nch)
        for offsets in OFFSET_SETS:
            want = masked_under_zero(ctx, chans, offsets, tables)
            got = batch(ctx, chans, [0], offsets, tables)
            assert not got['choice'].any() and not got['modes'].any()
            for k in ('units', 'taken', 'shifts'):
                assert np.array_equal(got[k], want[k]), (k, material, frames, offsets)
            assert np.array_equal(bits(got['distortion'][:, 0]), bits(want['distortion'])), (material, frames, offsets)
            assert np.array_equal(bits(got['energy'][:, 0]), bits(want['energy']))
            assert np.array_equal(bits(got['weights']), bits(want['weights']))
            for cand in ([0, 58], [58, 0], CAND8):
                k0 = cand.index(0)
                more = batch(ctx, chans, cand, offsets, tables, ask=('distortion', 'energy', 'weights'))
                assert np.array_equal(bits(more['distortion'][:, k0]), bits(want['distortion'])), (cand, material, frames, offsets)
                assert np.array_equal(bits(more['energy'][:, k0]), bits(want['energy']))
                assert np.array_equal(bits(more['weights']), bits(want['weights']))


# ---- consequence 4: weights is candidate-independent ----
@pytest.mark.parametrize('which', KINDS)
@pytest.mark.parametrize('tables', ['packaged', 'self'])
def test_weights_do_not_depend_on_candidates_or_offsets(two, mat, which, tables):
    """also for sets that never code long ([58], [10]): with tables given the all-long analysis always runs"""
    c = two[which]
    for material, nch, frames in (('pink', 2, 130), ('white', 1, 3), ('pink', 1, 1)):
        chans = cut(mat[material], frames, nch)
        want = masked_under_zero(c, chans, (0,), tables)['weights']
        assert (want > 0).all()
        for cand in CAND_SETS:
            for offsets in OFFSET_SETS:
                got = batch(c, chans, cand, offsets, tables)
                assert np.array_equal(bits(got['weights']), bits(want)), (cand, offsets, material)
                only = batch(c, chans, cand, offsets, tables, ask=('weights',))     # measure only: the same front end
                assert np.array_equal(bits(only['weights']), bits(want)), (cand, offsets, material)
    # a search that never codes long leaves a later one what it needs, and the other way round
    chans = mat['pink']
    a = batch(c, chans, [58], OFFSETS, tables)
    b = batch(c, chans, CAND8, OFFSETS, tables)
    assert same(batch(c, chans, [58], OFFSETS, tables), a) and same(batch(c, chans, CAND8, OFFSETS, tables), b)


# ---- consequence 5: scaling ----
@pytest.mark.parametrize('tables', ['packaged', 'specs', 'self'])
def test_scaling_both_tables_by_four(ctx, mat, tables):
    for material, cand, offsets in (('pink', CAND8, OFFSETS), ('white', CAND8, (0,)), ('pink', [58, 0], OFFSETS), ('pink', [10], (0,))):
        a, b = batch(ctx, mat[material], cand, offsets, tables), batch(ctx, mat[material], cand, offsets, tables + '*4')
        for k in ('units', 'choice', 'modes', 'taken', 'shifts'):
            assert np.array_equal(a[k], b[k]), (k, material, cand)
        for k in ('distortion', 'energy', 'weights'):
            assert np.array_equal(bits(a[k] * 0.25), bits(b[k])), (k, material, cand)
        if len(cand) > 1 and tables == 'packaged':
            assert len(set(a['choice'].tolist())) > 1


# ---- consequence 6: the candidate order ----
@pytest.mark.parametrize('tables', ['packaged', 'self'])
def test_candidate_order(ctx, mat, tables):
    for material in ('pink', 'white'):
        for offsets in OFFSET_SETS:
            a, b = batch(ctx, mat[material], [58, 0], offsets, tables), batch(ctx, mat[material], [0, 58], offsets, tables)
            assert set(a['choice'].tolist()) == {0, 1} and np.array_equal(a['choice'], 1 - b['choice'])
            for k in ('units', 'modes', 'taken', 'shifts'):
                assert np.array_equal(a[k], b[k]), k
            for k in ('distortion', 'energy'):
                assert np.array_equal(bits(a[k]), bits(b[k][:, ::-1])), k
            assert np.array_equal(bits(a['weights']), bits(b['weights']))


# ---- consequence 7: independence of the run ----
@pytest.mark.parametrize('env', [{'C1_CHUNK_FRAMES': 7}, {'C1_CHUNK_FRAMES': 64}, {'C1_CHUNK_FRAMES': 64, 'C1_PIPELINE': 0},
                                 {'C1_PIPELINE': 1}, {'C1_CHUNK_FRAMES': 33, 'C1_PIPELINE': 1, 'C1_OVERLAP': 1},
                                 {'C1_MEASURED_WIDE': 0, 'C1_CHUNK_FRAMES': 33}, {'C1_MEASURED_WIDE': 1, 'C1_CHUNK_FRAMES': 64}],
                         ids=['chunk7', 'chunk64', 'chunk64-unpiped', 'piped', 'chunk33-piped-overlap', 'narrow-chunk33', 'wide-chunk64'])
def test_outputs_do_not_depend_on_chunks_pipeline_or_speculation(mat, baseline, env):
    c = TM._context(**env)
    try:
        for mode in (0, 1, 2):
            c.set_speculation(mode)
            got = four_calls(c, mat)
            for kind in got:
                assert same(got[kind], baseline[kind]), (env, mode, kind)
        c.set_profiling(True)
        batch(c, mat['pink'], CAND8)
        chunks = -(-FRAMES // max(16, env['C1_CHUNK_FRAMES'])) if 'C1_CHUNK_FRAMES' in env else 1     # a context's chunk is at least 16 frames
        ms, launches = c.kernel_ms('measure')
        assert launches == chunks and ms > 0 and c.kernel_ms('choose')[1] == 0       # one launch per launch of the chain
        assert c.kernel_ms('allocate')[1] == 8 * chunks                              # one chain per candidate
        assert c.kernel_ms('analysis')[1] == 9 * chunks                              # the two analyses, and one composing per candidate
        assert c.kernel_ms('pack')[1] == chunks
        batch(c, mat['pink'], [58])
        assert c.kernel_ms('analysis')[1] == 2 * chunks                              # the all-long analysis runs all the same
        batch(c, mat['pink'], CAND8, ask=('choice', 'weights'))
        assert c.kernel_ms('pack')[1] == 0 and c.kernel_ms('measure')[1] == chunks   # units NULL: no packing runs
    finally:
        c.close()


def test_halo_and_repetition(ctx, mat, baseline):
    padded = [np.concatenate([np.zeros(2 * 512, dtype=np.float32), c]) for c in mat['pink']]
    assert same(batch(ctx, padded, CAND8, halo=2), baseline['pink'])
    with_halo = BB.material()[0]
    whole = batch(ctx, with_halo, CAND8)
    for halo in (1, 2):
        got = batch(ctx, [c[(2 - halo) * 512:] for c in with_halo], CAND8, halo=halo)
        assert same(got, TM.rows(whole, 2, 2 + FRAMES, 2)), halo
    assert same(batch(ctx, mat['pink'], CAND8), baseline['pink'])
    assert same(batch(ctx, mat['white'], CAND8, (0,), 'self'), baseline['white'])


def test_on_a_callers_stream(mat, baseline):
    """the device form on a caller's stream, queued behind work that writes the PCM and in front of work that overwrites inputs
    and outputs, with no host synchronisation in between, against the batch form"""
    import torch
    S = torch.cuda.Stream()
    c = TM._context(stream=S.cuda_stream)
    try:
        n = FRAMES * 2
        src = [torch.from_numpy(x).cuda() for x in mat['pink']]
        pcm = [torch.zeros_like(x) for x in src]
        shapes = {'units': (torch.uint8, n * 212), 'choice': (torch.uint8, n), 'modes': (torch.uint8, n), 'taken': (torch.uint8, n),
                  'shifts': (torch.int8, n * 52), 'distortion': (torch.float64, n * 16), 'energy': (torch.float64, n * 8),
                  'weights': (torch.float64, n * 52)}
        t = {k: torch.zeros(size, dtype=d, device='cuda') for k, (d, size) in shapes.items()}
        busy = torch.ones(1 << 26, dtype=torch.float32, device='cuda')
        torch.cuda.synchronize()
        call = lambda: c.encode_measured_modes_device([p.data_ptr() for p in pcm], FRAMES, CAND8, t['units'].data_ptr(), t['choice'].data_ptr(),
                                                      t['modes'].data_ptr(), t['taken'].data_ptr(), t['shifts'].data_ptr(),
                                                      t['distortion'].data_ptr(), t['energy'].data_ptr(), scale_factor_offsets=OFFSETS,
                                                      masking=True, weights_ptr=t['weights'].data_ptr())
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
        got['weights'] = got['weights'].reshape(-1, 52)
        assert same(got, dict(baseline['pink']))
    finally:
        c.close()


# ---- against the model ----
MODEL_CASES = [('pink', (0,), 'packaged', CAND8), ('pink', OFFSETS, 'packaged', X.PINK_SF_CANDIDATES), ('white', (0,), 'packaged', CAND8),
               ('white', OFFSETS, 'packaged', X.PINK_SF_CANDIDATES), ('white', (0,), 'self', CAND8)]


@pytest.mark.parametrize('material,offsets,tables,cand', MODEL_CASES, ids=['pink-0', 'pink-5', 'white-0', 'white-5', 'white-0-self'])
def test_against_the_model(two, mat, material, offsets, tables, cand):
    m = X.case(material, tables, offsets, cand)
    assert (MM.first_of_exact_ties(m['final']).sum(axis=1) == 1).all()                # exactly one admissible candidate per unit
    for which in KINDS:
        got = batch(two[which], mat[material], cand, offsets, tables)
        print(which, 'winners', np.bincount(got['choice'], minlength=len(cand)).tolist(), 'taken', int(got['taken'].sum()), 'of', len(got['taken']),
              'largest relative error of T %.3g, of E %.3g, of P %.3g' % (np.max(np.abs(got['distortion'] - m['D']) / m['D']),
                                                                           np.max(np.abs(got['energy'] - m['E']) / m['E']),
                                                                           np.max(np.abs(got['weights'] - m['P']) / m['P'])))
        assert X.check_outputs(m, got) is None
        ar = np.arange(len(got['choice']))
        assert SF.check_valid(got['units'], m['coefs'], got['taken'], None_plain(got, m), offsets) is None
        assert (np.abs(got['weights'] - MK.weights(MK.unit_tables(0, material, offsets)['EK'][:, 0, :, 0], *MK.named(tables))[0])
                <= X.REL * m['P']).all()
        # the reported weighted T_final of the winner is what the bytes give under the reported weights
        from_bytes = MK.weighted_errors(got['units'], m['coefs'], got['weights'])
        won = got['distortion'][ar, got['choice']]
        want = np.where(got['taken'] != 0, won[:, 1], won[:, 0])
        assert (np.abs(from_bytes - want) <= X.REL * want).all()
    # the Python wrapper: the same outputs, with and without the reports
    c = two['wide']
    wrapped = c.encode_measured_modes(mat[material], [BM.triple_of(b) for b in cand], scale_factor_offsets=offsets, return_distortion=True,
                                      return_shifts=True, masking=MK.named(tables), return_weights=True)
    assert same(dict(zip(OUTPUTS, wrapped)), got)
    assert same(dict(zip(OUTPUTS[:4], c.encode_measured_modes(mat[material], cand, scale_factor_offsets=offsets, masking=MK.named(tables)))),
                {k: got[k] for k in OUTPUTS[:4]})
    if tables == 'packaged':
        assert same(dict(zip(OUTPUTS[:4], c.encode_measured_modes(mat[material], cand, scale_factor_offsets=offsets, masking=True))),
                    {k: got[k] for k in OUTPUTS[:4]})


def None_plain(got, m):
    """scale_factor_choice_lib.check_valid judges the unweighted error of the bytes: hand it that error as both figures, as
    masked_alloc_lib.check_valid does -- the bytes do not reveal the weights"""
    plain = np.array([MK.MA.weighted_error(got['units'][u], m['coefs'][u]) for u in range(len(got['units']))])
    return np.stack([plain, plain], axis=1)


# ---- narrow against wide ----
@pytest.mark.parametrize('nch', [1, 2])
@pytest.mark.parametrize('material', ['pink', 'white', 'silence'])
def test_narrow_against_wide(two, mat, material, nch):
    for frames in COUNTS:
        chans = cut(mat[material], min(frames, len(mat[material][0]) // 512), nch)
        for cand in CAND_SETS:
            for offsets, tables in ((OFFSETS, 'packaged'), ((0,), 'self')):
                a, b = batch(two['narrow'], chans, cand, offsets, tables), batch(two['wide'], chans, cand, offsets, tables)
                assert same(a, b), (frames, cand, offsets)
                if material == 'silence':
                    assert not a['choice'].any() and not a['taken'].any() and not bits(a['distortion']).any() and not bits(a['energy']).any()
                    assert np.array_equal(bits(a['weights']), bits(np.broadcast_to(1.0 / MK.named(tables)[0], a['weights'].shape)))


# ---- seams ----
def test_seams_of_the_dispatch_and_of_the_grid(ctx, two):
    """8 192 units is the largest launch of the workgroup kernel on a default context and one sweep of the wave kernel's bounded
    grid: 8 192 and 8 193 units on a default context, 8 190 .. 8 194 on the wave-per-unit context, all as rows of one larger call"""
    large = 8400
    with_halo = BB.material()[0]
    reps = -(-(large + 2) // (FRAMES + 2))
    chans = [np.tile(with_halo[0], reps)[2 * 512:(large + 2) * 512]]
    for cand, offsets in (([10, 58], (0,)), (CAND8, OFFSETS)):
        whole = batch(two['narrow'], chans, cand, offsets)
        assert len(set(whole['choice'][-FRAMES:].tolist())) > 1
        for frames in (8192, 8193):
            assert same(batch(ctx, cut(chans, frames, 1), cand, offsets), TM.rows(whole, 0, frames, 1)), frames
        for frames in (8190, 8191, 8192, 8193, 8194):
            assert same(batch(two['narrow'], cut(chans, frames, 1), cand, offsets), TM.rows(whole, 0, frames, 1)), frames
        assert same(batch(ctx, chans, cand, offsets), whole)


# ---- hard inputs ----
def hard_model(name):
    cand = X.PINK_SF_CANDIDATES
    return H._once(('masked_modes', name), lambda: X.compose(cand, [H.tables(name, b) for b in cand], *MK.packaged()))


@pytest.mark.parametrize('name', H.NAMES)
def test_hard_material(two, name):
    """the five hard signals under the packaged tables, the five offsets and the candidates [0, 10, 58]: narrow against wide on
    every unit; the column of byte 0 and weights bit for bit the masked call's; against the model where no decision of the model
    is close; silent units choose candidate 0 with +0.0 figures"""
    chans, cand = H.material(name), X.PINK_SF_CANDIDATES
    m = hard_model(name)
    got = batch(two['narrow'], chans, cand)
    assert same(got, batch(two['wide'], chans, cand))
    zero = masked_under_zero(two['wide'], chans, OFFSETS, 'packaged')
    assert np.array_equal(bits(got['distortion'][:, 0]), bits(zero['distortion'])) and np.array_equal(bits(got['energy'][:, 0]), bits(zero['energy']))
    assert np.array_equal(bits(got['weights']), bits(zero['weights']))
    silent = (m['E'] == 0).all(axis=1)
    with np.errstate(invalid='ignore'):
        close = ((m['margin'] <= H.MARGIN) & (m['margin'] > 0)).any(axis=1) | (MM.first_of_exact_ties(m['final']).sum(axis=1) != 1)
    close &= ~silent
    print(name, 'close %d silent %d of %d' % (close.sum(), silent.sum(), len(close)), 'winners', np.bincount(got['choice'], minlength=3).tolist())
    assert close.sum() <= len(close) // 3
    assert X.check_outputs(H.rows(m, ~close), H.rows(got, ~close)) is None
    for g, want in ((got['distortion'][:, :, 0], m['D'][:, :, 0]), (got['energy'], m['E']), (got['weights'], m['P'])):   # every unit
        assert (np.abs(g - want) <= X.REL * want).all()
    assert not got['choice'][silent].any() and not got['taken'][silent].any()
    assert not bits(got['distortion'][silent]).any() and not bits(got['energy'][silent]).any()


@pytest.mark.parametrize('which', KINDS)
def test_non_finite_pcm(two, which):
    """one NaN and one +Inf in the PCM: C1_OK; a NaN M_b falls to the floor; a unit whose T_final is NaN under every candidate
    chooses candidate 0 and is not taken; the units before the first bad sample are the clean run's; the units the bad samples do
    not reach agree with the model"""
    c = two[which]
    chans, cand = H.nonfinite_material(), H.NONFINITE_CANDIDATES
    floor, spread = MK.packaged()
    m = H._once(('masked_modes', 'nonfinite'), lambda: X.case_of(chans, floor, spread, OFFSETS, cand))
    got = batch(c, chans, cand)                                                      # capi.check: C1_OK
    lost = np.isnan(m['final']).all(axis=1)
    sound = np.isfinite(m['D']).all(axis=(1, 2)) & np.isfinite(m['E']).all(axis=1)
    u = np.arange(2 * H.NONFINITE_FRAMES)
    clean_rows = u // 2 < np.array([H.NONFINITE_AT[ch][0] for ch in (0, 1)])[u % 2]
    assert lost.any() and not (lost & clean_rows).any() and sound[clean_rows].all()
    assert not got['choice'][lost].any() and not got['taken'][lost].any() and (got['modes'][lost] == cand[0]).all()
    assert np.array_equal(got['units'][lost], c.encode_modes(chans, got['modes'].reshape(-1, 2))[lost])
    # the unit that holds the bad sample in its all-long spectrum: every M_b is NaN, every threshold the floor
    bad = ~np.isfinite(masked_under_zero(c, chans, (0,), 'flat')['energy'])
    assert bad.any() and np.array_equal(bits(got['weights'][bad]), bits(np.broadcast_to(1.0 / floor, got['weights'][bad].shape)))
    assert np.isfinite(got['weights']).all() and (got['weights'] > 0).all()
    ar = np.arange(len(lost))
    fin = np.where(got['distortion'][:, :, 1] < got['distortion'][:, :, 0], got['distortion'][:, :, 1], got['distortion'][:, :, 0])
    assert not np.isnan(fin[ar, got['choice']])[~np.isnan(fin).all(axis=1)].any()      # a NaN never wins
    clean = batch(c, H.nonfinite_material(clean=True), cand)
    assert same(H.rows(got, clean_rows), H.rows(clean, clean_rows))
    assert X.check_outputs(H.rows(m, sound), H.rows(got, sound)) is None
    assert np.array_equal(bits(got['weights']), bits(masked_under_zero(c, chans, (0,), 'packaged')['weights']))


# ---- housekeeping ----
def test_outputs_do_not_depend_on_which_are_asked_for(two, mat, baseline):
    for which in KINDS:
        full = baseline['pink']
        asks = [(k,) for k in OUTPUTS] + [tuple(x for x in OUTPUTS if x != k) for k in OUTPUTS]
        for ask in asks:
            got = batch(two[which], mat['pink'], CAND8, ask=ask)
            assert same(got, {k: full[k] for k in ask}), (which, ask)


def test_other_calls_afterwards_give_their_usual_bits(ctx, mat, baseline):
    """a measure-only call hands no winner on; a plain call, an unweighted search and a masked call behind it see their own
    records only"""
    plain_modes = np.full((FRAMES, 2), 58, dtype=np.uint8)
    before = {'search': TM.batch(ctx, mat['pink'], CAND8), 'masked': masked_under_zero(ctx, mat['pink'], OFFSETS, 'specs')}
    for ask in (('choice', 'weights'), OUTPUTS):
        batch(ctx, mat['pink'], CAND8, ask=ask)
        assert np.array_equal(ctx.encode_modes(mat['pink'], plain_modes), BM.oracle_encode_modes(mat['pink'], plain_modes)[0])
        batch(ctx, mat['pink'], [58], ask=ask)
        assert same(TM.batch(ctx, mat['pink'], CAND8), before['search'])
        batch(ctx, mat['pink'], CAND8, ask=ask)
        assert same(masked_under_zero(ctx, mat['pink'], OFFSETS, 'specs'), before['masked'])
        assert same(batch(ctx, mat['pink'], CAND8), baseline['pink'])


def test_options_reach_the_allocation_only(ctx, mat, baseline):
    o = c1.EncoderOptions({'transientThresholdLow': 0.5, 'fixedBlockModes': [2, 0, 3]})
    assert same(batch(ctx, mat['pink'], CAND8, options=o), baseline['pink'])
    got = batch(ctx, mat['pink'], CAND8, options=c1.EncoderOptions({'allocationBias': 2.0}))
    assert not np.array_equal(got['distortion'][:, :, 0], baseline['pink']['distortion'][:, :, 0])           # T_ref follows the bias
    assert np.array_equal(bits(got['energy']), bits(baseline['pink']['energy']))
    assert np.array_equal(bits(got['weights']), bits(baseline['pink']['weights']))


def test_rejections_leave_the_outputs_untouched_and_the_next_call_unharmed(ctx, mat, baseline):
    import torch
    lib = capi.load()
    n = FRAMES * 2
    buf = {'units': (torch.uint8, n * 212, 0xA5), 'choice': (torch.uint8, n, 0xA5), 'modes': (torch.uint8, n, 0xA5), 'taken': (torch.uint8, n, 0xA5),
           'shifts': (torch.int8, n * 52, 0x5A), 'distortion': (torch.float64, n * 16, -1.0), 'energy': (torch.float64, n * 8, -1.0),
           'weights': (torch.float64, n * 52, -1.0)}
    t = {k: torch.full((size,), fill, dtype=d, device='cuda') for k, (d, size, fill) in buf.items()}
    dev = [torch.from_numpy(c).cuda() for c in mat['pink']]
    torch.cuda.synchronize()
    ptrs = capi.ptr_array([d.data_ptr() for d in dev])
    opts = c1.EncoderOptions().to_c()
    outs = [C.c_void_p(t[k].data_ptr()) for k in OUTPUTS]
    good_floor, good_spread = MK.packaged()

    def call(cand, offs=OFFSETS, n_cand=None, n_off=None, o=outs, frames=FRAMES, halo=0, channels=2, floor=good_floor, spread=good_spread):
        cb, ob = np.asarray(cand, dtype=np.uint8), np.asarray(offs, dtype=np.int8)
        fl = None if floor is None else np.ascontiguousarray(floor, dtype=np.float64)
        sp = None if spread is None else np.ascontiguousarray(spread, dtype=np.float64)
        return lib.c1_encode_measured_modes_masked_device(ctx._h, ptrs, channels, frames, halo, C.byref(opts), cb.ctypes.data,
                                                          len(cb) if n_cand is None else n_cand, ob.ctypes.data if ob.size else None,
                                                          len(ob) if n_off is None else n_off, None if fl is None else fl.ctypes.data,
                                                          None if sp is None else sp.ctypes.data, *o)

    def with_entry(a, at, value):
        a = np.array(a, dtype=np.float64)
        a.reshape(-1)[at] = value
        return a

    err = lambda: lib.c1_last_error().decode()
    assert call([0, 58, 0]) == C1_ERR_ARG and 'c1_encode_measured_modes_masked_device' in err() and 'candidate 2' in err(), err()
    assert call([0, 1]) == C1_ERR_ARG and 'candidate 1' in err() and 'low field' in err(), err()
    assert call([0, 64]) == C1_ERR_ARG and 'bits 6-7' in err(), err()
    assert call(CAND8 + [0], n_cand=9) == C1_ERR_ARG and 'n_cand = 9' in err(), err()
    assert call(CAND8, n_cand=0) == C1_ERR_ARG and 'n_cand = 0' in err(), err()
    assert call(CAND8, offs=()) == C1_ERR_ARG and 'n_offsets = 0' in err(), err()
    assert call(CAND8, offs=(0, 9)) == C1_ERR_ARG and 'outside -8..8' in err(), err()
    assert call(CAND8, offs=(0, 1, 1)) == C1_ERR_ARG and 'repeats' in err(), err()
    assert call(CAND8, offs=(1, 0)) == C1_ERR_ARG and 'not 0' in err(), err()
    assert call(CAND8, floor=None) == C1_ERR_ARG and 'c1_encode_measured_modes_masked_device: mask_floor is NULL' in err(), err()
    assert call(CAND8, floor=with_entry(good_floor, 7, 0.0)) == C1_ERR_ARG and 'mask_floor[7] = 0 is outside [1e-60, 1e60]' in err(), err()
    assert call(CAND8, floor=with_entry(good_floor, 51, np.nan)) == C1_ERR_ARG and 'mask_floor[51]' in err(), err()
    assert call(CAND8, spread=with_entry(good_spread, 52 * 3 + 5, -1.0)) == C1_ERR_ARG
    assert 'mask_spread[161] = -1 (masker 5 onto BFU 3) is outside [0, 1e60]' in err(), err()
    assert call(CAND8, spread=with_entry(good_spread, 2703, np.inf)) == C1_ERR_ARG and 'mask_spread[2703]' in err(), err()
    assert call(CAND8, o=[None] * 8) == C1_ERR_ARG and 'energy and weights are all NULL' in err(), err()
    assert call(CAND8, halo=3) == C1_ERR_ARG
    assert call(CAND8, channels=3) == C1_ERR_ARG
    assert call(CAND8, frames=-1) == C1_ERR_ARG
    assert call(CAND8, frames=0) == C1_OK                                            # frames = 0 writes nothing
    ctx.synchronize()
    for k, (d, size, fill) in buf.items():
        assert (t[k].cpu().numpy() == fill).all(), k
    assert same(batch(ctx, mat['pink'], CAND8), baseline['pink'])
    with pytest.raises(ValueError, match='weights_ptr needs masking'):
        ctx.encode_measured_modes_device([d.data_ptr() for d in dev], FRAMES, CAND8, t['units'].data_ptr(), weights_ptr=t['weights'].data_ptr())
