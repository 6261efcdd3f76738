"""GPU: the workgroup-per-unit kernel of the mode search (k_measured_modes_wide, c1_k_measured_modes_wide.hip) against the
wave-per-unit one (k_measured_modes), on two contexts of the module: `narrow` (C1_MEASURED_WIDE=0) and `wide` (C1_MEASURED_WIDE=1),
through c1_encode_measured_modes_batch.  Every output of every unit bit for bit, with no exemptions: 1, 2, 3, 63 and 130 frames,
mono and stereo, pink, white, silence and the hard material of tests/hard_material_lib.py; candidate sets that need the long plane
alone, the short plane alone and both; offsets {0} and the five.  Then the wide kernel against the CPU models exactly as the
narrow one is compared in tests/test_gpu_measured_modes.py and tests/test_gpu_measured_kernels.py, NaN and +Inf in the PCM,
measure-only calls, every subset of the outputs, one "measure" launch per call, and the seams of the dispatch."""
import os
import re

import numpy as np
import pytest

import best_bias_lib as BB
import hard_material_lib as H
import measured_modes_lib as MM
import test_gpu_measured_modes as TM

pytestmark = pytest.mark.gpu

KINDS = ('narrow', 'wide')
CAND8 = MM.CANDIDATES
CAND_SETS = ([0], [58], [10], [0, 58], [58, 0], CAND8)      # the long plane alone, the short plane alone, both
OFFSET_SETS = ((0,), MM.OFFSETS)
COUNTS = (1, 2, 3, 63, 130)
OUTPUTS = TM.OUTPUTS


def wide_units():
    """kMeasuredModesWideUnits of csrc/c1_internal.h: launches of at most this many units take the wide kernel by default"""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'carta1_amd', 'csrc', 'c1_internal.h')
    with open(path) as f:
        return int(re.search(r'constexpr int64_t kMeasuredModesWideUnits = (\d+);', f.read()).group(1))


@pytest.fixture(scope='module')
def two():
    ctxs = {'narrow': TM._context(C1_MEASURED_WIDE=0), 'wide': TM._context(C1_MEASURED_WIDE=1)}
    yield ctxs
    for c in ctxs.values():
        c.close()


@pytest.fixture(scope='module')
def mat():
    body = BB.material()[1]
    return {'pink': body, 'white': MM.BMO.material('white'), 'silence': [np.zeros(BB.FRAMES * 512, dtype=np.float32)] * 2}


def measure_launches(ctx, call):
    """(launches under "measure", launches under "pack") of one call"""
    ctx.set_profiling(True)
    try:
        call()
        ms, launches = ctx.kernel_ms('measure')
        assert ms > 0
        return launches, ctx.kernel_ms('pack')[1]
    finally:
        ctx.set_profiling(False)


# ---- 1. wide against narrow ----
@pytest.mark.parametrize('nch', [1, 2])
@pytest.mark.parametrize('material', ['pink', 'white', 'silence'])
def test_wide_and_narrow_give_the_same_bits(two, mat, material, nch):
    for frames in COUNTS:
        chans = [c[:frames * 512] for c in mat[material][:nch]]
        for cand in CAND_SETS:
            for offsets in OFFSET_SETS:
                a, b = TM.batch(two['narrow'], chans, cand, offsets), TM.batch(two['wide'], chans, cand, offsets)
                assert TM.same(a, b), (frames, cand, offsets, [k for k in a if not np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8))])
                if material == 'silence':
                    assert not b['choice'].any() and not b['taken'].any() and not b['distortion'].view(np.uint64).any()


@pytest.mark.parametrize('sf', [False, True], ids=['offset0', 'offsets'])
@pytest.mark.parametrize('name', H.NAMES)
def test_hard_material(two, name, sf):
    """the level-15 cap, scale-factor indices 0 .. 3 and 63, 20-BFU units, the fallback record, exact ties and silence between
    coded frames: the same bits on all units, and the wide kernel against the composed model where the unit is not close"""
    chans, cand = H.material(name), H.modes_candidates(sf)
    offsets = H.OFFSETS if sf else (0,)
    got = TM.batch(two['wide'], chans, cand, offsets)
    assert TM.same(TM.batch(two['narrow'], chans, cand, offsets), got)
    m = H.modes_model(name, sf)
    close = H.modes_classes(name, sf)[2]                                      # tests/test_hard_material_cpu.py: at most 4 of 24, on the tones
    assert MM.check_case(H.rows(m, ~close), H.rows(got, ~close)) is None
    for cand_set in ([0], [58], [0, 58]):
        assert TM.same(TM.batch(two['narrow'], chans, cand_set, offsets), TM.batch(two['wide'], chans, cand_set, offsets)), cand_set


# ---- 2. the wide kernel against the model ----
@pytest.mark.parametrize('material,sf', [('pink', False), ('pink', True), ('white', False), ('white', True)])
def test_wide_against_the_model(two, mat, material, sf):
    cand = MM.candidates_of(material, sf)
    got = TM.batch(two['wide'], mat[material], cand, MM.OFFSETS if sf else (0,))
    print('winners', np.bincount(got['choice'], minlength=len(cand)).tolist(), 'taken', int(got['taken'].sum()), 'of', len(got['taken']))
    assert MM.check_outputs(material, sf, got) is None


def test_wide_candidate_subsets_against_the_model(two, mat):
    at = MM.PINK_SF_CANDIDATES.index
    for cand in ([0], [58], [10], [0, 58], [58, 0]):
        got = TM.batch(two['wide'], mat['pink'], cand)
        assert MM.check_outputs('pink', True, got, [at(b) for b in cand]) is None, cand


# ---- 3. non-finite PCM ----
def test_non_finite_pcm(two):
    """one NaN and one +Inf sample in pink noise: both contexts give the same bits; a unit whose T_final are all NaN chooses
    candidate 0 and is not taken; a NaN never wins elsewhere; the units the bad samples do not reach against the model"""
    chans, cand = H.nonfinite_material(), H.NONFINITE_CANDIDATES
    got = TM.batch(two['wide'], chans, cand, H.OFFSETS)
    assert TM.same(TM.batch(two['narrow'], chans, cand, H.OFFSETS), got)
    d = got['distortion']
    with np.errstate(invalid='ignore'):
        fin = np.where(d[:, :, 1] < d[:, :, 0], d[:, :, 1], d[:, :, 0])
    lost = np.isnan(fin).all(axis=1)
    m = H.nonfinite_modes_model()
    assert lost.any() and np.array_equal(lost, np.isnan(m['final']).all(axis=1))
    assert not got['choice'][lost].any() and not got['taken'][lost].any() and (got['modes'][lost] == cand[0]).all()
    ar = np.arange(len(lost))
    assert not np.isnan(fin[ar, got['choice']])[~lost].any()
    sound = np.isfinite(m['D']).all(axis=(1, 2)) & np.isfinite(m['E']).all(axis=1)
    assert MM.check_case(H.rows(m, sound), H.rows(got, sound)) is None


# ---- 4. which outputs are asked for; the launches ----
@pytest.mark.parametrize('which', KINDS)
def test_output_subsets_and_launches(two, mat, which):
    ctx = two[which]
    chans = [c[:33 * 512] for c in mat['pink']]
    full = TM.batch(ctx, chans, CAND8)
    subsets = [(k,) for k in OUTPUTS] + [tuple(j for j in OUTPUTS if j != k) for k in OUTPUTS]
    for ask in subsets:
        got = TM.batch(ctx, chans, CAND8, ask=ask)
        assert TM.same(got, {k: full[k] for k in ask}), ask
    assert measure_launches(ctx, lambda: TM.batch(ctx, chans, CAND8)) == (1, 1)
    assert measure_launches(ctx, lambda: TM.batch(ctx, chans, [58, 0], (0,))) == (1, 1)
    # measure only (units NULL): the search runs, no packing does
    assert measure_launches(ctx, lambda: TM.batch(ctx, chans, CAND8, ask=OUTPUTS[1:])) == (1, 0)
    assert measure_launches(ctx, lambda: TM.batch(ctx, chans, [10], ask=('distortion',))) == (1, 0)


# ---- 5. the seams of the dispatch ----
def test_threshold_of_the_default_dispatch(two, mat):
    """T and T + 1 units on a context without the variable -- the last launch of the wide kernel and the first of the narrow one --
    are rows of one larger call"""
    T = wide_units()
    if T == 0:
        pytest.skip('kMeasuredModesWideUnits is 0: the wide kernel is reachable under C1_MEASURED_WIDE=1 alone')
    ctx = TM._context()
    try:
        reps = -(-(T + 64) // BB.FRAMES)
        chans = [np.tile(mat['pink'][0], reps)[:(T + 64) * 512]]
        large = TM.batch(two['narrow'], chans, [10, 58])
        for frames in (T, T + 1):
            got = TM.batch(ctx, [chans[0][:frames * 512]], [10, 58])
            assert TM.same(got, TM.rows(large, 0, frames, 1)), frames
    finally:
        ctx.close()


def test_bounded_grid_seam_of_the_narrow_kernel(two, mat):
    """8 190 .. 8 194 units on the context that never takes the wide kernel: 2 048 workgroups of 4 waves, past which the waves
    stride; rows of one larger call, two candidates"""
    reps = -(-8400 // BB.FRAMES)
    chans = [np.tile(mat['pink'][0], reps)[:8400 * 512]]
    large = TM.batch(two['narrow'], chans, [10, 58], (0,))
    for frames in (8190, 8191, 8192, 8193, 8194):
        got = TM.batch(two['narrow'], [chans[0][:frames * 512]], [10, 58], (0,))
        assert TM.same(got, TM.rows(large, 0, frames, 1)), frames
    # the same launch on the wide kernel: a grid of 8 194 workgroups
    assert TM.same(TM.batch(two['wide'], [chans[0][:8194 * 512]], [10, 58], (0,)), TM.rows(large, 0, 8194, 1))
