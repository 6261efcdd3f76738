"""CPU: how the frame-walking kernels lay out their work, without a GPU (geometry_lib.py restates it from the sources).
 1. c1k_pick_run, compiled from c1_internal.h as it stands, gives every batch a run of 4 to 64 frames, equal to the
    restatement and to test_gpu_spec.run_length, and clamps a forced C1_RUN_FRAMES below 4 up to 4;
 2. the speculative path's deferred-run slots and open-scale-factor masks fit their share of d_redo for every run the
    library can pick or be forced to, and would not for runs of 1 to 3 frames (the reason for that clamp);
 3. spread_block, the workgroup permutation of k_analysis_spec, is a bijection on [0, n) for every grid size."""
import os

import numpy as np
import pytest

import geometry_lib as G

MAX_UNITS = 1 << 18
FORCED = list(range(1, G.K_RUN_DEFAULT + 1))


@pytest.fixture(scope='module')
def picked():
    return G.compiled_runs(MAX_UNITS)


@pytest.fixture(scope='module')
def forced_runs():
    """C1_RUN_FRAMES = k -> the run the compiled rule gives (for every frames count of a small batch)"""
    out = {}
    for k in FORCED + [0, -3]:
        r = G.compiled_runs(64, forced=k)
        assert len(np.unique(np.concatenate([r[1], r[2]]))) == 1, (k, r)
        out[k] = int(r[1][0])
    return out


def test_constants_are_read_from_the_sources():
    assert G.K_RUN_DEFAULT == 64 and G.RUN_FLOOR == 4 and G.SPLIT == 2048
    assert G.K_LIST_HEAD >= 6                   # the counters the speculative path keeps (c1_k_spec.hip k_spec_totals reads [0..5])
    assert 0 < G.K_SPEC_MIN_UNITS <= G.K_RUN_DEFAULT * G.SPLIT


@pytest.mark.parametrize('channels', [1, 2])
def test_run_length_rule(picked, channels):
    import test_gpu_spec
    runs = picked[channels].astype(np.int64)
    frames = np.arange(1, runs.size + 1, dtype=np.int64)
    assert frames[-1] * channels == MAX_UNITS
    assert runs.min() == G.RUN_FLOOR and runs.max() == G.K_RUN_DEFAULT
    assert np.array_equal(runs, G.pick_run(frames, channels))
    assert np.all(np.diff(runs) >= 0)                                      # never shorter for a larger batch
    env = os.environ.pop('C1_RUN_FRAMES', None)
    try:
        for f in np.concatenate([frames[:5000], frames[5000::97], frames[-5:]]):
            assert test_gpu_spec.run_length(int(f), channels) == runs[f - 1], f
    finally:
        if env is not None:
            os.environ['C1_RUN_FRAMES'] = env
    # every run between the floor and the default is reached, and where the issue's sweep looks for it
    for r in range(G.RUN_FLOOR + 1, G.K_RUN_DEFAULT):
        lo, hi = G.frames_for_run(r, channels)
        assert runs[lo - 1] == r and runs[hi - 1] == r and runs[lo - 2] == r - 1 and runs[hi] == r + 1


def test_forced_run_is_clamped(forced_runs, monkeypatch):
    import test_gpu_spec
    for k, r in forced_runs.items():
        want = G.pick_run(1, 1) if k <= 0 else max(G.RUN_FLOOR, k)
        assert r == want, (k, r)
        if k > 0:
            assert G.pick_run(1000, 2, forced=k) == r
            monkeypatch.setenv('C1_RUN_FRAMES', str(k))
            assert test_gpu_spec.run_length(1000, 2) == r


def _layout_cases():
    """(frames, channels, ws_units) of one chunk: every frames count to 4096, then sampled to 2^20; a workspace exactly
    the chunk's size and larger ones (up to 4x: a context keeps the workspace of its largest call)"""
    rng = np.random.RandomState(5)
    frames = np.concatenate([np.arange(1, 4097), rng.randint(4097, 1 << 20, 4000), [(1 << 20) - 1, 1 << 20]]).astype(np.int64)
    out = []
    for ch in (1, 2):
        u = frames * ch
        for ws in (u, u + 1, u + 3, 2 * u - 1, 2 * u + 5, 3 * u + 2, 4 * u):
            out.append((frames, ch, np.maximum(ws, u)))
    return out


def test_redo_lists_fit_every_run(forced_runs):
    """every run the library can use: picked for the chunk, or forced to any C1_RUN_FRAMES from 1 to 64"""
    runs = sorted(set(forced_runs[k] for k in FORCED))
    for frames, ch, ws in _layout_cases():
        picked_run = G.pick_run(frames, ch)
        for run in runs + [picked_run]:
            fits, defer_hi, mask_lo, mask_hi, words = G.redo_layout(frames, ch, ws, run)
            bad = np.flatnonzero(~fits)
            assert bad.size == 0, ('run', run if np.ndim(run) == 0 else run[bad[0]], 'frames', frames[bad[0]], 'channels', ch,
                                   'ws_units', ws[bad[0]], 'defer end', defer_hi[bad[0]], 'masks', mask_lo[bad[0]], mask_hi[bad[0]],
                                   'words', words[bad[0]])


@pytest.mark.parametrize('run', [1, 2, 3])
def test_redo_lists_do_not_fit_runs_below_four(run):
    """why c1k_pick_run clamps a forced run: with 1 to 3 frames per run the slots outgrow their share of d_redo"""
    frames = np.arange(1, 1 << 16, dtype=np.int64)
    for ch in (1, 2):
        fits = G.redo_layout(frames, ch, frames * ch, run)[0]
        assert not fits.all(), (run, ch)
        assert not fits[-1000:].any()                # large chunks never fit


def _check_bijection(n, table, bits):
    x = G.spread_block(np.arange(n, dtype=np.uint32), n, bits, table)
    assert x.max(initial=0) < n
    seen = np.zeros(n, dtype=bool)
    seen[x] = True
    assert seen.all(), n


def _check_bijections(table, bits):
    """_check_bijection for every n with ceil(log2 n) = bits, sharing the work: block b's first step is table[b]"""
    for n in range((1 << bits) // 2 + 1, (1 << bits) + 1):
        assert G.spread_bits(n) == bits
        if bits < 4 or n < 64:
            _check_bijection(n, table, bits)
            continue
        x = table[:n].copy()
        todo = np.flatnonzero(x >= n)
        while todo.size:
            x[todo] = table[x[todo]]
            todo = todo[x[todo] >= n]
        seen = np.zeros(n, dtype=bool)
        seen[x] = True
        assert seen.all(), n


def test_spread_block_is_a_bijection_for_every_grid_to_2_16():
    for bits in range(0, 17):
        table = G.spread_round(np.arange(1 << bits, dtype=np.uint32), bits)
        assert np.array_equal(np.sort(table), np.arange(1 << bits))            # one round permutes [0, 2^bits)
        _check_bijections(table, bits)
        if bits < 4:
            assert np.array_equal(G.spread_block(np.arange(1 << bits), 1 << bits, bits), np.arange(1 << bits))


def test_spread_block_is_a_bijection_for_sampled_grids_to_2_22():
    rng = np.random.RandomState(11)
    for bits in range(17, 23):
        table = G.spread_round(np.arange(1 << bits, dtype=np.uint32), bits)
        lo = (1 << bits) // 2 + 1
        for n in [lo, lo + 1, (1 << bits) - 1, 1 << bits] + list(rng.randint(lo, (1 << bits) + 1, 3)):
            _check_bijection(int(n), table, bits)
    # the permutation really moves workgroups (it is not the identity) once it is on, and the shared walk above is the
    # function's own
    assert not np.array_equal(G.spread_block(np.arange(1000), 1000, 10), np.arange(1000))
    for n in (65, 1000, 40000):
        bits = G.spread_bits(n)
        table = G.spread_round(np.arange(1 << bits, dtype=np.uint32), bits)
        walk = G.spread_block(np.arange(n), n, bits)
        assert np.array_equal(walk, G.spread_block(np.arange(n), n, bits, table))
        assert all(int(G.spread_block(np.array([b]), n, bits)[0]) == walk[b] for b in (0, 1, n // 2, n - 1))
