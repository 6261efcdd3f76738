"""GPU: the heap step of the bit-allocation kernels (heap_phase, c1_k_allocate.hip) at the shapes where a sift can go
wrong, against the oracle's allocateBits (c1o_allocate) bit for bit: BFU count, scale-factor indices and all 52 word
lengths through Context.quantize_frames, the chosen candidate and every candidate's total through alloc_bounds_device.

The heap keeps slots 0..2 in registers and slots 3..51 in rows of LDS, with one sentinel row behind them, and sifts a
hole down at most six levels in two round trips.  So the cases are chosen by what the heap holds, not by what the
signal is: live BFU counts at every boundary between registers and rows, at every heap level and at the sentinel;
entries that leave while the last element is the root, one of its children, or in a row; priorities that tie at every
step; end-games in which large BFUs stop fitting while bits are left; launches of partial waves; the table path
(no integer rank form) beside the affine one; and tonal vectors, which keep several candidates alive so that both
rounds of k_alloc_rest run.  Index vectors are realised as coefficient frames the way tests/test_gpu_alloc_diet.py
does it."""
import numpy as np
import pytest

import oracle_lib as O
from test_alloc_tables_cpu import host_tables
from test_gpu_alloc_diet import SPECS, _check, _coefs, _defeating_tables

pytestmark = pytest.mark.gpu

LIVE_COUNTS = (0, 1, 2, 3, 4, 7, 8, 15, 16, 31, 32, 51, 52)


@pytest.fixture(scope='module')
def ctx():
    import carta1_amd as c1
    c = c1.Context(0)
    yield c
    c.close()


def _live_counts(rng):
    """exactly k live BFUs: the first k, the last k, k anywhere; loud, quiet and mixed"""
    out = []
    for k in LIVE_COUNTS:
        for where in range(3):
            for level in range(4):
                v = np.zeros(52, int)
                at = np.arange(k) if where == 0 else (np.arange(52 - k, 52) if where == 1 else rng.permutation(52)[:k])
                v[at] = (rng.randint(1, 64, size=k), rng.randint(1, 8, size=k), rng.randint(56, 64, size=k),
                         np.full(k, rng.randint(1, 64)))[level]
                out.append(v)
    return np.array(out)


def _leaving(rng):
    """one loud BFU that reaches the last word length while 0..5 quiet ones are live: the element that replaces the
    root comes from the root itself, from either of its children and from the first rows in turn"""
    out = []
    for loud in (0, 3, 4, 7, 11, 23, 24, 35, 43, 44, 51):
        for others in range(6):
            for quiet in (1, 9, 30, 62):
                v = np.zeros(52, int)
                rest = np.array([b for b in rng.permutation(52) if b != loud][:others], int)
                v[rest] = np.clip(quiet + rng.randint(0, 2, size=others), 1, 63)
                v[loud] = 63
                out.append(v)
    return np.array(out)


def _ties(rng):
    out = [np.repeat(np.arange(64)[:, None], 52, axis=1)]                                       # all equal: all 0 .. all 63
    out.append(np.clip(rng.randint(1, 12, size=(192, 1)) + 3 * rng.randint(0, 18, size=(192, 52)), 0, 63))   # three apart
    two = np.where(rng.uniform(size=(64, 52)) < 0.5, 40, 43)                                    # two levels, one step apart
    out.append(two)
    return np.concatenate(out)


def _end_games(rng):
    """loud BFUs of 20 coefficients next to quiet small ones: near the end the large ones stop fitting with bits left"""
    out = []
    for n_loud in range(1, 9):
        for base in (1, 6, 12, 20, 33):
            for _ in range(4):
                v = np.zeros(52, int)
                v[:44] = np.clip(base + rng.randint(0, 4, size=44), 0, 63) * (rng.uniform(size=44) < 0.8)
                v[44 + rng.permutation(8)[:n_loud]] = rng.randint(52, 64, size=n_loud)
                out.append(v)
    return np.array(out)


def _tonal(rng):
    """falling spectra whose upper BFUs are silent or nearly so: smaller candidates stay alive and win"""
    n = 384
    tilt = -rng.uniform(0.8, 3.0, size=(n, 1)) * np.arange(52)[None, :]
    v = np.clip(rng.randint(45, 64, size=(n, 1)) + tilt + rng.randint(-2, 3, size=(n, 52)), 0, 63).astype(int)
    peaks = rng.randint(0, 52, size=(n, 3))
    for i in range(n):
        v[i, peaks[i]] = np.minimum(63, v[i, peaks[i]] + rng.randint(5, 25, size=3))
    return v


def _cases():
    rng = np.random.RandomState(20261)
    groups = {'live counts': _live_counts(rng), 'leaving': _leaving(rng), 'ties': _ties(rng), 'end-games': _end_games(rng),
              'tonal': _tonal(rng), 'anything': rng.randint(0, 64, size=(2048, 52))}
    return {k: v.astype(np.int32) for k, v in groups.items()}


@pytest.fixture(scope='module')
def cases():
    return _cases()


def test_cases_are_what_they_claim(cases):
    live = (cases['live counts'] != 0).sum(axis=1)
    assert set(live) == set(LIVE_COUNTS)
    assert set((cases['leaving'] != 0).sum(axis=1)) == {1, 2, 3, 4, 5, 6}
    assert (np.array(SPECS)[44:] == 20).all()
    assert sum(len(v) for v in cases.values()) >= 3000


@pytest.mark.parametrize('table_name', ['default', 'no integer rank form'])
def test_heap_step_against_the_oracle(ctx, cases, table_name):
    table = O.biased_table(1.0) if table_name == 'default' else _defeating_tables()[0]
    t = host_tables(table)
    assert t['affine'] == (1 if table_name == 'default' else 0)             # which instance of heap_phase runs
    for name, vectors in cases.items():
        _check(ctx, _coefs(vectors), table, '%s, %s' % (table_name, name), vectors)


def test_tonal_vectors_keep_smaller_candidates_alive(cases):
    """both rounds of k_alloc_rest have work: on these vectors the oracle itself chooses several BFU counts below 52"""
    from test_gpu_alloc_diet import _oracle
    nb, _, _ = _oracle(_coefs(cases['tonal']), O.biased_table(1.0))
    assert len(set(nb[nb < 52])) >= 3, np.unique(nb)


@pytest.mark.parametrize('units', [1, 63, 64, 65, 129])
def test_partial_waves(ctx, cases, units):
    """launches that end inside a wave: the lanes past the end hold empty heaps beside full ones"""
    pool = np.concatenate([cases['anything'][:96], cases['live counts'][-24:], cases['tonal'][:32]])
    rng = np.random.RandomState(units)
    vectors = pool[rng.permutation(len(pool))[:units]]
    for table in (O.biased_table(1.0), _defeating_tables()[0]):
        _check(ctx, _coefs(vectors), table, '%d units' % units, vectors)
