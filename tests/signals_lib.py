"""n signals of any lengths from their own pools in one call (c1_*_signals*): the shared shapes of the GPU tests and the
oracle's answers for them, computed once per key and never modified.  The oracle is n separate closures: signal i alone through
stream_state_lib.oracle_encode / oracle_decode from its own pool."""
import numpy as np

import oracle_lib as O
import stream_state_lib as SS

# empty signals; only the first fix-up; both fix-ups and no bulk frame; the first bulk frame; short neighbours back to back;
# more than one 64-frame run
LENGTHS = [0, 1, 2, 3, 1, 0, 7, 66, 2, 130, 1]
OPTION_SETS = {
    'detect': {'transientThresholdLow': 1.0},
    'long': {'fixedBlockModes': [0, 0, 0], 'allocationBias': 1},
    'short_bias2': {'fixedBlockModes': [2, 2, 3], 'allocationBias': 2},
    'mixed_bias05': {'fixedBlockModes': [0, 2, 0], 'allocationBias': 0.5},
}
FIXED = [k for k, v in OPTION_SETS.items() if 'fixedBlockModes' in v]
ENC_POOL_SEED, DEC_POOL_SEED = 0x5151, 0x7171

_cache = {}


def _once(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def frozen(a):
    a.setflags(write=False)
    return a


def signals(material='pink', lengths=None):
    """'pink': gen_pinkT with one seed per signal (bursts at frame 5 of every 8: detection switches blocks inside the signals
    of 7 frames and more).  'loud_quiet': the same, but the 66-frame signal is full-scale white noise and is followed by an
    all-zero signal and by one at 1e-30."""
    lengths = LENGTHS if lengths is None else lengths

    def make():
        sigs = [O.gen_pinkT(100 + i, n * 512) for i, n in enumerate(lengths)]
        if material == 'loud_quiet':
            sigs[7] = O.gen_white(77, lengths[7] * 512)
            sigs[8] = np.zeros(lengths[8] * 512, dtype=np.float32)
            sigs[9] = (O.gen_white(78, lengths[9] * 512).astype(np.float64) * 1e-30).astype(np.float32)
        return [frozen(s) for s in sigs]
    return _once(('signals', material, tuple(lengths)), make)


def enc_pools(n=len(LENGTHS), seed=ENC_POOL_SEED):
    return _once(('enc_pools', n, seed), lambda: frozen(SS.random_pools(seed, n, SS.ENC_FLOATS)))


def dec_pools(n=len(LENGTHS), seed=DEC_POOL_SEED):
    return _once(('dec_pools', n, seed), lambda: frozen(SS.random_pools(seed, n, SS.DEC_FLOATS)))


def oracle_encode_signals(sigs, oset, start=None):
    """-> (list of (frames_i, 212) units, (n, 483) pools after each signal): one oracle closure per signal"""
    units, states = [], np.zeros((len(sigs), SS.ENC_FLOATS), dtype=np.float32)
    for i, x in enumerate(sigs):
        u, st = SS.oracle_encode([np.ascontiguousarray(x)], oset, None if start is None else start[i:i + 1].copy())
        units.append(u)
        states[i] = st[0]
    return units, states


def oracle_decode_signals(units_list, start=None):
    pcm, states = [], np.zeros((len(units_list), SS.DEC_FLOATS), dtype=np.float32)
    for i, u in enumerate(units_list):
        p, st = SS.oracle_decode(np.ascontiguousarray(u), 1, None if start is None else start[i:i + 1].copy())
        pcm.append(p[0])
        states[i] = st[0]
    return pcm, states


def want_encode(material, oname, pools):
    """the shared shapes under option set `oname`, from fresh pools (pools False) or from enc_pools()"""
    def make():
        u, st = oracle_encode_signals(signals(material), OPTION_SETS[oname], enc_pools() if pools else None)
        return [frozen(x) for x in u], frozen(st)
    return _once(('want_encode', material, oname, bool(pools)), make)


def want_decode(material, oname, pools):
    """the oracle's PCM and pools for the oracle's units of want_encode(material, oname, False)"""
    def make():
        p, st = oracle_decode_signals(want_encode(material, oname, False)[0], dec_pools() if pools else None)
        return [frozen(x) for x in p], frozen(st)
    return _once(('want_decode', material, oname, bool(pools)), make)


def offsets(lengths):
    off = np.zeros(len(lengths) + 1, dtype=np.int64)
    off[1:] = np.cumsum(lengths)
    return off


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def same_units(got, want):
    return len(got) == len(want) and all(g.shape == w.shape and np.array_equal(g, w) for g, w in zip(got, want))


def first_bad(got, want):
    for i, (g, w) in enumerate(zip(got, want)):
        if g.shape != w.shape:
            return ('signal', i, 'shape', g.shape, w.shape)
        bad = np.flatnonzero((np.asarray(g).reshape(len(g), -1) != np.asarray(w).reshape(len(w), -1)).any(axis=1)) if len(g) else []
        if len(bad):
            return ('signal', i, 'frames', list(bad[:6]))
    return None


# the five items of the AEA tests: mono of 700 samples, stereo of 1 sample, stereo with channels of unequal length, mono of 0
# samples, stereo of 40 000 samples
def aea_items():
    def make():
        w = O.gen_white
        return [[w(1, 700)], [w(2, 1), w(3, 1)], [w(4, 1300), w(5, 900)], [np.zeros(0, dtype=np.float32)], [O.gen_pinkT(6, 40000), w(7, 40000)]]
    return _once('aea_items', make)
