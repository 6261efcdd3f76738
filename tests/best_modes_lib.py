"""The block modes of every sound unit chosen from candidates by least coding error (c1_encode_best_modes_*): the CPU model of
the weighted distortion D(u, k) and energy E(u, k), built from the oracle alone, and the material the CPU and GPU tests share.

Per candidate byte k the units come from block_modes_lib.oracle_encode_modes with that byte constant, the coefficients c_k from
best_bias_lib.coefficients (the oracle's QMF analysis and MDCT under the modes the units record) and d_k from
best_bias_lib.dequantized.  W is 1 for a band coded long, 1/4 for the low or mid band coded short and 1/2 for the high band
coded short; band(i) is low for i < 128, mid for i < 256, high otherwise.  Sums in numpy float64."""
import numpy as np

import best_bias_lib as BB
import block_modes_lib as BM
import oracle_lib as O

CANDIDATES = list(BM.DOMAIN_BYTES)               # all eight bytes of the domain, in DOMAIN_BYTES order
BIAS = 1.0
WHITE_FRAMES = 64
WHITE_SEEDS = (1, 2)
REL = 1e-12                                      # |D - model| <= REL * model: two roundings per term, W exact, and at most 511 * 2^-53 =
                                                 # 6e-14 for a sum of 512 non-negative terms in any order (the best-bias tests' bound)
CHOICE_REL = 3e-12                               # an admissible choice: model D <= model minimum * (1 + CHOICE_REL)
UNIQUE_REL = 1e-9                                # the material: every unit's model minimum is unique by more than this
BANDS = (slice(0, 128), slice(128, 256), slice(256, 512))
SHORT_WEIGHT = (0.25, 0.25, 0.5)


def material(kind):
    """'pink': best_bias_lib.material()'s body (130 stereo frames of pink noise with transients; the tests that need its
    2-frame halo take it from best_bias_lib.material()); 'white': 64 stereo frames of O.gen_white, seeds 1 and 2"""
    if kind == 'pink':
        return BB.material()[1]
    return [O.gen_white(s, WHITE_FRAMES * 512) for s in WHITE_SEEDS]


def weights(byte):
    """W per coefficient index for one mode byte, float64 [512]"""
    w = np.ones(512, dtype=np.float64)
    for b in range(3):
        if (byte >> (2 * b)) & 3:
            w[BANDS[b]] = SHORT_WEIGHT[b]
    return w


def model(chans, candidates=CANDIDATES, bias=BIAS):
    """-> {'units': [n][units, 212] per candidate, 'coefs': [n][units, 512], 'D', 'E': float64 [units, n]}"""
    nch = len(chans)
    frames = len(chans[0]) // 512
    D = np.zeros((frames * nch, len(candidates)), dtype=np.float64)
    E = np.zeros_like(D)
    per_cand, per_coefs = [], []
    for k, byte in enumerate(candidates):
        units = BM.oracle_encode_modes(chans, np.full((frames, nch), byte, dtype=np.uint8), bias)[0]
        coefs = BB.coefficients(chans, units)
        assert (BM.modes_of_units(units) == byte).all()
        c64, w = coefs.astype(np.float64), weights(byte)
        for u in range(frames * nch):
            D[u, k] = np.sum(w * (c64[u] - BB.dequantized(units[u]).astype(np.float64)) ** 2)
        E[:, k] = np.sum(w * c64 ** 2, axis=1)
        per_cand.append(units)
        per_coefs.append(coefs)
    return {'units': per_cand, 'coefs': per_coefs, 'D': D, 'E': E}


_cases = {}


def case(kind):
    """the model of 'pink' or 'white' under all eight candidates; computed once per process, shared, never written"""
    if kind not in _cases:
        m = model(material(kind))
        for a in m['units'] + m['coefs'] + [m['D'], m['E']]:
            a.setflags(write=False)
        _cases[kind] = m
    return _cases[kind]


def admissible(D):
    """bool [units, n]: the candidates whose model distortion is within CHOICE_REL of the unit's model minimum"""
    return D <= D.min(axis=1, keepdims=True) * (1.0 + CHOICE_REL)


unique_margin = BB.unique_margin


def chosen_units(kind, choice, candidates=CANDIDATES):
    """the oracle under the per-unit chosen bytes -> units [units, 212]"""
    chans = material(kind)
    modes = np.asarray(candidates, dtype=np.uint8)[np.asarray(choice)].reshape(-1, len(chans))
    return BM.oracle_encode_modes(chans, modes, BIAS)[0]


def check_outputs(kind, units, choice, modes_out, dist, energy, columns=None):
    """the GPU's five outputs on the shared material against the model (columns: the candidates of the call as indices into
    CANDIDATES, default all eight in order): None, or what is wrong"""
    m = case(kind)
    cols = list(range(len(CANDIDATES))) if columns is None else list(columns)
    cand = [CANDIDATES[k] for k in cols]
    D, E = m['D'][:, cols], m['E'][:, cols]
    if dist.shape != D.shape or energy.shape != E.shape:
        return 'shapes %r %r' % (dist.shape, energy.shape)
    for name, got, want in (('distortion', dist, D), ('energy', energy, E)):
        bad = ~(np.abs(got - want) <= REL * want)
        if bad.any():
            at = np.argwhere(bad)[0]
            return '%s at %r: %r against the model %r' % (name, at.tolist(), got[tuple(at)], want[tuple(at)])
        if ((want == 0) & (got != 0)).any():
            return '%s: an exact zero of the model is not zero' % name
    ok = admissible(D)
    if (ok.sum(axis=1) != 1).any():
        return 'the model leaves more than one admissible candidate for some unit'
    if (np.asarray(choice) >= len(cand)).any():
        return 'a choice is not below n_cand'
    if not ok[np.arange(len(choice)), choice].all():
        u = int(np.flatnonzero(~ok[np.arange(len(choice)), choice])[0])
        return 'unit %d: choice %d, model D %r' % (u, int(choice[u]), D[u].tolist())
    if not np.array_equal(modes_out, np.asarray(cand, dtype=np.uint8)[choice]):
        return 'modes_out is not cand_modes[choice]'
    want_units = chosen_units(kind, choice, cand)
    if not np.array_equal(units, want_units):
        return 'units differ from the oracle under the chosen bytes at %r' % np.flatnonzero((units != want_units).any(axis=1))[:4].tolist()
    return None
