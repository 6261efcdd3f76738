"""The measured block-mode search under one masking threshold per unit (c1_encode_measured_modes_masked_*): the CPU model, on
top of tests/masked_alloc_lib.py, tests/scale_factor_choice_lib.py, tests/measured_alloc_lib.py and tests/measured_modes_lib.py,
none of which it changes.

Per candidate byte k masked_alloc_lib.unit_tables(byte, material, offsets) (or tables_of for any other material) gives the
unweighted e_k(b, w) of every unit under that constant byte, the composed scale-factor indices and the reference's record.  The
weights are ONE row per unit, whatever the candidate: P = masked_alloc_lib.weights over byte 0's level-0 errors
(EK[:, 0, :, 0] of the all-long tables: sum_j x[j]^2 with W = 1).  On P * EK run scale_factor_choice_lib.least,
measured_alloc_lib.greedy, the fallback against the reference's record under the weighted offset-0 table and the packing with the
chosen indices, statement by statement as masked_alloc_lib.model_of runs them under a unit's own weights.  The candidates are then
composed by measured_modes_lib.compose and judged by measured_modes_lib.check_case: T_final = taken ? T(n*) : T_ref, the first
candidate of least T_final wins, and every output of the winner is that candidate's model's."""
import numpy as np

import best_modes_lib as BMO
import block_modes_lib as BM
import masked_alloc_lib as MK
import measured_alloc_lib as MA
import measured_modes_lib as MM
import scale_factor_choice_lib as SF

CANDIDATES = MM.CANDIDATES                       # [0, 48, 8, 56, 2, 50, 10, 58]
PINK_SF_CANDIDATES = MM.PINK_SF_CANDIDATES       # the pink five-offset model costs several seconds a candidate
OFFSETS = MM.OFFSETS
REL = MM.REL
UNIQUE_REL = MM.UNIQUE_REL


def shared_weights(t0, floor, spread):
    """t0: the tables under byte 0 -> (P float64 [U, 52], at_floor bool [U, 52]); what masked_alloc_lib.model_of reports as 'P'
    for the same units under constant modes 0"""
    return MK.weights(t0['EK'][:, 0, :, 0], floor, spread)


def model_under(t, P):
    """masked_alloc_lib.model_of's decision over the units behind `t` with the weights given instead of the units' own -> the
    per-candidate dict measured_modes_lib.compose reads ('D', 'E', 'taken', 'shifts', 'units', 'coefs') and 'margin'"""
    EK0, valid, s0 = t['EK'], t['valid'], t['s0']
    U = EK0.shape[0]
    EK = P[:, None, :, None] * EK0                                   # the multiply on the finished e_k(b, w)
    E, pick = SF.least(EK, valid)
    wl, T, margin = MA.greedy(E, s0)
    Tn = np.where(np.isnan(T), np.inf, T)
    star = Tn.argmin(axis=1)                                         # the first amount with the least T
    have = ~np.isnan(T).all(axis=1)
    ar, bs = np.arange(U), np.arange(52)
    t_star = T[ar, star]
    order = np.sort(Tn, axis=1)
    margin = np.minimum(margin, MA._rel(order[:, 0], order[:, 1]))
    wl_ref = t['wl_ref']
    t_ref = np.cumsum(EK[ar[:, None], 0, bs[None, :], wl_ref], axis=1)[:, -1]
    taken = have & (t_star < t_ref)
    margin = np.minimum(margin, MA._rel(np.minimum(t_star, t_ref), np.maximum(t_star, t_ref)))
    units = np.array(t['ref'], dtype=np.uint8)
    shifts = np.zeros((U, 52), dtype=np.int8)
    off = t['offsets']
    for u in np.flatnonzero(taken):
        nbfu = MA.AMOUNTS[star[u]]
        wl_out = wl[u, star[u]]
        coded = (bs < nbfu) & (wl_out > 0)
        shifts[u] = np.where(coded, off[np.where(coded, pick[u, bs, wl_out], 0)], 0)
        units[u] = MA.pack_fields(nbfu, t['modes'][u], wl_out, s0[u] + shifts[u], t['slots'][u])
    return {'units': units, 'taken': taken.astype(np.uint8), 'D': np.stack([t_ref, t_star], axis=1),
            'E': np.cumsum(E[:, :, 0], axis=1)[:, -1], 'margin': margin, 'coefs': np.array(t['coefs']), 'shifts': shifts}


def compose(cand, tables, floor, spread, t0=None):
    """the joint model of the candidate bytes `cand` from their unweighted tables (one per candidate, in order) and the tables
    under byte 0 (t0; taken from `tables` where 0 is a candidate) -> measured_modes_lib.case's dict, and besides 'P' [U, 52],
    'at_floor' bool [U, 52] and 'margin' [U, n] (the least relative margin of any decision inside a candidate's model)"""
    cand = [int(b) for b in cand]
    if t0 is None:
        t0 = tables[cand.index(0)]
    with np.errstate(all='ignore'):
        P, at_floor = shared_weights(t0, floor, spread)
        per = [model_under(t, P) for t in tables]
        m = dict(MM.compose(cand, per, True))
    m['P'], m['at_floor'], m['margin'] = P, at_floor, np.stack([p['margin'] for p in per], axis=1)
    for a in m.values():
        a.setflags(write=False)
    return m


_cases = {}


def case(material, tables='packaged', offsets=OFFSETS, candidates=None, frames=None):
    """the model of the shared material ('pink': best_bias_lib.material()'s body, 'white': best_modes_lib's; `frames`: their first
    frames only) under the named tables of masked_alloc_lib.named; computed once per process, shared, never written"""
    cand = list(CANDIDATES if candidates is None else candidates)
    key = (material, tables, tuple(offsets), tuple(cand), frames)
    if key not in _cases:
        floor, spread = MK.named(tables)
        _cases[key] = compose(cand, [MK.unit_tables(b, material, offsets, frames) for b in cand], floor, spread,
                              MK.unit_tables(0, material, offsets, frames))
    return _cases[key]


def case_of(chans, floor, spread, offsets=OFFSETS, candidates=CANDIDATES):
    """the same for any other material (states from zero); computed here, not cached"""
    frames, nch = len(chans[0]) // 512, len(chans)
    with np.errstate(all='ignore'):
        tab = {b: MK.tables_of(chans, BM.oracle_encode_modes(chans, np.full((frames, nch), b, dtype=np.uint8), BMO.BIAS)[0], offsets)
               for b in sorted(set([0] + [int(b) for b in candidates]))}
    return compose(candidates, [tab[int(b)] for b in candidates], floor, spread, tab[0])


def own_thresholds(byte, material='pink', tables='packaged', offsets=(0,)):
    """the thresholds c1_encode_measured_masked_* forms for every unit under the constant byte, from that byte's own spectrum ->
    float64 [U, 52]"""
    floor, spread = MK.named(tables)
    return 1.0 / MK.weights(MK.unit_tables(byte, material, offsets)['EK'][:, 0, :, 0], floor, spread)[0]


def weighted_total(units, coefs, P):
    """the aggregate error of the units, judged from their bytes under the weights P"""
    return float(MK.weighted_errors(units, coefs, P).sum())


def detector_baseline(material, tables, offsets):
    """what a masking caller has without the search: the masked allocation under the detector's modes, under its own weights ->
    (units, coefs)"""
    m = MK.case('detect', material, tables, offsets)
    return m['units'], m['coefs']


def two_call_composition(material, tables, offsets, cand):
    """the composition that needs no new call: the unweighted search for modes_out (measured_modes_lib), then the masked allocation
    under those modes with each unit's own-mode weights -> (units, coefs, modes)"""
    sf = tuple(offsets) != (0,)
    unweighted = MM.case(material, sf, list(cand))
    per = {int(b): MK.case(int(b), material, tables, offsets) for b in set(unweighted['modes'].tolist())}
    units = np.stack([per[int(b)]['units'][u] for u, b in enumerate(unweighted['modes'])])
    coefs = np.stack([per[int(b)]['coefs'][u] for u, b in enumerate(unweighted['modes'])])
    return units, coefs, unweighted['modes']


def gain_db(worse, better):
    return 10.0 * np.log10(worse / better)


def check_outputs(m, out):
    """the GPU's outputs (dict: units, choice, modes, taken, shifts, distortion [U, n, 2], energy [U, n], weights [U, 52]) against
    the model `m`: None, or what is wrong"""
    bad = MM.check_case(m, out)
    if bad is not None:
        return bad
    w = out['weights']
    if w.shape != m['P'].shape or not (np.abs(w - m['P']) <= REL * m['P']).all():
        return 'weights differ from the model'
    return None
