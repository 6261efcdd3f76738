"""The measured allocation with every BFU's error divided by a masking threshold (c1_encode_measured_masked_*): the CPU model, on
top of tests/scale_factor_choice_lib.py and tests/measured_alloc_lib.py, neither of which it changes.

scale_factor_choice_lib.error_tables gives e_k(b, w) of a unit.  The weights follow include/carta1_hip.h in numpy, in its order:
E_c = e(c, 0); M_b = sum_c spread[b][c] * E_c with c ascending, each product rounded and then added to a sum that starts at
+0.0; thr_b = M_b > floor[b] ? M_b : floor[b]; P_b = 1 / thr_b; e'_k(b, w) = P_b * e_k(b, w).  scale_factor_choice_lib.least,
measured_alloc_lib.greedy, the fallback against the reference's record under the weighted offset-0 table and the packing with the
chosen indices then run on e'.  The model reports the decision and candidate margins as its parents do, and besides, per unit,
the weighted error of any other decision (word lengths, candidates) under its own weights, so that two allocations can be judged
under the same P."""
import numpy as np

import best_bias_lib as BB
import best_modes_lib as BMO
import block_modes_lib as BM
import measured_alloc_lib as MA
import oracle_lib as O
import pack_model_lib as PM
import scale_factor_choice_lib as SF

OFFSETS = SF.OFFSETS
FLAT = (np.ones(52), None)


def packaged():
    """the package's tables (carta1_amd/masking_default.json) -> (floor [52], spread [52, 52])"""
    import carta1_amd as c1
    return c1.MASKING_DEFAULT[0], c1.MASKING_DEFAULT[1]


def explicit(name):
    """the explicit tables of the tests: 'specs' (floor = SPECS_PER_BFU), 'ramp' (floor[b] = 10^(b / 13 - 2)), both without a
    spread, and 'self' (floor 1e-12, spread = identity: pure self-masking)"""
    if name == 'specs':
        return MA.SIZES.astype(np.float64), None
    if name == 'ramp':
        return 10.0 ** (np.arange(52) / 13.0 - 2.0), None
    if name == 'self':
        return np.full(52, 1e-12), np.eye(52)
    raise KeyError(name)


def weights(E0, floor, spread):
    """E0 float64 [U, 52] (e(c, 0)) -> (P float64 [U, 52], at_floor bool [U, 52])"""
    floor = np.asarray(floor, dtype=np.float64)
    M = np.zeros(E0.shape, dtype=np.float64)
    if spread is not None:
        spread = np.asarray(spread, dtype=np.float64).reshape(52, 52)
        for c in range(52):
            prod = spread[None, :, c] * E0[:, c:c + 1]               # rounded ...
            M = M + prod                                             # ... then added
    above = M > floor[None, :]                                       # a NaN M_b falls to the floor
    thr = np.where(above, M, floor[None, :])
    return 1.0 / thr, ~above


_tables = {}


def unit_tables(kind, material='pink', offsets=OFFSETS, frames=None):
    """the unweighted e_k of the shared material's units, computed once per process and shared by every table set -> dict"""
    key = (kind, material, tuple(offsets), frames)
    if key not in _tables:
        chans, ref = BMO.material(material), MA.reference_units(kind, material)
        if frames is not None:
            chans, ref = [c[:frames * 512] for c in chans], ref[:frames * len(chans)]
        _tables[key] = tables_of(chans, ref, offsets)
    return _tables[key]


def tables_of(chans, ref_units, offsets):
    offsets = [int(v) for v in offsets]
    coefs = BB.coefficients(chans, ref_units)
    U, K = coefs.shape[0], len(offsets)
    t = {'EK': np.zeros((U, K, 52, 16)), 'valid': np.zeros((U, K, 52), dtype=bool), 's0': np.zeros((U, 52), dtype=np.int64),
         'slots': np.zeros((U, 512), dtype=np.float32), 'coefs': coefs, 'ref': np.array(ref_units, dtype=np.uint8),
         'offsets': np.asarray(offsets, dtype=np.int64)}
    fields = [O.unpack_unit(u) for u in ref_units]
    t['modes'] = np.array([[f.modes[0], f.modes[1], f.modes[2]] for f in fields], dtype=np.int64).reshape(U, 3)
    t['nbfu_ref'] = np.array([f.nbfu for f in fields], dtype=np.int64)
    t['wl_ref'] = np.zeros((U, 52), dtype=np.int64)
    for u in range(U):
        t['slots'][u] = MA.bfu_coefficients(coefs[u], fields[u].modes)
        t['EK'][u], t['valid'][u], t['s0'][u] = SF.error_tables(t['slots'][u], fields[u].modes, offsets)
        t['wl_ref'][u, :fields[u].nbfu] = np.array(fields[u].wl[:fields[u].nbfu])
    for a in t.values():
        a.setflags(write=False)
    return t


def model_of(t, floor, spread):
    """the model of the units behind `t` (tables_of) under the tables -> scale_factor_choice_lib.model's dict on the weighted
    errors, and besides 'P' [U, 52] (the weights), 'at_floor' bool [U, 52], 'cand' int [U, 52] (the candidate whose index each BFU
    carries in the final unit; 0 where none), 'wl_final' [U, 52] (the final word lengths, 0 at and above nBfu) and 'D_plain'
    [U] (the final unit's unweighted error, what its bytes alone show)"""
    EK0, valid, s0 = t['EK'], t['valid'], t['s0']
    U = EK0.shape[0]
    P, at_floor = weights(EK0[:, 0, :, 0], floor, spread)
    EK = P[:, None, :, None] * EK0                                   # the multiply on the finished e_k(b, w)
    E, pick = SF.least(EK, valid)
    cand_margin, ties = SF.candidate_margin(EK, valid, E)
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
    nbfu = np.array(t['nbfu_ref'])
    wl_out = wl_ref.copy()
    sfi = s0.copy()
    shifts = np.zeros((U, 52), dtype=np.int8)
    cand = np.zeros((U, 52), dtype=np.int64)
    off = t['offsets']
    for u in np.flatnonzero(taken):
        nbfu[u] = MA.AMOUNTS[star[u]]
        wl_out[u] = wl[u, star[u]]
        coded = (bs < nbfu[u]) & (wl_out[u] > 0)
        cand[u] = np.where(coded, pick[u, bs, wl_out[u]], 0)
        shifts[u] = np.where(coded, off[cand[u]], 0)
        sfi[u] = s0[u] + shifts[u]
        units[u] = MA.pack_fields(nbfu[u], t['modes'][u], wl_out[u], sfi[u], t['slots'][u])
    wl_final = np.where(bs[None, :] < nbfu[:, None], wl_out, 0)
    m = {'units': units, 'taken': taken.astype(np.uint8), 'nbfu': nbfu, 'wl': wl_out, 'D': np.stack([t_ref, t_star], axis=1),
         'E': np.cumsum(E[:, :, 0], axis=1)[:, -1], 'margin': margin, 'coefs': t['coefs'], 'ref': t['ref'], 'sfi': sfi, 's0': s0,
         'shifts': shifts, 'cand_margin': np.float64(cand_margin), 'ties': np.int64(ties), 'P': P, 'at_floor': at_floor,
         'cand': cand, 'wl_final': wl_final}
    m['D_plain'] = error_under(t, np.ones((U, 52)), m)
    for a in m.values():
        a.setflags(write=False)
    return m


def error_under(t, P, m):
    """the error of the final units of model `m` (any model_of over the same `t`) weighted with P [U, 52] -> float64 [U]"""
    U = P.shape[0]
    e = t['EK'][np.arange(U)[:, None], m['cand'], np.arange(52)[None, :], m['wl_final']]
    return np.cumsum(P * e, axis=1)[:, -1]


_cases = {}


def case(kind, material='pink', tables='packaged', offsets=OFFSETS, frames=None):
    """the model of the shared material under `kind` (measured_alloc_lib.reference_units), the offsets and the named tables
    ('packaged', 'flat', 'specs', 'ramp', 'self', or one of them + '*4': both tables times 4.0); computed once per process, shared,
    never written"""
    key = (kind, material, tables, tuple(offsets), frames)
    if key not in _cases:
        _cases[key] = model_of(unit_tables(kind, material, offsets, frames), *named(tables))
    return _cases[key]


def named(tables):
    if tables.endswith('*4'):
        floor, spread = named(tables[:-2])
        return floor * 4.0, None if spread is None else spread * 4.0
    if tables == 'packaged':
        return packaged()
    if tables == 'flat':
        return FLAT
    return explicit(tables)


def gain_db(m):
    return MA.gain_db(m)


def gain_over_db(t, m, other):
    """how far the weighted error of m's units lies below that of other's units (a model over the same `t` under other tables,
    e.g. flat ones: 6j's units), both judged under m's weights, in dB"""
    return 10.0 * np.log10(error_under(t, m['P'], other).sum() / error_under(t, m['P'], m).sum())


def weight_per_coefficient(P, modes):
    """P [52] laid over the 512 coefficients of a unit with these block modes"""
    out = np.zeros(512, dtype=np.float64)
    for b in range(52):
        n = int(PM.SPECS[b])
        st = int((PM.START_LONG if modes[int(PM.BAND_OF_BFU[b])] == 0 else PM.START_SHORT)[b])
        out[st:st + n] = P[b]
    return out


def weighted_errors(units, coefs, weights_):
    """the error of every unit, from its bytes, with BFU b's terms multiplied by W_b and weights_[u, b] -> float64 [U]"""
    out = np.zeros(units.shape[0], dtype=np.float64)
    for u in range(units.shape[0]):
        f = O.unpack_unit(units[u])
        w = BMO.weights(BM.byte_of(tuple(f.modes))) * weight_per_coefficient(weights_[u], f.modes)
        d = coefs[u].astype(np.float64) - BB.dequantized(units[u]).astype(np.float64)
        out[u] = np.sum(w * d * d)
    return out


def check_valid(units, coefs, taken, dist, weights_, offsets=OFFSETS, nch=2):
    """scale_factor_choice_lib.check_valid -- the bytes do not reveal the weights, so what makes them ordinary sound units of
    these coefficients under these offsets is unchanged -- and then the reported weighted error against the one the bytes give
    under `weights_` [U, 52]: None, or what is wrong"""
    plain = np.array([MA.weighted_error(units[u], coefs[u]) for u in range(units.shape[0])])
    bad = SF.check_valid(units, coefs, taken, np.stack([plain, plain], axis=1), offsets, nch)
    if bad is not None:
        return bad
    got = weighted_errors(units, coefs, weights_)
    want = np.where(np.asarray(taken) != 0, dist[:, 1], dist[:, 0])
    wrong = np.flatnonzero(~(np.abs(got - want) <= MA.REL * want))   # three roundings per term now: still far inside REL
    if wrong.size:
        return 'unit %d: its weighted error %r against the reported %r' % (wrong[0], got[wrong[0]], want[wrong[0]])
    return None


def check_outputs(m, units, taken, shifts, dist, energy, weights_):
    """the GPU's outputs against the model `m` of the same input: None, or what is wrong"""
    bad = SF.check_outputs(m, units, taken, shifts, dist, energy)
    if bad is not None:
        return bad
    if weights_.shape != m['P'].shape or not (np.abs(weights_ - m['P']) <= MA.REL * m['P']).all():
        return 'weights differ from the model'
    return None


def bitwise(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))
