"""The measured allocation with every BFU's scale-factor index chosen by the same error (c1_encode_measured_sf_*): the CPU model,
built on tests/measured_alloc_lib.py and the oracle alone.

e_k(b, w) comes from c1o_find_scale_factor, c1o_quantize_bfu and c1o_dequantize_bfu at findScaleFactor's index plus offset k,
summed in binary64 with j ascending; the table is the least e_k over the candidates whose index lies in 1 .. 63, the pick the
first candidate, in the order given, that attains it.  measured_alloc_lib.greedy runs over that table; the fallback compares
with the reference's record under the offset-0 table; a taken unit is packed with the chosen indices.  Besides the greedy
margins the model reports the candidate margin: the least relative gap between the best and the second-best candidate over the
table entries with e < e(b, 0)."""
import ctypes as C

import numpy as np

import best_bias_lib as BB
import measured_alloc_lib as MA
import oracle_lib as O
import pack_model_lib as PM

OFFSETS = (0, -1, 1, -2, -3)                     # the suggested set


def error_tables(slots, modes, offsets):
    """one unit: -> (ek float64 [K, 52, 16], valid bool [K, 52], s0 int [52]); an invalid candidate's row is +inf beyond w = 0"""
    lib = O.lib()
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int)
    x = np.ascontiguousarray(slots, dtype=np.float32)
    x64 = x.astype(np.float64)
    q = np.zeros(20, dtype=np.int32)
    d = np.zeros(20, dtype=np.float32)
    qp, dp = q.ctypes.data_as(ip), d.ctypes.data_as(fp)
    W = MA.weights_of_modes(modes)
    K = len(offsets)
    ek = np.zeros((K, 52, 16), dtype=np.float64)
    valid = np.zeros((K, 52), dtype=bool)
    s0 = np.zeros(52, dtype=np.int64)
    for b in range(52):
        first, n = int(PM.FIRST[b]), int(PM.SPECS[b])
        xp = C.cast(x.ctypes.data + 4 * first, fp)
        s = int(lib.c1o_find_scale_factor(xp, n))
        s0[b] = s
        xb = x64[first:first + n]
        e0 = W[b] * np.cumsum(xb * xb)[-1]
        ek[:, b, :] = e0
        if s == 0:
            continue
        for k, off in enumerate(offsets):
            sk = s + int(off)
            if not 1 <= sk <= 63:
                ek[k, b, 1:] = np.inf
                continue
            valid[k, b] = True
            for w in range(1, 16):
                lib.c1o_quantize_bfu(xp, n, sk, int(MA.BITS[w]), qp)
                lib.c1o_dequantize_bfu(qp, n, sk, int(MA.BITS[w]), dp)
                t = xb - d[:n].astype(np.float64)
                ek[k, b, w] = W[b] * np.cumsum(t * t)[-1]
    return ek, valid, s0


def least(ek, valid):
    """ek [..., K, 52, 16], valid [..., K, 52] -> (e [..., 52, 16], pick int [..., 52, 16]): a later candidate replaces an earlier
    one only when it is valid and its error is strictly smaller"""
    e = ek[..., 0, :, :].copy()
    pick = np.zeros(e.shape, dtype=np.int64)
    for k in range(1, ek.shape[-3]):
        better = valid[..., k, :, None] & (ek[..., k, :, :] < e)
        better[..., 0] = False
        e = np.where(better, ek[..., k, :, :], e)
        pick = np.where(better, k, pick)
    return e, pick


def candidate_margin(ek, valid, e):
    """-> (the least relative gap between the best and the second-best valid candidate over the entries with e < e(b, 0), the
    number of exact ties among them)"""
    K = ek.shape[-3]
    if K < 2:
        return np.inf, 0
    v = np.where(valid[..., :, :, None], ek, np.inf)             # [..., K, 52, 16]
    order = np.sort(np.moveaxis(v, -3, -1), axis=-1)             # [..., 52, 16, K]
    below = (e < e[..., :, 0:1]) & np.isfinite(order[..., 1])
    below[..., 0] = False
    if not below.any():
        return np.inf, 0
    best, second = order[..., 0][below], order[..., 1][below]
    return float(MA._rel(best, second).min()), int((best == second).sum())


def model(chans, ref_units, offsets=OFFSETS):
    """measured_alloc_lib.model's dict under the candidate offsets, and besides: 'sfi' [U, 52] (the indices a unit carries: the
    chosen ones below nBfu of a taken unit where wl > 0, findScaleFactor's elsewhere), 's0' [U, 52], 'shifts' int8 [U, 52],
    'cand_margin' (candidate_margin's gap) and 'ties' (its count)"""
    offsets = [int(v) for v in offsets]
    coefs = BB.coefficients(chans, ref_units)
    U = coefs.shape[0]
    K = len(offsets)
    EK = np.zeros((U, K, 52, 16), dtype=np.float64)
    valid = np.zeros((U, K, 52), dtype=bool)
    s0 = np.zeros((U, 52), dtype=np.int64)
    slots = np.zeros((U, 512), dtype=np.float32)
    fields = [O.unpack_unit(u) for u in ref_units]
    for u in range(U):
        slots[u] = MA.bfu_coefficients(coefs[u], fields[u].modes)
        EK[u], valid[u], s0[u] = error_tables(slots[u], fields[u].modes, offsets)
    E, pick = least(EK, valid)
    cand_margin, ties = candidate_margin(EK, valid, E)
    wl, T, margin = MA.greedy(E, s0)
    Tn = np.where(np.isnan(T), np.inf, T)
    star = Tn.argmin(axis=1)                                     # the first amount with the least T
    have = ~np.isnan(T).all(axis=1)
    ar = np.arange(U)
    t_star = T[ar, star]
    order = np.sort(Tn, axis=1)
    margin = np.minimum(margin, MA._rel(order[:, 0], order[:, 1]))
    wl_ref = np.zeros((U, 52), dtype=np.int64)
    for u in range(U):
        wl_ref[u, :fields[u].nbfu] = np.array(fields[u].wl[:fields[u].nbfu])
    t_ref = np.cumsum(EK[ar[:, None], 0, np.arange(52)[None, :], wl_ref], axis=1)[:, -1]      # the offset-0 table
    taken = have & (t_star < t_ref)
    margin = np.minimum(margin, MA._rel(np.minimum(t_star, t_ref), np.maximum(t_star, t_ref)))
    units = np.array(ref_units, dtype=np.uint8)
    nbfu = np.array([f.nbfu for f in fields], dtype=np.int64)
    wl_out = wl_ref.copy()
    sfi = s0.copy()
    shifts = np.zeros((U, 52), dtype=np.int8)
    off = np.asarray(offsets, dtype=np.int64)
    for u in np.flatnonzero(taken):
        nbfu[u] = MA.AMOUNTS[star[u]]
        wl_out[u] = wl[u, star[u]]
        coded = (np.arange(52) < nbfu[u]) & (wl_out[u] > 0)
        shifts[u] = np.where(coded, off[pick[u, np.arange(52), wl_out[u]]], 0)
        sfi[u] = s0[u] + shifts[u]
        units[u] = MA.pack_fields(nbfu[u], fields[u].modes, wl_out[u], sfi[u], slots[u])
    return {'units': units, 'taken': taken.astype(np.uint8), 'nbfu': nbfu, 'wl': wl_out, 'D': np.stack([t_ref, t_star], axis=1),
            'E': np.cumsum(E[:, :, 0], axis=1)[:, -1], 'margin': margin, 'coefs': coefs, 'ref': np.array(ref_units, dtype=np.uint8),
            'sfi': sfi, 's0': s0, 'shifts': shifts, 'cand_margin': np.float64(cand_margin), 'ties': np.int64(ties)}


_cases = {}


def case(kind, material='pink', offsets=OFFSETS, frames=None):
    """the model of measured_alloc_lib's shared material under `kind` (see measured_alloc_lib.reference_units) and the offsets,
    of its first `frames` frames when given (the encoder is causal: their units are those of the whole signal); computed once
    per process, shared, never written"""
    key = (kind, material, tuple(offsets), frames)
    if key not in _cases:
        import best_modes_lib as BMO
        chans, ref = BMO.material(material), MA.reference_units(kind, material)
        if frames is not None:
            chans, ref = [c[:frames * 512] for c in chans], ref[:frames * len(chans)]
        m = model(chans, ref, offsets)
        for a in m.values():
            a.setflags(write=False)
        _cases[key] = m
    return _cases[key]


def check_valid(units, coefs, taken, dist, offsets=OFFSETS, nch=2):
    """what makes `units` ordinary sound units of these coefficients under these offsets, from the bytes alone: None, or what is
    wrong"""
    lib = O.lib()
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int)
    q = np.zeros(20, dtype=np.int32)
    allowed = set(int(v) for v in offsets)
    for u in range(units.shape[0]):
        f = O.unpack_unit(units[u])
        if f.nbfu not in MA.AMOUNTS.tolist():
            return 'unit %d: nBfu %d' % (u, f.nbfu)
        wl = np.array(f.wl[:f.nbfu])
        used = int(np.sum(MA.BITS[wl] * MA.SIZES[:f.nbfu]))
        if used > 1696 - 40 - 10 * f.nbfu:
            return 'unit %d: %d mantissa bits with %d BFUs' % (u, used, f.nbfu)
        slots = MA.bfu_coefficients(coefs[u], f.modes)
        for b in range(f.nbfu):
            first, n = int(PM.FIRST[b]), int(PM.SPECS[b])
            xp = C.cast(slots.ctypes.data + 4 * first, fp)
            s0 = int(lib.c1o_find_scale_factor(xp, n))
            if f.wl[b] == 0 or s0 == 0:
                if f.sfi[b] != s0:
                    return 'unit %d, BFU %d: scale-factor index %d where nothing is coded, findScaleFactor gives %d' % (u, b, f.sfi[b], s0)
            elif f.sfi[b] - s0 not in allowed or not 1 <= f.sfi[b] <= 63:
                return 'unit %d, BFU %d: scale-factor index %d, findScaleFactor gives %d' % (u, b, f.sfi[b], s0)
            want = np.zeros(n, dtype=np.int32)
            if f.wl[b] != 0:
                lib.c1o_quantize_bfu(xp, n, int(f.sfi[b]), int(MA.BITS[f.wl[b]]), q.ctypes.data_as(ip))
                want = q[:n]
            if not np.array_equal(np.array(f.q[first:first + n]), want):
                return 'unit %d, BFU %d: mantissas' % (u, b)
        again = np.zeros(212, dtype=np.uint8)
        lib.c1o_pack_unit(C.byref(f), again.ctypes.data_as(C.POINTER(C.c_uint8)))
        if not np.array_equal(again, units[u]):
            return 'unit %d: packing its fields again gives other bytes' % u
        want = float(dist[u, 1 if taken[u] else 0])
        got = MA.weighted_error(units[u], coefs[u])
        if not abs(got - want) <= MA.REL * want:
            return 'unit %d: its weighted error %r against the reported %r' % (u, got, want)
    pcm, _ = O.decode_stream(units, nch)
    if not all(np.isfinite(p).all() for p in pcm):
        return 'the decoded stream is not finite'
    return None


def check_outputs(m, units, taken, shifts, dist, energy):
    """the GPU's outputs against the model `m` of the same input: None, or what is wrong"""
    bad = MA.check_outputs(m, units, taken, dist, energy)
    if bad is not None:
        return bad
    if shifts.shape != m['shifts'].shape or not np.array_equal(shifts, m['shifts']):
        return 'shifts differ from the model'
    for u in range(units.shape[0]):
        f = O.unpack_unit(units[u])
        if taken[u] and not np.array_equal(np.array(f.sfi[:f.nbfu]), m['sfi'][u, :f.nbfu]):
            return 'unit %d: scale-factor indices %r, the model %r' % (u, list(f.sfi[:f.nbfu]), m['sfi'][u, :f.nbfu].tolist())
    return None


def gain_db(m):
    return MA.gain_db(m)
