"""The word lengths of every sound unit allocated by the measured coding error (c1_encode_measured_*): the CPU model, built from
the oracle alone, and the material the CPU and GPU tests share.

The reference's units come from block_modes_lib.oracle_encode_modes (given modes) or oracle_lib.encode_stream (detection, fixed
modes), the coefficients from best_bias_lib.coefficients under the modes those units record.  e(b, w) comes from
c1o_find_scale_factor, c1o_quantize_bfu and c1o_dequantize_bfu, summed in binary64 with j ascending (cumsum); the greedy
allocation, the totals in BFU order and the fallback are those of include/carta1_hip.h, run over all units and all eight
amounts at once in numpy.  The model also reports, per unit, the smallest relative margin of any decision it took: the top gain
against the runner-up at every greedy step, the least T against the next, and T(n*) against T_ref."""
import ctypes as C

import numpy as np

import best_bias_lib as BB
import best_modes_lib as BMO
import block_modes_lib as BM
import oracle_lib as O
import pack_model_lib as PM

AMOUNTS = np.array([20, 28, 32, 36, 40, 44, 48, 52])
BITS = np.array([0] + list(range(2, 17)))        # WORD_LENGTH_BITS
SIZES = np.asarray(PM.SPECS, dtype=np.int64)[:52]
MAX_STEPS = 52 * 15
REL = 1e-12                                      # |got - model| <= REL * model: two roundings per term and at most 511 * 2^-53 = 6e-14
                                                 # for a sum of at most 512 non-negative terms in any order (the best-bias tests' bound)
MARGIN = 1e-9                                    # the material: every decision of the model is decided by more than this
FIXED = [2, 0, 3]
CONSTANT = {'pink': (0, 10, 58), 'white': (0, 58)}


def weights_of_modes(modes):
    """W per BFU for one unit's three block modes, float64 [52]"""
    w = np.ones(52, dtype=np.float64)
    for b in range(52):
        band = int(PM.BAND_OF_BFU[b])
        if modes[band] != 0:
            w[b] = BMO.SHORT_WEIGHT[band]
    return w


def bfu_coefficients(coefs, modes):
    """the coefficients of one unit in BFU-major slot order, float32 [512]"""
    out = np.zeros(512, dtype=np.float32)
    for b in range(52):
        n = int(PM.SPECS[b])
        st = int((PM.START_LONG if modes[int(PM.BAND_OF_BFU[b])] == 0 else PM.START_SHORT)[b])
        out[int(PM.FIRST[b]):int(PM.FIRST[b]) + n] = coefs[st:st + n]
    return out


def error_table(slots, modes):
    """one unit: -> (e float64 [52, 16], sfi int [52]) from its coefficients in slot order and its block modes"""
    lib = O.lib()
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int)
    x = np.ascontiguousarray(slots, dtype=np.float32)
    x64 = x.astype(np.float64)
    q = np.zeros(20, dtype=np.int32)
    d = np.zeros(20, dtype=np.float32)
    qp, dp = q.ctypes.data_as(ip), d.ctypes.data_as(fp)
    W = weights_of_modes(modes)
    e = np.zeros((52, 16), dtype=np.float64)
    sfi = np.zeros(52, dtype=np.int64)
    for b in range(52):
        first, n = int(PM.FIRST[b]), int(PM.SPECS[b])
        xp = C.cast(x.ctypes.data + 4 * first, fp)
        s = int(lib.c1o_find_scale_factor(xp, n))
        sfi[b] = s
        xb = x64[first:first + n]
        e0 = W[b] * np.cumsum(xb * xb)[-1]
        e[b, :] = e0
        if s == 0:
            continue
        for w in range(1, 16):
            lib.c1o_quantize_bfu(xp, n, s, int(BITS[w]), qp)
            lib.c1o_dequantize_bfu(qp, n, s, int(BITS[w]), dp)
            t = xb - d[:n].astype(np.float64)
            e[b, w] = W[b] * np.cumsum(t * t)[-1]
    return e, sfi


def _rel(a, b):
    """(b - a) / a for b >= a >= 0; inf where a is 0 or either is not finite"""
    with np.errstate(divide='ignore', invalid='ignore'):
        r = (b - a) / a
    return np.where(np.isfinite(r) & (a > 0), r, np.inf)


def greedy(E, sfi):
    """E float64 [U, 52, 16], sfi [U, 52] -> (wl int [U, 8, 52], T float64 [U, 8], margin float64 [U]): the greedy allocation of
    every unit for every amount, all at once; margin = the least relative gap between the top gain and the runner-up"""
    U = E.shape[0]
    wl = np.zeros((U, 8, 52), dtype=np.int64)
    rem = np.broadcast_to((1696 - 40 - 10 * AMOUNTS)[None, :], (U, 8)).copy()
    active = (np.arange(52)[None, None, :] < AMOUNTS[None, :, None]) & (sfi[:, None, :] != 0)
    e_cur = np.broadcast_to(E[:, None, :, 0], (U, 8, 52)).copy()
    e_next = np.broadcast_to(E[:, None, :, 1], (U, 8, 52)).copy()
    cost = np.broadcast_to((2 * SIZES)[None, None, :], (U, 8, 52)).copy()
    with np.errstate(divide='ignore', invalid='ignore'):
        gain = (e_cur - e_next) / cost
    margin = np.full((U, 8), np.inf)
    ui, ai = np.meshgrid(np.arange(U), np.arange(8), indexing='ij')
    for _ in range(MAX_STEPS):
        elig = active & (wl < 15) & (cost <= rem[:, :, None]) & (gain > 0)
        G = np.where(elig, gain, -np.inf)
        win = G.argmax(axis=2)                                   # the first index of the maximum: the smallest BFU on a tie
        top = G[ui, ai, win]
        go = top > -np.inf
        if not go.any():
            break
        G[ui, ai, win] = -np.inf
        second = G.max(axis=2)
        margin = np.minimum(margin, np.where(go & (second > -np.inf), _rel(np.where(go, second, 1.0), np.where(go, top, 1.0)), np.inf))
        u, a, b = ui[go], ai[go], win[go]
        rem[u, a] -= cost[u, a, b]
        wl[u, a, b] += 1
        w = wl[u, a, b]
        e_cur[u, a, b] = e_next[u, a, b]
        e_next[u, a, b] = E[u, b, np.minimum(w + 1, 15)]
        cost[u, a, b] = SIZES[b]
        with np.errstate(divide='ignore', invalid='ignore'):
            gain[u, a, b] = (e_cur[u, a, b] - e_next[u, a, b]) / cost[u, a, b]
    T = np.cumsum(e_cur, axis=2)[:, :, -1]                       # BFUs at or above the amount never moved: e(b, 0)
    return wl, T, margin.min(axis=1)


def pack_fields(nbfu, modes, wl, sfi, slots):
    """the sound unit of these fields, its mantissas from c1o_quantize_bfu at the word lengths -> uint8 [212]"""
    lib = O.lib()
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int)
    f = O.Fields()
    f.nbfu = int(nbfu)
    x = np.ascontiguousarray(slots, dtype=np.float32)
    q = np.zeros(20, dtype=np.int32)
    for k in range(3):
        f.modes[k] = int(modes[k])
    for b in range(int(nbfu)):
        f.wl[b] = int(wl[b])
        f.sfi[b] = int(sfi[b])
        if wl[b] == 0:
            continue
        first, n = int(PM.FIRST[b]), int(PM.SPECS[b])
        lib.c1o_quantize_bfu(C.cast(x.ctypes.data + 4 * first, fp), n, int(sfi[b]), int(BITS[wl[b]]), q.ctypes.data_as(ip))
        for j in range(n):
            f.q[first + j] = int(q[j])
    unit = np.zeros(212, dtype=np.uint8)
    lib.c1o_pack_unit(C.byref(f), unit.ctypes.data_as(C.POINTER(C.c_uint8)))
    return unit


def model(chans, ref_units):
    """chans: the PCM the reference's units `ref_units` [frames * nch, 212] were encoded from (states from zero) -> dict:
    'units' [U, 212], 'taken' uint8 [U], 'nbfu' [U], 'wl' [U, 52] (the packed record's), 'D' float64 [U, 2] (T_ref, T(n*)),
    'E' float64 [U], 'margin' float64 [U], 'coefs' float32 [U, 512], 'ref' = ref_units"""
    coefs = BB.coefficients(chans, ref_units)
    U = coefs.shape[0]
    E = np.zeros((U, 52, 16), dtype=np.float64)
    sfi = np.zeros((U, 52), dtype=np.int64)
    slots = np.zeros((U, 512), dtype=np.float32)
    fields = [O.unpack_unit(u) for u in ref_units]
    for u in range(U):
        slots[u] = bfu_coefficients(coefs[u], fields[u].modes)
        E[u], sfi[u] = error_table(slots[u], fields[u].modes)
    wl, T, margin = greedy(E, sfi)
    Tn = np.where(np.isnan(T), np.inf, T)
    star = Tn.argmin(axis=1)                                     # the first amount with the least T
    have = ~np.isnan(T).all(axis=1)
    ar = np.arange(U)
    t_star = T[ar, star]
    order = np.sort(Tn, axis=1)
    margin = np.minimum(margin, _rel(order[:, 0], order[:, 1]))
    wl_ref = np.zeros((U, 52), dtype=np.int64)
    for u in range(U):
        wl_ref[u, :fields[u].nbfu] = np.array(fields[u].wl[:fields[u].nbfu])
    t_ref = np.cumsum(E[ar[:, None], np.arange(52)[None, :], wl_ref], axis=1)[:, -1]
    taken = have & (t_star < t_ref)
    margin = np.minimum(margin, _rel(np.minimum(t_star, t_ref), np.maximum(t_star, t_ref)))
    units = np.array(ref_units, dtype=np.uint8)
    nbfu = np.array([f.nbfu for f in fields], dtype=np.int64)
    wl_out = wl_ref.copy()
    for u in np.flatnonzero(taken):
        nbfu[u] = AMOUNTS[star[u]]
        wl_out[u] = wl[u, star[u]]
        units[u] = pack_fields(nbfu[u], fields[u].modes, wl_out[u], sfi[u], slots[u])
    return {'units': units, 'taken': taken.astype(np.uint8), 'nbfu': nbfu, 'wl': wl_out, 'D': np.stack([t_ref, t_star], axis=1),
            'E': np.cumsum(E[:, :, 0], axis=1)[:, -1], 'margin': margin, 'coefs': coefs, 'ref': np.array(ref_units, dtype=np.uint8)}


def reference_units(kind, material):
    """the reference's units of the shared material: kind = a constant mode byte, 'modes' (best_bias_lib.given_modes),
    'detect' or 'fixed' ([2, 0, 3]); bias 1"""
    chans = BMO.material(material)
    frames = len(chans[0]) // 512
    if kind == 'detect':
        return O.encode_stream(chans)[0]
    if kind == 'fixed':
        return O.encode_stream(chans, fixed_modes=FIXED)[0]
    modes = BB.given_modes() if kind == 'modes' else np.full((frames, len(chans)), kind, dtype=np.uint8)
    return BM.oracle_encode_modes(chans, modes, 1.0)[0]


_cases = {}


def case(kind, material='pink'):
    """the model of 'pink' (best_bias_lib.material()'s body, 130 stereo frames) or 'white' (best_modes_lib's, 64 stereo frames)
    under `kind` (see reference_units); computed once per process, shared, never written"""
    key = (kind, material)
    if key not in _cases:
        m = model(BMO.material(material), reference_units(kind, material))
        for a in m.values():
            a.setflags(write=False)
        _cases[key] = m
    return _cases[key]


def gain_db(m):
    """the aggregate gain of T_final against T_ref over all units, in dB"""
    final = np.where(m['taken'] != 0, m['D'][:, 1], m['D'][:, 0])
    return 10.0 * np.log10(m['D'][:, 0].sum() / final.sum())


def weighted_error(unit, coefs):
    """the W-weighted squared error between the coefficients and what the decoder dequantizes from `unit`, binary64"""
    f = O.unpack_unit(unit)
    w = BMO.weights(BM.byte_of(tuple(f.modes)))
    t = coefs.astype(np.float64) - BB.dequantized(unit).astype(np.float64)
    return float(np.sum(w * t * t))


def check_valid(units, coefs, taken, dist, nch=2):
    """what makes `units` ordinary sound units of these coefficients, from the bytes alone: None, or what is wrong"""
    lib = O.lib()
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int)
    q = np.zeros(20, dtype=np.int32)
    for u in range(units.shape[0]):
        f = O.unpack_unit(units[u])
        if f.nbfu not in AMOUNTS.tolist():
            return 'unit %d: nBfu %d' % (u, f.nbfu)
        wl = np.array(f.wl[:f.nbfu])
        used = int(np.sum(BITS[wl] * SIZES[:f.nbfu]))
        if used > 1696 - 40 - 10 * f.nbfu:
            return 'unit %d: %d mantissa bits with %d BFUs' % (u, used, f.nbfu)
        slots = bfu_coefficients(coefs[u], f.modes)
        for b in range(f.nbfu):
            first, n = int(PM.FIRST[b]), int(PM.SPECS[b])
            xp = C.cast(slots.ctypes.data + 4 * first, fp)
            if f.sfi[b] != lib.c1o_find_scale_factor(xp, n):
                return 'unit %d, BFU %d: scale-factor index %d' % (u, b, f.sfi[b])
            want = np.zeros(n, dtype=np.int32)
            if f.wl[b] != 0:
                lib.c1o_quantize_bfu(xp, n, int(f.sfi[b]), int(BITS[f.wl[b]]), q.ctypes.data_as(ip))
                want = q[:n]
            if not np.array_equal(np.array(f.q[first:first + n]), want):
                return 'unit %d, BFU %d: mantissas' % (u, b)
        again = np.zeros(212, dtype=np.uint8)
        lib.c1o_pack_unit(C.byref(f), again.ctypes.data_as(C.POINTER(C.c_uint8)))
        if not np.array_equal(again, units[u]):
            return 'unit %d: packing its fields again gives other bytes' % u
        want = float(dist[u, 1 if taken[u] else 0])
        got = weighted_error(units[u], coefs[u])
        if not abs(got - want) <= REL * want:
            return 'unit %d: its weighted error %r against the reported %r' % (u, got, want)
    pcm, _ = O.decode_stream(units, nch)
    if not all(np.isfinite(p).all() for p in pcm):
        return 'the decoded stream is not finite'
    return None


def check_outputs(m, units, taken, dist, energy):
    """the GPU's outputs against the model `m` of the same input: None, or what is wrong"""
    if dist.shape != m['D'].shape or energy.shape != m['E'].shape or taken.shape != m['taken'].shape:
        return 'shapes %r %r %r' % (dist.shape, energy.shape, taken.shape)
    for name, got, want in (('distortion', dist, m['D']), ('energy', energy, m['E'])):
        bad = ~(np.abs(got - want) <= REL * want)
        if bad.any():
            at = np.argwhere(bad)[0]
            return '%s at %r: %r against the model %r' % (name, at.tolist(), got[tuple(at)], want[tuple(at)])
        if ((want == 0) & (got != 0)).any():
            return '%s: an exact zero of the model is not zero' % name
    if not np.array_equal(taken, m['taken']):
        return 'taken differs from the model at %r' % np.flatnonzero(taken != m['taken'])[:4].tolist()
    if (dist[:, 1][taken != 0] >= dist[:, 0][taken != 0]).any() or (np.where(taken != 0, dist[:, 1], dist[:, 0]) > dist[:, 0]).any():
        return 'T_final exceeds T_ref'
    for u in range(units.shape[0]):
        f = O.unpack_unit(units[u])
        if f.nbfu != m['nbfu'][u]:
            return 'unit %d: nBfu %d, the model %d' % (u, f.nbfu, int(m['nbfu'][u]))
        if taken[u] and not np.array_equal(np.array(f.wl[:f.nbfu]), m['wl'][u, :f.nbfu]):
            return 'unit %d: word lengths %r, the model %r' % (u, list(f.wl[:f.nbfu]), m['wl'][u, :f.nbfu].tolist())
    fallback = taken == 0
    if not np.array_equal(units[fallback], m['ref'][fallback]):
        return 'a unit not taken differs from the reference\'s bytes'
    if not np.array_equal(units, m['units']):
        return 'units differ from the model at %r' % np.flatnonzero((units != m['units']).any(axis=1))[:4].tolist()
    return None
