"""CPU: the tables the host derives from a biased scale-factor table for the bit-allocation kernels (c1_alloc_tables),
against the reference's own formulas for every (BFU size, sfi, word length):
  * the heap order (bitallocation.js:226-231, 267-269): the rank field of every entry orders like the Float32 priorities
    biasedSF[sfi] * DISTORTION_DELTA_FACTORS[wl] / WORD_LENGTH_DELTA_BITS[wl], ties included, and -- where the host found
    an integer form -- adding one of the two step words to an entry gives the entry of the next word length exactly;
  * the distortion terms (:157-190): the zero-bit term is Float32(biasedSF * 2 * size), and biasedSF * size with the bit
    count subtracted from its exponent is biasedSF * INV_POWER_OF_TWO[bits] * size in the reference's order of operations.
The checker below is the model; it is shown to notice one table entry or one step off by an ulp."""
import ctypes as C

import numpy as np
import pytest

import option_domain_lib as L
import table_variants_lib as TV
from test_alloc_bound_cpu import DB, DDF

SIZES = [4, 6, 7, 8, 9, 10, 12, 20]
PACKAGED = ['0', '0.25', '0.5', '1', '1.5', '2', '3.3', '5']


def host_tables(table):
    import carta1_amd as c1
    from carta1_amd import capi
    o = c1.EncoderOptions({}, biased_table=[float(x) for x in table]).to_c()
    affine, ok = C.c_int(-1), C.c_int(-1)
    steps, rank, dist = np.zeros(2, np.uint32), np.zeros((64, 16), np.uint16), np.zeros((8, 64, 2), np.float64)
    capi.check(capi.load().c1_alloc_tables(C.byref(o), C.byref(affine), steps.ctypes.data, rank.ctypes.data, C.byref(ok), dist.ctypes.data))
    return {'affine': affine.value, 'steps': steps, 'rank': rank, 'dist_ok': ok.value, 'dist': dist}


def identity_holds(table):
    """does (b * n) with `bits` taken off its exponent equal b * 2^-bits * n for every case, inside the normal range?"""
    b = np.asarray(table, np.float64)[1:, None, None]
    n = np.array(SIZES, np.float64)[None, :, None]
    bits = np.arange(2, 17)[None, None, :]
    cs = np.broadcast_to(b * n, (63, 8, 15))
    exp = (cs.view(np.uint64) >> np.uint64(52)) & np.uint64(0x7ff)
    if (exp <= 16).any() or (exp == 0x7ff).any():
        return False
    want = (b * np.exp2(-bits.astype(np.float64))) * n
    got = cs.view(np.uint64) - (bits.astype(np.uint64) << np.uint64(52))
    z = (b * 2.0 * n).astype(np.float32)
    return bool((got == want.view(np.uint64)).all() and (z >= np.finfo(np.float32).tiny).all())


def problems(table, t):
    """every way the host's tables differ from the reference's formulas"""
    table = np.asarray(table, np.float64)
    out = []
    # ---- heap order ----
    pri = np.array([[np.float32(table[s] * DDF[wl] / DB[wl]) for wl in range(15)] for s in range(1, 64)]).ravel()
    key = t['rank'][1:, :15].astype(np.int64).ravel()
    if key.min() < 1 or key.max() > 1022:
        out.append('rank outside 1..1022')
    order = np.argsort(pri, kind='stable')
    dp, dk = np.diff(pri[order]), np.diff(key[order])
    if not (((dp == 0) == (dk == 0)).all() and (dk[dp > 0] > 0).all()):
        out.append('ranks do not order like the Float32 priorities')
    if t['affine']:
        for s in range(1, 64):
            e = (int(t['rank'][s, 0]) << 21) | (s << 10) | (20 << 16) | 51          # some size and BFU: the steps leave them alone
            for wl in range(14):
                e = (e + int(t['steps'][0 if wl == 0 else 1])) & 0xFFFFFFFF
                want = (int(t['rank'][s, wl + 1]) << 21) | (s << 10) | ((wl + 1) << 6) | (20 << 16) | 51
                if e != want:
                    out.append('step from (sfi %d, wl %d): %08x, not %08x' % (s, wl, e, want))
    elif t['steps'].any():
        out.append('steps without an integer form')
    # ---- distortion terms ----
    if t['dist_ok']:
        for c, n in enumerate(SIZES):
            zb = np.where(np.arange(64) != 0, (table * 2.0 * float(n)).astype(np.float32).astype(np.float64), 0.0)
            if not np.array_equal(zb.view(np.uint64), t['dist'][c, :, 0].view(np.uint64)):
                out.append('zero-bit terms of size %d' % n)
            cs = t['dist'][c, 1:, 1].copy()
            for wl in range(1, 16):
                bits = wl + 1
                want = table[1:] * 2.0 ** -bits * float(n)                            # (:183-187), left to right
                got = (cs.view(np.uint64) - (np.uint64(bits) << np.uint64(52))).view(np.float64)
                if not np.array_equal(want.view(np.uint64), got.view(np.uint64)):
                    out.append('coded terms of size %d at %d bits' % (n, bits))
    if bool(t['dist_ok']) != identity_holds(table):
        out.append('dist_ok = %d where the identity %s' % (t['dist_ok'], 'holds' if identity_holds(table) else 'fails'))
    return out


def _tables():
    import carta1_amd as c1
    from carta1_amd import capi, codec
    d = capi.EncodeOptions()
    capi.check(capi.load().c1_default_encode_options(C.byref(d)))
    out = [('default', np.array(list(d.biased_scale_factors), np.float64))]
    out += [('packaged %s' % b, np.array(codec.packaged_biased_table(float(b)), np.float64)) for b in PACKAGED]
    out += [('variant %s' % n, TV.variant(n)['biased']) for n in TV.names()]
    out += [('fixture %s' % b, L.biased(b)) for b in L.fixture()['biases'] if b not in PACKAGED]
    return out


def test_every_table_entry_and_step_is_the_references():
    seen_affine = seen_dist = 0
    for name, table in _tables():
        t = host_tables(table)
        assert problems(table, t) == [], name
        seen_affine += t['affine']
        seen_dist += t['dist_ok']
        if name in ('default', 'packaged 1'):
            assert t['affine'] == 1 and t['dist_ok'] == 1, name
    assert len(TV.names()) == 5
    assert seen_affine >= 8 and seen_dist >= 14, (seen_affine, seen_dist)


def test_tables_the_shortcuts_do_not_cover_fall_back():
    rng = np.random.RandomState(5)
    shuffled = np.concatenate([[2.0 ** -21], rng.permutation(2.0 ** (np.arange(1, 64) / 3.0 - 21))])   # no order in sfi: no integer form
    t = host_tables(shuffled)
    assert t['affine'] == 0 and not t['steps'].any() and t['dist_ok'] == 1 and problems(shuffled, t) == []
    tiny = L.biased('1') * 2.0 ** -1010                            # coded terms of the last word lengths are subnormal
    t = host_tables(tiny)
    assert t['dist_ok'] == 0 and problems(tiny, t) == []
    holes = L.biased('1').copy()
    holes[7] = 0.0                                                 # a zero has no exponent to subtract from
    t = host_tables(holes)
    assert t['dist_ok'] == 0 and problems(holes, t) == []


def test_the_checker_notices_one_ulp_and_one_step():
    table = L.biased('1')
    t = host_tables(table)
    assert t['affine'] == 1 and t['dist_ok'] == 1 and problems(table, t) == []
    for c, s, k in ((0, 1, 0), (3, 40, 1), (7, 63, 0), (7, 63, 1), (5, 17, 1)):
        for towards in (0.0, np.inf):
            m = {**t, 'dist': t['dist'].copy()}
            m['dist'][c, s, k] = np.nextafter(m['dist'][c, s, k], towards)
            assert problems(table, m) != [], (c, s, k, towards)
    for which in (0, 1):
        for delta in (1 << 21, -(1 << 21), 1 << 6, 1):
            m = {**t, 'steps': t['steps'].copy()}
            m['steps'][which] = np.uint32((int(m['steps'][which]) + delta) & 0xFFFFFFFF)
            assert problems(table, m) != [], (which, delta)
    m = {**t, 'rank': t['rank'].copy()}
    m['rank'][30, 4] += 1
    assert problems(table, m) != []
    m = {**t, 'dist_ok': 0}
    assert problems(table, m) != []
    up = table.copy()
    up[20] = np.nextafter(up[20], np.inf)                          # the tables of another biased table are not this one's
    assert problems(up, t) != []
