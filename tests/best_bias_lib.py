"""The allocation bias of every sound unit chosen from a palette by least coding error (c1_encode_best_bias_*): the CPU model of
the distortion D(u, k) and the energy E(u), built from the oracle alone, and the test material the CPU and GPU tests share.

Per palette entry k the units come from bias_palette_lib.oracle_encode_schedule with the constant index k; the coefficients c
from c1o_qmf_analysis_frame + c1o_mdct_frame with the state carried and the block modes read back from the unit; d_k from
c1o_unpack_unit + c1o_dequantize_bfu, each BFU placed by pack_model_lib's START_LONG / START_SHORT and the slot order of the
mantissas.  Sums in numpy float64."""
import ctypes as C

import numpy as np

import bias_palette_lib as BP
import block_modes_lib as BM
import oracle_lib as O
import pack_model_lib as PM

FRAMES = 130
HALO = 2
SEEDS = (11, 12)                                 # O.gen_pinkT per channel; tests/test_best_bias_cpu.py checks what they must give (seeds
                                                 # 3, 4 and 5, 6 leave a unit whose two best entries tie exactly under detection)
BIASES = list(BP.PACKAGED_BIASES)
FIXED = {'fixedBlockModes': [2, 0, 3]}
MODES_SEED = 20261019
REL = 1e-12                                      # |D - model| <= REL * model: two roundings per term and at most 511 * 2^-53 = 6e-14
                                                 # for a sum of 512 non-negative terms in any order, more than tenfold margin
CHOICE_REL = 3e-12                               # an admissible choice: model D <= model minimum * (1 + CHOICE_REL), two such tolerances
UNIQUE_REL = 1e-9                                # the material: every unit's model minimum is unique by more than this


def material():
    """stereo pink noise with transients, FRAMES frames behind a HALO-frame halo -> (with_halo, body)"""
    chans = [O.gen_pinkT(s, (FRAMES + HALO) * 512) for s in SEEDS]
    return chans, [c[HALO * 512:] for c in chans]


def given_modes(frames=FRAMES, nch=2):
    m = BM.random_modes(MODES_SEED, frames, nch)
    assert set(m.reshape(-1).tolist()) == set(BM.DOMAIN_BYTES)
    return m


def coefficients(chans, units):
    """the Float32 MDCT coefficients quantizationStage receives (encoder.js:365) for every unit, [frames * nch, 512]: the
    oracle's QMF analysis and MDCT with the state carried, under the block modes the unit itself records"""
    nch = len(chans)
    frames = len(chans[0]) // 512
    out = np.zeros((frames * nch, 512), dtype=np.float32)
    fp = C.POINTER(C.c_float)
    for c in range(nch):
        st = O.EncState()
        pcm = np.ascontiguousarray(chans[c], dtype=np.float32)
        for f in range(frames):
            bands = np.zeros(512, dtype=np.float32)
            coefs = np.zeros(512, dtype=np.float32)
            x = np.ascontiguousarray(pcm[f * 512:(f + 1) * 512])
            O.lib().c1o_qmf_analysis_frame(C.byref(st), x.ctypes.data_as(fp), bands.ctypes.data_as(fp))
            fields = O.unpack_unit(units[f * nch + c])
            modes = (C.c_int * 3)(*fields.modes)
            O.lib().c1o_mdct_frame(C.byref(st), bands.ctypes.data_as(fp), modes, coefs.ctypes.data_as(fp))
            out[f * nch + c] = coefs
    return out


def dequantized(unit):
    """dequantizationStage (decoder.js:52-98) of one sound unit -> 512 Float32 coefficients in quantizationStage's order;
    zero where a BFU is at or above nBfu or has word length 0"""
    f = O.unpack_unit(unit)
    d = np.zeros(512, dtype=np.float32)
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int)
    for b in range(f.nbfu):
        n = int(PM.SPECS[b])
        wl = int(f.wl[b])
        bits = 0 if wl == 0 else wl + 1
        q = np.ascontiguousarray(np.array(f.q[PM.FIRST[b]:PM.FIRST[b] + n], dtype=np.int32))
        out = np.zeros(n, dtype=np.float32)
        O.lib().c1o_dequantize_bfu(q.ctypes.data_as(ip), n, int(f.sfi[b]), bits, out.ctypes.data_as(fp))
        st = int((PM.START_LONG if f.modes[PM.BAND_OF_BFU[b]] == 0 else PM.START_SHORT)[b])
        d[st:st + n] = out
    return d


def model(chans, palette, modes=None, base=None):
    """-> {'units': [n][units, 212] per entry, 'D': float64 [units, n], 'E': float64 [units], 'coefs'}"""
    nch = len(chans)
    frames = len(chans[0]) // 512
    per_entry = [BP.oracle_encode_schedule(chans, palette, np.full((frames, nch), k, dtype=np.uint8), modes, base)[0] for k in range(len(palette))]
    coefs = coefficients(chans, per_entry[0])        # the block modes do not depend on the bias: any entry's units record them
    c64 = coefs.astype(np.float64)
    D = np.zeros((frames * nch, len(palette)), dtype=np.float64)
    for k, units in enumerate(per_entry):
        for u in range(frames * nch):
            D[u, k] = np.sum((c64[u] - dequantized(units[u]).astype(np.float64)) ** 2)
    return {'units': per_entry, 'D': D, 'E': np.sum(c64 ** 2, axis=1), 'coefs': coefs}


_cases = {}


def case(kind):
    """the model of the shared material under 'modes' (given random modes over the whole domain), 'detect' or 'fixed' ([2,0,3]);
    computed once per process, shared, never written"""
    if kind not in _cases:
        _, body = material()
        modes = given_modes() if kind == 'modes' else None
        base = None if kind == 'modes' else (dict(FIXED) if kind == 'fixed' else {})
        m = model(body, BIASES, modes, base)
        m['modes'], m['base'] = modes, base
        for a in m['units'] + [m['D'], m['E'], m['coefs']]:
            a.setflags(write=False)
        _cases[kind] = m
    return _cases[kind]


def admissible(D):
    """bool [units, n]: the entries whose model distortion is within CHOICE_REL of the unit's model minimum"""
    return D <= D.min(axis=1, keepdims=True) * (1.0 + CHOICE_REL)


def unique_margin(D):
    """per unit: (second smallest - smallest) / smallest of the model distortions (inf for one entry or a zero minimum)"""
    s = np.sort(D, axis=1)
    if s.shape[1] < 2:
        return np.full(s.shape[0], np.inf)
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where(s[:, 0] > 0, (s[:, 1] - s[:, 0]) / s[:, 0], np.inf)


def check_outputs(kind, units, choice, dist, energy):
    """the GPU's outputs on the shared material against the model: None, or what is wrong"""
    m = case(kind)
    D, E = m['D'], m['E']
    if dist.shape != D.shape or energy.shape != E.shape:
        return 'shapes %r %r' % (dist.shape, energy.shape)
    for name, got, want in (('distortion', dist, D), ('energy', energy, E)):
        bad = np.abs(got - want) > REL * want
        if bad.any():
            at = np.argwhere(bad)[0]
            return '%s at %r: %r against the model %r' % (name, at.tolist(), got[tuple(at)], want[tuple(at)])
        if ((want == 0) & (got != 0)).any():
            return '%s: an exact zero of the model is not zero' % name
    ok = admissible(D)
    if (ok.sum(axis=1) != 1).any():
        return 'the model leaves more than one admissible entry for some unit'
    if not ok[np.arange(len(choice)), choice].all():
        u = int(np.flatnonzero(~ok[np.arange(len(choice)), choice])[0])
        return 'unit %d: choice %d, model D %r' % (u, int(choice[u]), D[u].tolist())
    want_units = BP.oracle_encode_schedule(material()[1], BIASES, choice.reshape(-1, 2), m['modes'], m['base'])[0]
    if not np.array_equal(units, want_units):
        return 'units differ from the oracle schedule at %r' % np.flatnonzero((units != want_units).any(axis=1))[:4].tolist()
    return None
