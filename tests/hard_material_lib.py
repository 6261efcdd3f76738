"""Material at the edges of the measured allocation's definition (include/carta1_hip.h, c1_encode_measured_*), and its models.

The shared pink and white material keeps every BFU in the middle of the tables: word length levels up to 8, scale-factor indices
30 .. 58, nBfu 36 .. 52.  Five stereo signals of 12 frames each, states from zero, reach what it leaves out:
    tone     one strong low sine against three weaker ones in the three QMF bands: the level-15 cap of the greedy
    loud     white * 40 and pink * 1000, far beyond full scale: index 63, where quantize clips and a positive offset is invalid
    quiet    pink * 1e-4 and pink * 1e-6: indices 0 .. 3, where a negative offset is invalid, BFUs that code nothing, units whose
             reference record is allocateBits' own fallback, exact ties between amounts and between T(n*) and T_ref
    impulse  a full-scale 100 Hz square wave and one unit sample per frame
    dc_gap   a constant 0.75, and white noise in frames 0, 3, 6, 9 with zeros between: the frame after the noise codes only its
             tail (the codec delay), and every third frame is exactly silent, between coded frames
Per material and mode byte (0, 10, 58; 'detect' for detection) the models are those of measured_alloc_lib, scale_factor_choice_lib
(OFFSETS), masked_alloc_lib (packaged tables) and measured_modes_lib (composed), each computed once per process and never written.

A unit is `decided` when the least relative margin of the model's decisions is above MARGIN, `tied` when it is exactly 0 and
`close` in between.  A tie is structural -- the same e(b, w) summed in the same order on both sides -- so the header's tie rules
(the smallest b, the first amount, T(n*) == T_ref is not taken) decide it on the device as in the model; only a close unit is
exempt from the comparison of decisions."""
import numpy as np

import block_modes_lib as BM
import masked_alloc_lib as MK
import measured_alloc_lib as MA
import measured_modes_lib as MM
import oracle_lib as O
import scale_factor_choice_lib as SF

FRAMES = 12
RATE = 44100.0
NAMES = ('tone', 'loud', 'quiet', 'impulse', 'dc_gap')
BYTES = (0, 10, 58)
OFFSETS = SF.OFFSETS
MARGIN = MA.MARGIN
MODELS = ('plain', 'sf', 'masked')
CLOSE_CAP = {'tone': 4, 'quiet': 2, 'loud': 0, 'impulse': 0, 'dc_gap': 0}      # close units of 24, per (material, byte, model)
EDGES = ('level15', 'low_index', 'top_index', 'zero_index', 'nbfu20', 'fallback_ref', 'tie_kept')

_cache = {}


def _once(key, make):
    if key not in _cache:
        v = make()
        for a in (v.values() if isinstance(v, dict) else v):
            a.setflags(write=False)
        _cache[key] = v
    return _cache[key]


def _sine(hz, amp, n):
    return amp * np.sin(2.0 * np.pi * hz * np.arange(n) / RATE)


def _make(name):
    n = FRAMES * 512
    if name == 'tone':
        a = _sine(1234.5, 0.9, n)
        b = _sine(5000.0, 0.3, n) + _sine(9000.0, 0.3, n) + _sine(17000.0, 0.3, n)
    elif name == 'loud':
        a, b = O.gen_white(21, n) * np.float32(40.0), O.gen_pinkT(22, n) * np.float32(1000.0)
    elif name == 'quiet':
        # seeds 7 and 107: of the seeds 1 .. 40 one whose plain model takes 20-BFU units under every byte, with no close unit
        a, b = O.gen_pinkT(7, n).astype(np.float64) * 1e-4, O.gen_pinkT(107, n).astype(np.float64) * 1e-6
    elif name == 'impulse':
        a = np.where(_sine(100.0, 1.0, n) >= 0.0, 1.0, -1.0)
        b = np.zeros(n)
        b[np.arange(FRAMES) * 512 + 37 * (np.arange(FRAMES) % 13) + 5] = 1.0      # one unit sample per frame, at moving places
    elif name == 'dc_gap':
        a = np.full(n, 0.75)
        b = O.gen_white(25, n).astype(np.float64)
        b = b.reshape(FRAMES, 512)
        b[1::3] = 0.0                              # the tail of the noise frame still reaches this frame's coefficients ...
        b[2::3] = 0.0                              # ... and this one, every third, is silent to the last coefficient
        b = b.reshape(-1)
    else:
        raise KeyError(name)
    return [np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)]


def material(name):
    """the two channels of a named material, float32 [FRAMES * 512] each"""
    return _once(('material', name), lambda: _make(name))


def modes_of(kind):
    """the mode bytes a call is given under `kind`: uint8 [FRAMES, 2], or None under detection"""
    return None if kind == 'detect' else np.full((FRAMES, 2), kind, dtype=np.uint8)


def reference(name, kind):
    """the reference's units under a constant mode byte, or under detection with default options"""
    def make():
        chans = material(name)
        return [O.encode_stream(chans)[0] if kind == 'detect' else BM.oracle_encode_modes(chans, modes_of(kind), 1.0)[0]]
    return _once(('ref', name, kind), make)[0]


def tables(name, kind):
    """masked_alloc_lib.tables_of of the material: the unweighted e_k(b, w), s0 and the reference's record"""
    return _once(('tables', name, kind), lambda: MK.tables_of(material(name), reference(name, kind), OFFSETS))


def model(which, name, kind):
    """the model `which` ('plain', 'sf', 'masked') of the material under `kind`"""
    def make():
        if which == 'plain':
            return MA.model(material(name), reference(name, kind))
        if which == 'sf':
            return SF.model(material(name), reference(name, kind), OFFSETS)
        return dict(MK.model_of(tables(name, kind), *MK.packaged()))
    return _once((which, name, kind), make)


def modes_candidates(sf):
    return MM.PINK_SF_CANDIDATES if sf else MM.CANDIDATES


def modes_model(name, sf):
    """the joint-modes model over MM.CANDIDATES with the single offset 0, or over MM.PINK_SF_CANDIDATES with OFFSETS"""
    cand = modes_candidates(sf)
    return _once(('modes', name, bool(sf)),
                 lambda: MM.case(material(name), sf, cand, [model('sf' if sf else 'plain', name, b) for b in cand]))


NONFINITE_FRAMES = 12
NONFINITE_AT = {1: (3, 100, np.nan), 0: (6, 300, np.inf)}           # channel: (frame, sample within it, value)
NONFINITE_CANDIDATES = MM.PINK_SF_CANDIDATES


def nonfinite_material(clean=False):
    """the first frames of the shared pink material with one NaN in channel 1 and one +Inf in channel 0 (or without, `clean`)"""
    def make():
        import best_bias_lib as BB
        chans = [c[:NONFINITE_FRAMES * 512].copy() for c in BB.material()[1]]
        for c, (frame, at, value) in ({} if clean else NONFINITE_AT).items():
            chans[c][frame * 512 + at] = value
        return chans
    return _once(('nonfinite', clean), make)


def _nonfinite_modes():
    import best_bias_lib as BB
    m = BB.given_modes()[:NONFINITE_FRAMES].copy()
    m.setflags(write=False)
    return m


NONFINITE_MODES = _nonfinite_modes()             # the given modes of the non-finite calls: over the whole domain


def _quietly(make):
    """the models in numpy over NaN and Inf: what they compute is the point, not the warnings"""
    def run():
        with np.errstate(all='ignore'):
            return make()
    return run


def nonfinite_model(which, byte=None):
    """the model `which` of the non-finite material under NONFINITE_MODES, or under the constant `byte`.  A unit whose T are all
    NaN has a NaN 'D'[:, 1] and is not taken; 'margin' means nothing where a figure is not finite"""
    def make():
        chans = nonfinite_material()
        modes = NONFINITE_MODES if byte is None else np.full((NONFINITE_FRAMES, 2), byte, dtype=np.uint8)
        ref = BM.oracle_encode_modes(chans, modes, 1.0)[0]
        if which == 'plain':
            return MA.model(chans, ref)
        if which == 'sf':
            return SF.model(chans, ref, OFFSETS)
        return dict(MK.model_of(MK.tables_of(chans, ref, OFFSETS), *MK.packaged()))
    return _once(('nonfinite', which, byte), _quietly(make))


def nonfinite_modes_model():
    """the joint-modes model of the non-finite material over NONFINITE_CANDIDATES with OFFSETS"""
    return _once(('nonfinite', 'modes'), _quietly(lambda: MM.case(nonfinite_material(), True, NONFINITE_CANDIDATES,
                                                                  [nonfinite_model('sf', b) for b in NONFINITE_CANDIDATES])))


def untouched(m):
    """bool [U]: the units of a non-finite model every figure of which is finite -- the bad samples do not reach them"""
    return np.isfinite(m['D']).reshape(len(m['D']), -1).all(axis=1) & np.isfinite(m['E']).reshape(len(m['D']), -1).all(axis=1)


def classes(m):
    """-> (decided, tied, close) bool [U] by the model's own margin"""
    g = m['margin']
    return g > MARGIN, g == 0, (g > 0) & (g <= MARGIN)


def silent(m):
    return m['E'] == 0


def modes_classes(name, sf):
    """-> (firm, tied, close, silent) bool [U] of the joint-modes model.  Silent units have no energy under any candidate: choice 0.
    A unit is close when some candidate's own model is close there, or when several candidates are admissible within CHOICE_REL
    and their T_final are not all the same bits; tied when they are (measured_modes_lib.first_of_exact_ties: dc_gap's constant
    channel, whose mid and high bands are exactly zero however they are coded); firm otherwise.  Firm and tied units are compared"""
    m = modes_model(name, sf)
    quiet = (m['E'] == 0).all(axis=1)
    close = np.zeros(len(quiet), dtype=bool)
    for b in modes_candidates(sf):
        close |= classes(model('sf' if sf else 'plain', name, b))[2]
    close |= MM.first_of_exact_ties(m['final']).sum(axis=1) != 1
    close &= ~quiet
    with np.errstate(invalid='ignore'):
        tied = ~close & ~quiet & (MM.admissible(m['final']).sum(axis=1) > 1)
    return ~close & ~quiet & ~tied, tied, close, quiet


def rows(m, keep):
    """the units `keep` (bool [U]) of a model or of a call's outputs: every per-unit array cut, anything else as it is"""
    n = len(keep)
    return {k: (v[keep] if isinstance(v, np.ndarray) and v.ndim >= 1 and v.shape[0] == n and k != 'cand' else v) for k, v in m.items()}


def edges(name, kind, which):
    """how often the decided and tied units of one model reach each edge of the definition -> dict of counts (EDGES)"""
    m, t = model(which, name, kind), tables(name, kind)
    decided, tied, _ = classes(m)
    firm = (decided | tied)[:, None]
    s0, e0 = t['s0'], t['EK'][:, 0, :, 0]
    taken = m['taken'] != 0
    below = np.arange(52)[None, :] < m['nbfu'][:, None]
    coded = firm & taken[:, None] & below & (m['wl'] > 0)
    ref = [O.unpack_unit(u) for u in t['ref']]
    fallback = np.array([f.nbfu == 20 and not any(f.sfi[:20]) and not any(f.wl[:20]) for f in ref])
    return {'level15': int((coded & (m['wl'] == 15)).any(axis=1).sum()),
            'low_index': int((coded & (s0 >= 1) & (s0 <= 3)).sum()),
            'top_index': int((coded & (s0 == 63)).sum()),
            'zero_index': int((firm & (s0 == 0) & (e0 != 0)).sum()),
            'nbfu20': int((firm[:, 0] & taken & (m['nbfu'] == 20)).sum()),
            'fallback_ref': int((firm[:, 0] & fallback & (m['E'] != 0)).sum()),
            'tie_kept': int((tied & ~taken).sum())}
