"""The block modes of every sound unit chosen from candidates by the error of the measured allocation
(c1_encode_measured_modes_*): the CPU model, composed from the models the per-candidate calls already have.

For candidate byte k the figures are those of measured_alloc_lib.case(byte, material) (offsets (0,): the plain measured
allocation) or scale_factor_choice_lib.case(byte, material) (the suggested offsets) -- T_ref, T(n*), taken, the energy, the
shifts and the packed units under that constant byte.  T_final = taken ? T(n*) : T_ref; the choice is the first candidate of
least T_final; every output of the winner is that candidate's model's.  Nothing new is modelled here, so every figure of the
call has a pin that existed before it.

The scale-factor model of the pink material costs several seconds a candidate: it is used with PINK_SF_CANDIDATES only.  A
subset's margin of uniqueness is never below the full set's."""
import numpy as np

import best_modes_lib as BMO
import measured_alloc_lib as MA
import scale_factor_choice_lib as SF

CANDIDATES = list(BMO.CANDIDATES)                # [0, 48, 8, 56, 2, 50, 10, 58]
PINK_SF_CANDIDATES = [0, 10, 58]
OFFSETS = SF.OFFSETS                             # (0, -1, 1, -2, -3)
REL = MA.REL                                     # the per-candidate models' bound on T and the energy
UNIQUE_REL = 1e-9                                # the material: every unit's least T_final is unique by more than this
CHOICE_REL = 3e-12                               # an admissible choice: model T_final <= model minimum * (1 + CHOICE_REL)


def candidates_of(material, sf):
    return PINK_SF_CANDIDATES if (sf and material == 'pink') else CANDIDATES


def candidate_case(byte, material, sf):
    """the per-candidate model: scale_factor_choice_lib's under OFFSETS, or measured_alloc_lib's.  material: 'pink' / 'white' (the
    shared, cached cases) or the channels of any other material (states from zero; computed here, not cached)"""
    if isinstance(material, str):
        return SF.case(byte, material) if sf else MA.case(byte, material)
    import block_modes_lib as BM
    ref = BM.oracle_encode_modes(material, np.full((len(material[0]) // 512, len(material)), byte, dtype=np.uint8), BMO.BIAS)[0]
    return SF.model(material, ref, OFFSETS) if sf else MA.model(material, ref)


def final(m):
    """T_final of a per-candidate model, float64 [units]"""
    return np.where(m['taken'] != 0, m['D'][:, 1], m['D'][:, 0])


def compose(cand, per, sf):
    """the joint model of the candidate bytes `cand` from their per-candidate models `per`, in that order -> case's dict"""
    D = np.stack([m['D'] for m in per], axis=1)
    E = np.stack([m['E'] for m in per], axis=1)
    fin = np.stack([final(m) for m in per], axis=1)
    choice = np.where(np.isnan(fin), np.inf, fin).argmin(axis=1)
    ar = np.arange(len(choice))
    pick = lambda name: np.stack([m[name] for m in per], axis=1)[ar, choice]
    shifts = pick('shifts') if sf else np.zeros((len(choice), 52), dtype=np.int8)
    out = {'cand': np.asarray(cand, dtype=np.uint8), 'D': D, 'E': E, 'final': fin, 'choice': choice.astype(np.uint8),
           'modes': np.asarray(cand, dtype=np.uint8)[choice], 'taken': pick('taken'), 'shifts': shifts, 'units': pick('units'),
           'coefs': pick('coefs')}
    for a in out.values():
        a.setflags(write=False)
    return out


_cases = {}


def case(material, sf, candidates=None, per=None):
    """-> dict: 'cand' (the bytes), 'D' float64 [U, n, 2], 'E' [U, n], 'final' [U, n], 'choice' [U], 'modes' uint8 [U], 'taken'
    uint8 [U], 'shifts' int8 [U, 52], 'units' uint8 [U, 212] (the winner's), 'coefs' float32 [U, 512] (the winner's).
    material: 'pink' / 'white' -- computed once per process, shared, never written -- or the channels of any other material, whose
    per-candidate models may be handed in as `per` (one per candidate, in order); the caller caches those"""
    named = isinstance(material, str)
    cand = list(candidates_of(material if named else None, sf) if candidates is None else candidates)
    if not named:
        return compose(cand, [candidate_case(b, material, sf) for b in cand] if per is None else list(per), sf)
    key = (material, bool(sf), tuple(cand))
    if key not in _cases:
        _cases[key] = compose(cand, [candidate_case(b, material, sf) for b in cand], sf)
    return _cases[key]


def unique_margin(fin):
    """the relative gap between a unit's least and second-least T_final, float64 [units] (inf with one candidate)"""
    if fin.shape[1] < 2:
        return np.full(fin.shape[0], np.inf)
    order = np.sort(fin, axis=1)
    return (order[:, 1] - order[:, 0]) / order[:, 1]


def admissible(fin):
    """bool [units, n]: the candidates whose model T_final is within CHOICE_REL of the unit's model minimum"""
    return fin <= fin.min(axis=1, keepdims=True) * (1.0 + CHOICE_REL)


def first_of_exact_ties(fin):
    """admissible(fin), but where every admissible candidate of a unit has bit for bit the least T_final only the first of them:
    an exact tie comes from candidates that differ only in bands whose coefficients are all zero, so the same e(b, w) are summed in
    the same order under each, and the header's rule (the smallest k) decides.  With one admissible candidate nothing changes"""
    with np.errstate(invalid='ignore'):
        ok = admissible(fin)
        least = fin == fin.min(axis=1, keepdims=True)
    exact = (ok == least).all(axis=1) & least.any(axis=1)
    first = np.zeros_like(ok)
    first[np.arange(len(fin)), least.argmax(axis=1)] = True
    return np.where(exact[:, None], first, ok)


def sequence_choice(material, cand):
    """the two-call sequence's choice: the first candidate of least D of the best-modes model, as indices into cand"""
    cols = [BMO.CANDIDATES.index(b) for b in cand]
    return BMO.case(material)['D'][:, cols].argmin(axis=1)


def gain_over_sequence_db(material, sf, candidates=None):
    """the aggregate T_final of encode_best_modes followed by encode_measured(modes=modes_out) over the joint choice's, in dB"""
    m = case(material, sf, candidates)
    seq = sequence_choice(material, m['cand'].tolist())
    ar = np.arange(len(seq))
    return 10.0 * np.log10(m['final'][ar, seq].sum() / m['final'].min(axis=1).sum())


def check_outputs(material, sf, out, columns=None):
    """the GPU's outputs (dict: units, choice, modes, taken, shifts, distortion [U, n, 2], energy [U, n]) against the model of
    the candidates candidates_of(material, sf)[columns] in that order: None, or what is wrong"""
    base = candidates_of(material, sf)
    cand = base if columns is None else [base[k] for k in columns]
    return check_case(case(material, sf, cand), out)


def check_case(m, out):
    """the same against any model `m` of case's form"""
    cand = m['cand']
    if out['distortion'].shape != m['D'].shape or out['energy'].shape != m['E'].shape:
        return 'shapes %r %r' % (out['distortion'].shape, out['energy'].shape)
    for name, got, want in (('distortion', out['distortion'], m['D']), ('energy', out['energy'], m['E'])):
        bad = ~(np.abs(got - want) <= REL * want)
        if bad.any():
            at = np.argwhere(bad)[0]
            return '%s at %r: %r against the model %r' % (name, at.tolist(), got[tuple(at)], want[tuple(at)])
        if ((want == 0) & (got != 0)).any():
            return '%s: an exact zero of the model is not zero' % name
    ok = first_of_exact_ties(m['final'])
    if (ok.sum(axis=1) != 1).any():
        return 'the model leaves more than one admissible candidate for some unit'
    choice = np.asarray(out['choice'])
    if (choice >= len(cand)).any():
        return 'a choice is not below n_cand'
    ar = np.arange(len(choice))
    if not ok[ar, choice].all():
        u = int(np.flatnonzero(~ok[ar, choice])[0])
        return 'unit %d: choice %d, model T_final %r' % (u, int(choice[u]), m['final'][u].tolist())
    if not np.array_equal(out['modes'], m['modes']):
        return 'modes_out is not cand_modes[choice]'
    if not np.array_equal(out['taken'], m['taken']):
        return 'taken differs from the winner\'s model at %r' % np.flatnonzero(out['taken'] != m['taken'])[:4].tolist()
    if not np.array_equal(out['shifts'], m['shifts']):
        return 'shifts differ from the winner\'s model'
    if not np.array_equal(out['units'], m['units']):
        return 'units differ from the winner\'s model at %r' % np.flatnonzero((out['units'] != m['units']).any(axis=1))[:4].tolist()
    return None
