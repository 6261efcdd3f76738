"""CPU-only: the hard material of tests/hard_material_lib.py is what it claims.  From the models alone: every edge of the measured
allocation's definition that the shared pink and white material never reaches is reached by units the GPU tests compare (decided or
tied ones), for the plain and for the scale-factor model; few units are close, under every model; the models' own units are
ordinary sound units; and the joint-modes model leaves exactly one candidate for every unit that is compared.
Run with -s to see the counts per case."""
import numpy as np
import pytest

import hard_material_lib as H
import masked_alloc_lib as MK
import measured_alloc_lib as MA
import measured_modes_lib as MM
import scale_factor_choice_lib as SF

CASES = [(name, byte) for name in H.NAMES for byte in H.BYTES] + [('impulse', 'detect')]


def _counts(which, name, kind):
    decided, tied, close = H.classes(H.model(which, name, kind))
    return int(decided.sum()), int(tied.sum()), int(close.sum())


@pytest.mark.parametrize('which', H.MODELS)
@pytest.mark.parametrize('name,kind', CASES)
def test_few_units_are_close(name, kind, which):
    """Measured here, close units of 24 at worst per material: tone 2 (plain), 3 (sf), 0 (masked), all under byte 0; none anywhere
    else."""
    m = H.model(which, name, kind)
    decided, tied, close = _counts(which, name, kind)
    e = H.edges(name, kind, which)
    print('%-8s %-7s %-7s decided %2d tied %2d close %d taken %2d |' % (name, kind, which, decided, tied, close, int(m['taken'].sum())),
          ' '.join('%s %d' % (k, e[k]) for k in H.EDGES))
    assert decided + tied + close == 2 * H.FRAMES
    assert close <= H.CLOSE_CAP[name], (name, kind, which, close)
    assert not np.isnan(m['D']).any() and not np.isnan(m['E']).any()


@pytest.mark.parametrize('which', ['plain', 'sf'])
def test_every_edge_is_reached_by_a_unit_that_is_compared(which):
    """level15: a level-15 word length in a taken unit; low_index / top_index: a coded BFU of a taken unit with findScaleFactor's
    index in 1 .. 3 / at 63; zero_index: a BFU with index 0 and non-zero e(b, 0); nbfu20: a taken unit with 20 BFUs;
    fallback_ref: a non-silent unit whose reference record is allocateBits' all-zero fallback; tie_kept: a tied unit not taken"""
    total = dict.fromkeys(H.EDGES, 0)
    where = {k: [] for k in H.EDGES}
    for name, kind in CASES:
        for k, v in H.edges(name, kind, which).items():
            total[k] += v
            if v:
                where[k].append('%s/%s' % (name, kind))
    for k in H.EDGES:
        print('%-6s %-13s %5d  %s' % (which, k, total[k], ' '.join(where[k])))
    assert all(total[k] > 0 for k in H.EDGES), total


def test_the_shared_material_reaches_none_of_them():
    """what the table of the hard material is measured against: pink and white under their constant bytes keep the word length
    levels at or below 8, the indices of coded BFUs within 4 .. 62 and nBfu at or above 36, and have no tie"""
    for material, bytes_ in MA.CONSTANT.items():
        for byte in bytes_:
            m = MA.case(byte, material)
            assert m['wl'].max() <= 8 and m['nbfu'][m['taken'] != 0].min() >= 36 and (m['margin'] > 0).all(), (material, byte)


@pytest.mark.parametrize('name,kind', CASES)
def test_the_models_units_are_ordinary_sound_units(name, kind):
    m = H.model('plain', name, kind)
    assert MA.check_valid(m['units'], m['coefs'], m['taken'], m['D']) is None
    assert MA.check_outputs(m, m['units'], m['taken'], m['D'], m['E']) is None
    m = H.model('sf', name, kind)
    assert SF.check_valid(m['units'], m['coefs'], m['taken'], m['D']) is None
    assert SF.check_outputs(m, m['units'], m['taken'], m['shifts'], m['D'], m['E']) is None
    m = H.model('masked', name, kind)
    assert MK.check_valid(m['units'], m['coefs'], m['taken'], m['D'], m['P']) is None
    assert MK.check_outputs(m, m['units'], m['taken'], m['shifts'], m['D'], m['E'], m['P']) is None


def test_rows_cuts_every_per_unit_array():
    m = H.model('sf', 'quiet', 0)
    keep = H.classes(m)[1]
    cut = H.rows(m, keep)
    n = int(keep.sum())
    assert 0 < n < len(keep) and all(cut[k].shape[0] == n for k in ('units', 'taken', 'nbfu', 'wl', 'D', 'E', 'margin', 'coefs', 'ref', 'shifts'))
    assert SF.check_outputs(cut, cut['units'], cut['taken'], cut['shifts'], cut['D'], cut['E']) is None


@pytest.mark.parametrize('sf', [False, True])
@pytest.mark.parametrize('name', H.NAMES)
def test_joint_modes_leave_one_candidate(name, sf):
    """every non-silent unit has exactly one admissible candidate within CHOICE_REL -- or several whose T_final are the same bits,
    of which the first is the choice -- or counts as close.  Measured here, close units of 24: tone 4 (offset 0) and 3
    (OFFSETS), none elsewhere; dc_gap: 11 tied units (the constant channel) and 4 silent ones"""
    m = H.modes_model(name, sf)
    firm, tied, close, silent = H.modes_classes(name, sf)
    print('%-8s %-5s firm %2d tied %2d close %d silent %d winners %s' % (name, 'sf' if sf else 'plain', firm.sum(), tied.sum(), close.sum(),
                                                                         silent.sum(), np.bincount(m['choice'], minlength=len(m['cand'])).tolist()))
    assert (firm | tied | close | silent).all() and firm.sum() + tied.sum() + close.sum() + silent.sum() == 2 * H.FRAMES
    assert close.sum() <= H.CLOSE_CAP[name]
    keep = ~close
    ok = MM.first_of_exact_ties(m['final'][keep])
    assert (ok.sum(axis=1) == 1).all()
    assert np.array_equal(ok.argmax(axis=1), m['choice'][keep])
    assert not m['choice'][silent].any() and not m['D'][silent].view(np.uint64).any() and not m['E'][silent].view(np.uint64).any()
    if name == 'dc_gap':
        assert silent.sum() == 4 and tied.any()
    # the model against itself, cut to the units that are compared
    cut = H.rows(m, keep)
    out = {'units': cut['units'], 'choice': cut['choice'], 'modes': cut['modes'], 'taken': cut['taken'], 'shifts': cut['shifts'],
           'distortion': cut['D'], 'energy': cut['E']}
    assert MM.check_case(cut, out) is None


def test_the_shared_joint_modes_cases_have_no_exact_tie():
    """first_of_exact_ties changes nothing where one candidate is admissible: the pink and white cases are what they were"""
    for material, sf in (('pink', False), ('white', False), ('white', True)):
        fin = MM.case(material, sf)['final']
        assert np.array_equal(MM.first_of_exact_ties(fin), MM.admissible(fin)) and (MM.admissible(fin).sum(axis=1) == 1).all()
