"""CPU: the fixed-modes fixture (tests/golden/fixed_modes.json: the reference encoder under all 36 fixedBlockModes triples
the library accepts) against the CPU oracle, and the property that makes 36 triples 8 classes: triples with the same
bands in short blocks give the same unit but for the six mode bits of the header, and the same decoded PCM."""
import numpy as np
import pytest

import fixed_modes_lib as F
import option_domain_lib as L
import oracle_lib as O

FX = F.fixture()
IDS = ['m%d%d%d' % t for t in F.TRIPLES]


def test_the_fixture_covers_the_accepted_domain():
    st = F.stereo_cases()
    assert [F.modes_of(c) for c in st] == F.TRIPLES and len(F.TRIPLES) == 36
    assert all(c['frames'] == 40 and c['channels'] == 2 and c['bias'] == '1' and 1 <= c['cut'] < 40 for c in st)
    assert len({c['seed'] for c in FX['cases']}) == len(FX['cases'])
    sh = F.short_cases()
    assert len(sh) == 4 and all(c['frames'] == 3 for c in sh)
    assert not {F.modes_of(c) for c in sh} & set(F.CANONICAL_TESTED)
    cl = F.classes()
    assert len(cl) == 8 and sum(len(v) for v in cl.values()) == 36 and len(F.ALL_SHORT) == 12
    assert all(F.canonical(t) in v for k, v in cl.items() for t in v)
    for c in FX['cases']:                                           # the non-canonical fields reach the unit
        m = F.modes_of(c)
        assert int(c['header'][:2], 16) & 0xFC == F.mode_bits(m), (m, c['header'])
    assert next(c for c in st if F.modes_of(c) == (1, 1, 1))['header'][:2] == '58'


def test_inputs_are_rebuilt_bit_for_bit():
    for c in FX['cases']:
        assert [L.sha(x) for x in L.inputs(c)] == c['input_sha256'], c['id']


@pytest.mark.parametrize('case', FX['cases'], ids=lambda c: 'm%d%d%d_%df' % (F.modes_of(c) + (c['frames'],)))
def test_oracle_reproduces_every_case(case):
    c = case
    fm = F.modes_of(c)
    xs = L.inputs(c)
    units, _ = O.encode_stream(xs, fixed_modes=fm)
    assert L.sha(units) == c['units_sha256'], ('case', c['id'], fm, 'first wrong unit', L.first_wrong_unit(units, c))
    assert ((units[:, 0] & 0xFC) == F.mode_bits(fm)).all()
    pcm, _ = O.decode_stream(units, c['channels'])
    assert L.pcm_sha(pcm) == c['pcm_sha256'], ('pcm', c['id'])
    h, cut = c['halo'], c['cut']                                    # the tail from its halo, as the GPU tests encode it
    tail, _ = O.encode_stream([x[(cut - h) * 512:] for x in xs], fixed_modes=fm)
    tail = tail.reshape(-1, c['channels'], 212)[h:].reshape(-1, 212)
    assert np.array_equal(tail, units.reshape(-1, c['channels'], 212)[cut:].reshape(-1, 212)), ('halo', c['id'])


@pytest.mark.parametrize('cls', sorted(F.classes()), ids=lambda k: 'short%d%d%d' % k)
def test_triples_of_one_class_differ_in_the_six_mode_bits_only(cls):
    """one input (the canonical triple's case) under every triple of the class"""
    triples = F.classes()[cls]
    canon = F.canonical(triples[0])
    case = next(c for c in F.stereo_cases() if F.modes_of(c) == canon)
    xs = L.inputs(case)
    want, _ = O.encode_stream(xs, fixed_modes=canon)
    assert L.sha(want) == case['units_sha256']
    pcm_want = L.pcm_sha(O.decode_stream(want, 2)[0])
    for t in triples:
        units, _ = O.encode_stream(xs, fixed_modes=t)
        F.assert_same_but_mode_bits(units, t, want, canon, 'oracle')
        assert L.pcm_sha(O.decode_stream(units, 2)[0]) == pcm_want, t
    if len(triples) > 1:                                            # and the bits do differ: the triples are told apart
        assert len({F.mode_bits(t) for t in triples}) == len(triples)
