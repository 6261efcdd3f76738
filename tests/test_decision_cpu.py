"""CPU: the model of the decision functions (tests/model/decision_model.c) reproduces every record the reference's own
performFFT, detectTransient, findScaleFactor, allocateBits and Math.log2 produced (tests/golden/decision.json), and each of its
deliberate faults makes some record fail, so the records have teeth.  The GPU tests compare the kernels with this model."""
import numpy as np
import pytest

import decision_lib as D


def mismatches():
    """the records the model gets wrong, by function"""
    index, words = D.fixture()
    bad = {'log2': 0, 'fft': 0, 'detect': 0, 'sf': 0, 'alloc': 0}
    pairs = D.span(words, index['log2']).reshape(-1, 2)
    bad['log2'] = sum(not D.same([D.log2(x)], [y]) for x, y in pairs)
    for r in index['fft']:
        bad['fft'] += not D.same(D.perform_fft(D.span(words, r['x']), r['n'], D.span(words, r['w'])), D.span(words, r['y']))
    for r in index['detect']:
        prev = None if r['p'] is None else D.span(words, r['p'])
        flag, score = D.detect(D.span(words, r['c']), prev, words[r['t']])
        bad['detect'] += flag != r['r'] or not D.same([score], [words[r['s']]])
    for r in index['sf']:
        bad['sf'] += D.find_scale_factor(D.span(words, r['x']), r['len']) != r['r']
    for r in index['alloc']:
        count, wl, sfi, fallback = D.allocate(*D.alloc_record(index, words, r))
        n_sfi = 52 if fallback else r['mb']
        bad['alloc'] += (count != r['count'] or list(wl[:count]) != r['wl'] or list(sfi[:n_sfi]) != r['sfi'] or
                         len(r['sfi']) != n_sfi or any(wl[count:]) or any(sfi[n_sfi:]))
    return bad


def test_fixture_covers_the_issue_domain():
    index, words = D.fixture()
    assert {r['n'] for r in index['fft']} == {1 << k for k in range(13)}
    assert any(r['p'] is None for r in index['detect']) and any(r['p'] is not None and r['p'][1] == 0 for r in index['detect'])
    assert any(r['p'] is not None and 0 < r['p'][1] < r['c'][1] for r in index['detect'])
    assert any(r['p'] is not None and r['p'][1] > r['c'][1] for r in index['detect'])
    assert any(np.isnan(words[r['s']]) and r['p'] is not None for r in index['detect'])
    assert {r['name'] for r in index['sf']} >= {'boundary_f64', 'boundary_f32', 'inf', 'beyond', 'negative_length'}
    assert sum(r['name'] == 'boundary_f64' for r in index['sf']) == 64 * 9
    assert {r['bias'] for r in index['alloc']} >= {0, 1, 2, 3, 4, 5}
    mbs = {r['mb'] for r in index['alloc']}
    assert 0 in mbs and 52 in mbs and any(m < 20 for m in mbs)
    sizes = [s for r in index['alloc'] for s in r['sizes']]
    assert min(sizes) < 0 and max(sizes) > 20 and 0 in sizes
    assert any(len(r['sfi']) == 52 and r['mb'] != 52 for r in index['alloc'])          # the fallback's shape


def test_model_reproduces_every_record():
    D.broken(0)
    assert mismatches() == {'log2': 0, 'fft': 0, 'detect': 0, 'sf': 0, 'alloc': 0}


@pytest.mark.parametrize('mode,which', [(1, 'alloc'), (2, 'detect'), (3, 'log2'), (4, 'fft'), (5, 'alloc')])
def test_broken_model_fails(mode, which):
    D.broken(mode)
    try:
        assert mismatches()[which] > 0
    finally:
        D.broken(0)
