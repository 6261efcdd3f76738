"""CPU: c1_pack_units (serializeFrame) is declared, exported and bound; tests/golden/pack_units.json holds every category of
frame fields it claims; and a second implementation, the NumPy model of tests/pack_units_model.py (written from the
semantics include/carta1_hip.h states), reproduces every unit the reference's serializeFrame wrote."""
import os
import re

import numpy as np
import pytest

import pack_units_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = M.cases()
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1


def test_symbol_declared_exported_and_bound():
    from carta1_amd import build, capi
    build.build_library()
    lib = capi.load()
    header = open(os.path.join(ROOT, 'include', 'carta1_hip.h')).read()
    assert re.search(r'^int c1_pack_units\(', header, re.M)
    assert hasattr(lib, 'c1_pack_units')
    assert 'c1_pack_units' in capi.SIGNATURES
    import carta1_amd as c1
    assert callable(getattr(c1.Context, 'pack_units', None))


def test_fixture_covers_what_it_claims():
    kinds = {c['meta']['kind'] for c in CASES.values()}
    assert kinds == {'canonical', 'hand', 'random'}
    pink, white = CASES['kat_pinkT_detect'], CASES['kat_white_m000_b1']
    assert (pink['block_modes'] != 0).all(axis=1).any()            # short blocks in every band
    assert (white['block_modes'] == 0).all()
    assert {'quant_b0.5', 'quant_b1', 'quant_b2'} <= set(CASES)
    h = CASES['hand']
    n = h['nbfu']
    assert {0, 1, 19, 21, 52} <= set(n.tolist())
    assert {1, -1, 5, 7, I32_MIN, I32_MAX} <= set(h['block_modes'].ravel().tolist())
    active = np.arange(52)[None, :] < n[:, None]
    last = np.arange(52)[None, :] == n[:, None] - 1
    wl_mid = h['wl'][active & ~last]                               # in the middle of a frame: BFUs follow them
    assert {16, 31, -1, I32_MIN} <= set(wl_mid.tolist())
    assert {64, -1, I32_MAX} <= set(h['sfi'][active].tolist())
    bits = M.mantissa_bits(n, h['wl'])[:, M.BFU_OF_SLOT]
    live = bits > 0
    q = h['quantized'].astype(np.int64)
    rng = np.where(live, (1 << np.maximum(bits - 1, 0)) - 1, 0)
    assert (live & ((q > rng) | (q < -rng - 1))).any()             # beyond the word length
    assert (live & (q == I32_MIN)).any() and (live & (q == I32_MAX)).any()
    end = M.stream_bits(M.fields_of(h))
    assert (end == 1672).any()
    assert ((end > 1672) & (end < 1696)).any()                      # ends inside the zeroed last three bytes
    far = (n == 52) & (h['wl'] == 15).all(axis=1)
    assert far.any() and (end[far] > 4 * 1696).all()
    r = CASES['random']
    assert r['meta']['frames'] >= 53 and set(range(53)) <= set(r['nbfu'].tolist())


@pytest.mark.parametrize('name', sorted(CASES))
def test_model_reproduces_the_fixture(name):
    case = CASES[name]
    got = M.pack(M.fields_of(case))
    bad = np.nonzero((got != case['units']).any(axis=1))[0]
    assert bad.size == 0, 'first differing frame %d of %d' % (bad[0], bad.size)


def test_model_header_examples():
    """the two header values include/carta1_hip.h gives; the host serializers write ace0 and 4000 for them"""
    assert M.header(np.array([19, 20]), np.array([[0, 0, 0], [1, -2, 7]])).tolist() == [0xffe0, 0xf000]


@pytest.mark.parametrize('name', sorted(k for k, v in CASES.items() if v['meta']['kind'] == 'canonical'))
def test_canonical_mask_covers_canonical_units(name):
    u = CASES[name]['units']
    assert np.array_equal(u & M.canonical_mask(u), u)
