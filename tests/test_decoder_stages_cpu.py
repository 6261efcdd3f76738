"""CPU: the decoder's stage entry points (c1_unpack_units, c1_dequantize_frames, c1_imdct_batch, c1_qmf_synthesis_batch) are
declared, exported and bound, and the reference's stage outputs in tests/golden/decoder_stages.json are reproduced by a second
implementation, the CPU oracle: its unit parser gives the fixture's fields, its decoder the fixture's PCM."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import decoder_stages_golden as DG
import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('c1_unpack_units', 'c1_dequantize_frames', 'c1_imdct_batch', 'c1_qmf_synthesis_batch')
CASES = DG.cases()


def test_stage_symbols_declared_exported_and_bound():
    from carta1_amd import build, capi
    build.build_library()
    lib = capi.load()
    header = open(os.path.join(ROOT, 'include', 'carta1_hip.h')).read()
    for name in NAMES:
        assert re.search(r'^int %s\(' % name, header, re.M), name
        assert hasattr(lib, name), name
        assert name in capi.SIGNATURES, name
    import carta1_amd as c1
    for method in ('unpack_units', 'dequantize_frames', 'imdct', 'qmf_synthesis'):
        assert callable(getattr(c1.Context, method, None)), method


def test_fixture_covers_what_it_claims():
    pink, white, fields = CASES['pinkT_detect'], CASES['white_m000_b1'], CASES['fields']
    assert (pink['block_modes'] != 0).all(axis=1).any()            # short blocks in every band
    assert (white['block_modes'] == 0).all()
    n = fields['nbfu']
    assert 0 in n and 1 in n and not set(n.tolist()) <= {20, 28, 32, 36, 40, 44, 48, 52}
    assert (fields['block_modes'][:, :2] == 1).any(axis=0).all()
    active = np.arange(52)[None, :] < n[:, None]
    assert (fields['sfi'][active] == 0).any() and (fields['sfi'][active] == 63).any()
    wl = fields['wl'][active]
    assert (wl == 0).any() and (wl > 0).any()
    assert fields['quantized'].min() < -(1 << 30)


@pytest.mark.parametrize('name', ['pinkT_detect', 'white_m000_b1'])
def test_oracle_unpacks_the_fixture_fields(name):
    case = CASES[name]
    for f in range(case['meta']['frames']):
        o = O.unpack_unit(case['units'][f])
        assert o.nbfu == case['nbfu'][f]
        assert list(o.modes) == case['block_modes'][f].tolist()
        assert list(o.wl) == case['wl'][f].tolist()
        assert list(o.sfi) == case['sfi'][f].tolist()
        assert list(o.q) == case['quantized'][f].tolist()


@pytest.mark.parametrize('name', sorted(CASES))
def test_oracle_decodes_the_fixture_fields_to_the_fixture_pcm(name):
    case = CASES[name]
    st = O.DecState()
    for f in range(case['meta']['frames']):
        fl = O.Fields()
        fl.nbfu = int(case['nbfu'][f])
        fl.modes[:] = case['block_modes'][f].tolist()
        fl.wl[:] = case['wl'][f].tolist()
        fl.sfi[:] = case['sfi'][f].tolist()
        fl.q[:] = case['quantized'][f].tolist()
        pcm = np.zeros(512, dtype=np.float32)
        O.lib().c1o_decode_frame(C.byref(st), C.byref(fl), pcm.ctypes.data_as(C.POINTER(C.c_float)))
        assert np.array_equal(pcm.view(np.uint32), case['pcm'][f].view(np.uint32)), 'frame %d' % f
