"""CPU-only: block modes supplied per frame by the caller.  The mode-byte helpers and their validation; on the oracle, the
property the main GPU test rests on (a detection run's own modes, fed back frame by frame as fixedBlockModes, reproduce its
units and its states but for the detection history); the model of the GPU stream tests against the reference's bytes under
per-frame fixedBlockModes changes (tests/golden/option_changes.json); and the three new entry points in the built library."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import block_modes_lib as BM
import option_changes_lib as OC
import stream_state_lib as SL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = OC.fixture()
CASES = [(name, sig) for name, s in FIX['schedules'].items() for sig in s['results']]


def test_pack_unpack_round_trip_over_the_domain():
    import carta1_amd as c1
    assert sorted(BM.DOMAIN_BYTES) == [0x00, 0x02, 0x08, 0x0a, 0x30, 0x32, 0x38, 0x3a]
    packed = c1.pack_block_modes(BM.DOMAIN_TRIPLES)
    assert packed.dtype == np.uint8 and packed.tolist() == BM.DOMAIN_BYTES
    assert c1.unpack_block_modes(packed).tolist() == [list(t) for t in BM.DOMAIN_TRIPLES]
    assert c1.pack_block_modes((2, 0, 3)).tolist() == [0x32]
    assert c1.unpack_block_modes(np.array([[0x32, 0x08]], dtype=np.uint8)).tolist() == [[2, 0, 3], [0, 2, 0]]
    assert np.array_equal(c1.check_block_modes(packed, 4, 2), packed)
    assert np.array_equal(c1.check_block_modes(packed.reshape(4, 2), 4, 2), packed)


def _field_of(b):
    """the first field of a byte outside the domain, as the messages name it"""
    for k, name in enumerate(('low', 'mid', 'high')):
        if (b >> (2 * k)) & 3 not in (0, 3 if k == 2 else 2):
            return name + ' field'
    return 'bits 6-7'


def test_every_byte_outside_the_domain_is_rejected_with_its_position():
    import carta1_amd as c1
    outside = [b for b in range(256) if b not in BM.DOMAIN_BYTES]
    assert len(outside) == 248
    for b in outside:
        for nch, at in ((1, 0), (1, 6), (2, 0), (2, 13)):
            m = np.zeros((7, nch), dtype=np.uint8)
            m.reshape(-1)[at] = b
            with pytest.raises(ValueError) as e:
                c1.check_block_modes(m, 7, nch)
            msg = str(e.value)
            assert 'frame %d' % (at // nch) in msg and _field_of(b) in msg and '0x%02x' % b in msg, (b, msg)
            assert ('channel %d' % (at % nch) in msg) == (nch == 2), (b, msg)
    with pytest.raises(ValueError):
        c1.check_block_modes(np.zeros(5, dtype=np.uint8), 3, 2)


@pytest.mark.parametrize('gen,seed', [('pinkT', 3), ('pinkT', 4), ('white', 1), ('white', 2)])
def test_own_modes_reproduce_detection_on_the_oracle(gen, seed):
    frames = 96
    chans = OC.signal([[gen, seed]], frames)
    want, want_state = SL.oracle_encode(chans, {})
    modes = BM.modes_of_units(want)
    if gen == 'pinkT':
        assert 0 < np.count_nonzero(modes) < frames              # long and short units both
    per_frame = [{'transientThresholdLow': 1.0, 'allocationBias': 1.0, 'fixedBlockModes': list(BM.triple_of(int(b)))} for b in modes]
    assert np.array_equal(OC.oracle_encode(chans, per_frame), want)
    got, state = BM.oracle_encode_modes(chans, modes)
    assert np.array_equal(got, want)
    assert not state[:, BM.MAGS].any() and want_state[:, BM.MAGS].any()      # the detector never ran
    state[:, BM.MAGS] = want_state[:, BM.MAGS]
    assert np.array_equal(SL.bits(state), SL.bits(want_state))


@pytest.mark.parametrize('name,sig', CASES, ids=['%s-%s' % c for c in CASES])
def test_stream_model_reproduces_the_fixture(name, sig):
    s = FIX['schedules'][name]
    frames = FIX['frames']
    chans = OC.signal(FIX['signals'][sig], frames)
    per_frame = OC.options_at(s['initial'], s['changes'], frames)
    for split in (None, 5):
        steps = BM.plan(per_frame, len(chans), split)
        assert not any(st[0] == 'options' and st[1]['fixedBlockModes'] is not None for st in steps)
        units, _ = BM.run_plan_on_oracle(chans, steps)
        err = OC.check_against(s['results'][sig], units, len(chans))
        assert err is None, (err, split)


def test_per_channel_modes_equal_separate_mono_streams():
    frames = 40
    chans = OC.signal([['pinkT', 3], ['white', 2]], frames)
    m = BM.random_modes(5, frames, 2)
    assert (m[:, 0] != m[:, 1]).any()
    units, states = BM.oracle_encode_modes(chans, m, 0.5)
    for c in range(2):
        per_frame = [{'transientThresholdLow': 1.0, 'allocationBias': 0.5, 'fixedBlockModes': list(BM.triple_of(int(b)))} for b in m[:, c]]
        assert np.array_equal(units[c::2], OC.oracle_encode([chans[c]], per_frame))


def test_entry_points_are_exported_declared_and_bound():
    from carta1_amd import build, capi
    build.build_library()
    lib = capi.load()
    header = open(os.path.join(ROOT, 'include', 'carta1_hip.h')).read()
    opts_p = C.POINTER(capi.EncodeOptions)
    want = {
        'c1_encode_modes_device': [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_int64, C.c_int, opts_p, C.c_void_p, C.c_void_p],
        'c1_encode_modes_batch': [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_int64, C.c_int, opts_p, C.c_void_p, C.c_void_p],
        'c1_enc_stream_push_modes': [C.c_void_p, C.POINTER(C.c_void_p), C.c_int64, C.c_void_p, C.c_void_p],
    }
    for name, args in want.items():
        assert hasattr(lib, name), 'library does not export ' + name
        assert capi.SIGNATURES[name] == (C.c_int, args), name
        decl = re.search(r'^int %s\(([^;]*)\);' % name, header, re.M | re.S)
        assert decl, 'header does not declare ' + name
        params = [p for p in re.sub(r'/\*.*?\*/', '', decl.group(1), flags=re.S).split(',')]
        assert len(params) == len(args), (name, params)
        assert 'const uint8_t *modes' in decl.group(1)
    assert lib.c1_abi_version() == 3
