"""Stream state in the reference's BufferPool layout, without a device: the CPU oracle's states ARE the reference's dumped pools
(tests/golden/stream_state.json, gen_stream_state.mjs) and the oracle started from any of them -- foreign pools included --
reproduces what the reference's encode() / decode() computed from them.  That pins the yardstick the GPU tests use.  Then
the new ABI: symbols, struct sizes, and NULL arguments rejected before any device is touched."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
import stream_state_lib as SS

FIX = SS.fixture()
CASES = sorted(FIX['cases'])
DUMP, MORE = FIX['dump_at'], FIX['more']
C1_ERR_ARG = 1   # include/carta1_hip.h


def case_parts(name):
    sig, oname = name.split('/')
    return SS.signal(FIX['signals'][sig], DUMP + MORE), FIX['option_sets'][oname]


@pytest.mark.parametrize('name', CASES)
def test_oracle_states_are_the_reference_pools(name):
    chans, oset = case_parts(name)
    e = FIX['cases'][name]
    u5, st = SS.oracle_encode([c[:DUMP * 512] for c in chans], oset)
    assert np.array_equal(SS.bits(st), SS.bits(SS.states(e['enc_states'], SS.ENC_FLOATS)))
    _, dst = SS.oracle_decode(u5, len(chans))
    assert np.array_equal(SS.bits(dst), SS.bits(SS.states(e['dec_states'], SS.DEC_FLOATS)))


@pytest.mark.parametrize('name', CASES)
def test_oracle_continues_from_the_dumped_pools(name):
    chans, oset = case_parts(name)
    e = FIX['cases'][name]
    more, _ = SS.oracle_encode([c[DUMP * 512:] for c in chans], oset, SS.states(e['enc_states'], SS.ENC_FLOATS))
    assert np.array_equal(more, SS.units(e['units_more']))
    pcm, _ = SS.oracle_decode(SS.units(e['units_more']), len(chans), SS.states(e['dec_states'], SS.DEC_FLOATS))
    assert SS.pcm_sha(pcm, 0, MORE) == e['pcm_sha256']


def test_foreign_recipe_is_the_recorded_pool():
    f = FIX['foreign']
    for e in f['enc'].values():
        assert np.array_equal(SS.bits(SS.foreign_enc_state(f['enc_seed'])), SS.bits(SS.states(e['enc_state'], SS.ENC_FLOATS)))
    assert np.array_equal(SS.bits(SS.foreign_dec_state(f['dec_seed'])), SS.bits(SS.states(f['dec']['dec_state'], SS.DEC_FLOATS)))


@pytest.mark.parametrize('oname', sorted(FIX['foreign']['enc']))
def test_oracle_encodes_from_a_foreign_pool(oname):
    f = FIX['foreign']
    e = f['enc'][oname]
    x = SS.signal(f['pcm'], f['frames'])
    u, st = SS.oracle_encode(x, e['options'], SS.states(e['enc_state'], SS.ENC_FLOATS))
    assert np.array_equal(u, SS.units(e['units']))
    assert np.array_equal(SS.bits(st), SS.bits(SS.states(e['enc_state_end'], SS.ENC_FLOATS)))


def test_oracle_decodes_from_a_foreign_pool():
    d = FIX['foreign']['dec']
    pcm, st = SS.oracle_decode(SS.units(d['units']), 1, SS.states(d['dec_state'], SS.DEC_FLOATS))
    assert np.array_equal(SS.bits(pcm[0]), SS.bits(SS.blob(d['pcm'], np.float32)))
    assert np.array_equal(SS.bits(st), SS.bits(SS.states(d['dec_state_end'], SS.DEC_FLOATS)))


@pytest.mark.parametrize('sig', sorted(FIX['switch']['results']))
def test_oracle_follows_the_switch_schedule_from_the_dump(sig):
    s = FIX['switch']['schedule']
    r = FIX['switch']['results'][sig]
    chans = SS.signal(FIX['signals'][sig], s['frames'])
    fixed, detect = {'fixedBlockModes': s['fixed_modes']}, {}
    # from a fresh pool up to the dump: the oracle's pool under fixed modes carries the kept spectrum
    _, st = SS.oracle_encode([c[:s['fixed_from'] * 512] for c in chans], detect)
    _, st = SS.oracle_encode([c[s['fixed_from'] * 512:s['dump_at'] * 512] for c in chans], fixed, st)
    dumped = SS.states(r['enc_states'], SS.ENC_FLOATS)
    assert np.array_equal(SS.bits(st), SS.bits(dumped))
    assert np.any(dumped[:, 227:] != 0)
    # and from the dump on
    a, st = SS.oracle_encode([c[s['dump_at'] * 512:s['detect_from'] * 512] for c in chans], fixed, dumped)
    b, _ = SS.oracle_encode([c[s['detect_from'] * 512:] for c in chans], detect, st)
    assert np.array_equal(np.concatenate([a, b]), SS.units(r['units_from_dump']))


# ---- the ABI, no device ----
NEW_SYMBOLS = ['c1_encode_frames_from_states_device', 'c1_encode_frames_from_states', 'c1_decode_frames_from_states_device',
               'c1_decode_frames_from_states', 'c1_enc_stream_get_state', 'c1_enc_stream_set_state', 'c1_dec_stream_get_state',
               'c1_dec_stream_set_state']


def test_new_symbols_are_exported():
    from carta1_amd import capi
    lib = capi.load()
    for name in NEW_SYMBOLS:
        assert name in capi.SIGNATURES
        assert getattr(lib, name) is not None


def test_state_struct_sizes():
    from carta1_amd import capi
    assert C.sizeof(capi.EncState) == 1932 == 4 * SS.ENC_FLOATS == C.sizeof(O.EncState)
    assert C.sizeof(capi.DecState) == 716 == 4 * SS.DEC_FLOATS == C.sizeof(O.DecState)
    # field order is the oracle's, so one copies into the other
    assert [n for n, _ in capi.EncState._fields_] == ['qmf_low', 'qmf_mid', 'qmf_high', 'mdct_overlap', 'transient_mags']
    assert [n for n, _ in capi.DecState._fields_] == ['qmf_low', 'qmf_mid', 'qmf_high', 'imdct_tail']
    assert [C.sizeof(t) for _, t in capi.EncState._fields_] == [C.sizeof(t) for _, t in O.EncState._fields_]
    assert [C.sizeof(t) for _, t in capi.DecState._fields_] == [C.sizeof(t) for _, t in O.DecState._fields_]


def test_null_arguments_are_rejected_without_a_device():
    from carta1_amd import capi
    lib = capi.load()
    buf = (C.c_float * 1024)()
    p = C.addressof(buf)
    opts = capi.EncodeOptions()
    assert lib.c1_default_encode_options(C.byref(opts)) == 0
    assert lib.c1_encode_frames_from_states(None, 1, p, p, C.byref(opts), p, p) == C1_ERR_ARG
    assert lib.c1_encode_frames_from_states_device(None, 1, p, p, C.byref(opts), p, p) == C1_ERR_ARG
    assert lib.c1_decode_frames_from_states(None, 1, p, p, p, p) == C1_ERR_ARG
    assert lib.c1_decode_frames_from_states_device(None, 1, p, p, p, p) == C1_ERR_ARG
    for fn in (lib.c1_enc_stream_get_state, lib.c1_enc_stream_set_state, lib.c1_dec_stream_get_state, lib.c1_dec_stream_set_state):
        assert fn(None, p) == C1_ERR_ARG
        assert b'NULL' in lib.c1_last_error()
