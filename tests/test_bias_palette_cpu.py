"""CPU-only: the allocation bias supplied per frame and channel from a palette.  The oracle helper of the GPU tests against the
reference's own bytes under per-frame allocationBias changes (tests/golden/option_changes.json); the condition on the test
material (the biases must be told apart by the units they produce, or a wrong entry would pass unseen); the palette helper of
the Python host; and the three new entry points in the built library, with the checks they make before they need a device."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

import bias_palette_lib as BP
import block_modes_lib as BM
import oracle_lib as O
import option_changes_lib as OC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = OC.fixture()
CASES = [(name, sig) for name, s in FIX['schedules'].items() for sig in s['results']]
C1_OK, C1_ERR_ARG = 0, 1   # include/carta1_hip.h


@pytest.mark.parametrize('sig', list(FIX['schedules']['bias_fixed000']['results']))
def test_helper_reproduces_the_bias_schedule_of_the_fixture(sig):
    """bias 1, then 0.5 at frame 32, then 2 at frame 64, under fixedBlockModes [0,0,0]: as a palette and an index, with the
    modes from the options and as given mode bytes"""
    s = FIX['schedules']['bias_fixed000']
    frames = FIX['frames']
    chans = OC.signal(FIX['signals'][sig], frames)
    nch = len(chans)
    per_frame = OC.options_at(s['initial'], s['changes'], frames)
    values, index = BP.palette_of(np.repeat(np.array([v['allocationBias'] for v in per_frame])[:, None], nch, axis=1))
    assert values == [0.5, 1.0, 2.0] and index[0].tolist() == [1] * nch and index[32].tolist() == [0] * nch and index[64].tolist() == [2] * nch
    units, _ = BP.oracle_encode_schedule(chans, values, index, None, {'fixedBlockModes': [0, 0, 0]})
    assert OC.check_against(s['results'][sig], units, nch) is None
    units, _ = BP.oracle_encode_schedule(chans, values, index, np.zeros((frames, nch), dtype=np.uint8))
    assert OC.check_against(s['results'][sig], units, nch) is None


@pytest.mark.parametrize('name,sig', CASES, ids=['%s-%s' % c for c in CASES])
def test_stream_model_reproduces_the_fixture(name, sig):
    """every schedule (every_frame changes bias, threshold and modes before each frame) as the steps of one stream whose
    bias comes through the pushes alone"""
    s = FIX['schedules'][name]
    frames = FIX['frames']
    chans = OC.signal(FIX['signals'][sig], frames)
    per_frame = OC.options_at(s['initial'], s['changes'], frames)
    for split in (None, 5):
        steps = BP.plan(per_frame, len(chans), split)
        assert all(set(st[1]) == {'transientThresholdLow', 'fixedBlockModes'} and st[1]['fixedBlockModes'] is None for st in steps if st[0] == 'options')
        units, _ = BP.run_plan_on_oracle(chans, steps)
        err = OC.check_against(s['results'][sig], units, len(chans))
        assert err is None, (err, split)


@pytest.mark.parametrize('modes', [(0, 0, 0), (2, 2, 3), None], ids=['000', '223', 'detect'])
def test_material_tells_the_packaged_biases_apart(modes):
    """On pink noise with transients every pair of the eight packaged biases differs in at least three quarters of the units
    of each channel (measured: at least 108 of 130), so a unit allocated under a wrong entry shows.  White noise does not do
    that: 0.25 against 0.5 gives identical units for all 96 frames of gen_white(1), 0.5 against 1 differs in 7."""
    frames = 130
    for seed in (3, 4):
        ch = [O.gen_pinkT(seed, frames * 512)]
        units = {b: O.encode_stream(ch, fixed_modes=modes, bias=b)[0] for b in BP.PACKAGED_BIASES}
        for a, b in itertools.combinations(BP.PACKAGED_BIASES, 2):
            assert BP.differing_units(units[a], units[b]) * 4 >= frames * 3, (seed, a, b, BP.differing_units(units[a], units[b]))
    white = [O.gen_white(1, 96 * 512)]
    w = {b: O.encode_stream(white, fixed_modes=modes, bias=b)[0] for b in (0.25, 0.5, 1)}
    assert BP.differing_units(w[0.25], w[0.5]) == 0 and BP.differing_units(w[0.5], w[1]) < 96 // 4


def test_random_schedules_use_every_entry_and_differ_between_channels():
    idx = BP.random_index(20261018, 130, 2, 8)
    assert set(idx.reshape(-1).tolist()) == set(range(8)) and (idx[:, 0] != idx[:, 1]).any()
    runs = [len(list(g)) for c in range(2) for _, g in itertools.groupby(idx[:, c].tolist())]
    assert min(runs) >= 1 and max(runs) > 1
    assert BP.pattern_index('cycle', 7, 3).tolist() == [0, 1, 2, 0, 1, 2, 0]
    assert BP.pattern_index('last', 4, 3).tolist() == [2, 2, 2, 2]
    assert BP.pattern_index('single', 5, 3).tolist() == [2, 2, 0, 2, 2]


def test_python_palette_helper():
    from carta1_amd import codec
    pal, idx = codec.bias_palette([1, 0.5, 2, 0.5], 4, 2)
    assert len(pal) == 3 and idx.dtype == np.uint8 and idx.tolist() == [1, 1, 0, 0, 2, 2, 0, 0]
    for k, b in enumerate((0.5, 1.0, 2.0)):
        assert np.array_equal(np.array(pal[k].biased_scale_factors[:]), O.biased_table(b))
        assert list(pal[k].fixed_block_modes[:]) == [-1, -1, -1] and pal[k].transient_threshold == 1.0
    pal, idx = codec.bias_palette(np.array([[1, 2], [2, 1]]), 2, 2, codec.EncoderOptions({'fixedBlockModes': [2, 0, 3], 'transientThresholdLow': 0.5, 'allocationBias': 3.3}))
    assert len(pal) == 2 and idx.tolist() == [0, 1, 1, 0]
    assert all(list(p.fixed_block_modes[:]) == [2, 0, 3] and p.transient_threshold == 0.5 for p in pal)
    pal, idx = codec.bias_palette(BP.PACKAGED_BIASES, 8, 1)
    assert len(pal) == 8 and idx.tolist() == list(range(8))
    with pytest.raises(ValueError, match='at most 8 distinct'):
        codec.bias_palette(np.arange(9) * 0.5, 9, 1)
    with pytest.raises(ValueError, match='allocationBias must be between'):
        codec.bias_palette([1, 5.5], 2, 1)
    with pytest.raises(ValueError, match='frames'):
        codec.bias_palette([1, 1, 1], 2, 2)
    pal, idx = codec.bias_palette([], 0, 2)
    assert len(pal) == 1 and idx.size == 0


def test_entry_points_are_exported_declared_and_bound():
    from carta1_amd import build, capi
    build.build_library()
    lib = capi.load()
    header = open(os.path.join(ROOT, 'include', 'carta1_hip.h')).read()
    opts_p = C.POINTER(capi.EncodeOptions)
    call = [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_int64, C.c_int, opts_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    want = {
        'c1_encode_biases_device': call,
        'c1_encode_biases_batch': call,
        'c1_enc_stream_push_biases': [C.c_void_p, C.POINTER(C.c_void_p), C.c_int64, opts_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p],
    }
    for name, args in want.items():
        assert hasattr(lib, name), 'library does not export ' + name
        assert capi.SIGNATURES[name] == (C.c_int, args), name
        decl = re.search(r'^int %s\(([^;]*)\);' % name, header, re.M | re.S)
        assert decl, 'header does not declare ' + name
        params = [p for p in re.sub(r'/\*.*?\*/', '', decl.group(1), flags=re.S).split(',')]
        assert len(params) == len(args), (name, params)
        assert 'const c1_encode_options *palette' in decl.group(1) and 'const uint8_t *bias_index' in decl.group(1)
    assert re.search(r'^#define C1_MAX_BIAS_PALETTE 8$', header, re.M)
    assert lib.c1_abi_version() == 3


def test_argument_checks_that_need_no_device():
    """the batch and device calls look at their context first, as c1_encode_modes_* do; the stream call validates its palette
    before it looks at the stream: all of it C1_ERR_ARG, with or without a device"""
    from carta1_amd import build, capi, codec
    build.build_library()
    lib = capi.load()
    pal = codec.palette_array([codec.EncoderOptions({'allocationBias': b}).to_c() for b in BP.PACKAGED_BIASES] + [codec.EncoderOptions().to_c()])
    for fn in (lib.c1_encode_biases_batch, lib.c1_encode_biases_device):
        assert fn(None, None, 1, 4, 0, pal, 2, None, None, None) == C1_ERR_ARG
        assert 'context is NULL' in lib.c1_last_error().decode()
    for n in (0, 9, -1):
        assert lib.c1_enc_stream_push_biases(None, None, 4, pal, n, None, None, None) == C1_ERR_ARG
        msg = lib.c1_last_error().decode()
        assert 'n_palette = %d' % n in msg and '1..8' in msg, msg
    assert lib.c1_enc_stream_push_biases(None, None, 4, None, 3, None, None, None) == C1_ERR_ARG
    assert 'palette is NULL' in lib.c1_last_error().decode()
    bad = codec.palette_array([pal[k] for k in range(4)])
    bad[2].biased_scale_factors[17] = float('nan')
    assert lib.c1_enc_stream_push_biases(None, None, 4, bad, 4, None, None, None) == C1_ERR_ARG
    msg = lib.c1_last_error().decode()
    assert 'palette entry 2' in msg and 'biased_scale_factors[17]' in msg, msg
    assert lib.c1_enc_stream_push_biases(None, None, 4, bad, 2, None, None, None) == C1_ERR_ARG      # entry 2 is not part of this palette
    assert 'bias_index is NULL' in lib.c1_last_error().decode()
    idx = np.zeros(4, dtype=np.uint8)
    assert lib.c1_enc_stream_push_biases(None, None, 4, pal, 8, idx.ctypes.data, None, None) == C1_ERR_ARG
    assert 'stream is NULL' in lib.c1_last_error().decode()
