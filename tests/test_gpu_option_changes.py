"""c1_enc_stream_set_options on the device: a stream whose options change between pushes gives the reference's encode()
closures' bytes under the same changes (tests/golden/option_changes.json) and the CPU oracle's on random schedules."""
import ctypes as C
import math
import random

import numpy as np
import pytest

import carta1_amd as c1
from carta1_amd import capi
import oracle_lib as O
import option_changes_lib as OC

pytestmark = pytest.mark.gpu

C1_ERR_ARG = 1   # include/carta1_hip.h

FIX = OC.fixture()
CASES = [(name, sig) for name, s in FIX['schedules'].items() for sig in s['results']]

BIASES = [0, 0.25, 0.5, 1, 1.5, 2, 3.3, 5]
THRESHOLDS = [0.3, 0.5, 1.0, 1.5, 2.0]
MODES = [None, None, None, [0, 0, 0], [2, 2, 3], [2, 0, 3], [0, 2, 0], [0, 0, 3]]


@pytest.fixture(scope='module')
def ctx():
    c = c1.Context(0)
    yield c
    c.close()


def opts(v):
    return c1.EncoderOptions(v)


def run_stream(ctx, chans, per_frame, pushes, create_with=None):
    """pushes: frame counts summing to the signal; options are set before a push whenever the frame it starts at has other
    values than the stream's (a change inside a push splits it, as a frame closure would see it).  create_with: options to
    create the stream with, replaced before the first push"""
    nch = len(chans)
    s = c1.EncoderStream(ctx, nch, opts(per_frame[0] if create_with is None else create_with))
    cur = per_frame[0]
    out = []
    at = 0
    try:
        if create_with is not None:
            s.set_options(opts(cur))
        for n in pushes:
            while n > 0:
                if per_frame[at] != cur:
                    cur = per_frame[at]
                    s.set_options(opts(cur))
                k = 1
                while k < n and per_frame[at + k] == cur:
                    k += 1
                out.append(s.push([c[at * 512:(at + k) * 512] for c in chans]))
                at += k
                n -= k
    finally:
        s.close()
    return np.concatenate(out)


@pytest.mark.parametrize('name,sig', CASES, ids=['%s-%s' % c for c in CASES])
def test_stream_matches_reference_schedule(ctx, name, sig):
    s = FIX['schedules'][name]
    frames = FIX['frames']
    chans = OC.signal(FIX['signals'][sig], frames)
    per_frame = OC.options_at(s['initial'], s['changes'], frames)
    units = run_stream(ctx, chans, per_frame, [frames])
    err = OC.check_against(s['results'][sig], units, len(chans))
    assert err is None, err


@pytest.mark.parametrize('name', ['detect_000_223_detect', 'every_frame', 'fixed000_then_detect'])
def test_split_into_pushes_differently(ctx, name):
    s = FIX['schedules'][name]
    frames = FIX['frames']
    chans = OC.signal(FIX['signals']['pinkT34'], frames)
    per_frame = OC.options_at(s['initial'], s['changes'], frames)
    want = run_stream(ctx, chans, per_frame, [frames])
    for pushes in ([1] * frames, [7, 1, 30, 2, 56], [frames - 1, 1], [3] * 32):
        got = run_stream(ctx, chans, per_frame, pushes)
        assert np.array_equal(got, want), pushes
    assert OC.check_against(s['results']['pinkT34'], want, 2) is None


def random_values(rng):
    return {'transientThresholdLow': rng.choice(THRESHOLDS), 'allocationBias': rng.choice(BIASES),
            'fixedBlockModes': rng.choice(MODES)}


def random_schedule(rng, k):
    """per-frame options and push sizes 1..70; every fourth schedule switches after its first frame (a push of one frame)"""
    pushes = [rng.randint(1, 70) if rng.random() < 0.5 else rng.randint(1, 8) for _ in range(rng.randint(1, 5))]
    if k % 4 == 1:
        pushes = [1] + pushes
    starts = set(np.cumsum([0] + pushes[:-1]).tolist())
    per_frame = []
    cur = random_values(rng)
    for f in range(sum(pushes)):
        if (f in starts and rng.random() < 0.6) or rng.random() < 0.04 or (k % 4 == 1 and f == 1):
            cur = random_values(rng) if rng.random() < 0.8 else dict(cur)
        per_frame.append(cur)
    return per_frame, pushes


def test_random_schedules_match_oracle(ctx):
    """240 schedules, mono and stereo; every fourth stream is created under other options and switched before its first push"""
    rng = random.Random(20261016)
    for k in range(240):
        per_frame, pushes = random_schedule(rng, k)
        frames = len(per_frame)
        nch = 1 + (k % 3 == 0)
        gen = O.gen_pinkT if k % 2 else O.gen_white
        chans = [gen(100 + k + c, frames * 512) for c in range(nch)]
        want = OC.oracle_encode(chans, per_frame)
        got = run_stream(ctx, chans, per_frame, pushes, create_with=random_values(rng) if k % 4 == 2 else None)
        if not np.array_equal(got, want):
            bad = np.nonzero(np.any(got != want, axis=1))[0]
            pytest.fail('schedule %d (%d ch, pushes %s): first differing unit %d; options there %s' %
                        (k, nch, pushes, bad[0], per_frame[bad[0] // nch]))


@pytest.mark.parametrize('values', [{}, {'fixedBlockModes': [2, 0, 3], 'allocationBias': 0.5},
                                    {'transientThresholdLow': 0.5, 'allocationBias': 3.3}])
def test_unchanged_options_are_a_no_op(ctx, values):
    frames = 80
    chans = [O.gen_pinkT(7, frames * 512), O.gen_white(8, frames * 512)]
    want = ctx.encode(chans, opts(values))
    s = c1.EncoderStream(ctx, 2, opts(values))
    try:
        out = []
        for a, b in ((0, 1), (1, 17), (17, 18), (18, 50), (50, 80)):
            s.set_options(opts(values))
            s.set_options(opts(values))
            out.append(s.push([c[a * 512:b * 512] for c in chans]))
        assert np.array_equal(np.concatenate(out), want)
    finally:
        s.close()
    never = c1.EncoderStream(ctx, 2, opts(values))
    try:
        got = np.concatenate([never.push([c[a * 512:b * 512] for c in chans]) for a, b in ((0, 33), (33, 80))])
        assert np.array_equal(got, want)
    finally:
        never.close()


def test_argument_errors_leave_the_stream_usable(ctx):
    lib = capi.load()
    frames = 48
    chans = [O.gen_pinkT(11, frames * 512)]
    per_frame = [{'transientThresholdLow': 1.0, 'allocationBias': 1.0, 'fixedBlockModes': None}] * 20 + \
                [{'transientThresholdLow': 1.0, 'allocationBias': 1.0, 'fixedBlockModes': [0, 0, 0]}] * 10 + \
                [{'transientThresholdLow': 0.5, 'allocationBias': 1.0, 'fixedBlockModes': None}] * 18
    want = OC.oracle_encode(chans, per_frame)
    s = c1.EncoderStream(ctx, 1, opts(per_frame[0]))
    try:
        a = s.push([chans[0][:20 * 512]])
        bad_mode = opts({}).to_c()
        bad_mode.fixed_block_modes[0], bad_mode.fixed_block_modes[1], bad_mode.fixed_block_modes[2] = 0, 0, 4
        bad_threshold = opts({'fixedBlockModes': [0, 0, 0]}).to_c()
        bad_threshold.transient_threshold = math.nan
        bad_table = opts({'fixedBlockModes': [0, 0, 0]}).to_c()
        bad_table.biased_scale_factors[5] = -1.0
        for bad in (bad_mode, bad_threshold, bad_table):
            assert lib.c1_enc_stream_set_options(s._h, C.byref(bad)) == C1_ERR_ARG
        assert lib.c1_enc_stream_set_options(s._h, None) == C1_ERR_ARG
        assert lib.c1_enc_stream_set_options(None, C.byref(bad_mode)) == C1_ERR_ARG
        with pytest.raises(capi.Carta1Error):
            s.set_options(opts({'fixedBlockModes': [0, 3, 0]}))
        s.set_options(opts(per_frame[20]))
        b = s.push([chans[0][20 * 512:30 * 512]])
        with pytest.raises(capi.Carta1Error):
            s.set_options(opts({'fixedBlockModes': [9, 9, 9]}))
        s.set_options(opts(per_frame[30]))
        c = s.push([chans[0][30 * 512:]])
        assert np.array_equal(np.concatenate([a, b, c]), want)
    finally:
        s.close()
