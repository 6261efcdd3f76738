"""GPU: the measured allocation on live streams (c1_enc_stream_push_measured, EncoderStream.push_measured) and the
workgroup-per-unit kernel behind small launches (k_measured_wide, C1_MEASURED_WIDE).  Pushes of any run lengths against the
whole-buffer call on the whole signal, bit for bit, and against the CPU model of tests/masked_alloc_lib.py; given modes, fixed
modes, mono; the stream's state against a twin stream's after plain pushes; the three paths a pushed frame can take (the usual
one, the frames from an explicit state after a restore, the switch frame after an option change); the nesting of the three
whole-buffer calls; the wide kernel against the narrow ones on every output; the rejections; the call shapes.
tests/test_stream_measured_cpu.py and tests/test_masked_alloc_cpu.py show that every decision of the model on this material has
a margin above 1e-9."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

import carta1_amd as c1
from carta1_amd import capi
import best_bias_lib as BB
import best_modes_lib as BMO
import masked_alloc_lib as MK
import stream_measured_lib as SM

pytestmark = pytest.mark.gpu

C1_OK, C1_ERR_ARG = 0, 1   # include/carta1_hip.h
FRAMES = BB.FRAMES
OFFSETS = SM.OFFSETS
OUTPUTS = SM.OUTPUTS
OPTIONAL = OUTPUTS[1:]
FILL = {'units': 0xA5, 'taken': 0xA5, 'shifts': 0x5A, 'distortion': -1.0, 'energy': -1.0, 'weights': -1.0}
RUNS = (1, 1, 1, 2, 3, 5, 8, 13, 32, 64)         # 130 frames
SHORT = 48                                       # frames of the models under given modes (tests/test_gpu_masked_alloc.py's)
WIDE_UNITS = 8192                                # kMeasuredWideUnits (csrc/c1_internal.h): launches up to it take the wide kernel
same, rows = SM.same, SM.rows


def opts(v=None):
    return c1.EncoderOptions(v or {})


def _context(stream=None, **env_vars):
    old = {k: os.environ.get(k) for k in env_vars}
    os.environ.update({k: str(v) for k, v in env_vars.items()})
    try:
        return c1.Context(0, stream=stream)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


@pytest.fixture(scope='module')
def ctx():
    c = c1.Context(0)
    yield c
    c.close()


@pytest.fixture(scope='module')
def pink():
    return BMO.material('pink')


@pytest.fixture(scope='module')
def white():
    return BMO.material('white')


def frozen(d):
    for a in d.values():
        a.setflags(write=False)
    return d


def whole_call(c, chans, **kw):
    """Context.encode_measured under the packaged tables and OFFSETS, all six outputs"""
    return SM.as_dict(c.encode_measured(chans, return_distortion=True, scale_factor_offsets=OFFSETS, return_shifts=True, masking=True,
                                        return_weights=True, **kw))


@pytest.fixture(scope='module')
def whole(ctx, pink):
    """the whole-buffer masked call over the 130 frames of pink under detection: computed once, shared, never written"""
    return frozen(whole_call(ctx, pink))


def push(s, chans, a, b, modes=None, offsets=OFFSETS, masking=True):
    """one push_measured of frames a .. b - 1 with every output -> dict"""
    return SM.as_dict(s.push_measured([c[a * 512:b * 512] for c in chans], modes=None if modes is None else modes[a:b],
                                      scale_factor_offsets=offsets, masking=masking, return_distortion=True, return_shifts=True,
                                      return_weights=True))


def pushes(s, chans, runs, first=0, **kw):
    parts, at = [], first
    for n in runs:
        parts.append(push(s, chans, at, at + n, **kw))
        at += n
    return SM.concat(parts)


def raw_push(s, chans, a, b, modes=None, offsets=OFFSETS, tables='packaged', ask=OUTPUTS):
    """c1_enc_stream_push_measured itself, with any subset of the outputs; the others are passed as NULL -> (rc, dict of all
    six buffers, the ones not asked for still at their fill)"""
    chans = [np.ascontiguousarray(c[a * 512:b * 512], dtype=np.float32) for c in chans]
    n = (b - a) * len(chans)
    shape = {'units': ((n, 212), np.uint8), 'taken': ((n,), np.uint8), 'shifts': ((n, 52), np.int8), 'distortion': ((n, 2), np.float64),
             'energy': ((n,), np.float64), 'weights': ((n, 52), np.float64)}
    out = {k: np.full(sh, FILL[k], dtype=d) for k, (sh, d) in shape.items()}
    m = None if modes is None else np.ascontiguousarray(modes[a:b], dtype=np.uint8).reshape(-1)
    off = None if offsets is None else np.ascontiguousarray(list(offsets) + [0] * 9, dtype=np.int8)
    floor, spread = (None, None) if tables is None else (MK.named(tables) if isinstance(tables, str) else tables)
    floor = None if floor is None else np.ascontiguousarray(floor, dtype=np.float64)
    spread = None if spread is None else np.ascontiguousarray(spread, dtype=np.float64)
    data = lambda x: None if x is None else x.ctypes.data
    rc = capi.load().c1_enc_stream_push_measured(s._h, capi.ptr_array([c.ctypes.data for c in chans]), b - a, data(m), data(off),
                                                 0 if offsets is None else len(offsets), data(floor), data(spread),
                                                 *[out[k].ctypes.data if k in ask else None for k in OUTPUTS])
    return rc, out


def untouched(out, keys=OUTPUTS):
    return all((out[k] == FILL[k]).all() for k in keys)


def against(m, got, offsets=OFFSETS, nch=2):
    print('taken %d of %d; bit-equal: weights %s, T_ref %s, T(n*) %s, E %s' % (
        int(got['taken'].sum()), len(got['taken']), MK.bitwise(got['weights'], m['P']), MK.bitwise(got['distortion'][:, 0], m['D'][:, 0]),
        MK.bitwise(got['distortion'][:, 1], m['D'][:, 1]), MK.bitwise(got['energy'], m['E'])))
    assert MK.check_outputs(m, got['units'], got['taken'], got['shifts'], got['distortion'], got['energy'], got['weights']) is None
    assert MK.check_valid(got['units'], m['coefs'], got['taken'], got['distortion'], got['weights'], offsets, nch) is None


def every_other(m):
    """the rows of channel 0 of a stereo model: the model of that channel alone (the channels do not see each other)"""
    n = len(m['taken'])
    return {k: (v[::2] if getattr(v, 'ndim', 0) and v.shape[0] == n else v) for k, v in m.items()}


# ---- 1. run lengths ----
def test_run_lengths(ctx, pink, whole):
    """130 stereo frames under detection pushed in runs of 1, 1, 1, 2, 3, 5, 8, 13, 32 and 64: every output is bit for bit the
    whole-buffer call's over the whole signal, and passes the model's checks"""
    s = c1.EncoderStream(ctx, 2)
    try:
        got = pushes(s, pink, RUNS)
    finally:
        s.close()
    assert same(got, dict(whole))
    against(MK.case('detect', 'pink'), got)


# ---- 2. other streams ----
@pytest.mark.parametrize('kind', ['given-10', 'fixed-220', 'white-58-stereo', 'white-58-mono'])
def test_other_streams(ctx, pink, white, kind):
    chans = pink if kind in ('given-10', 'fixed-220') else (white if kind == 'white-58-stereo' else white[:1])
    nch, frames = len(chans), len(chans[0]) // 512
    byte = 10 if chans is pink else 58
    m = MK.case(byte, 'pink' if chans is pink else 'white')
    given = None if kind == 'fixed-220' else np.full((frames, nch), byte, dtype=np.uint8)
    s = c1.EncoderStream(ctx, nch, opts({'fixedBlockModes': [2, 2, 0]}) if kind == 'fixed-220' else None)
    try:
        got = pushes(s, chans, (1, 2, 5, frames - 8), modes=given)
    finally:
        s.close()
    against(every_other(m) if nch == 1 else m, got, nch=nch)
    want = whole_call(ctx, chans, modes=given, options=opts({'fixedBlockModes': [2, 2, 0]}) if kind == 'fixed-220' else None)
    assert same(got, want)


# ---- 3. state ----
def test_state_is_the_plain_pushes_state_and_pushes_mix(ctx, pink, whole):
    plain_units = ctx.encode(pink)
    a, b, mixed = c1.EncoderStream(ctx, 2), c1.EncoderStream(ctx, 2), c1.EncoderStream(ctx, 2)
    try:
        at = 0
        for i, n in enumerate((1, 1, 3, 8, 37)):
            push(a, pink, at, at + n)
            b.push([c[at * 512:(at + n) * 512] for c in pink])
            assert np.array_equal(a.get_state().view(np.uint32), b.get_state().view(np.uint32)), at   # as bits
            # one stream, plain and measured pushes in turn: each gives what it gives alone
            if i % 2:
                assert same(push(mixed, pink, at, at + n), rows(whole, at, at + n, 2)), at
            else:
                assert np.array_equal(mixed.push([c[at * 512:(at + n) * 512] for c in pink]), plain_units[at * 2:(at + n) * 2]), at
            at += n
        assert np.array_equal(mixed.get_state().view(np.uint32), b.get_state().view(np.uint32))
    finally:
        a.close(), b.close(), mixed.close()


def test_restore(ctx, pink, whole):
    """get_state at frame 50, a fresh stream, set_state, measured pushes of frames 50 .. 129 in runs of 1, 1, 3 and the rest:
    the frames from the explicit state (twice), then the usual path.  The rows of the uninterrupted stream"""
    first, second, third, fourth = (c1.EncoderStream(ctx, 2) for _ in range(4))
    try:
        first.push([c[:50 * 512] for c in pink])
        state = first.get_state()
        second.set_state(state)
        got = pushes(second, pink, (1, 1, 3, FRAMES - 55), first=50)
        assert same(got, rows(whole, 50, FRAMES, 2))
        # with given modes the frames from the state are encoded a pool at a time: against the uninterrupted stream's usual path
        given = np.full((FRAMES, 2), 10, dtype=np.uint8)
        want = push(first, pink, 50, 70, modes=given)
        third.set_state(state)
        assert same(pushes(third, pink, (1, 1, 18), first=50, modes=given), want)
        # one push that covers both frames from the state and the usual path behind them
        fourth.set_state(state)
        assert same(push(fourth, pink, 50, 60), rows(whole, 50, 60, 2))
        assert np.array_equal(fourth.get_state().view(np.uint32), ctx_state_after(ctx, pink, 60).view(np.uint32))
    finally:
        for s in (first, second, third, fourth):
            s.close()


def ctx_state_after(ctx, chans, frames):
    s = c1.EncoderStream(ctx, len(chans))
    try:
        s.push([c[:frames * 512] for c in chans])
        return s.get_state()
    finally:
        s.close()


def test_option_change(ctx):
    """fixed [2, 2, 0] for frames 0 .. 39, then detection; the first push after the switch is one frame (the switch-frame
    path).  All outputs against the model over the oracle's units"""
    chans = SM.option_change_material()
    m = SM.option_change_case()
    s, twin = (c1.EncoderStream(ctx, 2, opts(SM.CHANGE_INITIAL)) for _ in range(2))
    try:
        parts = [pushes(s, chans, (1, 7, SM.SWITCH - 8))]
        twin.push([c[:SM.SWITCH * 512] for c in chans])
        for x in (s, twin):
            x.set_options(opts({'fixedBlockModes': None}))
        parts.append(push(s, chans, SM.SWITCH, SM.SWITCH + 1))
        twin.push([c[SM.SWITCH * 512:(SM.SWITCH + 1) * 512] for c in chans])
        assert np.array_equal(s.get_state().view(np.uint32), twin.get_state().view(np.uint32))
        parts.append(pushes(s, chans, (1, SM.CHANGE_FRAMES - SM.SWITCH - 2), first=SM.SWITCH + 1))
    finally:
        s.close(), twin.close()
    got = SM.concat(parts)
    against(m, got)
    kept = got['taken'] == 0
    assert np.array_equal(got['units'][kept], m['ref'][kept])


# ---- 4. nesting ----
def test_nesting(ctx, pink):
    part = [c[:SHORT * 512] for c in pink]
    streams = [c1.EncoderStream(ctx, 2) for _ in range(5)]
    try:
        # tables NULL, offsets given: c1_encode_measured_sf_*
        rc, sf = raw_push(streams[0], part, 0, SHORT, tables=None, ask=OUTPUTS[:5])
        assert rc == C1_OK and untouched(sf, ('weights',))
        units, taken, shifts, dist, energy = ctx.encode_measured(part, return_distortion=True, scale_factor_offsets=OFFSETS, return_shifts=True)
        want = {'units': units, 'taken': taken, 'shifts': shifts, 'distortion': dist, 'energy': energy}
        assert same({k: sf[k] for k in want}, want)
        # both NULL: c1_encode_measured_*, and shifts written as zeros
        rc, plain = raw_push(streams[1], part, 0, SHORT, tables=None, offsets=None, ask=OUTPUTS[:5])
        assert rc == C1_OK and untouched(plain, ('weights',))
        units, taken, dist, energy = ctx.encode_measured(part, return_distortion=True)
        want = {'units': units, 'taken': taken, 'distortion': dist, 'energy': energy}
        assert same({k: plain[k] for k in want}, want) and not plain['shifts'].any()
        # flat tables: the NULL-table push, bit for bit, with every weight 1.0
        for i, tables in enumerate(('flat', (np.ones(52), np.zeros((52, 52))))):
            rc, flat = raw_push(streams[2 + i], part, 0, SHORT, tables=tables)
            assert rc == C1_OK and (flat.pop('weights') == 1.0).all()
            assert same(flat, {k: sf[k] for k in flat})
        # tables without offsets: the masked call with the single offset 0
        rc, own = raw_push(streams[4], part, 0, SHORT, offsets=None)
        assert rc == C1_OK and not own['shifts'].any()
        units, taken, dist, energy, weights = ctx.encode_measured(part, return_distortion=True, masking=True, return_weights=True)
        want = {'units': units, 'taken': taken, 'distortion': dist, 'energy': energy, 'weights': weights}
        assert same({k: own[k] for k in want}, want)
    finally:
        for s in streams:
            s.close()


# ---- 5. the wide kernel against the narrow ones ----
@pytest.fixture(scope='module')
def two():
    narrow, wide = _context(C1_MEASURED_WIDE=0), _context(C1_MEASURED_WIDE=1)
    yield narrow, wide
    narrow.close(), wide.close()


def batch(c, chans, options=None, modes=None, ask=OUTPUTS, offsets=OFFSETS, tables='packaged'):
    """c1_encode_measured_masked_batch with any subset of the outputs -> dict of the ones asked for"""
    chans = [np.ascontiguousarray(x, dtype=np.float32) for x in chans]
    nch, frames = len(chans), len(chans[0]) // 512
    n = frames * nch
    o = (options or opts()).to_c()
    shape = {'units': ((n, 212), np.uint8), 'taken': ((n,), np.uint8), 'shifts': ((n, 52), np.int8), 'distortion': ((n, 2), np.float64),
             'energy': ((n,), np.float64), 'weights': ((n, 52), np.float64)}
    out = {k: np.full(s, FILL[k], dtype=d) for k, (s, d) in shape.items()}
    m = None if modes is None else np.ascontiguousarray(modes, dtype=np.uint8).reshape(-1)
    off = np.ascontiguousarray(offsets, dtype=np.int8)
    floor, spread = MK.named(tables)
    floor = np.ascontiguousarray(floor, dtype=np.float64)
    spread = None if spread is None else np.ascontiguousarray(spread, dtype=np.float64)
    capi.check(capi.load().c1_encode_measured_masked_batch(
        c._h, capi.ptr_array([x.ctypes.data for x in chans]), nch, frames, 0, C.byref(o), None if m is None else m.ctypes.data,
        off.ctypes.data, len(off), floor.ctypes.data, None if spread is None else spread.ctypes.data,
        *[out[k].ctypes.data if k in ask else None for k in OUTPUTS]))
    return {k: out[k] for k in ask}


def test_wide_against_narrow_under_detection(two, pink, whole):
    narrow, wide = two
    for frames in (1, 2, 3, 63, FRAMES):
        part = [c[:frames * 512] for c in pink]
        got = batch(wide, part)
        assert same(got, batch(narrow, part)), frames
        assert same(got, rows(whole, 0, frames, 2)), frames     # the encoder is causal
        assert same(batch(wide, part[:1]), batch(narrow, part[:1])), frames             # mono: 1 unit, the seam of the grid
    against(MK.case('detect', 'pink'), batch(wide, pink))
    # measure only: no unit is packed, no record rewritten
    ask = OUTPUTS[1:]
    got = batch(wide, pink, ask=ask)
    assert same(got, batch(narrow, pink, ask=ask)) and same(got, {k: whole[k] for k in ask})
    wide.set_profiling(True)
    try:
        batch(wide, pink)
        ms, launches = wide.kernel_ms('measure')
        assert launches == 1 and ms > 0
    finally:
        wide.set_profiling(False)


def test_wide_against_narrow_on_other_material(two, pink, white):
    narrow, wide = two
    given = np.full((len(white[0]) // 512, 2), 58, dtype=np.uint8)
    got = batch(wide, white, modes=given)
    assert same(got, batch(narrow, white, modes=given))
    against(MK.case(58, 'white'), got)
    silence = [np.zeros(8 * 512, dtype=np.float32)] * 2
    got = batch(wide, silence)
    assert same(got, batch(narrow, silence))
    assert not got['taken'].any() and not got['distortion'].view(np.uint64).any() and not got['energy'].view(np.uint64).any()
    # floor = SPECS_PER_BFU without a matrix, the offset 0: both branches of the fallback occur
    ten = np.full((FRAMES, 2), 10, dtype=np.uint8)
    got = batch(wide, pink, modes=ten, tables='specs', offsets=(0,))
    assert same(got, batch(narrow, pink, modes=ten, tables='specs', offsets=(0,)))
    against(MK.case(10, 'pink', 'specs', (0,)), got, (0,))
    assert got['taken'].any() and not got['taken'].all()
    # all long by the options (the side records' mode byte is not read) and fixed short modes
    for o in (opts({'fixedBlockModes': [0, 0, 0]}), opts({'fixedBlockModes': [2, 0, 3]})):
        assert same(batch(wide, pink, o), batch(narrow, pink, o))


def test_wide_against_narrow_through_the_plain_and_sf_entry_points(two, pink):
    narrow, wide = two
    part = [c[:63 * 512] for c in pink]
    for kw in ({}, {'scale_factor_offsets': OFFSETS, 'return_shifts': True}, {'scale_factor_offsets': (0,), 'return_shifts': True}):
        a, b = (c.encode_measured(part, return_distortion=True, **kw) for c in (narrow, wide))
        assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, b)), kw


def test_streams_on_the_wide_and_the_narrow_kernel(two, pink, whole):
    """the three paths of a push under either kernel, whatever the threshold"""
    for c in two:
        s, t = c1.EncoderStream(c, 2), c1.EncoderStream(c, 2)
        try:
            assert same(pushes(s, pink, (1, 2, 47)), rows(whole, 0, 50, 2))
            t.set_state(s.get_state())
            assert same(pushes(t, pink, (1, 1, 3), first=50), rows(whole, 50, 55, 2))
        finally:
            s.close(), t.close()
    chans, m = SM.option_change_material(), SM.option_change_case()
    for c in two:
        s = c1.EncoderStream(c, 2, opts(SM.CHANGE_INITIAL))
        try:
            parts = [push(s, chans, 0, SM.SWITCH)]
            s.set_options(opts({'fixedBlockModes': None}))
            parts += [push(s, chans, SM.SWITCH, SM.SWITCH + 1), push(s, chans, SM.SWITCH + 1, SM.CHANGE_FRAMES)]
        finally:
            s.close()
        against(m, SM.concat(parts))


def test_the_threshold_between_the_kernels(ctx, two, pink, whole):
    """a context without the variable: 1 unit, and the largest count the threshold admits and the one past it, mono"""
    narrow = two[0]
    mono = np.tile(pink[0], -(-(WIDE_UNITS + 1) // FRAMES))
    for units in sorted({1, max(WIDE_UNITS, 1), WIDE_UNITS + 1}):
        part = [mono[:units * 512]]
        assert same(batch(ctx, part), batch(narrow, part)), units


# ---- 6. rejections ----
def test_rejections_leave_outputs_and_stream_as_they_were(ctx, pink, whole):
    s = c1.EncoderStream(ctx, 2)
    err = lambda: capi.load().c1_last_error().decode()
    floor, spread = (np.array(a) for a in MK.packaged())
    try:
        assert same(push(s, pink, 0, 3), rows(whole, 0, 3, 2))
        before = s.get_state()
        bad_modes = np.full((FRAMES, 2), 10, dtype=np.uint8)
        bad_modes[4, 1] = 0x10
        bad_floor = floor.copy()
        bad_floor[7] = 0.0
        bad_spread = spread.copy()
        bad_spread[3, 9] = -1.0
        cases = [(dict(tables=(None, spread)), 'mask_spread is given without mask_floor'),
                 (dict(tables=None), 'weights is given without mask_floor'),
                 (dict(offsets=(0, 9)), 'sf_offsets[1] = 9 is outside -8..8'),
                 (dict(offsets=(1, 0)), 'sf_offsets[0] = 1, not 0'),
                 (dict(tables=(bad_floor, spread)), 'mask_floor[7]'),
                 (dict(tables=(floor, bad_spread)), 'mask_spread[165]'),
                 (dict(modes=bad_modes), 'frame 1, channel 1'),
                 (dict(ask=OPTIONAL), 'units is NULL')]
        for kw, what in cases:
            rc, out = raw_push(s, pink, 3, 8, **kw)
            assert rc == C1_ERR_ARG and what in err(), (kw, err())
            assert untouched(out), kw
            assert np.array_equal(s.get_state().view(np.uint32), before.view(np.uint32)), kw
        # n_offsets without offsets
        out = raw_push(s, pink, 3, 8, ask=())[1]
        rc = capi.load().c1_enc_stream_push_measured(s._h, capi.ptr_array([c.ctypes.data for c in pink]), 5, None, None, 5, None, None,
                                                     out['units'].ctypes.data, None, None, None, None, None)
        assert rc == C1_ERR_ARG and 'n_offsets = 5, but sf_offsets is NULL' in err() and untouched(out)
        # the next push gives what it would have given without them
        assert same(push(s, pink, 3, 8), rows(whole, 3, 8, 2))
        rc, out = raw_push(s, pink, 8, 8)                                            # frames = 0 writes nothing
        assert rc == C1_OK and all(v.size == 0 for v in out.values())
    finally:
        s.close()


# ---- 7. call shapes ----
def test_on_a_callers_stream(pink, whole):
    import torch
    S = torch.cuda.Stream()
    c = _context(stream=S.cuda_stream)
    try:
        s = c1.EncoderStream(c, 2)
        try:
            assert same(pushes(s, pink, (1, 2, 13)), rows(whole, 0, 16, 2))
        finally:
            s.close()
    finally:
        c.close()


def test_outputs_do_not_depend_on_which_are_asked_for(ctx, pink, whole):
    """units with every single other output and with all but one of them"""
    subsets = [s for k in (0, 1, 4) for s in itertools.combinations(OPTIONAL, k)]
    for ask in subsets:
        s = c1.EncoderStream(ctx, 2)
        try:
            at = 0
            for n in (1, 4):
                rc, out = raw_push(s, pink, at, at + n, ask=('units',) + ask)
                assert rc == C1_OK, ask
                assert same({k: out[k] for k in ('units',) + ask}, {k: whole[k][at * 2:(at + n) * 2] for k in ('units',) + ask}), ask
                assert untouched(out, [k for k in OPTIONAL if k not in ask]), ask
                at += n
        finally:
            s.close()


def test_two_pushes_with_different_tables_back_to_back(ctx, pink):
    """each equals its own model; the caller's tables are free as soon as the push returns"""
    given = BB.given_modes()
    a, b = c1.EncoderStream(ctx, 2), c1.EncoderStream(ctx, 2)
    try:
        floor_a, spread_a = (np.array(x) for x in MK.packaged())
        floor_b, spread_b = (np.array(x) for x in MK.explicit('self'))
        rc_a, first = raw_push(a, pink, 0, SHORT, modes=given, tables=(floor_a, spread_a))
        floor_a[:] = 1.0
        spread_a[:] = 0.0
        rc_b, second = raw_push(b, pink, 0, SHORT, modes=given, tables=(floor_b, spread_b), offsets=(0,))
        floor_b[:] = 1.0
        spread_b[:] = 0.0
        assert rc_a == C1_OK and rc_b == C1_OK
    finally:
        a.close(), b.close()
    against(MK.case('modes', 'pink', 'packaged', OFFSETS, SHORT), first)
    against(MK.case('modes', 'pink', 'self', (0,), SHORT), second, (0,))
