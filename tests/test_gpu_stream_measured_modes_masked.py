"""GPU: the mode search under one masking threshold per unit on live streams (c1_enc_stream_push_measured_modes_masked,
EncoderStream.push_measured_modes(masking=...)).  Pushes of any run lengths against c1_encode_measured_modes_masked_batch over the
whole signal, bit for bit; streams under detection, under fixed modes, mono, white; the stream's state against a twin's after
push(modes=modes_out); plain, measured, searched and masked-searched pushes in turn; a restore at frame 50 (the frames from an
explicit state); both settings of C1_MEASURED_WIDE; the rejections.
tests/test_gpu_measured_modes_masked.py pins the whole-buffer call these rows are compared with."""
import numpy as np
import pytest

import carta1_amd as c1
from carta1_amd import capi
import best_bias_lib as BB
import best_modes_lib as BMO
import masked_alloc_lib as MK
import measured_modes_lib as MM
import test_gpu_measured_modes as TM
import test_gpu_measured_modes_masked as TK

pytestmark = pytest.mark.gpu

C1_OK, C1_ERR_ARG = 0, 1   # include/carta1_hip.h
FRAMES = BB.FRAMES
OUTPUTS = TK.OUTPUTS
OPTIONAL = OUTPUTS[1:]
FILL = {'units': 0xA5, 'choice': 0xA5, 'modes': 0xA5, 'taken': 0xA5, 'shifts': 0x5A, 'distortion': -1.0, 'energy': -1.0, 'weights': -1.0}
RUNS = (1, 1, 1, 2, 3, 5, 8, 13, 32, 64)         # 130 frames
CAND3, CAND8 = MM.PINK_SF_CANDIDATES, MM.CANDIDATES
CONFIGS = {'three-offsets': (CAND3, MM.OFFSETS, 'packaged'), 'eight-plain': (CAND8, None, 'self'), 'short-only': ([58], MM.OFFSETS, 'packaged')}
same, rows = TM.same, TM.rows


def opts(v=None):
    return c1.EncoderOptions(v or {})


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


_whole = {}


def whole(ctx, name, chans, config):
    """c1_encode_measured_modes_masked_batch over the whole signal: computed once per module, shared, never written"""
    key = (name, len(chans), config)
    if key not in _whole:
        cand, offsets, tables = CONFIGS[config]
        got = TK.batch(ctx, chans, cand, (0,) if offsets is None else offsets, tables)
        for a in got.values():
            a.setflags(write=False)
        _whole[key] = got
    return _whole[key]


def push(s, chans, a, b, config):
    """one push_measured_modes(masking=...) of frames a .. b - 1 with every output -> dict"""
    cand, offsets, tables = CONFIGS[config]
    return dict(zip(OUTPUTS, s.push_measured_modes([c[a * 512:b * 512] for c in chans], cand, scale_factor_offsets=offsets,
                                                   return_distortion=True, return_shifts=True, masking=MK.named(tables), return_weights=True)))


def pushes(s, chans, runs, config, first=0):
    parts, at = [], first
    for n in runs:
        parts.append(push(s, chans, at, at + n, config))
        at += n
    return {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}


def raw_push(s, chans, a, b, cand=CAND3, offsets=MM.OFFSETS, n_offsets=None, ask=OUTPUTS, floor=None, spread=None, no_floor=False):
    """c1_enc_stream_push_measured_modes_masked itself with any subset of the outputs -> (rc, dict of all eight buffers)"""
    chans = [np.ascontiguousarray(c[a * 512:b * 512], dtype=np.float32) for c in chans]
    n, k = (b - a) * len(chans), len(cand)
    shape = {'units': ((n, 212), np.uint8), 'choice': ((n,), np.uint8), 'modes': ((n,), np.uint8), 'taken': ((n,), np.uint8),
             'shifts': ((n, 52), np.int8), 'distortion': ((n, k, 2), np.float64), 'energy': ((n, k), np.float64),
             'weights': ((n, 52), np.float64)}
    out = {key: np.full(sh, FILL[key], dtype=d) for key, (sh, d) in shape.items()}
    cb = np.ascontiguousarray(list(cand) + [0] * 9, dtype=np.uint8)
    off = None if offsets is None else np.ascontiguousarray(list(offsets) + [0] * 9, dtype=np.int8)
    no = n_offsets if n_offsets is not None else (0 if offsets is None else len(offsets))
    fl = np.ascontiguousarray(MK.packaged()[0] if floor is None else floor, dtype=np.float64)
    sp = np.ascontiguousarray(MK.packaged()[1] if spread is None else spread, dtype=np.float64)
    rc = capi.load().c1_enc_stream_push_measured_modes_masked(
        s._h, capi.ptr_array([c.ctypes.data for c in chans]), b - a, cb.ctypes.data, k, None if off is None else off.ctypes.data, no,
        None if no_floor else fl.ctypes.data, sp.ctypes.data, *[out[key].ctypes.data if key in ask else None for key in OUTPUTS])
    return rc, out


def untouched(out, keys=OUTPUTS):
    return all((out[k] == FILL[k]).all() for k in keys)


def bits(state):
    return state.view(np.uint32)


# ---- 1. run lengths ----
@pytest.mark.parametrize('config', list(CONFIGS))
def test_run_lengths(ctx, pink, config):
    s = c1.EncoderStream(ctx, 2)
    try:
        got = pushes(s, pink, RUNS, config)
    finally:
        s.close()
    assert same(got, dict(whole(ctx, 'pink', pink, config)))
    if config == 'eight-plain':
        assert not got['shifts'].any()
    if config == 'short-only':
        assert np.array_equal(got['weights'].view(np.uint64), whole(ctx, 'pink', pink, 'three-offsets')['weights'].view(np.uint64))


# ---- 2. other streams ----
@pytest.mark.parametrize('config', ['three-offsets', 'eight-plain'])
@pytest.mark.parametrize('kind', ['detect', 'fixed-220', 'mono', 'white', 'white-mono'])
def test_other_streams(ctx, pink, white, kind, config):
    """whatever the stream's block-mode options are, the rows are the whole-buffer call's"""
    chans = white if kind.startswith('white') else pink
    chans = chans[:1] if kind.endswith('mono') else chans
    name = 'white' if kind.startswith('white') else 'pink'
    s = c1.EncoderStream(ctx, len(chans), opts({'fixedBlockModes': [2, 2, 0]}) if kind == 'fixed-220' else None)
    try:
        got = pushes(s, chans, (1, 2, 5, len(chans[0]) // 512 - 8), config)
    finally:
        s.close()
    assert same(got, dict(whole(ctx, name, chans, config)))


# ---- 3. state; the kinds of push mixed ----
def test_state_is_that_of_push_modes_and_pushes_mix(ctx, pink):
    config = 'three-offsets'
    W = whole(ctx, 'pink', pink, config)
    for options in (None, opts({'fixedBlockModes': [2, 2, 0]})):
        a, b = c1.EncoderStream(ctx, 2, options), c1.EncoderStream(ctx, 2, options)
        try:
            at = 0
            for n in (1, 1, 3, 8, 37):
                got = push(a, pink, at, at + n, config)
                b.push([c[at * 512:(at + n) * 512] for c in pink], modes=got['modes'].reshape(-1, 2))
                assert np.array_equal(bits(a.get_state()), bits(b.get_state())), at
                at += n
            assert np.array_equal(a.push([c[at * 512:(at + 2) * 512] for c in pink]), b.push([c[at * 512:(at + 2) * 512] for c in pink]))
            assert np.array_equal(bits(a.get_state()), bits(b.get_state()))
        finally:
            a.close(), b.close()
    # one stream under detection: masked-searched, plain, measured and searched pushes in turn.  The masked-searched pushes give
    # the whole-buffer call's rows; the twin is pushed the same frames with push(modes=...) or plainly
    U = TM.batch(ctx, pink, CAND3, MM.OFFSETS)                                       # the unweighted search over the whole signal
    mixed, twin = c1.EncoderStream(ctx, 2), c1.EncoderStream(ctx, 2)
    try:
        at = 0
        for i, n in enumerate((1, 2, 1, 3, 5, 8, 2, 20, 4, 1, 2, 7)):
            part = [c[at * 512:(at + n) * 512] for c in pink]
            given = W['modes'][at * 2:(at + n) * 2].reshape(-1, 2)
            if i % 4 == 0:
                assert same(push(mixed, pink, at, at + n, config), rows(W, at, at + n, 2)), at
                twin.push(part, modes=given)
            elif i % 4 == 1:
                assert np.array_equal(mixed.push(part), twin.push(part)), at
            elif i % 4 == 2:
                units, taken, weights = mixed.push_measured(part, modes=np.zeros((n, 2), dtype=np.uint8), scale_factor_offsets=MM.OFFSETS,
                                                            masking=True, return_weights=True)
                assert np.array_equal(weights.view(np.uint64), W['weights'][at * 2:(at + n) * 2].view(np.uint64)), at
                twin.push(part, modes=np.zeros((n, 2), dtype=np.uint8))
            else:
                got = dict(zip(TM.OUTPUTS, mixed.push_measured_modes(part, CAND3, scale_factor_offsets=MM.OFFSETS, return_distortion=True,
                                                                      return_shifts=True)))
                assert same(got, rows(U, at, at + n, 2)), at
                twin.push(part, modes=got['modes'].reshape(-1, 2))
            assert np.array_equal(bits(mixed.get_state()), bits(twin.get_state())), at
            at += n
    finally:
        mixed.close(), twin.close()


# ---- 4. restore ----
@pytest.mark.parametrize('config', list(CONFIGS))
def test_restore(ctx, pink, config):
    """get_state at frame 50 from a twin, set_state: a one-frame push, a one-frame push, then the rest (the frames from the
    explicit state, twice, then the usual path); and one push across both paths.  The rows of the uninterrupted stream"""
    W = whole(ctx, 'pink', pink, config)
    first, second, third = (c1.EncoderStream(ctx, 2) for _ in range(3))
    try:
        first.push([c[:50 * 512] for c in pink])
        state = first.get_state()
        second.set_state(state)
        got = pushes(second, pink, (1, 1, FRAMES - 52), config, first=50)
        assert same(got, rows(W, 50, FRAMES, 2))
        third.set_state(state)
        assert same(push(third, pink, 50, 60, config), rows(W, 50, 60, 2))
        second.set_state(state)
        second.push([c[50 * 512:60 * 512] for c in pink], modes=W['modes'][100:120].reshape(-1, 2))
        assert np.array_equal(bits(third.get_state()), bits(second.get_state()))
        third.set_state(state)
        push(third, pink, 50, 51, config)
        second.set_state(state)
        second.push([c[50 * 512:51 * 512] for c in pink], modes=W['modes'][100:102].reshape(-1, 2))
        assert np.array_equal(bits(third.get_state()), bits(second.get_state()))
        assert same(push(third, pink, 51, 54, config), rows(W, 51, 54, 2))
    finally:
        for s in (first, second, third):
            s.close()


# ---- 5. both kernels ----
def test_streams_on_the_wide_and_the_narrow_kernel(ctx, pink):
    two = [TM._context(C1_MEASURED_WIDE=0), TM._context(C1_MEASURED_WIDE=1)]
    try:
        for config in CONFIGS:
            W = whole(ctx, 'pink', pink, config)
            for c in two:
                for frames in (1, 2, 3, 63):
                    for nch in (1, 2):
                        s = c1.EncoderStream(c, nch)
                        try:
                            got = push(s, pink[:nch], 0, frames, config)
                        finally:
                            s.close()
                        want = rows(W, 0, frames, 2)
                        assert same(got, want if nch == 2 else {k: v[::2] for k, v in want.items()}), (config, frames, nch)
                s, t = c1.EncoderStream(c, 2), c1.EncoderStream(c, 2)
                try:
                    assert same(pushes(s, pink, (1, 2, 47), config), rows(W, 0, 50, 2))
                    t.set_state(s.get_state())
                    assert same(pushes(t, pink, (1, 1, 3), config, first=50), rows(W, 50, 55, 2))
                finally:
                    s.close(), t.close()
                c.set_profiling(True)
                s = c1.EncoderStream(c, 2)
                try:
                    push(s, pink, 0, 5, config)
                    ms, launches = c.kernel_ms('measure')
                    assert launches == 1 and ms > 0
                finally:
                    s.close()
                    c.set_profiling(False)
    finally:
        for c in two:
            c.close()


# ---- 6. rejections ----
def test_rejections_leave_outputs_and_stream_as_they_were(ctx, pink):
    W = whole(ctx, 'pink', pink, 'three-offsets')
    s = c1.EncoderStream(ctx, 2)
    err = lambda: capi.load().c1_last_error().decode()
    bad_floor = np.array(MK.packaged()[0])
    bad_floor[9] = 1e61
    bad_spread = np.array(MK.packaged()[1])
    bad_spread[1, 2] = np.nan
    try:
        assert same(push(s, pink, 0, 3, 'three-offsets'), rows(W, 0, 3, 2))
        before = s.get_state()
        cases = [(dict(cand=[0, 1]), 'candidate 1: low field of mode byte 0x01'),
                 (dict(cand=[10, 58, 10]), "candidate 2: mode byte 0x0a is candidate 0's"),
                 (dict(cand=list(range(0, 18, 2))), 'n_cand = 9 is outside 1..8'),
                 (dict(offsets=(0, 9)), 'sf_offsets[1] = 9 is outside -8..8'),
                 (dict(offsets=(1, 0)), 'sf_offsets[0] = 1, not 0'),
                 (dict(offsets=None, n_offsets=5), 'n_offsets = 5, but sf_offsets is NULL'),
                 (dict(no_floor=True), 'c1_enc_stream_push_measured_modes_masked: mask_floor is NULL'),
                 (dict(floor=bad_floor), 'mask_floor[9] = 1e+61 is outside [1e-60, 1e60]'),
                 (dict(spread=bad_spread), 'mask_spread[54] = nan (masker 2 onto BFU 1) is outside [0, 1e60]'),
                 (dict(ask=OPTIONAL), 'pcm or units is NULL')]
        for kw, what in cases:
            rc, out = raw_push(s, pink, 3, 8, **kw)
            assert rc == C1_ERR_ARG and what in err(), (kw, err())
            assert untouched(out), kw
            assert np.array_equal(bits(s.get_state()), bits(before)), kw
        # what the arguments alone decide is decided before the stream is looked at
        class NoStream:
            _h = None
        rc, out = raw_push(NoStream, pink, 3, 8, cand=[0, 1])
        assert rc == C1_ERR_ARG and 'candidate 1' in err() and untouched(out)
        rc, out = raw_push(NoStream, pink, 3, 8, floor=bad_floor)
        assert rc == C1_ERR_ARG and 'mask_floor[9]' in err() and untouched(out)
        rc, out = raw_push(NoStream, pink, 3, 8)
        assert rc == C1_ERR_ARG and 'stream is NULL' in err() and untouched(out)
        # the next push gives what it would have given without them
        assert same(push(s, pink, 3, 8, 'three-offsets'), rows(W, 3, 8, 2))
        rc, out = raw_push(s, pink, 8, 8)                                            # frames = 0 writes nothing
        assert rc == C1_OK and all(v.size == 0 for v in out.values())
        # units alone, and units with each other output: the same bits, the others untouched
        for ask in [()] + [(k,) for k in OPTIONAL]:
            t = c1.EncoderStream(ctx, 2)
            try:
                rc, out = raw_push(t, pink, 0, 4, ask=('units',) + ask)
                assert rc == C1_OK and same({k: out[k] for k in ('units',) + ask}, {k: W[k][:8] for k in ('units',) + ask}), ask
                assert untouched(out, [k for k in OPTIONAL if k not in ask]), ask
            finally:
                t.close()
    finally:
        s.close()
