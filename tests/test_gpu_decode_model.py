"""GPU: the decode model C1_DECODE_BINARY32 (c1_ctx_set_decode_model(ctx, 2)): every decode entry of a context in the
arithmetic of k_decode<float>, operation for operation.

The yardstick for bits is one c1_decode_device call under model 1 (c1_ctx_set_decode_precision(ctx, 1)) on a fresh context:
the k_decode<float> that tests/test_gpu_decode32_pinned.py pins.  It is never the code under test: under model 2 the entries
below run k_decode_fields<float> and k_decode_from_state<float, .>, or are compared with the yardstick of another context.
Every comparison with it is bit for bit on the uint32 views.  Fields no sound unit can carry have no yardstick; there model 2
is held to decode32_lib's device bounds for streams against the exact decode of the same fields."""
import numpy as np
import pytest

import decode32_lib as D

pytestmark = pytest.mark.gpu
PER = {'nbfu': 1, 'block_modes': 3, 'sfi': 52, 'wl': 52, 'quantized': 512}
KEYS = ('nbfu', 'block_modes', 'sfi', 'wl', 'quantized')
PIECES = (1, 31, 33)                                         # then the rest
_material = None
_yard = {}


def material():
    """{name: units uint8 [n, 212], n even}: arbitrary bytes, crafted overruns, encoded pink noise with bursts under detection
    and under [2, 2, 3], and responses under each of the eight mode triples followed by silence under the complement"""
    global _material
    if _material is None:
        levels = D.level_streams()
        triples = np.concatenate([D.basis_batch(t, D.LEVELS[1], 'complement', order=range(5, 512, 37)) for t in D.TRIPLES])
        _material = {'random': D.random_units(), 'overrun': D.overrun_units(),
                     'detect': np.ascontiguousarray(levels[(1.0, 'detect', 1)]), 'short': np.ascontiguousarray(levels[(1.0, 'short', 1)]),
                     'detect2': np.ascontiguousarray(levels[(1.0, 'detect', 2)]), 'triples': triples}
        for u in _material.values():
            assert u.shape[0] % 2 == 0
            u.setflags(write=False)
    return _material


NAMES = ('random', 'overrun', 'detect', 'short', 'detect2', 'triples')


def yardstick(units, channels=1):
    """c1_decode_batch (one c1_decode_device call) under model 1 on a context of its own"""
    import carta1_amd as c1
    key = (units.tobytes(), channels)
    if key not in _yard:
        c = c1.Context(0)
        try:
            c.set_decode_precision(True)
            assert c.decode_model == c1.DECODE_BINARY32_BULK
            out = c.decode(units, channels)
        finally:
            c.close()
        for o in out:
            o.setflags(write=False)
        _yard[key] = out
    return _yard[key]


@pytest.fixture(scope='module')
def c2():
    import carta1_amd as c1
    c = c1.Context(0)
    c.set_decode_model(c1.DECODE_BINARY32)
    yield c
    c.close()


@pytest.fixture(scope='module')
def c0():
    import carta1_amd as c1
    c = c1.Context(0)
    yield c
    c.close()


def same(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def sub(fields, start, stop):
    return {k: np.ascontiguousarray(np.asarray(v)[start:stop]) for k, v in fields.items()}


def short_streams():
    """48-unit mono streams, one per kind of material (the overruns: 6 units under each triple, silent ones included)"""
    m = material()
    over = m['overrun'].reshape(8, 64, 212)[:, [0, 1, 17, 40, 62, 63]].reshape(-1, 212)
    return [np.ascontiguousarray(u[:48]) for u in (m['random'], over, m['detect'][-48:], m['short'][100:], m['triples'][40:])]


def chain(ctx, streams):
    """n one-frame from-state calls over the streams side by side, from zero states -> (pcm [streams, n * 512], last states)"""
    n = streams[0].shape[0]
    st = np.zeros((len(streams), 179), dtype=np.float32)
    pcm = np.zeros((len(streams), n, 512), dtype=np.float32)
    for f in range(n):
        pcm[:, f], st = ctx.decode_frames_from_states(np.stack([s[f] for s in streams]), st)
    return pcm.reshape(len(streams), -1), st


# ---- units ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', NAMES)
def test_decode_equals_the_yardstick(c2, name):
    units = material()[name]
    for channels in (1, 2):
        want = yardstick(units, channels)
        got = c2.decode(units, channels)
        again = c2.decode(units, channels)
        halo = c2.decode(units, channels, halo_units=1)
        for c in range(channels):
            assert same(got[c], want[c]), '%d channel(s), channel %d' % (channels, c)
            assert same(again[c], got[c]), 'two runs differ'
            assert same(halo[c], want[c][512:]), 'halo_units 1, %d channel(s), channel %d' % (channels, c)
    stereo = c2.decode(units, 2)
    for c in range(2):
        mono = np.ascontiguousarray(units[c::2])
        assert same(stereo[c], c2.decode(mono, 1)[0]) and same(stereo[c], yardstick(mono)[0]), 'stereo channel %d is its mono decode' % c


@pytest.mark.parametrize('name', NAMES)
def test_decode_fields_of_unpacked_units_equals_the_yardstick(c2, name):
    units = material()[name]
    fields = c2.unpack_units(units)
    want = yardstick(units)[0]
    assert same(c2.decode_fields(fields)[0], want)
    # the launch walks runs of four frames up to 8 192 units: below, at and above one run
    for frames in (1, 2, 3, 4, 5):
        assert same(c2.decode_fields(sub(fields, 0, frames))[0], want[:frames * 512]), '%d frames' % frames
    assert same(c2.decode_fields(fields, halo_frames=1)[0], want[512:])
    st = c2.decode_fields(fields, channels=2)
    want2 = yardstick(units, 2)
    st_halo = c2.decode_fields(fields, channels=2, halo_frames=1)
    for c in range(2):
        assert same(st[c], want2[c]) and same(st_halo[c], want2[c][512:]), 'stereo channel %d' % c


def test_decode_fields_longer_runs(c2):
    # more than 8 192 units: runs of five frames, and a last run of one
    units = np.ascontiguousarray(np.concatenate([material()['random']] * 2 + [material()['overrun'], material()['triples']])[:8196 + 5])
    assert same(c2.decode_fields(c2.unpack_units(units))[0], yardstick(units)[0])


def test_wav16_is_the_binary32_pcm(c2):
    units = material()['detect2']
    a = c2.decode_wav16(units, 2)
    c2.set_decode_model(1)
    try:
        b = c2.decode_wav16(units, 2)
    finally:
        c2.set_decode_model(2)
    assert np.array_equal(a, b)


# ---- states -----------------------------------------------------------------------------------------------------------

def test_chain_of_from_state_calls_and_stream_state(c2):
    import carta1_amd as c1
    streams = short_streams()
    pcm, last = chain(c2, streams)
    for i, s in enumerate(streams):
        assert same(pcm[i], yardstick(s)[0]), 'stream %d' % i
        ds = c1.DecoderStream(c2, 1)
        ds.push(s)
        a = ds.get_state()
        ds.close()
        ds = c1.DecoderStream(c2, 1)
        ds.push_fields(c2.unpack_units(s))
        b = ds.get_state()
        ds.close()
        assert same(a[0], last[i]) and same(b[0], last[i]), 'stream %d: get_state' % i


def test_decode_signals(c2):
    streams = short_streams()
    m = material()
    # one signal
    got = c2.decode_signals([m['random']])
    assert same(got[0], yardstick(m['random'])[0])
    # lengths 0, 1, 2 and 33 beside whole streams: each its own one-call decode
    sigs = [m['detect'][:0], m['detect'][7:8], m['overrun'][63:65], m['short'][10:43], m['triples'][:33]] + streams
    got, states = c2.decode_signals(sigs, return_states=True)
    assert got[0].size == 0 and not states[0].any()
    for i, s in enumerate(sigs[1:], 1):
        s = np.ascontiguousarray(s)
        assert same(got[i], yardstick(s)[0]) and same(got[i], c2.decode(s, 1)[0]), 'signal %d' % i
    _, last = chain(c2, streams)
    assert same(states[5:], last), 'return_states equals the chain of from-state calls'
    # states= given: each signal continues the stream the state came from
    for k in (1, 2, 31):
        _, st = c2.decode_signals([s[:k] for s in streams], return_states=True)
        cont = c2.decode_signals([s[k:] for s in streams], states=st)
        for i, s in enumerate(streams):
            assert same(cont[i], yardstick(s)[0][k * 512:]), 'continuation of stream %d after %d frames' % (i, k)


# ---- streams ----------------------------------------------------------------------------------------------------------

def pieces(total):
    at, out = 0, []
    for p in PIECES:
        out.append((at, at + p))
        at += p
    out.append((at, total))
    return out


@pytest.mark.parametrize('name,channels', [('random', 1), ('random', 2), ('overrun', 1), ('detect2', 2), ('short', 1), ('triples', 2)])
@pytest.mark.parametrize('how', ['units', 'alternating', 'fields_first', 'restored'])
def test_stream_in_pieces_equals_the_yardstick(c2, name, channels, how):
    import carta1_amd as c1
    units = material()[name][:400]
    want = yardstick(np.ascontiguousarray(units), channels)
    fields = c2.unpack_units(units)
    frames = units.shape[0] // channels
    s = c1.DecoderStream(c2, channels)
    outs = []
    for i, (a, b) in enumerate(pieces(frames)):
        if how == 'restored' and i == 2:
            st = s.get_state()
            s.close()
            s = c1.DecoderStream(c2, channels)
            s.set_state(st)
        as_fields = (how == 'alternating' and i % 2 == 1) or (how == 'fields_first' and i % 2 == 0)
        outs.append(s.push_fields(sub(fields, a * channels, b * channels)) if as_fields else s.push(units[a * channels:b * channels]))
    s.close()
    for c in range(channels):
        assert same(np.concatenate([o[c] for o in outs]), want[c]), 'channel %d' % c


def test_model_changes_mid_stream(c0):
    """0 -> 2 -> 0 -> 2 -> 0 on one stream, unit and field pushes: every frame is the from-state frame under the model in force,
    from the state the frame before it left"""
    import carta1_amd as c1
    units = np.ascontiguousarray(np.concatenate([material()['detect'][-40:], material()['random'][:40]]))
    plan = [(0, 0, 3, 'U'), (2, 3, 4, 'U'), (2, 4, 20, 'F'), (0, 20, 21, 'F'), (0, 21, 40, 'U'), (2, 40, 61, 'U'), (0, 61, 80, 'U')]
    ctx = c1.Context(0)
    ref = c1.Context(0)
    try:
        fields = ctx.unpack_units(units)
        s = c1.DecoderStream(ctx, 1)
        got, want = [], []
        st = np.zeros((1, 179), dtype=np.float32)
        for model, a, b, kind in plan:
            ctx.set_decode_model(model)
            ref.set_decode_model(model)
            got.append(s.push(units[a:b])[0] if kind == 'U' else s.push_fields(sub(fields, a, b))[0])
            for f in range(a, b):
                p, st = ref.decode_frames_from_states(units[f:f + 1], st)
                want.append(p[0])
            assert same(s.get_state(), st), 'state after frame %d' % (b - 1)
        s.close()
        got, want = np.concatenate(got).reshape(-1, 512), np.stack(want)
        bad = [f for f in range(len(want)) if not same(got[f], want[f])]
        assert not bad, 'frames %r' % bad
        # the binary32 stretches really ran in binary32
        exact = c0.decode(units, 1)[0].reshape(-1, 512)
        assert not same(got[4:20], exact[4:20]) and same(got[:3], exact[:3])
    finally:
        ctx.close()
        ref.close()


def test_models_0_and_1_keep_what_they_computed(c0):
    """under models 0 and 1 the field and from-state entries stay exact, model 1's unit decode is the yardstick, and
    set_decode_precision is set_decode_model"""
    import carta1_amd as c1
    from carta1_amd import capi
    units = np.ascontiguousarray(np.concatenate([material()['detect'][-60:], material()['overrun'][60:70]]))
    exact = c0.decode(units, 1)[0]
    fields = c0.unpack_units(units)
    states = np.zeros((len(units), 179), dtype=np.float32)
    from_zero = c0.decode_frames_from_states(units, states)
    sig = c0.decode_signals([units[:1], units[1:34], units[34:]], return_states=True)
    c = c1.Context(0)
    try:
        assert c.decode_model == c1.DECODE_EXACT
        for bad in (-1, 3, 7):
            with pytest.raises(capi.Carta1Error):
                c.set_decode_model(bad)
            assert c.decode_model == c1.DECODE_EXACT
        for model in (0, 1):
            if model:
                c.set_decode_precision(True)
            assert c.decode_model == model
            assert same(c.decode(units, 1)[0], yardstick(units)[0] if model else exact)
            assert same(c.decode_fields(fields)[0], exact)
            p, st = c.decode_frames_from_states(units, states)
            assert same(p, from_zero[0]) and same(st, from_zero[1])
            got = c.decode_signals([units[:1], units[1:34], units[34:]], return_states=True)
            assert same(got[1], sig[1])
            for i in range(3):
                assert same(got[0][i][:512], sig[0][i][:512]), 'first frame of signal %d' % i
                if not model:
                    assert same(got[0][i], sig[0][i])
            s = c1.DecoderStream(c, 1)
            a = s.push(units[:30])[0]
            assert same(s.get_state(), c0.decode_frames_from_states(units[29:30], states[:1])[1])
            b = s.push_fields(sub(fields, 30, 70))[0]
            s.close()
            assert same(b, exact[30 * 512:])
            assert same(a, (yardstick(units)[0] if model else exact)[:30 * 512])
        c.set_decode_precision(False)
        assert c.decode_model == c1.DECODE_EXACT
    finally:
        c.close()


def test_the_meter_stays_exact(c0, c2):
    import oracle_lib as O
    frames = 24
    x = O.gen_pinkT(3, frames * 512)
    import carta1_amd as c1
    units = c0.encode([x], c1.EncoderOptions())
    want = c0.measure_pcm([x], units)
    got = c2.measure_pcm([x], units)
    for a, b in zip(got, want):
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64))


def test_precision_keyword(c0):
    import carta1_amd as c1
    units = material()['detect2'][:96]
    exact = c0.decode(units, 2)
    want = yardstick(np.ascontiguousarray(units), 2)
    image = c1.aea_header('t', units.shape[0], 2) + units.tobytes()
    for c in range(2):
        assert same(c1.decode_units(units, 2, ctx=c0, precision='binary32')[c], want[c])
        assert same(c1.decode_aea_pcm(image, ctx=c0, precision='binary32')[c], want[c])
        assert same(c1.decode_aea_pcm_many([image, image], ctx=c0, precision='binary32')[1][c], want[c])
        assert same(c1.decode_units(units, 2, ctx=c0)[c], exact[c])
        assert same(c1.decode_aea_pcm(image, ctx=c0, precision='exact')[c], exact[c])
    assert c0.decode_model == c1.DECODE_EXACT
    with pytest.raises(Exception):
        c1.decode_units(units[:1], 3, ctx=c0, precision='binary32')
    assert c0.decode_model == c1.DECODE_EXACT, 'the model is put back after an error'


# ---- fields no unit can carry -----------------------------------------------------------------------------------------

def random_fields(frames, seed):
    # as tests/test_gpu_decode_fields.py draws them: any nBfu 0..52, modes beyond the short codes (1 among them), wide and
    # extreme mantissas far beyond their word lengths, junk above nBfu
    rng = np.random.default_rng(seed)
    nbfu = rng.integers(0, 53, frames).astype(np.int32)
    modes = rng.choice(np.array([0, 0, 0, 1, 2, 3, -1, 7], dtype=np.int32), (frames, 3))
    wl = rng.integers(0, 16, (frames, 52)).astype(np.int32)
    wl[rng.random((frames, 52)) < 0.25] = 0
    sfi = rng.integers(0, 64, (frames, 52)).astype(np.int32)
    unread = np.arange(52)[None, :] >= nbfu[:, None]
    wl[unread] = 99
    sfi[unread] = -5
    q = rng.integers(-(1 << 31), 1 << 31, (frames, 512), dtype=np.int64)
    small = rng.random((frames, 512)) < 0.6
    q[small] = rng.integers(-40000, 40000, int(small.sum()))
    q[0, :4] = (-(1 << 31), (1 << 31) - 1, -(1 << 31), (1 << 31) - 1)
    return {'nbfu': nbfu, 'block_modes': modes, 'sfi': sfi, 'wl': wl, 'quantized': q.astype(np.int32)}


def test_fields_no_unit_can_carry_stay_within_the_stream_bounds(c0, c2):
    """Measured on an MI355X (4 000 frames, seed 31): frame maximum 10.79 u of the running peak, stream RMS 2.85 u, against the
    bounds 72 u and 24 u; 3 996 of the 4 000 frames differ from the exact decode."""
    import carta1_amd as c1
    fields = random_fields(4000, 31)
    assert not np.isin(fields['nbfu'], D.BFU_AMOUNTS).all() and (fields['block_modes'] == 1).any()
    ref = c0.decode_fields(fields)[0]
    got = c2.decode_fields(fields)[0]
    assert same(c2.decode_fields(fields)[0], got), 'two runs differ'
    per, rel, loud = D.stream_metrics(got, ref)
    print('fields no unit can carry, model 2 against exact: frame max %.2f u, stream RMS %.2f u, differing frames %d of %d'
          % (per.max(), rel, int((got.reshape(-1, 512) != ref.reshape(-1, 512)).any(axis=1).sum()), per.size))
    assert loud == 0
    assert per.max() <= D.GPU['frame_max'], per.max()
    assert rel <= D.GPU['stream_rms'], rel
    assert not same(got, ref), 'the arithmetic really changed'
    # the same frames through a stream and through the from-state kernel: one result
    s = c1.DecoderStream(c2, 1)
    parts = [s.push_fields(sub(fields, a, b))[0] for a, b in pieces(300)]
    s.close()
    assert same(np.concatenate(parts), got[:300 * 512])
