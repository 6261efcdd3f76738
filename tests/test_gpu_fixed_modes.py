"""GPU: the library against the reference under every fixedBlockModes triple it accepts (tests/golden/fixed_modes.json: the
reference encoder under all 36, fixed_modes_lib.py).  The 12 triples without a zero take the speculative all-short analysis,
which records the mode byte itself; the 23 mixed ones the exact analysis and the mixed-mode packer; only six of the 36 were
run before.  Every case is encoded in speculation modes 0, 1 and 2, as a whole and as a tail from its halo, and decoded;
then the same cases go through the other calls that take options, which must give the plain call's bytes; and the
property that makes 36 triples 8 classes (same bands short: same unit but for the six mode bits, same PCM) is checked on
the device outputs alone."""
import ctypes as C

import numpy as np
import pytest

import fixed_modes_lib as F
import option_domain_lib as L

pytestmark = pytest.mark.gpu
FX = F.fixture()
C1_OK, C1_ERR_ARG = 0, 1   # include/carta1_hip.h
tid = lambda t: 'm%d%d%d' % tuple(t)
BY_MODES = {F.modes_of(c): c for c in F.stereo_cases()}


@pytest.fixture(scope='module')
def ctx():
    import carta1_amd as c1
    c = c1.Context(0)
    yield c
    c.close()


def options(modes):
    import carta1_amd as c1
    return c1.EncoderOptions({'fixedBlockModes': list(modes), 'allocationBias': 1})


_inputs, _plain = {}, {}


def inputs(case):
    if case['id'] not in _inputs:
        _inputs[case['id']] = L.inputs(case)
    return _inputs[case['id']]


def plain(ctx, modes):
    """Context.encode of the triple's own case, checked against the fixture once"""
    if modes not in _plain:
        c = BY_MODES[modes]
        units = ctx.encode(inputs(c), options(modes))
        assert L.sha(units) == c['units_sha256'], ('case', c['id'], modes, 'first wrong unit', L.first_wrong_unit(units, c))
        _plain[modes] = units
    return _plain[modes]


@pytest.mark.parametrize('case', FX['cases'], ids=lambda c: '%s_%df' % (tid(F.modes_of(c)), c['frames']))
def test_encode_reproduces_every_triple(ctx, case):
    c = case
    modes, nch = F.modes_of(c), c['channels']
    xs, eo = inputs(c), options(modes)
    try:
        for mode in (0, 1, 2):
            ctx.set_speculation(mode)
            units = ctx.encode(xs, eo)
            assert L.sha(units) == c['units_sha256'], ('case', c['id'], modes, 'speculation', mode, 'first wrong unit',
                                                       L.first_wrong_unit(units, c))
            assert units[0, :2].tobytes().hex() == c['header']
            h, cut = c['halo'], c['cut']
            tail = ctx.encode([x[(cut - h) * 512:] for x in xs], eo, halo_frames=h)
            assert np.array_equal(tail, units.reshape(-1, nch, 212)[cut:].reshape(-1, 212)), ('halo', c['id'], mode, cut, h)
    finally:
        ctx.set_speculation(1)
    pcm = ctx.decode(units, nch)
    assert L.pcm_sha(pcm) == c['pcm_sha256'], ('pcm', c['id'], modes)


@pytest.mark.parametrize('cls', sorted(F.classes()), ids=lambda k: 'short%d%d%d' % k)
def test_triples_of_one_class_differ_in_the_six_mode_bits_only(ctx, cls):
    """one input under every triple of the class, device outputs only: units, decode() under the exact model and
    decode(precision='binary32')"""
    import carta1_amd as c1
    triples = F.classes()[cls]
    canon = F.canonical(triples[0])
    xs = inputs(BY_MODES[canon])
    want = ctx.encode(xs, options(canon))
    pcm_exact = L.pcm_sha(ctx.decode(want, 2))
    pcm_b32 = L.pcm_sha(c1.decode_units(want, 2, ctx, precision='binary32'))
    assert ctx.decode_model == c1.codec.DECODE_EXACT
    for t in triples:
        units = ctx.encode(xs, options(t))
        F.assert_same_but_mode_bits(units, t, want, canon, 'device')
        assert L.pcm_sha(ctx.decode(units, 2)) == pcm_exact, t
        assert L.pcm_sha(c1.decode_units(units, 2, ctx, precision='binary32')) == pcm_b32, t


@pytest.mark.parametrize('modes', F.ALL_SHORT, ids=tid)
def test_every_all_short_triple_takes_the_speculative_path(ctx, modes):
    """speculation_stats() after an always-speculate call: all 80 units of the case counted, as many redone as under
    [2,2,3] on the same input -- a triple that fell off the speculative path would show here"""
    c = BY_MODES[modes]
    xs = inputs(c)
    try:
        ctx.set_speculation(2)
        ctx.speculation_stats(reset=True)
        units = ctx.encode(xs, options(modes))
        got = ctx.speculation_stats(reset=True)
        ctx.encode(xs, options((2, 2, 3)))
        want = ctx.speculation_stats(reset=True)
    finally:
        ctx.set_speculation(1)
    assert L.sha(units) == c['units_sha256']
    print('speculation', tid(modes), '(units, redone)', got, 'under [2,2,3]', want)
    assert got[0] == 80 and got == want


@pytest.mark.parametrize('modes', F.TRIPLES, ids=tid)
def test_the_other_option_taking_calls_give_the_plain_bytes(ctx, modes):
    import carta1_amd as c1
    c = BY_MODES[modes]
    xs, eo = inputs(c), options(modes)
    want = plain(ctx, modes)
    frames = c['frames']
    # a live stream pushed one frame, then 7, then the rest
    s = c1.EncoderStream(ctx, 2, eo)
    try:
        got, states = [], [np.zeros((2, c1.capi.ENC_STATE_FLOATS), dtype=np.float32)]
        for a, b in ((0, 1), (1, 8), (8, frames)):
            got.append(s.push([x[a * 512:b * 512] for x in xs]))
            states.append(s.get_state())
    finally:
        s.close()
    assert np.array_equal(np.concatenate(got), want), ('stream', modes)
    # the case cut into three signals per channel, each restored from the stream's own state at its start
    sig = [xs[ch][a * 512:b * 512] for a, b in ((0, 1), (1, 8), (8, frames)) for ch in range(2)]
    st = np.stack([states[k][ch] for k in range(3) for ch in range(2)])
    res = ctx.encode_signals(sig, eo, states=st)
    by_channel = want.reshape(frames, 2, 212)
    for ch in range(2):
        assert np.array_equal(np.concatenate([res[2 * k + ch] for k in range(3)]), by_channel[:, ch]), ('signals', modes, ch)
    # a bias per frame from a palette of one entry; the best of one candidate
    assert np.array_equal(ctx.encode_biases(xs, np.ones(frames), modes=None, options=eo), want), ('biases', modes)
    units, choice = ctx.encode_best_bias(xs, [1.0], modes=None, options=eo)
    assert np.array_equal(units, want) and not choice.any(), ('best bias', modes)


def test_spec_stages_under_every_all_short_triple(ctx):
    """c1_spec_stages_device: coefficients and bounds are bit for bit those under [2,2,3], side[..., 52] is the triple's own
    byte; a mixed triple is still C1_ERR_ARG"""
    import carta1_amd as c1
    from test_gpu_spec import spec_stages
    xs = inputs(BY_MODES[(2, 2, 3)])
    co, eps, side = spec_stages(ctx, xs, (2, 2, 3))
    for t in F.ALL_SHORT:
        co_t, eps_t, side_t = spec_stages(ctx, xs, t)
        assert np.array_equal(co_t.view(np.uint32), co.view(np.uint32)), t
        assert np.array_equal(eps_t.view(np.uint32), eps.view(np.uint32)), t
        assert np.array_equal(side_t[..., :52], side[..., :52]), t
        assert (side_t[..., 52] == F.mode_byte(t)).all(), (t, np.unique(side_t[..., 52]))
    for t in ((1, 0, 2), (0, 1, 1), (2, 2, 0)):
        with pytest.raises(c1.capi.Carta1Error) as e:
            spec_stages(ctx, xs, t)
        assert e.value.code == C1_ERR_ARG, t


MEASURED = {'plain': {}, 'offsets': {'scale_factor_offsets': (0, -1, 1, -2, -3), 'return_shifts': True},
            'masked': {'masking': True, 'scale_factor_offsets': (0, -1, 1, -2, -3), 'return_shifts': True, 'return_weights': True}}


@pytest.mark.parametrize('kind', sorted(MEASURED))
@pytest.mark.parametrize('modes', [(1, 1, 1), (1, 0, 2), (2, 2, 1)], ids=tid)
def test_measured_allocation_under_non_canonical_triples(ctx, modes, kind):
    """encode_measured with modes=None (the fixed modes of the options): the six mode bits are the triple's, a unit that is
    not taken is the plain encode's, and every other output is what the same call gives under the class's canonical triple"""
    canon = F.canonical(modes)
    xs = inputs(BY_MODES[modes])
    kw = dict(MEASURED[kind], return_distortion=True)
    got = ctx.encode_measured(xs, modes=None, options=options(modes), **kw)            # raises unless C1_OK
    want = ctx.encode_measured(xs, modes=None, options=options(canon), **kw)
    units, taken = got[0], got[1]
    F.assert_same_but_mode_bits(units, modes, want[0], canon, 'measured ' + kind)
    base = ctx.encode(xs, options(modes))
    keep = taken == 0
    assert np.array_equal(units[keep], base[keep]), (modes, kind)
    assert len(got) == len(want)
    for k in range(1, len(got)):                                                       # taken, shifts, distortion, energy, weights
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k].view(np.uint8), want[k].view(np.uint8)), (modes, kind, k)
    print('measured', kind, tid(modes), 'units', len(taken), 'taken', int(taken.sum()))
