"""GPU: the measured block-mode search for n signals of any lengths in one call (c1_encode_signals_measured_modes*,
Context.encode_signals_measured_modes) against the composition the header defines it by (tests/signals_measured_modes_lib.py: one
mono EncoderStream per signal, set_state, one push_measured_modes, get_state), and against the CPU model of
tests/measured_modes_lib.py.  Every comparison is bitwise (doubles as bit patterns); only the model's own check_outputs keeps its
REL."""
import ctypes as C
import os

import numpy as np
import pytest

import carta1_amd as c1
from carta1_amd import capi
import best_modes_lib as BMO
import measured_modes_lib as MM
import signals_lib as SL
import signals_measured_modes_lib as SMM
import stream_state_lib as SS

pytestmark = pytest.mark.gpu

C1_OK, C1_ERR_ARG = 0, 1   # include/carta1_hip.h
I64P = C.POINTER(C.c_int64)
OUTPUTS = SMM.OUTPUTS
FILL = {'units': 0xA5, 'choice': 0xA5, 'modes': 0xA5, 'taken': 0xA5, 'shifts': 0x5A, 'distortion': -1.0, 'energy': -1.0}
CAND3, OFFS = SMM.CONFIGS['three-offsets']


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


def run3(ctx, oname='detect', pools=True, **kw):
    return SMM.run(ctx, oname, CAND3, OFFS, pools, **kw)


# ---- 1. composition -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('config', list(SMM.CONFIGS))
@pytest.mark.parametrize('pools', [False, True], ids=['fresh', 'pools'])
@pytest.mark.parametrize('oname', SMM.ONAMES)
def test_equals_the_composition(ctx, oname, pools, config):
    """units, choice, modes, taken, shifts, distortion, energy and the pools of the shared shapes equal one stream per signal"""
    cand, offs = SMM.CONFIGS[config]
    want = SMM.want(ctx, 'c', oname, config, pools)
    got = SMM.run(ctx, oname, cand, offs, pools)
    assert SMM.first_bad(got, want) is None, (oname, pools, config, SMM.first_bad(got, want))
    assert sum(int(t.sum()) for t in got['taken']) > 0
    assert len(set(np.concatenate(got['choice']).tolist())) > 1                      # the search decides something
    if offs is None:
        assert not np.concatenate(got['shifts']).any()
    if pools:                                                                        # transient_mags passes from in[i] to out[i]
        assert np.array_equal(SS.bits(got['states'][:, 227:]), SS.bits(SMM.enc_pools()[:, 227:]))
    if oname == 'long':                                              # the same bias as 'detect': threshold and fixed modes are not read
        other = SMM.want(ctx, 'c', 'detect', config, pools)
        assert SMM.first_bad(got, other) is None, ('the options decided', SMM.first_bad(got, other))


# ---- 2. candidate sets ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cand', [(0,), (58,)], ids=['long', 'short'])
def test_single_candidates(ctx, cand):
    """one candidate: one of the two analyses is not made"""
    want = SMM.compose(ctx, SMM.signals('pink'), 'detect', cand, OFFS, SMM.enc_pools())
    got = SMM.run(ctx, 'detect', cand, OFFS, True)
    assert SMM.first_bad(got, want) is None, SMM.first_bad(got, want)
    assert not np.concatenate(got['choice']).any() and (np.concatenate(got['modes']) == cand[0]).all()


def test_candidate_order_swaps_the_columns(ctx):
    a = SMM.run(ctx, 'detect', (0, 58), OFFS, True)
    b = SMM.run(ctx, 'detect', (58, 0), OFFS, True)
    want = SMM.compose(ctx, SMM.signals('pink'), 'detect', (58, 0), OFFS, SMM.enc_pools())
    assert SMM.first_bad(b, want) is None, SMM.first_bad(b, want)
    for i in range(len(SL.LENGTHS)):
        assert np.array_equal(SMM.bits(b['distortion'][i]), SMM.bits(a['distortion'][i][:, ::-1]))
        assert np.array_equal(SMM.bits(b['energy'][i]), SMM.bits(a['energy'][i][:, ::-1]))
        fin = a['distortion'][i].min(axis=2)                           # T_final = taken ? T(n*) : T_ref, and taken = T(n*) < T_ref
        tie = fin[:, 0] == fin[:, 1]                                   # a tie goes to the first candidate, whichever that is
        assert not a['choice'][i][tie].any() and not b['choice'][i][tie].any()
        assert np.array_equal(b['modes'][i][~tie], a['modes'][i][~tie])
        assert np.array_equal(b['choice'][i][~tie], 1 - a['choice'][i][~tie])
        assert np.array_equal(b['units'][i][~tie], a['units'][i][~tie])


# ---- 3. against the CPU model ---------------------------------------------------------------------------------------------
def test_against_the_model(ctx):
    """the two channels of the decided pink material as two signals from fresh pools: the model's checks hold on the rows
    interleaved the way the model's stereo stream lays them out"""
    chans = BMO.material('pink')
    res = ctx.encode_signals_measured_modes(chans, list(MM.PINK_SF_CANDIDATES), scale_factor_offsets=MM.OFFSETS, return_distortion=True,
                                            return_shifts=True)
    got = {}
    for k, per_signal in zip(OUTPUTS, res):
        a = np.zeros((2 * len(per_signal[0]),) + per_signal[0].shape[1:], dtype=per_signal[0].dtype)
        a[0::2], a[1::2] = per_signal[0], per_signal[1]
        got[k] = a
    assert MM.check_outputs('pink', True, got) is None


# ---- 4. loud and quiet neighbours -----------------------------------------------------------------------------------------
def test_loud_then_silent_neighbours(ctx):
    want = SMM.want(ctx, 'c', 'detect', 'three-offsets', True, material='loud_quiet')
    got = run3(ctx, material='loud_quiet')
    assert SMM.first_bad(got, want) is None, SMM.first_bad(got, want)
    # the all-zero signal behind the full-scale one, from a fresh pool: nothing to code, nothing of its neighbour in its rows
    zero = SL.LENGTHS.index(2, 8)
    assert not SMM.signals('loud_quiet')[zero].any()
    fresh = run3(ctx, pools=False, material='loud_quiet')
    assert not fresh['energy'][zero].any() and not fresh['distortion'][zero].any() and not fresh['taken'][zero].any()
    assert not fresh['choice'][zero].any()                                           # a tie of zeros: the first candidate


# ---- 5. chunking, the measuring kernel, the route -------------------------------------------------------------------------
def test_internal_chunking_is_invisible(ctx):
    small = _context(C1_CHUNK_FRAMES=96)                               # bulk chunks that cut the 130-frame signal
    try:
        for oname in ('detect', 'long'):
            got = run3(small, oname)
            want = SMM.want(ctx, 'c', oname, 'three-offsets', True)
            assert SMM.first_bad(got, want) is None, (oname, SMM.first_bad(got, want))
    finally:
        small.close()
    lengths = [(1, 2, 3)[i % 3] for i in range(40)]                    # row chunks of 16 over 40 and 27 start rows
    sigs = SL.signals('pink', lengths)
    pools = SL.enc_pools(40, 0x5252)
    want = SMM.compose(ctx, sigs, 'detect', CAND3, OFFS, pools)
    tiny = _context(C1_CHUNK_FRAMES=16)
    try:
        got = run3(tiny, sigs=sigs, states=pools)
        assert SMM.first_bad(got, want) is None, SMM.first_bad(got, want)
    finally:
        tiny.close()
    got = run3(ctx, sigs=sigs, states=pools)
    assert SMM.first_bad(got, want) is None, ('one chunk', SMM.first_bad(got, want))


@pytest.mark.parametrize('env', [{'C1_MEASURED_WIDE': 0}, {'C1_MEASURED_WIDE': 1}, {'C1_SIGNAL_STARTS': 0}, {'C1_SIGNAL_STARTS': 1}],
                         ids=['narrow', 'wide', 'starts0', 'starts1'])
def test_context_settings_give_the_same_bits(ctx, env):
    other = _context(**env)
    try:
        for config, (cand, offs) in SMM.CONFIGS.items():
            got = SMM.run(other, 'detect', cand, offs, True)
            want = SMM.want(ctx, 'c', 'detect', config, True)
            assert SMM.first_bad(got, want) is None, (env, config, SMM.first_bad(got, want))
    finally:
        other.close()


def test_speculation_mode_does_not_matter(ctx):
    want = SMM.want(ctx, 'c', 'detect', 'three-offsets', True)
    other = c1.Context(0)
    try:
        for mode in (0, 1, 2):
            other.set_speculation(mode)
            got = run3(other)
            assert SMM.first_bad(got, want) is None, (mode, SMM.first_bad(got, want))
    finally:
        other.close()


# ---- 6. edge calls --------------------------------------------------------------------------------------------------------
def raw(ctx, lengths, sigs, states, ask, out_states='new', oname='detect', cand=CAND3, offsets=OFFS):
    """c1_encode_signals_measured_modes itself with any subset of the outputs, the others NULL -> (rc, dict of all buffers, the
    ones not asked for still at their fill, 'out' the states written)"""
    off = SL.offsets(lengths)
    total, n, k = int(off[-1]), len(lengths), len(cand)
    pcm = np.ascontiguousarray(np.concatenate(sigs) if total else np.zeros(0, dtype=np.float32), dtype=np.float32)
    shape = {'units': ((total, 212), np.uint8), 'choice': ((total,), np.uint8), 'modes': ((total,), np.uint8), 'taken': ((total,), np.uint8),
             'shifts': ((total, 52), np.int8), 'distortion': ((total, k, 2), np.float64), 'energy': ((total, k), np.float64)}
    out = {key: np.full(sh, FILL[key], dtype=d) for key, (sh, d) in shape.items()}
    st = None if states is None else np.ascontiguousarray(states, dtype=np.float32).copy()
    st_out = st if out_states == 'in_place' else (np.full((n, SS.ENC_FLOATS), 7.5, dtype=np.float32) if out_states == 'new' else None)
    cb = np.ascontiguousarray(list(cand) + [0] * 9, dtype=np.uint8)
    o = None if offsets is None else np.ascontiguousarray(list(offsets) + [0] * 9, dtype=np.int8)
    data = lambda a: None if a is None else a.ctypes.data
    copts = SMM.opts(oname).to_c()
    rc = capi.load().c1_encode_signals_measured_modes(ctx._h, n, off.ctypes.data_as(I64P), pcm.ctypes.data, data(st), C.byref(copts),
                                                      cb.ctypes.data, k, data(o), 0 if offsets is None else len(offsets),
                                                      out['units'].ctypes.data if 'units' in ask else None, data(st_out),
                                                      *[out[key].ctypes.data if key in ask else None for key in OUTPUTS[1:]])
    out['out'] = st_out
    return rc, out


def untouched(out, keys):
    return all((out[k] == FILL[k]).all() for k in keys)


def test_edge_calls(ctx):
    sigs, pools = SMM.signals('pink'), SMM.enc_pools()
    full = SMM.want(ctx, 'c', 'detect', 'three-offsets', True)
    cat = {k: np.concatenate(full[k]) for k in OUTPUTS}
    # n == 0
    rc, out = raw(ctx, [], [], None, OUTPUTS)
    assert rc == C1_OK
    # all signals empty: out == in rows, nothing else written
    rc, out = raw(ctx, [0, 0, 0], [np.zeros(0, dtype=np.float32)] * 3, pools[:3], OUTPUTS)
    assert rc == C1_OK and np.array_equal(SS.bits(out['out']), SS.bits(pools[:3]))
    rc, out = raw(ctx, [0, 0], [np.zeros(0, dtype=np.float32)] * 2, None, OUTPUTS)
    assert rc == C1_OK and not out['out'].view(np.uint32).any()
    # in place, and out NULL
    rc, out = raw(ctx, SL.LENGTHS, sigs, pools, OUTPUTS, out_states='in_place')
    assert rc == C1_OK and np.array_equal(SS.bits(out['out']), SS.bits(full['states']))
    assert all(np.array_equal(SMM.bits(out[k]), SMM.bits(cat[k])) for k in OUTPUTS)
    rc, out = raw(ctx, SL.LENGTHS, sigs, pools, OUTPUTS, out_states=None)
    assert rc == C1_OK and all(np.array_equal(SMM.bits(out[k]), SMM.bits(cat[k])) for k in OUTPUTS)
    rc, out = raw(ctx, SL.LENGTHS, sigs, None, OUTPUTS, out_states=None)              # fresh pools, no states at all
    fresh = SMM.want(ctx, 'c', 'detect', 'three-offsets', False)
    assert rc == C1_OK and all(np.array_equal(SMM.bits(out[k]), SMM.bits(np.concatenate(fresh[k]))) for k in OUTPUTS)
    # units NULL with only choice asked for: measure only
    rc, out = raw(ctx, SL.LENGTHS, sigs, pools, ('choice',))
    assert rc == C1_OK and np.array_equal(out['choice'], cat['choice']) and untouched(out, [k for k in OUTPUTS if k != 'choice'])
    assert np.array_equal(SS.bits(out['out']), SS.bits(full['states']))
    # the optional outputs NULL one at a time: the others, units included, unchanged
    for missing in OUTPUTS[1:]:
        rc, out = raw(ctx, SL.LENGTHS, sigs, pools, [k for k in OUTPUTS if k != missing])
        assert rc == C1_OK and untouched(out, [missing]), missing
        assert all(np.array_equal(SMM.bits(out[k]), SMM.bits(cat[k])) for k in OUTPUTS if k != missing), missing
    # shifts without offsets are zeros; nothing to report is an error and writes nothing
    rc, out = raw(ctx, SL.LENGTHS, sigs, pools, ('units', 'shifts'), offsets=None)
    assert rc == C1_OK and not out['shifts'].any()
    rc, out = raw(ctx, SL.LENGTHS, sigs, pools, ())
    assert rc == C1_ERR_ARG and untouched(out, OUTPUTS) and (out['out'] == 7.5).all()
    rc, out = raw(ctx, SL.LENGTHS, sigs, pools, OUTPUTS, cand=(0, 58, 0))
    assert rc == C1_ERR_ARG and untouched(out, OUTPUTS) and (out['out'] == 7.5).all()


# ---- 7. launch counts -----------------------------------------------------------------------------------------------------
def test_launch_counts(ctx):
    """one 11-signal call: the search runs once per bulk chunk and once over each of the two passes of start rows"""
    sigs = SMM.signals('pink')
    whole = [np.concatenate(sigs)]
    ctx.set_profiling(True)
    try:
        ctx.encode_measured_modes(whole, list(CAND3), options=SMM.opts('detect'), scale_factor_offsets=OFFS)
        bulk = ctx.kernel_ms('measure')[1]
        run3(ctx)
        measure, starts = ctx.kernel_ms('measure')[1], ctx.kernel_ms('signal_starts')[1]
    finally:
        ctx.set_profiling(False)
    assert bulk >= 1 and measure == bulk + 2, (bulk, measure)
    assert starts >= 2 * 2 + 2 + 1, starts               # two analyses and a scatter per pass, then the signal ends


# ---- 8. stability ---------------------------------------------------------------------------------------------------------
def test_the_same_call_gives_the_same_bytes(ctx):
    want = SMM.want(ctx, 'c', 'detect', 'three-offsets', True)
    assert SMM.first_bad(run3(ctx), want) is None
    assert SMM.first_bad(run3(ctx), want) is None
    ctx.encode_signals_measured(SMM.signals('pink'), options=SMM.opts('short_bias2'), states=SMM.enc_pools(), scale_factor_offsets=OFFS,
                                masking=True)
    assert SMM.first_bad(run3(ctx), want) is None


# ---- 9. the device form, a caller's stream --------------------------------------------------------------------------------
def device_call(ctx, config='three-offsets'):
    import torch
    cand, offs = SMM.CONFIGS[config]
    off = SL.offsets(SL.LENGTHS)
    n, total, k = len(SL.LENGTHS), int(off[-1]), len(cand)
    GUARD = 4096
    dev = 'cuda:0'
    pcm = torch.from_numpy(np.concatenate(SMM.signals('pink'))).to(dev)
    st_in = torch.from_numpy(SMM.enc_pools().copy()).to(dev)
    st_out = torch.full((n * SS.ENC_FLOATS + GUARD,), 7.5, dtype=torch.float32, device=dev)
    width = {'units': 212, 'choice': 1, 'modes': 1, 'taken': 1, 'shifts': 52, 'distortion': 2 * k, 'energy': k}
    dtype = {'units': torch.uint8, 'choice': torch.uint8, 'modes': torch.uint8, 'taken': torch.uint8, 'shifts': torch.int8,
             'distortion': torch.float64, 'energy': torch.float64}
    t = {key: torch.full((total * width[key] + GUARD,), FILL[key], dtype=dtype[key], device=dev) for key in OUTPUTS}
    torch.cuda.synchronize()
    ctx.encode_signals_measured_modes_device(off, pcm.data_ptr(), list(cand), units_ptr=t['units'].data_ptr(), states_ptr=st_in.data_ptr(),
                                             out_states_ptr=st_out.data_ptr(), options=SMM.opts('detect'), scale_factor_offsets=offs,
                                             choice_ptr=t['choice'].data_ptr(), modes_ptr=t['modes'].data_ptr(),
                                             taken_ptr=t['taken'].data_ptr(), shifts_ptr=t['shifts'].data_ptr(),
                                             distortion_ptr=t['distortion'].data_ptr(), energy_ptr=t['energy'].data_ptr())
    ctx.synchronize()
    got = {}
    for key in OUTPUTS:
        a = t[key].cpu().numpy()
        assert (a[total * width[key]:] == FILL[key]).all(), (key, 'stored past its buffer')
        shape = {'units': (total, 212), 'shifts': (total, 52), 'distortion': (total, k, 2), 'energy': (total, k)}.get(key, (total,))
        rows = a[:total * width[key]].reshape(shape)
        got[key] = [rows[int(off[i]):int(off[i + 1])] for i in range(n)]
    s = st_out.cpu().numpy()
    assert (s[n * SS.ENC_FLOATS:] == 7.5).all()
    got['states'] = s[:n * SS.ENC_FLOATS].reshape(n, -1)
    return got


@pytest.mark.parametrize('config', list(SMM.CONFIGS))
def test_device_form_from_torch_tensors(ctx, config):
    got = device_call(ctx, config)
    want = SMM.want(ctx, 'c', 'detect', config, True)
    assert SMM.first_bad(got, want) is None, SMM.first_bad(got, want)


def test_on_a_callers_stream(ctx):
    import torch
    S = torch.cuda.Stream()
    c = _context(stream=S.cuda_stream)
    try:
        want = SMM.want(ctx, 'c', 'detect', 'three-offsets', True)
        got = run3(c)
        assert SMM.first_bad(got, want) is None, SMM.first_bad(got, want)
        with torch.cuda.stream(S):
            got = device_call(c)
        assert SMM.first_bad(got, want) is None, ('device form', SMM.first_bad(got, want))
    finally:
        c.close()
