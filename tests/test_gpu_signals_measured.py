"""GPU: the measured allocation for n signals of any lengths in one call (c1_encode_signals_measured*,
Context.encode_signals_measured) against the composition the header defines it by (tests/signals_measured_lib.py: one mono
EncoderStream per signal, set_state, one push_measured, get_state), on both routes of the signal starts (C1_SIGNAL_STARTS 0: two
passes of the from-state kernel, 1: one pass of k_encode_signal_starts), and against the CPU model of tests/masked_alloc_lib.py.
Every comparison is bitwise (doubles as bit patterns); only the model's own check_outputs keeps its REL."""
import ctypes as C
import os

import numpy as np
import pytest

import carta1_amd as c1
from carta1_amd import capi
import best_modes_lib as BMO
import masked_alloc_lib as MK
import measured_alloc_lib as MA
import scale_factor_choice_lib as SF
import signals_lib as SL
import signals_measured_lib as SGM
import stream_state_lib as SS

pytestmark = pytest.mark.gpu

C1_OK, C1_ERR_ARG = 0, 1   # include/carta1_hip.h
I64P = C.POINTER(C.c_int64)
ONAMES = list(SL.OPTION_SETS)
DEFS = list(SGM.DEFINITIONS)
SHORT = 48                                       # frames of the decided models (tests/test_gpu_masked_alloc.py's)
FILL = {'units': 0xA5, 'taken': 0xA5, 'shifts': 0x5A, 'distortion': -1.0, 'energy': -1.0, 'weights': -1.0}


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
def fused():
    c = _context(C1_SIGNAL_STARTS=1)
    yield c
    c.close()


@pytest.fixture(scope='module')
def twopass():
    c = _context(C1_SIGNAL_STARTS=0)
    yield c
    c.close()


def run(ctx, oname, definition, pools, material='pink', modes=None, sigs=None, states=None):
    """Context.encode_signals_measured with everything the definition reports and the pools after -> dict"""
    sigs = SGM.signals(material) if sigs is None else sigs
    st = states if states is not None else (SGM.enc_pools() if pools else None)
    res = ctx.encode_signals_measured(sigs, modes=modes, options=SGM.opts(oname), states=st, return_states=True, **SGM.ask(definition))
    return SGM.named(res, definition)


# ---- 1. composition -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('definition', DEFS)
@pytest.mark.parametrize('pools', [False, True], ids=['fresh', 'pools'])
@pytest.mark.parametrize('oname', ONAMES)
def test_fused_route_equals_the_composition(fused, oname, pools, definition):
    """units, taken, shifts, distortion, energy, weights and the pools of the shared shapes equal one stream per signal"""
    want = SGM.want(fused, 'c', oname, definition, pools)
    got = run(fused, oname, definition, pools)
    assert SGM.first_bad(got, want) is None, (oname, pools, definition, SGM.first_bad(got, want))
    assert sum(int(t.sum()) for t in got['taken']) > 0


@pytest.mark.parametrize('pools', [False, True], ids=['fresh', 'pools'])
@pytest.mark.parametrize('oname', ONAMES)
def test_two_pass_route_equals_the_composition_and_the_fused_route(fused, twopass, oname, pools):
    want = SGM.want(fused, 'c', oname, 'masked_offsets', pools)
    got = run(twopass, oname, 'masked_offsets', pools)
    assert SGM.first_bad(got, want) is None, (oname, pools, SGM.first_bad(got, want))
    other = run(fused, oname, 'masked_offsets', pools)
    assert SGM.first_bad(got, other) is None, ('route against route', oname, pools, SGM.first_bad(got, other))


# ---- 2. given modes -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('route', ['fused', 'twopass'])
def test_given_modes(fused, twopass, route):
    """the eight domain bytes cycling by frame under detection options, from pools: the rows are the composition's under the same
    mode rows, and transient_mags passes from in[i] to out[i]"""
    ctx = fused if route == 'fused' else twopass
    want = SGM.want(fused, 'c', 'detect', 'masked_offsets', True, with_modes=True)
    got = run(ctx, 'detect', 'masked_offsets', True, modes=SGM.mode_rows())
    assert SGM.first_bad(got, want) is None, SGM.first_bad(got, want)
    assert np.array_equal(SS.bits(got['states'][:, 227:]), SS.bits(SGM.enc_pools()[:, 227:]))
    # the modes decide: the units carry their byte's block modes, and differ from the call without modes
    free = run(ctx, 'detect', 'masked_offsets', True)
    assert SGM.first_bad(got, free) is not None
    rows = np.concatenate(SGM.mode_rows())
    first = np.concatenate(got['units'])[:, 0]
    want_first = np.array([((2 - (b & 3)) << 6) | ((2 - ((b >> 2) & 3)) << 4) | ((3 - ((b >> 4) & 3)) << 2) for b in rows])
    assert np.array_equal(first & 0xfc, want_first)


# ---- 3. against the CPU model ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('route', ['fused', 'twopass'])
@pytest.mark.parametrize('kind', ['detect', 'fixed'])
def test_against_the_model(fused, twopass, route, kind):
    """the two channels of the decided material as two signals from fresh pools: the model's checks hold per signal on the rows
    de-interleaved from the model's"""
    ctx = fused if route == 'fused' else twopass
    chans = [c[:SHORT * 512] for c in BMO.material('pink')]
    m = MK.case(kind, 'pink', 'packaged', SF.OFFSETS, SHORT)
    o = c1.EncoderOptions({'fixedBlockModes': MA.FIXED} if kind == 'fixed' else {})
    res = SGM.named(ctx.encode_signals_measured(chans, options=o, return_states=True, **SGM.ask('masked_offsets')), 'masked_offsets')
    n = len(m['taken'])
    for c in range(2):
        mc = {k: (v[c::2] if getattr(v, 'ndim', 0) and v.shape[0] == n else v) for k, v in m.items()}
        bad = MK.check_outputs(mc, res['units'][c], res['taken'][c], res['shifts'][c], res['distortion'][c], res['energy'][c], res['weights'][c])
        assert bad is None, (kind, c, bad)


# ---- 4. loud and quiet neighbours -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('route', ['fused', 'twopass'])
def test_loud_then_silent_neighbours(fused, twopass, route):
    ctx = fused if route == 'fused' else twopass
    want = SGM.want(fused, 'c', 'detect', 'masked_offsets', True, material='loud_quiet')
    got = run(ctx, 'detect', 'masked_offsets', True, material='loud_quiet')
    assert SGM.first_bad(got, want) is None, SGM.first_bad(got, want)
    # the all-zero signal behind the full-scale one, from a fresh pool: nothing to code, nothing of its neighbour in its rows
    zero = SL.LENGTHS.index(2, 8)
    assert not SGM.signals('loud_quiet')[zero].any()
    fresh = run(ctx, 'detect', 'masked_offsets', False, material='loud_quiet')
    assert not fresh['energy'][zero].any() and not fresh['distortion'][zero].any() and not fresh['taken'][zero].any()

# ---- 5. chunking ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('route', [1, 0], ids=['fused', 'twopass'])
def test_internal_chunking_is_invisible(fused, route):
    base = fused
    small = _context(C1_CHUNK_FRAMES=96, C1_SIGNAL_STARTS=route)       # bulk chunks that cut the 130-frame signal
    try:
        for oname in ('detect', 'long'):
            got = run(small, oname, 'masked_offsets', True)
            want = run(base, oname, 'masked_offsets', True)
            assert SGM.first_bad(got, want) is None, (oname, SGM.first_bad(got, want))
    finally:
        small.close()
    lengths = [(1, 2, 3, 5)[i % 4] for i in range(40)]                 # row chunks of 16: pairs must not be split
    sigs = SL.signals('pink', lengths)
    pools = SL.enc_pools(40, 0x5252)
    tiny = _context(C1_CHUNK_FRAMES=16, C1_SIGNAL_STARTS=route)
    try:
        got = run(tiny, 'detect', 'masked_offsets', True, sigs=sigs, states=pools)
        want = run(base, 'detect', 'masked_offsets', True, sigs=sigs, states=pools)
        assert SGM.first_bad(got, want) is None, SGM.first_bad(got, want)
        m = SGM.mode_rows(lengths)
        got = run(tiny, 'detect', 'masked_offsets', True, sigs=sigs, states=pools, modes=m)
        want = run(base, 'detect', 'masked_offsets', True, sigs=sigs, states=pools, modes=m)
        assert SGM.first_bad(got, want) is None, ('modes', SGM.first_bad(got, want))
    finally:
        tiny.close()


# ---- 6. the measuring kernel ----------------------------------------------------------------------------------------------
def test_narrow_measuring_kernel_gives_the_same_bits(fused):
    narrow = _context(C1_MEASURED_WIDE=0, C1_SIGNAL_STARTS=1)
    try:
        for definition in DEFS:
            got = run(narrow, 'detect', definition, True)
            want = run(fused, 'detect', definition, True)
            assert SGM.first_bad(got, want) is None, (definition, SGM.first_bad(got, want))
    finally:
        narrow.close()


# ---- 7. edge calls --------------------------------------------------------------------------------------------------------
def raw(ctx, lengths, sigs, states, ask, out_states='new', oname='detect', offsets=SF.OFFSETS, tables='packaged'):
    """c1_encode_signals_measured itself with any subset of the outputs, the others NULL -> (rc, dict of all buffers, the ones
    not asked for still at their fill, 'out' the states written)"""
    off = SL.offsets(lengths)
    total, n = int(off[-1]), len(lengths)
    pcm = np.ascontiguousarray(np.concatenate(sigs) if total else np.zeros(0, dtype=np.float32), dtype=np.float32)
    shape = {'units': ((total, 212), np.uint8), 'taken': ((total,), np.uint8), 'shifts': ((total, 52), np.int8),
             'distortion': ((total, 2), np.float64), 'energy': ((total,), np.float64), 'weights': ((total, 52), np.float64)}
    out = {k: np.full(sh, FILL[k], dtype=d) for k, (sh, d) in shape.items()}
    st = None if states is None else np.ascontiguousarray(states, dtype=np.float32).copy()
    st_out = st if out_states == 'in_place' else (np.full((n, SS.ENC_FLOATS), 7.5, dtype=np.float32) if out_states == 'new' else None)
    o = None if offsets is None else np.ascontiguousarray(list(offsets) + [0] * 9, dtype=np.int8)
    floor, spread = (None, None) if tables is None else MK.named(tables)
    floor = None if floor is None else np.ascontiguousarray(floor, dtype=np.float64)
    spread = None if spread is None else np.ascontiguousarray(spread, dtype=np.float64)
    data = lambda a: None if a is None else a.ctypes.data
    copts = SGM.opts(oname).to_c()
    rc = capi.load().c1_encode_signals_measured(ctx._h, n, off.ctypes.data_as(I64P), pcm.ctypes.data, data(st), C.byref(copts), None, data(o),
                                                0 if offsets is None else len(offsets), data(floor), data(spread),
                                                out['units'].ctypes.data if 'units' in ask else None, data(st_out),
                                                *[out[k].ctypes.data if k in ask else None for k in SGM.OUTPUTS[1:]])
    out['out'] = st_out
    return rc, out


def untouched(out, keys):
    return all((out[k] == FILL[k]).all() for k in keys)


@pytest.mark.parametrize('route', ['fused', 'twopass'])
def test_edge_calls(fused, twopass, route):
    ctx = fused if route == 'fused' else twopass
    sigs, pools = SGM.signals('pink'), SGM.enc_pools()
    full = run(ctx, 'detect', 'masked_offsets', True)
    cat = {k: np.concatenate(full[k]) for k in SGM.OUTPUTS}
    # n == 0
    rc, out = raw(ctx, [], [], None, SGM.OUTPUTS)
    assert rc == C1_OK
    # all signals empty: out == in rows, nothing else written
    rc, out = raw(ctx, [0, 0, 0], [np.zeros(0, dtype=np.float32)] * 3, pools[:3], SGM.OUTPUTS)
    assert rc == C1_OK and np.array_equal(SS.bits(out['out']), SS.bits(pools[:3]))
    rc, out = raw(ctx, [0, 0], [np.zeros(0, dtype=np.float32)] * 2, None, SGM.OUTPUTS)
    assert rc == C1_OK and not out['out'].view(np.uint32).any()
    # in place, and out NULL
    rc, out = raw(ctx, SL.LENGTHS, sigs, pools, SGM.OUTPUTS, out_states='in_place')
    assert rc == C1_OK and np.array_equal(SS.bits(out['out']), SS.bits(full['states']))
    assert all(np.array_equal(SGM.bits(out[k]), SGM.bits(cat[k])) for k in SGM.OUTPUTS)
    rc, out = raw(ctx, SL.LENGTHS, sigs, pools, SGM.OUTPUTS, out_states=None)
    assert rc == C1_OK and all(np.array_equal(SGM.bits(out[k]), SGM.bits(cat[k])) for k in SGM.OUTPUTS)
    # units NULL with only taken asked for: measure only
    rc, out = raw(ctx, SL.LENGTHS, sigs, pools, ('taken',))
    assert rc == C1_OK and np.array_equal(out['taken'], cat['taken']) and untouched(out, [k for k in SGM.OUTPUTS if k != 'taken'])
    assert np.array_equal(SS.bits(out['out']), SS.bits(full['states']))
    # the optional outputs NULL one at a time: the others, units included, unchanged
    for missing in SGM.OUTPUTS[1:]:
        rc, out = raw(ctx, SL.LENGTHS, sigs, pools, [k for k in SGM.OUTPUTS if k != missing])
        assert rc == C1_OK and untouched(out, [missing]), missing
        assert all(np.array_equal(SGM.bits(out[k]), SGM.bits(cat[k])) for k in SGM.OUTPUTS if k != missing), missing
    # shifts without offsets are zeros; nothing to report is an error and writes nothing
    rc, out = raw(ctx, SL.LENGTHS, sigs, pools, ('units', 'shifts'), offsets=None, tables=None)
    assert rc == C1_OK and not out['shifts'].any()
    rc, out = raw(ctx, SL.LENGTHS, sigs, pools, ())
    assert rc == C1_ERR_ARG and untouched(out, SGM.OUTPUTS) and (out['out'] == 7.5).all()


# ---- 8. launch counts -----------------------------------------------------------------------------------------------------
def test_launch_counts(fused, twopass):
    """one 11-signal call: the measured step runs once over the signal starts on the fused route, twice on the two-pass one"""
    sigs = SGM.signals('pink')
    whole = [np.concatenate(sigs)]
    counts = {}
    for name, ctx in (('fused', fused), ('twopass', twopass)):
        ctx.set_profiling(True)
        try:
            ctx.encode_measured(whole, options=SGM.opts('detect'), scale_factor_offsets=SGM.OFFSETS, masking=True)
            bulk = ctx.kernel_ms('measure')[1]
            ctx.encode_signals_measured(sigs, options=SGM.opts('detect'), states=SGM.enc_pools(), return_states=True, **SGM.ask('masked_offsets'))
            counts[name] = (bulk, ctx.kernel_ms('measure')[1], ctx.kernel_ms('signal_starts')[1])
        finally:
            ctx.set_profiling(False)
    assert counts['fused'][0] >= 1 and counts['fused'][0] == counts['twopass'][0]
    assert counts['fused'][1] == counts['fused'][0] + 1, counts
    assert counts['twopass'][1] == counts['twopass'][0] + 2, counts
    assert counts['fused'][2] < counts['twopass'][2], counts


# ---- 9. stability ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('route', ['fused', 'twopass'])
def test_the_same_call_gives_the_same_bytes(fused, twopass, route):
    ctx = fused if route == 'fused' else twopass
    first = run(ctx, 'detect', 'masked_offsets', True)
    assert SGM.first_bad(run(ctx, 'detect', 'masked_offsets', True), first) is None
    plain = ctx.encode_signals(SGM.signals('pink'), SGM.opts('short_bias2'), states=SGM.enc_pools())
    assert SL.same_units(plain, SL.want_encode('pink', 'short_bias2', True)[0])
    assert SGM.first_bad(run(ctx, 'detect', 'masked_offsets', True), first) is None


# ---- 10. the device form --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('with_modes', [False, True], ids=['detect', 'modes'])
@pytest.mark.parametrize('route', ['fused', 'twopass'])
def test_device_form_from_torch_tensors(fused, twopass, route, with_modes):
    import torch
    ctx = fused if route == 'fused' else twopass
    want = SGM.want(fused, 'c', 'detect', 'masked_offsets', True, with_modes=with_modes)
    off = SL.offsets(SL.LENGTHS)
    n, total = len(SL.LENGTHS), int(off[-1])
    GUARD = 4096
    dev = 'cuda:0'
    pcm = torch.from_numpy(np.concatenate(SGM.signals('pink'))).to(dev)
    modes = torch.from_numpy(np.concatenate(SGM.mode_rows())).to(dev) if with_modes else None
    st_in = torch.from_numpy(SGM.enc_pools().copy()).to(dev)
    st_out = torch.full((n * SS.ENC_FLOATS + GUARD,), 7.5, dtype=torch.float32, device=dev)
    units = torch.full((total * 212 + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    taken = torch.full((total + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    shifts = torch.full((total * 52 + GUARD,), 0x5A, dtype=torch.int8, device=dev)
    dist = torch.full((total * 2 + GUARD,), -1.0, dtype=torch.float64, device=dev)
    energy = torch.full((total + GUARD,), -1.0, dtype=torch.float64, device=dev)
    weights = torch.full((total * 52 + GUARD,), -1.0, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    ctx.encode_signals_measured_device(off, pcm.data_ptr(), units.data_ptr(), st_in.data_ptr(), st_out.data_ptr(), options=SGM.opts('detect'),
                                       modes_ptr=modes.data_ptr() if with_modes else None, scale_factor_offsets=SGM.OFFSETS, masking=True,
                                       taken_ptr=taken.data_ptr(), shifts_ptr=shifts.data_ptr(), distortion_ptr=dist.data_ptr(),
                                       energy_ptr=energy.data_ptr(), weights_ptr=weights.data_ptr())
    ctx.synchronize()
    host = {'units': (units, 212, 0xA5), 'taken': (taken, 1, 0xA5), 'shifts': (shifts, 52, 0x5A), 'distortion': (dist, 2, -1.0),
            'energy': (energy, 1, -1.0), 'weights': (weights, 52, -1.0)}
    got = {}
    for k, (t, width, fill) in host.items():
        a = t.cpu().numpy()
        assert (a[total * width:] == fill).all(), (k, 'stored past its buffer')
        rows = a[:total * width].reshape((total, width) if width > 1 else (total,))
        got[k] = [rows[int(off[i]):int(off[i + 1])] for i in range(n)]
    s = st_out.cpu().numpy()
    assert (s[n * SS.ENC_FLOATS:] == 7.5).all()
    got['states'] = s[:n * SS.ENC_FLOATS].reshape(n, -1)
    assert SGM.first_bad(got, want) is None, SGM.first_bad(got, want)
