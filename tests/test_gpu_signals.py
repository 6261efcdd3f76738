"""n signals of any lengths from their own pools in one call (c1_*_signals*, Context.encode_signals / decode_signals, the
*_aea_pcm_many functions) against n separate oracle closures (tests/signals_lib.py) or an existing oracle-pinned entry point.
Everything compares bytes or uint32 views for equality, except the opt-in binary32 decoder, which keeps
test_gpu_decode32.py's tolerance."""
import ctypes as C
import os

import numpy as np
import pytest

import carta1_amd as c1
from carta1_amd import capi
import oracle_lib as O
import signals_lib as SL
import stream_state_lib as SS

pytestmark = pytest.mark.gpu

C1_ERR_ARG = 1   # include/carta1_hip.h
ONAMES = list(SL.OPTION_SETS)
I64P = C.POINTER(C.c_int64)


@pytest.fixture(scope='module')
def ctx():
    c = c1.Context(0)
    yield c
    c.close()


def opts(oname):
    return c1.EncoderOptions(dict(SL.OPTION_SETS[oname]))


def check_encode(got_u, got_s, want_u, want_s, where):
    assert SL.same_units(got_u, want_u), (where, SL.first_bad(got_u, want_u))
    if got_s is not None:
        bad = np.flatnonzero((SS.bits(got_s) != SS.bits(want_s)).any(axis=1))
        assert bad.size == 0, (where, 'pools of signals', list(bad[:8]))


def check_decode(got_p, got_s, want_p, want_s, where):
    assert len(got_p) == len(want_p)
    for i, (g, w) in enumerate(zip(got_p, want_p)):
        assert SL.same_bits(g, w), (where, 'signal', i, list(np.flatnonzero((SS.bits(g) != SS.bits(w)).reshape(-1, 512).any(axis=1))[:6]))
    if got_s is not None:
        bad = np.flatnonzero((SS.bits(got_s) != SS.bits(want_s)).any(axis=1))
        assert bad.size == 0, (where, 'pools of signals', list(bad[:8]))


# ---- 1, 2: the oracle, every option set, fresh pools and random pools, in place -------------------------------------------
@pytest.mark.parametrize('pools', [False, True], ids=['fresh', 'pools'])
@pytest.mark.parametrize('oname', ONAMES)
def test_encode_signals_equal_the_oracle(ctx, oname, pools):
    """Units and pools of the shared shapes equal n oracle closures.  For [0,0,0] and detection under every speculation mode;
    in mode 2 the statistics show that the call did speculate: c1_ctx_speculation_stats counts the units of the binary32
    analysis, which only fixed modes take, so under detection the counter read is the speculative
    detector's (c1_ctx_detection_stats)."""
    sigs = SL.signals('pink')
    start = SL.enc_pools() if pools else None
    want_u, want_s = SL.want_encode('pink', oname, pools)
    modes = (1, 0, 2) if oname in ('long', 'detect') else (1,)
    try:
        for mode in modes:
            ctx.set_speculation(mode)
            ctx.speculation_stats(reset=True)
            got_u, got_s = ctx.encode_signals(sigs, opts(oname), states=start, return_states=True)
            check_encode(got_u, got_s, want_u, want_s, (oname, pools, mode))
            if mode == 2:
                n = ctx.speculation_stats()[0] if oname == 'long' else ctx.detection_stats()[0]
                assert n > 0, ('the call never speculated', oname)
            if pools and oname in SL.FIXED:
                assert SL.same_bits(got_s[:, 227:], start[:, 227:])          # transient_mags passes through under fixed modes
            if not pools:
                for i, n in enumerate(SL.LENGTHS):
                    if n == 0:
                        assert not got_s[i].view(np.uint32).any()             # an empty signal from a fresh pool: zeros
    finally:
        ctx.set_speculation(1)
    if pools:                                                                 # out == in
        work = start.copy()
        got_u, got_s = ctx.encode_signals(sigs, opts(oname), states=work, in_place=True)
        assert np.shares_memory(got_s, work)
        check_encode(got_u, work, want_u, want_s, (oname, 'in place'))
    got_u = ctx.encode_signals(sigs, opts(oname), states=start)               # out == NULL
    check_encode(got_u, None, want_u, None, (oname, pools, 'no pools out'))


@pytest.mark.parametrize('oname', ['detect', 'long'])
def test_encode_signals_loud_then_silent_neighbours(ctx, oname):
    """a full-scale white signal followed by an all-zero one and by one at 1e-30: nothing of a neighbour leaks into a signal"""
    want_u, want_s = SL.want_encode('loud_quiet', oname, True)
    for mode in (1, 2):
        ctx.set_speculation(mode)
        try:
            got_u, got_s = ctx.encode_signals(SL.signals('loud_quiet'), opts(oname), states=SL.enc_pools(), return_states=True)
        finally:
            ctx.set_speculation(1)
        check_encode(got_u, got_s, want_u, want_s, (oname, mode))


# ---- 3: chunk seams inside the 130-frame signal and next to signal starts -----------------------------------------------
def test_encode_signals_internal_chunking_is_invisible():
    old = os.environ.get('C1_CHUNK_FRAMES')
    os.environ['C1_CHUNK_FRAMES'] = '96'
    try:
        small = c1.Context(0)
    finally:
        if old is None:
            del os.environ['C1_CHUNK_FRAMES']
        else:
            os.environ['C1_CHUNK_FRAMES'] = old
    try:
        for oname in ONAMES:
            want_u, want_s = SL.want_encode('pink', oname, True)
            got_u, got_s = small.encode_signals(SL.signals('pink'), opts(oname), states=SL.enc_pools(), return_states=True)
            check_encode(got_u, got_s, want_u, want_s, oname)
    finally:
        small.close()


# ---- 4: ticks -----------------------------------------------------------------------------------------------------------
def test_encode_signals_ticks_carry_the_pools(ctx):
    """eight streams, three calls, a few frames per stream and call, pools carried in place; detection, then [0,2,0], then
    detection again: transient_mags survives the fixed-mode tick and is what the third tick's first frames are compared with"""
    rng = np.random.RandomState(4)
    schedule = ['detect', 'mixed_bias05', 'detect']
    lens = rng.choice([1, 2, 5], size=(3, 8))
    streams = [O.gen_pinkT(300 + s, int(lens[:, s].sum()) * 512) for s in range(8)]
    pools = np.zeros((8, SS.ENC_FLOATS), dtype=np.float32)
    want_pools = np.zeros_like(pools)
    at = np.zeros(8, dtype=np.int64)
    got = [[] for _ in range(8)]
    want = [[] for _ in range(8)]
    for t, oname in enumerate(schedule):
        parts = [streams[s][at[s] * 512:(at[s] + lens[t, s]) * 512] for s in range(8)]
        u, _ = ctx.encode_signals(parts, opts(oname), states=pools, in_place=True)
        wu, want_pools = SL.oracle_encode_signals(parts, SL.OPTION_SETS[oname], want_pools)
        for s in range(8):
            got[s].append(u[s])
            want[s].append(wu[s])
        at += lens[t]
    check_encode([np.concatenate(g) for g in got], pools, [np.concatenate(w) for w in want], want_pools, 'ticks')
    assert pools[:, 227:].any()


# ---- 5: equivalences with the existing entry points -----------------------------------------------------------------------
def test_encode_signals_of_one_frame_are_the_from_state_call(ctx):
    n = 9
    pcm = O.gen_pinkT(55, n * 512).reshape(n, 512)
    pools = SS.random_pools(0x321, n, SS.ENC_FLOATS)
    for oname in ('detect', 'short_bias2'):
        wu, ws = ctx.encode_frames_from_states(pcm, pools, opts(oname))
        u, s = ctx.encode_signals(list(pcm), opts(oname), states=pools, return_states=True)
        assert np.array_equal(np.concatenate(u), wu) and SL.same_bits(s, ws), oname


def test_one_signal_from_a_fresh_pool_is_encode(ctx):
    x = O.gen_pinkT(56, 70 * 512)
    for oname in ONAMES:
        assert np.array_equal(ctx.encode_signals([x], opts(oname))[0], ctx.encode([x], opts(oname))), oname


@pytest.mark.parametrize('name', sorted(SS.fixture()['cases']))
def test_signals_continue_the_references_dumped_pools(ctx, name):
    """tests/golden/stream_state.json: the reference's own pools after dump_at frames and its units of the frames after them;
    a stereo case is two signals"""
    fix = SS.fixture()
    e, dump, more = fix['cases'][name], fix['dump_at'], fix['more']
    sig, oname = name.split('/')
    oset = fix['option_sets'][oname]
    chans = SS.signal(fix['signals'][sig], dump + more)
    nch = len(chans)
    want = SS.units(e['units_more'])
    parts = [c[dump * 512:] for c in chans]
    u, s = ctx.encode_signals(parts, c1.EncoderOptions(dict(oset)), states=SS.states(e['enc_states'], SS.ENC_FLOATS), return_states=True)
    for c in range(nch):
        assert np.array_equal(u[c], want[c::nch]), (name, c)
    _, ws = SL.oracle_encode_signals(parts, oset, SS.states(e['enc_states'], SS.ENC_FLOATS))
    assert SL.same_bits(s, ws)
    p, d = ctx.decode_signals([want[c::nch] for c in range(nch)], states=SS.states(e['dec_states'], SS.DEC_FLOATS), return_states=True)
    wp, wd = SL.oracle_decode_signals([want[c::nch] for c in range(nch)], SS.states(e['dec_states'], SS.DEC_FLOATS))
    check_decode(p, d, wp, wd, name)


# ---- 6: past the grid step --------------------------------------------------------------------------------------------------
def test_signals_past_the_grid_step(ctx):
    """more signals than the bounded grid of the row kernels has workgroups (256 * 12), lengths alternating 1 and 2; in place"""
    n = 256 * 12 + 5
    lengths = [1 + (i & 1) for i in range(n)]
    off = SL.offsets(lengths)
    x = O.gen_pinkT(57, int(off[-1]) * 512)
    sigs = [x[off[i] * 512:off[i + 1] * 512] for i in range(n)]
    rng = np.random.default_rng(0x516)
    pools = rng.uniform(-1, 1, (n, SS.ENC_FLOATS)).astype(np.float32)
    dpools = rng.uniform(-1, 1, (n, SS.DEC_FLOATS)).astype(np.float32)
    want_u, want_s = SL.oracle_encode_signals(sigs, SL.OPTION_SETS['detect'], pools)
    work = pools.copy()
    u, _ = ctx.encode_signals(sigs, opts('detect'), states=work, in_place=True)
    check_encode(u, work, want_u, want_s, 'grid')
    want_p, want_d = SL.oracle_decode_signals(want_u, dpools)
    work = dpools.copy()
    p, _ = ctx.decode_signals(want_u, states=work, in_place=True)
    check_decode(p, work, want_p, want_d, 'grid')


# ---- 7: guards, on device pointers ------------------------------------------------------------------------------------------
def test_signals_device_pointers_keep_inside_their_buffers(ctx):
    import torch
    lengths, n, total = SL.LENGTHS, len(SL.LENGTHS), sum(SL.LENGTHS)
    off = SL.offsets(lengths)
    want_u, want_s = SL.want_encode('pink', 'detect', True)
    want_p, want_d = SL.want_decode('pink', 'detect', True)
    pcm = torch.from_numpy(np.concatenate(SL.signals('pink'))).to('cuda:0')
    GUARD = 4096
    units = torch.full((total * 212 + GUARD,), 0xA5, dtype=torch.uint8, device='cuda:0')
    st_in = torch.from_numpy(SL.enc_pools().copy()).to('cuda:0')
    st_out = torch.full(((n * SS.ENC_FLOATS + GUARD),), 7.5, dtype=torch.float32, device='cuda:0')
    torch.cuda.synchronize()
    ctx.encode_signals_device(off, pcm.data_ptr(), units.data_ptr(), st_in.data_ptr(), st_out.data_ptr(), options=opts('detect'))
    ctx.synchronize()
    u = units.cpu().numpy()
    assert np.array_equal(u[:total * 212].reshape(-1, 212), np.concatenate(want_u)) and (u[total * 212:] == 0xA5).all()
    s = st_out.cpu().numpy()
    got_s = s[:n * SS.ENC_FLOATS].reshape(n, -1)
    assert SL.same_bits(got_s, want_s) and (s[n * SS.ENC_FLOATS:] == 7.5).all()
    assert SL.same_bits(st_in.cpu().numpy(), SL.enc_pools())                 # `in` is only read
    for i, m in enumerate(lengths):
        if m == 0:
            assert SL.same_bits(got_s[i], SL.enc_pools()[i])                  # an empty signal's pool passes through bit for bit
    # in NULL, out given: empty signals export zeros
    st_out.fill_(7.5)
    ctx.encode_signals_device(off, pcm.data_ptr(), units.data_ptr(), None, st_out.data_ptr(), options=opts('detect'))
    ctx.synchronize()
    s = st_out.cpu().numpy()
    assert SL.same_bits(s[:n * SS.ENC_FLOATS].reshape(n, -1), SL.want_encode('pink', 'detect', False)[1]) and (s[n * SS.ENC_FLOATS:] == 7.5).all()
    # decode twin
    du = torch.from_numpy(np.concatenate(SL.want_encode('pink', 'detect', False)[0]).reshape(-1)).to('cuda:0')   # want_decode's units
    out = torch.full((total * 512 + GUARD,), 7.5, dtype=torch.float32, device='cuda:0')
    d_in = torch.from_numpy(SL.dec_pools().copy()).to('cuda:0')
    d_out = torch.full((n * SS.DEC_FLOATS + GUARD,), 7.5, dtype=torch.float32, device='cuda:0')
    torch.cuda.synchronize()
    ctx.decode_signals_device(off, du.data_ptr(), out.data_ptr(), d_in.data_ptr(), d_out.data_ptr())
    ctx.synchronize()
    p = out.cpu().numpy()
    assert SL.same_bits(p[:total * 512], np.concatenate(want_p)) and (p[total * 512:] == 7.5).all()
    d = d_out.cpu().numpy()
    got_d = d[:n * SS.DEC_FLOATS].reshape(n, -1)
    assert SL.same_bits(got_d, want_d) and (d[n * SS.DEC_FLOATS:] == 7.5).all()
    for i, m in enumerate(lengths):
        if m == 0:
            assert SL.same_bits(got_d[i], SL.dec_pools()[i])
    lib = capi.load()
    o = opts('detect').to_c()
    bad = np.array([0, 2, 1], dtype=np.int64)
    assert lib.c1_encode_signals_device(ctx._h, 2, bad.ctypes.data_as(I64P), pcm.data_ptr(), None, C.byref(o), units.data_ptr(), None) == C1_ERR_ARG
    assert lib.c1_decode_signals_device(ctx._h, 2, bad.ctypes.data_as(I64P), du.data_ptr(), None, out.data_ptr(), None) == C1_ERR_ARG


# ---- 8: a caller's stream ---------------------------------------------------------------------------------------------------
def test_signals_on_a_callers_stream():
    """on a torch stream: a delay, the producer's copy of the real PCM over a decoy, the signals call, a clone of the units, then
    the decoy over the PCM again and zeros over the units.  One synchronise; the clone holds the oracle's units and pools."""
    import torch
    S = torch.cuda.Stream()
    assert S.cuda_stream != 0
    sctx = c1.Context(0, stream=S.cuda_stream)
    try:
        off = SL.offsets(SL.LENGTHS)
        n, total = len(SL.LENGTHS), int(off[-1])
        want_u, want_s = SL.want_encode('pink', 'detect', True)
        real = torch.from_numpy(np.concatenate(SL.signals('pink'))).to('cuda:0')
        decoy = torch.from_numpy(O.gen_white(99, total * 512)).to('cuda:0')
        pcm = decoy.clone()
        units = torch.zeros(total * 212, dtype=torch.uint8, device='cuda:0')
        pools = torch.from_numpy(SL.enc_pools().copy()).to('cuda:0')
        spin = torch.ones(1 << 24, dtype=torch.float32, device='cuda:0')
        copts = opts('detect').to_c()
        torch.cuda.synchronize()
        with torch.cuda.stream(S):
            sctx.encode_signals_device(off, pcm.data_ptr(), units.data_ptr(), pools.data_ptr(), pools.data_ptr(), c_options=copts)   # warms: workspace, options
            warm = units.clone()
            S.synchronize()
            del warm
            pools.copy_(torch.from_numpy(SL.enc_pools().copy()))
            S.synchronize()
            for _ in range(150):
                spin.mul_(-1.0)
            pcm.copy_(real)
            sctx.encode_signals_device(off, pcm.data_ptr(), units.data_ptr(), pools.data_ptr(), pools.data_ptr(), c_options=copts)
            snap, snap_pools = units.clone(), pools.clone()
            units.zero_()
            pcm.copy_(decoy)
            busy = not S.query()
            S.synchronize()
        assert busy, 'not exercised: the stream was idle when the call returned'
        assert np.array_equal(snap.cpu().numpy().reshape(-1, 212), np.concatenate(want_u))
        assert SL.same_bits(snap_pools.cpu().numpy(), want_s)
        torch.cuda.synchronize()
        assert not units.cpu().numpy().any(), 'units were stored after the consumer had zeroed the buffer'
    finally:
        sctx.close()


# ---- 9: decode ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('pools', [False, True], ids=['fresh', 'pools'])
@pytest.mark.parametrize('oname', ONAMES)
def test_decode_signals_equal_the_oracle(ctx, oname, pools):
    units = SL.want_encode('pink', oname, False)[0]
    start = SL.dec_pools() if pools else None
    want_p, want_d = SL.want_decode('pink', oname, pools)
    p, d = ctx.decode_signals(units, states=start, return_states=True)
    check_decode(p, d, want_p, want_d, (oname, pools))
    if pools:
        work = start.copy()
        p, d = ctx.decode_signals(units, states=work, in_place=True)
        assert np.shares_memory(d, work)
        check_decode(p, work, want_p, want_d, (oname, 'in place'))
    check_decode(ctx.decode_signals(units, states=start), None, want_p, None, (oname, pools, 'no pools out'))


def test_decode_signals_of_random_bytes(ctx):
    rng = np.random.default_rng(0xd3c)
    units = [rng.integers(0, 256, (m, 212), dtype=np.uint8) for m in SL.LENGTHS]
    want_p, want_d = SL.oracle_decode_signals(units, SL.dec_pools())
    p, d = ctx.decode_signals(units, states=SL.dec_pools(), return_states=True)
    check_decode(p, d, want_p, want_d, 'random bytes')


def test_decode_signals_equivalences(ctx):
    units = np.concatenate(SL.want_encode('pink', 'detect', False)[0])
    n = 9
    pools = SS.random_pools(0x654, n, SS.DEC_FLOATS)
    wp, wd = ctx.decode_frames_from_states(units[20:20 + n], pools)
    p, d = ctx.decode_signals([units[20 + i:21 + i] for i in range(n)], states=pools, return_states=True)
    assert SL.same_bits(np.concatenate(p).reshape(n, 512), wp) and SL.same_bits(d, wd)
    assert SL.same_bits(ctx.decode_signals([units[14:80]])[0], ctx.decode(units[14:80], 1)[0])


def test_decode_signals_in_binary32_keep_the_first_frames_exact():
    """c1_ctx_set_decode_precision(1) applies to the bulk: the result stays within test_gpu_decode32.py's tolerance of the
    oracle (RMS < 1e-6, maximum < 1e-5), and the first frame of every signal, which the from-state kernel computes, is the
    oracle's bit for bit"""
    c = c1.Context(0)
    try:
        c.set_decode_precision(True)
        units = SL.want_encode('pink', 'detect', False)[0]
        want_p, want_d = SL.want_decode('pink', 'detect', True)
        p, d = c.decode_signals(units, states=SL.dec_pools(), return_states=True)
        inexact = 0
        for i, (g, w) in enumerate(zip(p, want_p)):
            assert g.shape == w.shape
            if not len(w):
                continue
            assert SL.same_bits(g[:512], w[:512]), i
            err = g.astype(np.float64) - w
            print('binary32 decode, signal %d: rms %.3g max %.3g' % (i, np.sqrt(np.mean(err ** 2)), np.abs(err).max()))
            assert np.sqrt(np.mean(err ** 2)) < 1e-6 and np.abs(err).max() < 1e-5, i
            inexact += int(np.abs(err).max() > 0)
        assert inexact > 0                                        # the bulk really ran in another arithmetic
        assert SL.same_bits(d, want_d)                            # the pools come from the from-state kernel
    finally:
        c.close()


# ---- 10: the host forms reject bad input and write nothing --------------------------------------------------------------
def test_host_forms_reject_bad_arguments(ctx):
    lib = capi.load()
    lengths = [2, 1, 0, 3, 1]
    n, total = 5, 7
    off = SL.offsets(lengths)
    x = O.gen_white(5, total * 512)
    pools, dpools = SS.random_pools(11, n, SS.ENC_FLOATS), SS.random_pools(12, n, SS.DEC_FLOATS)
    o = opts('detect').to_c()
    units = np.full((total, 212), 0x5A, dtype=np.uint8)
    out = np.full((n, SS.ENC_FLOATS), 3.5, dtype=np.float32)
    pcm_out = np.full(total * 512, 3.5, dtype=np.float32)
    dout = np.full((n, SS.DEC_FLOATS), 3.5, dtype=np.float32)

    def enc(n_=n, off_=off, pcm=x.ctypes.data, st=pools, o_=C.byref(o), u=units.ctypes.data, out_=out):
        return lib.c1_encode_signals(ctx._h, n_, off_.ctypes.data_as(I64P) if off_ is not None else None, pcm,
                                     st.ctypes.data if st is not None else None, o_, u, out_.ctypes.data if out_ is not None else None)

    def dec(n_=n, off_=off, u=units.ctypes.data, st=dpools, pcm=pcm_out.ctypes.data, out_=dout):
        return lib.c1_decode_signals(ctx._h, n_, off_.ctypes.data_as(I64P) if off_ is not None else None, u,
                                     st.ctypes.data if st is not None else None, pcm, out_.ctypes.data if out_ is not None else None)

    def untouched():
        return (units == 0x5A).all() and (out == 3.5).all() and (pcm_out == 3.5).all() and (dout == 3.5).all()

    not_zero, decreasing = off + 1, np.array([0, 2, 3, 2, 6, 7], dtype=np.int64)
    too_many = np.array([0, (1 << 22) + 1], dtype=np.int64)
    for call in (enc, dec):
        assert call(off_=not_zero) == C1_ERR_ARG and 'start at 0' in lib.c1_last_error().decode()
        assert call(off_=decreasing) == C1_ERR_ARG and 'decreases at signal 2' in lib.c1_last_error().decode()
        assert call(n_=-1) == C1_ERR_ARG
        assert call(n_=(1 << 20) + 1) == C1_ERR_ARG
        assert call(n_=1, off_=too_many) == C1_ERR_ARG
        assert call(off_=None) == C1_ERR_ARG
        assert call(pcm=None) == C1_ERR_ARG
        assert call(u=None) == C1_ERR_ARG
        assert untouched()
    assert enc(o_=None) == C1_ERR_ARG and untouched()
    keep = pools.copy()
    for value, field, k in ((np.nan, 'qmf_mid[7]', 46 + 7), (np.inf, 'transient_mags[255]', 227 + 255)):
        bad = pools.copy()
        bad[3, k] = value
        with pytest.raises(capi.Carta1Error) as err:
            ctx.encode_signals([x[off[i] * 512:off[i + 1] * 512] for i in range(n)], opts('detect'), states=bad, in_place=True)
        assert err.value.code == C1_ERR_ARG and 'signal 3' in str(err.value) and field in str(err.value)
        bad[3, k] = keep[3, k]
        assert SL.same_bits(bad, keep)                                             # `in` (== out) as it was
    for value, field, k in ((np.nan, 'qmf_high[38]', 92 + 38), (-np.inf, 'imdct_tail[0]', 131)):
        bad = dpools.copy()
        bad[3, k] = value
        with pytest.raises(capi.Carta1Error) as err:
            ctx.decode_signals([np.zeros((m, 212), dtype=np.uint8) for m in lengths], states=bad, in_place=True)
        assert err.value.code == C1_ERR_ARG and 'signal 3' in str(err.value) and field in str(err.value)
    assert untouched()
    # n == 0, and signals that are all empty, succeed
    empty = np.zeros(1, dtype=np.int64)
    assert enc(n_=0, off_=empty) == 0 and dec(n_=0, off_=empty) == 0 and untouched()
    assert ctx.encode_signals([]) == [] and ctx.decode_signals([]) == []
    z = np.zeros(0, dtype=np.float32)
    u, s = ctx.encode_signals([z, z, z], opts('detect'), states=pools[:3], return_states=True)
    assert [a.shape for a in u] == [(0, 212)] * 3 and SL.same_bits(s, pools[:3])
    p, d = ctx.decode_signals([np.zeros((0, 212), dtype=np.uint8)] * 3, states=dpools[:3], return_states=True)
    assert [a.shape for a in p] == [(0,)] * 3 and SL.same_bits(d, dpools[:3])
    u, s = ctx.encode_signals([z, z], return_states=True)
    assert not s.any()


# ---- 11: profiling ----------------------------------------------------------------------------------------------------------------
def test_signal_starts_time_is_reported(ctx):
    ctx.set_profiling(True)
    try:
        ctx.encode_signals(SL.signals('pink'), opts('detect'), states=SL.enc_pools(), return_states=True)
        ms, launches = ctx.kernel_ms('signal_starts')
        total, all_launches = ctx.kernel_ms('total')
        assert ms > 0 and launches > 0 and total > ms and all_launches > launches
        assert ctx.kernel_ms('analysis')[1] > 0                                   # the bulk pass of the same call
        ctx.decode_signals(SL.want_encode('pink', 'detect', False)[0], states=SL.dec_pools(), return_states=True)
        ms, launches = ctx.kernel_ms('signal_starts')
        assert ms > 0 and launches > 0 and ctx.kernel_ms('decode')[1] == 1
    finally:
        ctx.set_profiling(False)


# ---- 12: the AEA functions over many items ------------------------------------------------------------------------------
def test_aea_many_equal_the_per_item_functions(ctx):
    items = SL.aea_items()
    for options in (None, {'fixedBlockModes': [0, 2, 0], 'allocationBias': 0.5, 'title': ['a', 'b', 'c', 'd', 'e']}):
        many = c1.encode_aea_pcm_many(items, options, ctx=ctx)
        for i, item in enumerate(items):
            o = dict(options or {})
            if 'title' in o:
                o['title'] = o['title'][i]
            assert many[i] == c1.encode_aea_pcm(item, o, ctx=ctx), i
    images = c1.encode_aea_pcm_many(items, ctx=ctx)
    odd = images[4][:2048 + 5 * 212]                                              # a stereo image that ends on a lone left unit
    cut = images[2][:-100]                                                        # and one with a trailing partial unit
    images = images + [odd, cut]
    pcm = c1.decode_aea_pcm_many(images, ctx=ctx)
    for i, image in enumerate(images):
        want = c1.decode_aea_pcm(image, ctx=ctx)
        assert len(pcm[i]) == len(want), i
        for g, w in zip(pcm[i], want):
            assert SL.same_bits(g, w), i
