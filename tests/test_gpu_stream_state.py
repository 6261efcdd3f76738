"""Stream state in the reference's BufferPool layout, on the device: c1_*_stream_get_state / set_state and the batched frame
closures over explicit pools (c1_k_state.hip) against the reference's dumped pools (tests/golden/stream_state.json) and the
CPU oracle, which tests/test_stream_state_cpu.py pins to them.  Everything compares uint32 views (or bytes) for equality."""
import ctypes as C

import numpy as np
import pytest

import carta1_amd as c1
from carta1_amd import capi
import stream_state_lib as SS

pytestmark = pytest.mark.gpu

C1_ERR_ARG = 1   # include/carta1_hip.h
FIX = SS.fixture()
CASES = sorted(FIX['cases'])
DUMP, MORE = FIX['dump_at'], FIX['more']
LONG = 12                      # frames of the round-trip streams
DETECT, FIXED203 = {}, {'fixedBlockModes': [2, 0, 3]}


@pytest.fixture(scope='module')
def ctx():
    c = c1.Context(0)
    yield c
    c.close()


@pytest.fixture(scope='module')
def ctx2():
    c = c1.Context(0)
    yield c
    c.close()


def opts(oset):
    return c1.EncoderOptions(dict(oset))


def same(a, b):
    return np.array_equal(SS.bits(a), SS.bits(b))


_model = {}


def model(name):
    """per case, computed once: the signal (LONG frames), the oracle's units of all of it, and its states after 0 .. LONG frames"""
    if name not in _model:
        sig, oname = name.split('/')
        chans = SS.signal(FIX['signals'][sig], LONG)
        oset = FIX['option_sets'][oname]
        st = np.zeros((len(chans), SS.ENC_FLOATS), dtype=np.float32)
        dst = np.zeros((len(chans), SS.DEC_FLOATS), dtype=np.float32)
        states, dstates, units, pcm = [st], [dst], [], []
        for f in range(LONG):
            u, st = SS.oracle_encode([c[f * 512:(f + 1) * 512] for c in chans], oset, st)
            p, dst = SS.oracle_decode(u, len(chans), dst)
            states.append(st); dstates.append(dst); units.append(u); pcm.append(p)
        _model[name] = dict(chans=chans, oset=oset, states=states, dstates=dstates, units=np.concatenate(units),
                            pcm=[np.concatenate([p[c] for p in pcm]) for c in range(len(chans))])
    return _model[name]


def frames_of(chans, a, b):
    return [c[a * 512:b * 512] for c in chans]


# ---- export ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', CASES)
def test_encoder_export(ctx, name):
    m = model(name)
    nch = len(m['chans'])
    for pushes in ((1, 1, 3), (5,), (2, 3), (3, 2)):
        s = c1.EncoderStream(ctx, nch, opts(m['oset']))
        try:
            assert not s.get_state().any()                                   # a fresh stream exports zeros
            at = 0
            for n in pushes:
                u = s.push(frames_of(m['chans'], at, at + n))
                assert np.array_equal(u, m['units'][at * nch:(at + n) * nch])
                at += n
                assert same(s.get_state(), m['states'][at]), (pushes, at)
            assert same(s.get_state(), SS.states(FIX['cases'][name]['enc_states'], SS.ENC_FLOATS))   # the reference's pool
        finally:
            s.close()


@pytest.mark.parametrize('name', CASES)
def test_decoder_export(ctx, name):
    m = model(name)
    nch = len(m['chans'])
    for pushes in ((1, 1, 3), (5,), (2, 3), (3, 2)):
        s = c1.DecoderStream(ctx, nch)
        try:
            assert not s.get_state().any()
            at = 0
            for n in pushes:
                s.push(m['units'][at * nch:(at + n) * nch])
                at += n
                assert same(s.get_state(), m['dstates'][at]), (pushes, at)
            assert same(s.get_state(), SS.states(FIX['cases'][name]['dec_states'], SS.DEC_FLOATS))
        finally:
            s.close()


# ---- import from the reference's pools -----------------------------------------------------------------------------------
@pytest.mark.parametrize('name', CASES)
def test_encoder_import_reference_pool(ctx, name):
    m = model(name)
    e = FIX['cases'][name]
    nch = len(m['chans'])
    want = SS.units(e['units_more'])
    for pushes in ((1, 1, 1, 1), (4,)):
        s = c1.EncoderStream(ctx, nch, opts(m['oset']))
        try:
            s.set_state(SS.states(e['enc_states'], SS.ENC_FLOATS))
            at, got = DUMP, []
            for n in pushes:
                got.append(s.push(frames_of(m['chans'], at, at + n)))
                at += n
            assert np.array_equal(np.concatenate(got), want), pushes
            assert same(s.get_state(), m['states'][DUMP + MORE])
        finally:
            s.close()


@pytest.mark.parametrize('name', CASES)
def test_decoder_import_reference_pool(ctx, name):
    m = model(name)
    e = FIX['cases'][name]
    nch = len(m['chans'])
    un = SS.units(e['units_more'])
    for pushes in ((1, 1, 1, 1), (4,)):
        s = c1.DecoderStream(ctx, nch)
        try:
            s.set_state(SS.states(e['dec_states'], SS.DEC_FLOATS))
            at, got = 0, []
            for n in pushes:
                got.append(s.push(un[at * nch:(at + n) * nch]))
                at += n
            pcm = [np.concatenate([g[c] for g in got]) for c in range(nch)]
            assert SS.pcm_sha(pcm, 0, MORE) == e['pcm_sha256'], pushes         # the reference's PCM bits
            for c in range(nch):
                assert same(pcm[c], m['pcm'][c][DUMP * 512:(DUMP + MORE) * 512])
            assert same(s.get_state(), m['dstates'][DUMP + MORE])
        finally:
            s.close()


@pytest.mark.parametrize('oname', sorted(FIX['foreign']['enc']))
def test_encoder_import_foreign_pool(ctx, oname):
    f = FIX['foreign']
    e = f['enc'][oname]
    x = SS.signal(f['pcm'], f['frames'])
    for pushes in ((1, 1, 1), (3,)):
        s = c1.EncoderStream(ctx, 1, opts(e['options']))
        try:
            s.set_state(SS.foreign_enc_state(f['enc_seed']))
            at, got = 0, []
            for n in pushes:
                got.append(s.push(frames_of(x, at, at + n)))
                at += n
            assert np.array_equal(np.concatenate(got), SS.units(e['units'])), pushes
            assert same(s.get_state(), SS.states(e['enc_state_end'], SS.ENC_FLOATS)), pushes
        finally:
            s.close()


def test_decoder_import_foreign_pool(ctx):
    f = FIX['foreign']
    d = f['dec']
    un = SS.units(d['units'])
    for pushes in ((1, 1, 1), (3,)):
        s = c1.DecoderStream(ctx, 1)
        try:
            s.set_state(SS.foreign_dec_state(f['dec_seed']))
            at, got = 0, []
            for n in pushes:
                got.append(s.push(un[at:at + n])[0])
                at += n
            assert same(np.concatenate(got), SS.blob(d['pcm'], np.float32)), pushes
            assert same(s.get_state(), SS.states(d['dec_state_end'], SS.DEC_FLOATS)), pushes
        finally:
            s.close()


# ---- round trip ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', CASES)
def test_encoder_round_trip_across_contexts(ctx, ctx2, name):
    m = model(name)
    nch = len(m['chans'])
    for k in range(5):
        a = c1.EncoderStream(ctx, nch, opts(m['oset']))
        b = c1.EncoderStream(ctx2, nch, opts(m['oset']))
        try:
            if k:
                a.push(frames_of(m['chans'], 0, k))
            snap = a.get_state()
            b.set_state(snap)
            assert same(b.get_state(), snap)
            got = [b.push(frames_of(m['chans'], k, k + 1)), b.push(frames_of(m['chans'], k + 1, LONG))]
            assert np.array_equal(np.concatenate(got), m['units'][k * nch:]), k
            assert same(b.get_state(), m['states'][LONG]), k
        finally:
            a.close()
            b.close()


@pytest.mark.parametrize('name', CASES)
def test_decoder_round_trip_across_contexts(ctx, ctx2, name):
    m = model(name)
    nch = len(m['chans'])
    for k in range(5):
        a = c1.DecoderStream(ctx, nch)
        b = c1.DecoderStream(ctx2, nch)
        try:
            if k:
                a.push(m['units'][:k * nch])
            snap = a.get_state()
            b.set_state(snap)
            assert same(b.get_state(), snap)
            got = [b.push(m['units'][k * nch:(k + 1) * nch]), b.push(m['units'][(k + 1) * nch:])]
            for c in range(nch):
                assert same(np.concatenate([g[c] for g in got]), m['pcm'][c][k * 512:]), k
        finally:
            a.close()
            b.close()


@pytest.mark.parametrize('mode', [0, 1, 2])
@pytest.mark.parametrize('name', ['white12/fixed000', 'white12/detect_t1', 'pinkT34/fixed223'])
def test_speculative_path_behind_a_restored_state(ctx, name, mode):
    """40 stereo frames in one push after the restore: the two from-state frames, then 38 on the usual path under every speculation mode"""
    sig, oname = name.split('/')
    oset = FIX['option_sets'][oname]
    chans = SS.signal(FIX['signals'][sig], DUMP + 40)
    want, _ = SS.oracle_encode(frames_of(chans, DUMP, DUMP + 40), oset, SS.states(FIX['cases'][name]['enc_states'], SS.ENC_FLOATS))
    c = c1.Context(0)
    c.set_speculation(mode)
    s = c1.EncoderStream(c, 2, opts(oset))
    try:
        s.set_state(SS.states(FIX['cases'][name]['enc_states'], SS.ENC_FLOATS))
        assert np.array_equal(s.push(frames_of(chans, DUMP, DUMP + 40)), want)
    finally:
        s.close()
        c.close()


def test_set_then_get_returns_the_same_bits(ctx):
    enc = SS.random_pools(0xabc1, 2, SS.ENC_FLOATS)
    dec = SS.random_pools(0xabc2, 2, SS.DEC_FLOATS)
    s = c1.EncoderStream(ctx, 2)
    d = c1.DecoderStream(ctx, 2)
    try:
        s.set_state(enc)
        assert same(s.get_state(), enc)
        d.set_state(dec)
        assert same(d.get_state(), dec)
    finally:
        s.close()
        d.close()


def test_mid_stream_set_state_discards_the_history(ctx):
    name = 'pinkT34/detect_t03'
    m = model(name)
    e = FIX['cases'][name]
    other = SS.signal(FIX['signals']['white12'], 3)
    s = c1.EncoderStream(ctx, 2, opts(m['oset']))
    d = c1.DecoderStream(ctx, 2)
    try:
        d.push(s.push(other))
        s.set_state(SS.states(e['enc_states'], SS.ENC_FLOATS))
        d.set_state(SS.states(e['dec_states'], SS.DEC_FLOATS))
        u = s.push(frames_of(m['chans'], DUMP, DUMP + MORE))
        assert np.array_equal(u, SS.units(e['units_more']))
        pcm = d.push(u)
        assert SS.pcm_sha(pcm, 0, MORE) == e['pcm_sha256']
    finally:
        s.close()
        d.close()


def test_non_finite_state_is_rejected_and_changes_nothing(ctx):
    name = 'white12/detect_t1'
    m = model(name)
    s = c1.EncoderStream(ctx, 2, opts(m['oset']))
    d = c1.DecoderStream(ctx, 2)
    try:
        s.push(frames_of(m['chans'], 0, 2))
        d.push(m['units'][:4])
        bad = SS.random_pools(7, 2, SS.ENC_FLOATS)
        bad[1, 227 + 5] = np.nan
        with pytest.raises(capi.Carta1Error) as err:
            s.set_state(bad)
        assert err.value.code == C1_ERR_ARG and 'channel 1' in str(err.value) and 'transient_mags[5]' in str(err.value)
        badd = SS.random_pools(8, 2, SS.DEC_FLOATS)
        badd[0, 131 + 17] = np.inf
        with pytest.raises(capi.Carta1Error) as err:
            d.set_state(badd)
        assert err.value.code == C1_ERR_ARG and 'channel 0' in str(err.value) and 'imdct_tail[17]' in str(err.value)
        assert np.array_equal(s.push(frames_of(m['chans'], 2, 4)), m['units'][4:8])
        pcm = d.push(m['units'][4:8])
        for c in range(2):
            assert same(pcm[c], m['pcm'][c][2 * 512:4 * 512])
    finally:
        s.close()
        d.close()


# ---- the switch schedule ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('sig', sorted(FIX['switch']['results']))
def test_switch_schedule(ctx, ctx2, sig):
    sc = FIX['switch']['schedule']
    r = FIX['switch']['results'][sig]
    chans = SS.signal(FIX['signals'][sig], sc['frames'])
    fixed = {'fixedBlockModes': sc['fixed_modes']}
    dumped = SS.states(r['enc_states'], SS.ENC_FLOATS)
    want = SS.units(r['units_from_dump'])
    a = c1.EncoderStream(ctx, 2, opts(DETECT))
    b = c1.EncoderStream(ctx2, 2, opts(fixed))
    try:
        # a stream that followed the schedule exports the kept spectrum under fixed modes ...
        a.push(frames_of(chans, 0, sc['fixed_from']))
        a.set_options(opts(fixed))
        a.push(frames_of(chans, sc['fixed_from'], sc['dump_at']))
        assert same(a.get_state(), dumped)
        # ... and restored elsewhere, that spectrum is the one compared when detection comes back
        b.set_state(dumped)
        got = [b.push(frames_of(chans, sc['dump_at'], sc['detect_from']))]
        b.set_options(opts(DETECT))
        got.append(b.push(frames_of(chans, sc['detect_from'], sc['frames'])))
        assert np.array_equal(np.concatenate(got), want)
        # the exporting stream goes on as well
        got = [a.push(frames_of(chans, sc['dump_at'], sc['detect_from']))]
        a.set_options(opts(DETECT))
        got.append(a.push(frames_of(chans, sc['detect_from'], sc['frames'])))
        assert np.array_equal(np.concatenate(got), want)
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize('sig', sorted(FIX['switch']['results']))
def test_restored_spectrum_survives_fixed_mode_frames(ctx, sig):
    """restore under fixed modes, push past the two from-state frames so the stream is back on its usual path, snapshot, and
    only then return to detection: the restored magnitudes are exported and compared (the oracle is the model)"""
    sc = FIX['switch']['schedule']
    chans = SS.signal(FIX['signals'][sig], sc['frames'])
    fixed = {'fixedBlockModes': sc['fixed_modes']}
    dumped = SS.states(FIX['switch']['results'][sig]['enc_states'], SS.ENC_FLOATS)
    d0 = sc['dump_at']
    u_fixed, st = SS.oracle_encode(frames_of(chans, d0, d0 + 4), fixed, dumped)
    u_detect, st_end = SS.oracle_encode(frames_of(chans, d0 + 4, sc['frames']), DETECT, st)
    s = c1.EncoderStream(ctx, 2, opts(fixed))
    try:
        s.set_state(dumped)
        assert np.array_equal(s.push(frames_of(chans, d0, d0 + 3)), u_fixed[:6])
        assert np.array_equal(s.push(frames_of(chans, d0 + 3, d0 + 4)), u_fixed[6:])
        assert same(s.get_state(), st)
        assert same(s.get_state()[:, 227:], dumped[:, 227:])
        s.set_options(opts(DETECT))
        assert np.array_equal(s.push(frames_of(chans, d0 + 4, sc['frames'])), u_detect)
        assert same(s.get_state(), st_end)
    finally:
        s.close()


# ---- decoder: restore, then fields, then units -----------------------------------------------------------------------------
def test_decoder_restore_then_fields_then_units(ctx):
    name = 'pinkT34/detect_t1'
    m = model(name)
    e = FIX['cases'][name]
    un = SS.units(e['units_more'])
    want = [m['pcm'][c][DUMP * 512:(DUMP + MORE) * 512] for c in range(2)]
    for n_fields in (1, 2):
        s = c1.DecoderStream(ctx, 2)
        try:
            s.set_state(SS.states(e['dec_states'], SS.DEC_FLOATS))
            got = [s.push_fields(ctx.unpack_units(un[:2 * n_fields])), s.push(un[2 * n_fields:])]
            for c in range(2):
                assert same(np.concatenate([g[c] for g in got]), want[c]), n_fields
            assert same(s.get_state(), m['dstates'][DUMP + MORE])
        finally:
            s.close()


# ---- the batched entries ---------------------------------------------------------------------------------------------------
def batch_inputs(n):
    pcm = (SS.xorshift_values(0x51 + n, n * 512) * np.float32(0.5)).reshape(n, 512)
    return pcm, SS.random_pools(0x77 + n, n, SS.ENC_FLOATS), SS.random_pools(0x99 + n, n, SS.DEC_FLOATS)


@pytest.mark.parametrize('oset', [DETECT, FIXED203], ids=['detect', 'fixed203'])
@pytest.mark.parametrize('n', [0, 1, 2, 65, 200])
def test_batched_closures(ctx, n, oset):
    pcm, pools, dpools = batch_inputs(n)
    want_u, want_s = SS.oracle_encode_pools(pcm, pools, oset)
    u, st = ctx.encode_frames_from_states(pcm, pools, opts(oset))
    assert u.shape == (n, 212) and st.shape == (n, SS.ENC_FLOATS)
    assert np.array_equal(u, want_u)
    assert same(st, want_s)
    if oset is FIXED203:
        assert same(st[:, 227:], pools[:, 227:])                   # transient_mags passes through under fixed modes
    work = pools.copy()                                             # out == in
    u2, st2 = ctx.encode_frames_from_states(pcm, work, opts(oset), in_place=True)
    assert np.array_equal(u2, want_u) and same(work, want_s) and same(st2, want_s)   # `work` itself was overwritten
    # the units just made, decoded from random decoder pools
    want_p, want_d = SS.oracle_decode_pools(want_u, dpools)
    p, d = ctx.decode_frames_from_states(want_u, dpools)
    assert same(p, want_p) and same(d, want_d)
    work = dpools.copy()
    p2, d2 = ctx.decode_frames_from_states(want_u, work, in_place=True)
    assert same(p2, want_p) and same(work, want_d) and same(d2, want_d)


def test_batched_closures_past_the_grid_step(ctx):
    """the kernels stride a bounded grid of 256 * 12 one-wave workgroups over the pools (c1_k_state.hip): a few pools more than
    that, so that some workgroups take a second pool; in place"""
    n = 256 * 12 + 5
    rng = np.random.default_rng(0x57a7e)                   # (this many xorshift32 values in Python would take seconds)
    pcm = rng.uniform(-0.5, 0.5, (n, 512)).astype(np.float32)
    pools = rng.uniform(-1, 1, (n, SS.ENC_FLOATS)).astype(np.float32)
    dpools = rng.uniform(-1, 1, (n, SS.DEC_FLOATS)).astype(np.float32)
    want_u, want_s = SS.oracle_encode_pools(pcm, pools, DETECT)
    u, st = ctx.encode_frames_from_states(pcm, pools.copy(), opts(DETECT), in_place=True)
    assert np.array_equal(u, want_u) and same(st, want_s)
    want_p, want_d = SS.oracle_decode_pools(want_u, dpools)
    p, d = ctx.decode_frames_from_states(want_u, dpools.copy(), in_place=True)
    assert same(p, want_p) and same(d, want_d)


def test_batched_closures_on_device_pointers_in_place(ctx):
    import torch
    n = 65
    pcm, pools, dpools = batch_inputs(n)
    want_u, want_s = SS.oracle_encode_pools(pcm, pools, DETECT)
    want_p, want_d = SS.oracle_decode_pools(want_u, dpools)
    lib = capi.load()
    o = opts(DETECT).to_c()
    t_pcm = torch.from_numpy(pcm).to('cuda:0')
    t_st = torch.from_numpy(pools.copy()).to('cuda:0')
    t_u = torch.zeros(n * 212, dtype=torch.uint8, device='cuda:0')
    torch.cuda.synchronize()
    capi.check(lib.c1_encode_frames_from_states_device(ctx._h, n, t_pcm.data_ptr(), t_st.data_ptr(), C.byref(o), t_u.data_ptr(), t_st.data_ptr()))
    t_dst = torch.from_numpy(dpools.copy()).to('cuda:0')
    t_out = torch.zeros(n * 512, dtype=torch.float32, device='cuda:0')
    torch.cuda.synchronize()
    capi.check(lib.c1_decode_frames_from_states_device(ctx._h, n, t_u.data_ptr(), t_dst.data_ptr(), t_out.data_ptr(), t_dst.data_ptr()))
    ctx.synchronize()
    assert np.array_equal(t_u.cpu().numpy().reshape(n, 212), want_u)
    assert same(t_st.cpu().numpy(), want_s)
    assert same(t_out.cpu().numpy().reshape(n, 512), want_p)
    assert same(t_dst.cpu().numpy(), want_d)
    # out == NULL: units and PCM only
    capi.check(lib.c1_encode_frames_from_states_device(ctx._h, 0, t_pcm.data_ptr(), t_st.data_ptr(), C.byref(o), t_u.data_ptr(), None))
    assert lib.c1_encode_frames_from_states_device(ctx._h, -1, t_pcm.data_ptr(), t_st.data_ptr(), C.byref(o), t_u.data_ptr(), None) == C1_ERR_ARG
    assert lib.c1_decode_frames_from_states_device(ctx._h, 1, None, t_dst.data_ptr(), t_out.data_ptr(), None) == C1_ERR_ARG


def test_batched_host_entries_reject_bad_arguments(ctx):
    pcm, pools, dpools = batch_inputs(4)
    bad = pools.copy()
    bad[3, 46 + 7] = np.nan
    with pytest.raises(capi.Carta1Error) as err:
        ctx.encode_frames_from_states(pcm, bad)
    assert err.value.code == C1_ERR_ARG and 'pool 3' in str(err.value) and 'qmf_mid[7]' in str(err.value)
    badd = dpools.copy()
    badd[2, 92 + 38] = -np.inf
    with pytest.raises(capi.Carta1Error) as err:
        ctx.decode_frames_from_states(np.zeros((4, 212), dtype=np.uint8), badd)
    assert err.value.code == C1_ERR_ARG and 'pool 2' in str(err.value) and 'qmf_high[38]' in str(err.value)
    lib = capi.load()
    o = opts(DETECT).to_c()
    assert lib.c1_encode_frames_from_states(ctx._h, (1 << 20) + 1, pcm.ctypes.data, pools.ctypes.data, C.byref(o), pcm.ctypes.data, None) == C1_ERR_ARG
    assert lib.c1_encode_frames_from_states(ctx._h, 4, pcm.ctypes.data, None, C.byref(o), pcm.ctypes.data, None) == C1_ERR_ARG
    assert lib.c1_decode_frames_from_states(ctx._h, -1, pcm.ctypes.data, dpools.ctypes.data, pcm.ctypes.data, None) == C1_ERR_ARG


def test_from_state_kernel_time_is_reported(ctx):
    pcm, pools, _ = batch_inputs(65)
    ctx.set_profiling(True)
    try:
        ctx.encode_frames_from_states(pcm, pools)
        ms, launches = ctx.kernel_ms('from_state')
        assert launches == 1 and ms > 0
    finally:
        ctx.set_profiling(False)
