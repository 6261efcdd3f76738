"""GPU: encode with the block modes supplied per frame by the caller (c1_encode_modes_device / _batch,
c1_enc_stream_push_modes).  A detection run's own modes fed back reproduce its bytes; constant modes reproduce fixed modes;
random per-frame, per-channel modes give the CPU oracle's bytes whatever the chunking, the pipeline and the speculation mode;
one stream follows every schedule of tests/golden/option_changes.json with modes pushes where fixedBlockModes is set, and its
state is the reference's pool; the host entry points reject bytes outside the domain and change nothing; the device entry
point stays inside its buffers for any byte; and the call is ordered on a caller's stream."""
import ctypes as C
import os

import numpy as np
import pytest

import carta1_amd as c1
from carta1_amd import capi
import block_modes_lib as BM
import oracle_lib as O
import option_changes_lib as OC
import stream_state_lib as SL

pytestmark = pytest.mark.gpu

C1_OK, C1_ERR_ARG = 0, 1   # include/carta1_hip.h
FIX = OC.fixture()
CASES = [(name, sig) for name, s in FIX['schedules'].items() for sig in s['results']]
COUNTS = (1, 2, 3, 63, 64, 65, 130, 257, 1025)    # one run, the run seams, a 256-unit list block seam (mono and stereo)
MAX_FRAMES = max(COUNTS) + 2
R_FRAMES, R_BIASES = 130, (0.5, 1, 2)              # the random-modes case


def opts(v):
    return c1.EncoderOptions(v)


@pytest.fixture(scope='module')
def ctx():
    c = c1.Context(0)
    yield c
    c.close()


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
def material():
    return {'pinkT': [O.gen_pinkT(3, MAX_FRAMES * 512), O.gen_pinkT(4, MAX_FRAMES * 512)], 'white': [O.gen_white(1, MAX_FRAMES * 512)]}


@pytest.fixture(scope='module')
def random_case():
    """stereo, 130 frames, the two channels on different schedules; the oracle's units per bias, and for the alternating
    schedule: computed once, shared, never written"""
    chans = [O.gen_pinkT(3, R_FRAMES * 512), O.gen_white(2, R_FRAMES * 512)]
    modes = BM.random_modes(20261018, R_FRAMES, 2)
    assert (modes[:, 0] != modes[:, 1]).any() and set(modes.reshape(-1).tolist()) == set(BM.DOMAIN_BYTES)
    alt = BM.alternating_modes(R_FRAMES, 2)
    want = {b: BM.oracle_encode_modes(chans, modes, b)[0] for b in R_BIASES}
    return {'chans': chans, 'modes': modes, 'alt': alt, 'want': want, 'want_alt': BM.oracle_encode_modes(chans, alt, 1)[0]}


def dev_encode_modes(ctx, dev, frames, modes, options, halo=0):
    """c1_encode_modes_device on torch buffers: dev = per-channel tensors that start `halo` frames before frame 0"""
    import torch
    nch = len(dev)
    d_modes = modes if isinstance(modes, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(modes, dtype=np.uint8).reshape(-1)).cuda()
    units = torch.zeros(frames * nch * 212, dtype=torch.uint8, device='cuda')
    torch.cuda.synchronize()
    ctx.encode_modes_device([d.data_ptr() + halo * 2048 for d in dev], frames, d_modes.data_ptr(), units.data_ptr(), options, halo_frames=halo)
    ctx.synchronize()
    return units.cpu().numpy().reshape(-1, 212)


# ---- 1. a detection run's own modes reproduce it ----
@pytest.mark.parametrize('halo', [0, 1, 2])
@pytest.mark.parametrize('sig', ['pinkT', 'white'])
def test_own_modes_reproduce_detection(ctx, material, sig, halo):
    import torch
    chans = material[sig]
    nch = len(chans)
    dev = [torch.from_numpy(c).cuda() for c in chans]
    mags = torch.zeros(max(COUNTS) * nch * 256, dtype=torch.float32, device='cuda')
    for frames in COUNTS:
        ptrs = [d.data_ptr() + halo * 2048 for d in dev]
        modes = torch.full((frames * nch,), 0xEE, dtype=torch.uint8, device='cuda')
        want = torch.zeros(frames * nch * 212, dtype=torch.uint8, device='cuda')
        torch.cuda.synchronize()
        ctx.detect_stages_device(ptrs, frames, mags.data_ptr(), modes.data_ptr(), opts({}), halo_frames=halo)
        ctx.encode_device(ptrs, frames, want.data_ptr(), opts({}), halo_frames=halo)
        ctx.synchronize()
        m = modes.cpu().numpy()
        assert set(m.tolist()) <= set(BM.DOMAIN_BYTES)
        if sig == 'pinkT' and frames >= 130:
            assert 0 < np.count_nonzero(m) < m.size                       # both lists of the MDCT stage were used
        got = dev_encode_modes(ctx, dev, frames, modes, opts({}), halo)
        want = want.cpu().numpy().reshape(-1, 212)
        assert np.array_equal(BM.modes_of_units(got), m), (frames, 'modes')
        assert np.array_equal(got, want), (frames, np.flatnonzero((got != want).any(axis=1))[:4])


# ---- 2. constant modes reproduce fixed modes ----
def check_constant_modes(ctx, chans, frames=65):
    import torch
    dev = [torch.from_numpy(c[:frames * 512]).cuda() for c in chans]
    for triple in BM.DOMAIN_TRIPLES:
        want = ctx.encode([c[:frames * 512] for c in chans], opts({'fixedBlockModes': list(triple)}))
        got = dev_encode_modes(ctx, dev, frames, np.full(frames * len(chans), BM.byte_of(triple), dtype=np.uint8), opts({}))
        assert np.array_equal(got, want), triple


def test_constant_modes_reproduce_fixed_modes(ctx, material):
    check_constant_modes(ctx, material['pinkT'])


# ---- 3. random per-frame, per-channel modes against the oracle ----
@pytest.mark.parametrize('bias', R_BIASES)
def test_random_modes_match_oracle(ctx, random_case, bias):
    r = random_case
    got = ctx.encode_modes(r['chans'], r['modes'], opts({'allocationBias': bias}))
    assert np.array_equal(got, r['want'][bias]), np.flatnonzero((got != r['want'][bias]).any(axis=1))[:4]
    # transient_threshold and fixed_block_modes of the options are not read
    other = ctx.encode_modes(r['chans'], r['modes'].reshape(-1), opts({'allocationBias': bias, 'transientThresholdLow': 0.3, 'fixedBlockModes': [2, 0, 3]}))
    assert np.array_equal(other, got)


def test_alternating_modes_match_oracle(ctx, random_case):
    r = random_case
    assert np.array_equal(ctx.encode_modes(r['chans'], r['alt']), r['want_alt'])


# ---- 4. chunk seams, pipeline, speculation ----
@pytest.mark.parametrize('env', [{'C1_CHUNK_FRAMES': 16}, {'C1_CHUNK_FRAMES': 33}, {'C1_CHUNK_FRAMES': 16, 'C1_PIPELINE': 1, 'C1_OVERLAP': 1}],
                         ids=['chunk16', 'chunk33', 'chunk16-piped'])
def test_bytes_do_not_depend_on_chunks_or_speculation(random_case, env):
    r = random_case
    c = _context(**env)
    try:
        for mode in (0, 1, 2):
            c.set_speculation(mode)
            for bias in R_BIASES:
                got = c.encode_modes(r['chans'], r['modes'], opts({'allocationBias': bias}))
                assert np.array_equal(got, r['want'][bias]), (env, mode, bias)
            assert np.array_equal(c.encode_modes(r['chans'], r['alt']), r['want_alt']), (env, mode)
        c.set_profiling(True)
        c.encode_modes(r['chans'], r['modes'])
        ms, launches = c.kernel_ms('analysis')
        assert launches == -(-R_FRAMES // env['C1_CHUNK_FRAMES']) > 1 and ms > 0
    finally:
        c.close()


def test_bytes_do_not_depend_on_speculation(ctx, random_case):
    r = random_case
    try:
        for mode in (0, 1, 2):
            ctx.set_speculation(mode)
            assert np.array_equal(ctx.encode_modes(r['chans'], r['modes']), r['want'][1]), mode
    finally:
        ctx.set_speculation(1)


# ---- 5. one stream through the reference's option schedules ----
@pytest.mark.parametrize('name,sig', CASES, ids=['%s-%s' % c for c in CASES])
def test_stream_follows_reference_schedule(ctx, name, sig):
    s = FIX['schedules'][name]
    frames = FIX['frames']
    chans = OC.signal(FIX['signals'][sig], frames)
    per_frame = OC.options_at(s['initial'], s['changes'], frames)
    for split in (None, 1, 5, 17):
        steps = BM.plan(per_frame, len(chans), split)
        stream = c1.EncoderStream(ctx, len(chans), opts(BM.detection_options(per_frame[0])))
        try:
            units = BM.run_plan_on_stream(stream, opts, chans, steps)
        finally:
            stream.close()
        err = OC.check_against(s['results'][sig], units, len(chans))
        assert err is None, (err, split)


@pytest.mark.parametrize('first', [0, 20])
def test_stream_state_after_a_modes_push_is_the_references(ctx, first):
    """`first` frames under detection (none: a fresh pool), a modes push, the state; then a fresh stream restored from that
    state continues like the original, and like the oracle, under detection and under further modes pushes"""
    frames = 60
    chans = [O.gen_pinkT(3, frames * 512), O.gen_white(2, frames * 512)]
    modes = BM.random_modes(7, frames, 2)
    a, b, c = first, first + 13, first + 30
    seg = lambda x, y: [ch[x * 512:y * 512] for ch in chans]
    u0, st = SL.oracle_encode(seg(0, a), {}) if a else (np.zeros((0, 212), np.uint8), np.zeros((2, SL.ENC_FLOATS), np.float32))
    mags_before = st[:, BM.MAGS].copy()
    u1, st = BM.oracle_encode_modes(seg(a, b), modes[a:b], 1.0, st)
    assert np.array_equal(SL.bits(st[:, BM.MAGS]), SL.bits(mags_before)) and mags_before.any() == (a > 0)
    u2, st2 = SL.oracle_encode(seg(b, c), {}, st)
    u3, _ = BM.oracle_encode_modes(seg(c, frames), modes[c:], 1.0, st2)
    s1, s2 = c1.EncoderStream(ctx, 2, opts({})), c1.EncoderStream(ctx, 2, opts({}))
    try:
        got0 = s1.push(seg(0, a)) if a else u0
        got1 = s1.push(seg(a, b), modes=modes[a:b])
        state = s1.get_state()
        assert np.array_equal(got0, u0) and np.array_equal(got1, u1)
        assert np.array_equal(SL.bits(state), SL.bits(st)), [k for k, (o, n) in SL.ENC_FIELDS.items() if not np.array_equal(SL.bits(state[:, o:o + n]), SL.bits(st[:, o:o + n]))]
        s2.set_state(state)
        for s in (s1, s2):
            assert np.array_equal(s.push(seg(b, c)), u2)
            assert np.array_equal(s.push(seg(c, frames), modes=modes[c:]), u3)
        # and the first frames after a restore under given modes (encoded from the explicit state)
        s2.set_state(state)
        assert np.array_equal(s2.push(seg(b, b + 1), modes=modes[a:a + 1]), BM.oracle_encode_modes(seg(b, b + 1), modes[a:a + 1], 1.0, st)[0])
    finally:
        s1.close()
        s2.close()


def test_modes_push_on_a_fixed_mode_stream(ctx):
    frames = 40
    chans = [O.gen_pinkT(4, frames * 512)]
    modes = BM.random_modes(9, frames, 1)
    fixed = {'fixedBlockModes': [2, 0, 3], 'allocationBias': 0.5}
    u0, st = SL.oracle_encode([chans[0][:10 * 512]], fixed)
    u1, st = BM.oracle_encode_modes([chans[0][10 * 512:25 * 512]], modes[10:25], 0.5, st)
    u2, _ = SL.oracle_encode([chans[0][25 * 512:]], fixed, st)
    s = c1.EncoderStream(ctx, 1, opts(fixed))
    try:
        got = [s.push([chans[0][:10 * 512]]), s.push([chans[0][10 * 512:25 * 512]], modes=modes[10:25]), s.push([chans[0][25 * 512:]])]
    finally:
        s.close()
    assert np.array_equal(np.concatenate(got), np.concatenate([u0, u1, u2]))


# ---- 6. host validation ----
@pytest.mark.parametrize('bad', [0x01, 0x10, 0x40, 0xFF])
def test_host_entry_points_reject_bytes_outside_the_domain(ctx, random_case, bad):
    lib = capi.load()
    r = random_case
    chans, nch, frames = r['chans'], 2, R_FRAMES
    field = 'low field' if bad & 1 else ('high field' if bad == 0x10 else 'bits 6-7')
    o = opts({}).to_c()
    ptrs = capi.ptr_array([c.ctypes.data for c in chans])
    s = c1.EncoderStream(ctx, nch, opts({}))
    try:
        head = s.push([c[:512 * 7] for c in chans])
        for at in (0, frames * nch - 1):
            m = r['modes'].reshape(-1).copy()
            m[at] = bad
            where = 'frame %d, channel %d' % (at // 2, at % 2)
            units = np.full((frames * nch, 212), 0xA5, dtype=np.uint8)
            assert lib.c1_encode_modes_batch(ctx._h, ptrs, nch, frames, 0, C.byref(o), m.ctypes.data, units.ctypes.data) == C1_ERR_ARG
            msg = lib.c1_last_error().decode()
            assert where in msg and field in msg and '0x%02x' % bad in msg, msg
            assert (units == 0xA5).all()
            assert lib.c1_enc_stream_push_modes(s._h, ptrs, frames, m.ctypes.data, units.ctypes.data) == C1_ERR_ARG
            msg = lib.c1_last_error().decode()
            assert where in msg and field in msg, msg
            assert (units == 0xA5).all()
            with pytest.raises(ValueError, match=where):
                ctx.encode_modes(chans, m)
        mono = np.zeros(5, dtype=np.uint8)
        mono[3] = bad
        assert lib.c1_encode_modes_batch(ctx._h, ptrs, 1, 5, 0, C.byref(o), mono.ctypes.data, units.ctypes.data) == C1_ERR_ARG
        msg = lib.c1_last_error().decode()
        assert 'frame 3' in msg and 'channel' not in msg, msg
        # the stream continues as if the calls had not been made
        rest = s.push([c[512 * 7:] for c in chans])
        assert np.array_equal(np.concatenate([head, rest]), ctx.encode(chans, opts({})))
        # frames = 0 writes nothing
        assert lib.c1_encode_modes_batch(ctx._h, ptrs, nch, 0, 0, C.byref(o), None, units.ctypes.data) == C1_OK
        assert lib.c1_enc_stream_push_modes(s._h, ptrs, 0, None, units.ctypes.data) == C1_OK
        assert lib.c1_encode_modes_device(ctx._h, ptrs, nch, 0, 0, C.byref(o), None, None) == C1_OK
        assert (units == 0xA5).all()
        assert ctx.encode_modes([c[:0] for c in chans], np.zeros(0, dtype=np.uint8)).shape == (0, 212)
    finally:
        s.close()


# ---- 7. the device entry point on bytes outside the domain ----
def test_device_entry_point_stays_in_bounds_for_any_byte(material):
    import torch
    c = c1.Context(0)
    try:
        frames = 256
        dev = [torch.from_numpy(material['white'][0][:frames * 512].copy()).cuda()]
        every = np.arange(256, dtype=np.uint8)
        got = dev_encode_modes(c, dev, frames, every, opts({}))
        assert got.shape == (frames, 212)
        inside = np.isin(every, BM.DOMAIN_BYTES)
        assert np.array_equal(BM.modes_of_units(got)[inside], every[inside])     # units of bytes in the domain took their modes
        check_constant_modes(c, material['pinkT'])
    finally:
        c.close()


# ---- the worked example of DESIGN.md 6e: per-band thresholds applied to the detector's scores on the host ----
def test_equal_thresholds_on_the_scores_reproduce_detection(ctx, material):
    import torch
    frames = 130
    chans = [c[:frames * 512] for c in material['pinkT']]
    dev = [torch.from_numpy(c.copy()).cuda() for c in chans]
    units = frames * 2
    scores = torch.zeros(units * 6, dtype=torch.float64, device='cuda')
    modes = torch.zeros(units, dtype=torch.uint8, device='cuda')
    opened = torch.zeros(1, dtype=torch.int32, device='cuda')
    torch.cuda.synchronize()
    ctx.detect_scores_device([d.data_ptr() for d in dev], frames, scores.data_ptr(), modes.data_ptr(), opened.data_ptr(), opts({}), speculative=False)
    ctx.synchronize()
    score = scores.cpu().numpy().reshape(units, 3, 2)[:, :, 0]
    own = c1.pack_block_modes((score > np.array([1.0, 1.0, 1.0])) * np.array([2, 2, 3]))
    assert np.array_equal(own, modes.cpu().numpy())
    assert np.array_equal(ctx.encode_modes(chans, own), ctx.encode(chans, opts({})))
    high_only = c1.pack_block_modes((score > np.array([np.inf, np.inf, 1.0])) * np.array([2, 2, 3]))
    assert set(high_only.tolist()) == {0x00, 0x30}
    assert np.array_equal(ctx.encode_modes(chans, high_only), BM.oracle_encode_modes(chans, high_only)[0])


# ---- 8. on a caller's stream ----
def test_on_a_callers_stream(random_case):
    """PCM and modes are written by work queued just before the call and the units are read by work queued just after, with
    no host synchronisation in between; then inputs and output are overwritten behind it"""
    import torch
    r = random_case
    S = torch.cuda.Stream()
    c = _context(stream=S.cuda_stream)
    try:
        src = [torch.from_numpy(x).cuda() for x in r['chans']]
        src_modes = torch.from_numpy(r['modes'].reshape(-1).copy()).cuda()
        pcm = [torch.zeros_like(x) for x in src]
        modes = torch.full_like(src_modes, 0x3a)
        units = torch.zeros(R_FRAMES * 2 * 212, dtype=torch.uint8, device='cuda')
        busy = torch.ones(1 << 26, dtype=torch.float32, device='cuda')
        torch.cuda.synchronize()
        o = opts({})
        call = lambda: c.encode_modes_device([p.data_ptr() for p in pcm], R_FRAMES, modes.data_ptr(), units.data_ptr(), o)
        with torch.cuda.stream(S):
            call()                                   # warm: options on the device, workspace grown (both drain the stream)
            S.synchronize()
            for _ in range(200):
                busy.mul_(-1.0)
            for p, x in zip(pcm, src):
                p.copy_(x)
            modes.copy_(src_modes)
            call()
            snapshot = units.clone()
            for p in pcm:
                p.zero_()
            modes.zero_()
            units.fill_(0xA5)
            queued_behind_busy_stream = not S.query()
            S.synchronize()
        assert queued_behind_busy_stream
        assert np.array_equal(snapshot.cpu().numpy().reshape(-1, 212), r['want'][1])
    finally:
        c.close()
