"""GPU: the decoded PCM error of given sound units, per 32 samples (c1_measure_pcm_device / _batch, k_measure_pcm).  Every
comparison is bit for bit: there are no decisions and no ties here.  Against the CPU model of tests/measure_pcm_lib.py (the
oracle's decoder and NumPy) for the units of plain and measured encodes over frame counts on, before and after the run seams;
against the library's own composition (c1_decode_device copied out, the definition applied in NumPy) for foreign bytes between
guard words, a corrupted stream and a context set to the binary32 decoder; the halos; silence, non-finite PCM, every subset of
the outputs, repeatability, a caller's stream; the timing kind; _batch against _device, chunked; the rejections."""
import itertools
import os

import numpy as np
import pytest

import carta1_amd as c1
from carta1_amd import capi
import best_bias_lib as BB
import measure_pcm_lib as MP
import measure_units_lib as MU
import oracle_lib as O
import scale_factor_choice_lib as SF

pytestmark = pytest.mark.gpu

C1_OK, C1_ERR_ARG = 0, 1   # include/carta1_hip.h
FRAMES = BB.FRAMES         # 130
HALO = BB.HALO             # 2
OUTPUTS = ('noise', 'signal', 'totals')
WIDTH = {'noise': 16, 'signal': 16, 'totals': 2}
FILL = -1.0
COUNTS = (1, 2, 3, 4, 5, 63, 64, 65, 130)        # the run length is 4 up to 8 192 units: on, before and after run seams
KINDS = ('detect', 'fixed203', 'fixed000', 'measured')


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


def measure(ctx, chans, units, hf=0, hu=0, ask=OUTPUTS):
    """c1_measure_pcm_batch with any subset of the outputs, the others passed as NULL -> dict of the ones asked for.  chans: hf
    frames of history first; units: the hu halo unit rows first"""
    chans = [np.ascontiguousarray(c, dtype=np.float32) for c in chans]
    nch, frames = len(chans), len(chans[0]) // 512 - hf
    n = frames * nch
    u = np.ascontiguousarray(units, dtype=np.uint8).reshape(-1, 212)
    assert u.shape[0] == n + hu * nch
    out = {k: np.full((n, WIDTH[k]), FILL) for k in OUTPUTS}
    ptrs = capi.ptr_array([c.ctypes.data + hf * 2048 for c in chans])
    capi.check(capi.load().c1_measure_pcm_batch(ctx._h, ptrs, nch, frames, hf, u.ctypes.data + hu * nch * 212, hu,
                                                *[out[k].ctypes.data if k in ask else None for k in OUTPUTS]))
    assert all((out[k] == FILL).all() for k in OUTPUTS if k not in ask)
    return {k: out[k] for k in ask}


def composed(ctx, chans, units, hf=0, hu=0):
    """the library's second opinion: c1_decode_batch of the same units on `ctx` (the exact decoder unless the context says
    otherwise), the definition applied in NumPy"""
    nch = len(chans)
    y = ctx.decode(units, nch, halo_units=hu)
    return MP.sums(y, [MP.delayed(c, hf) for c in chans])


def same(a, b):
    """bitwise equality of two output dicts (doubles compared as bit patterns)"""
    return a.keys() == b.keys() and all(np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) for k in a)


def rows(out, a, b, nch):
    return {k: v[a * nch:b * nch] for k, v in out.items()}


def channel(out, c):
    return {k: v[c::2] for k, v in out.items()}


def report(got, want):
    print('bit-equal: ' + ', '.join('%s %s' % (k, MP.bitwise(got[k], want[k])) for k in got))


@pytest.fixture(scope='module')
def mat(ctx):
    """two materials, HALO frames of history then FRAMES frames, stereo; per kind the units of the whole signal (history
    included, so that every frame has its real past)"""
    m = {'pink': BB.material()[0], 'white': [O.gen_white(s, (FRAMES + HALO) * 512) for s in (1, 2)]}
    m['units'] = {}
    for name in ('pink', 'white'):
        chans = m[name]
        for kind in KINDS:
            if kind == 'detect':
                u = ctx.encode(chans)
            elif kind == 'measured':
                u = ctx.encode_measured(chans, scale_factor_offsets=SF.OFFSETS, masking=True)[0]
            else:
                u = ctx.encode(chans, c1.EncoderOptions({'fixedBlockModes': [2, 0, 3] if kind == 'fixed203' else [0, 0, 0]}))
            u.setflags(write=False)
            m['units'][name, kind] = u
    return m


def body(mat, name):
    return [c[HALO * 512:] for c in mat[name]]


_models = {}


def model_of(mat, name, kind):
    """the model of the FRAMES frames from a zero decoder state and zero history (what a call without halos sees)"""
    if (name, kind) not in _models:
        _models[name, kind] = MP.model(body(mat, name), mat['units'][name, kind][HALO * 2:])
    return _models[name, kind]


# ---- 1. against the model ----
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('name', ['pink', 'white'])
def test_units_against_the_model(ctx, mat, name, kind):
    chans, units = body(mat, name), mat['units'][name, kind][HALO * 2:]
    m = model_of(mat, name, kind)
    got = measure(ctx, chans, units)
    report(got, m)
    assert same(got, m)
    assert (got['noise'] > 0).any() and (got['signal'] > 0).all(axis=1).any()
    if kind != 'measured':                                                    # the library's units are the oracle's
        opts = {'detect': None, 'fixed203': [2, 0, 3], 'fixed000': [0, 0, 0]}[kind]
        assert np.array_equal(O.encode_stream(mat[name], fixed_modes=opts)[0], mat['units'][name, kind])
    # the Python host: the same call
    assert same(dict(zip(OUTPUTS, ctx.measure_pcm(chans, units))), got)


@pytest.mark.parametrize('nch', [1, 2])
@pytest.mark.parametrize('name,kind', [('pink', 'detect'), ('white', 'measured')])
def test_frame_counts_against_the_model(ctx, mat, name, kind, nch):
    """the decoder is causal: the model of a prefix is the prefix of the model, and a mono call sees channel 0 alone"""
    chans, units = body(mat, name)[:nch], mat['units'][name, kind][HALO * 2:]
    m = model_of(mat, name, kind)
    if nch == 1:
        units, m = np.ascontiguousarray(units[0::2]), channel(m, 0)
    for frames in COUNTS:
        got = measure(ctx, [c[:frames * 512] for c in chans], units[:frames * nch])
        assert same(got, rows(m, 0, frames, nch)), (frames, nch)


def test_4097_stereo_frames_against_the_model(ctx, mat):
    """8 194 units: the run length is 5 there and the last run is partial"""
    frames = 4097
    reps = -(-frames // (FRAMES + HALO))
    chans = [np.tile(c, reps)[:frames * 512] for c in mat['pink']]
    units = ctx.encode(chans)
    m = MP.model(chans, units)
    got = measure(ctx, chans, units)
    report(got, m)
    assert same(got, m)


# ---- 2. against composition ----
def _device_buffers(torch, n, guard):
    g = guard // 8
    return {k: torch.full((2 * g + n * WIDTH[k],), FILL, dtype=torch.float64, device='cuda') for k in OUTPUTS}


def _device_call(c, pcm, frames, units, t, guard=0, hf=0, hu=0, nch=2, ask=OUTPUTS):
    p = {k: (t[k].data_ptr() + guard if k in ask else None) for k in OUTPUTS}
    c.measure_pcm_device([x.data_ptr() + hf * 2048 for x in pcm], frames, units.data_ptr() + hu * nch * 212, p['noise'], p['signal'],
                         p['totals'], halo_frames=hf, halo_units=hu)


def _to_host(t, n, guard=0):
    g = guard // 8
    out = {}
    for k, v in t.items():
        a = v.cpu().numpy()
        assert (a[:g] == FILL).all() and (a[len(a) - g:] == FILL).all(), k          # the words around the output are untouched
        out[k] = a[g:len(a) - g].reshape(n, WIDTH[k])
    return out


@pytest.mark.parametrize('domain', [True, False])
def test_foreign_bytes_through_the_device_entry_point(ctx, mat, domain):
    """512 units of random bytes (domain False: the mode bits random too): every unit is measured, the outputs are the
    composition's, and the 4 096 bytes on either side of every output keep their fill"""
    import torch
    frames, G = 256, 4096
    chans = [np.tile(c, 2)[:frames * 512] for c in body(mat, 'pink')]
    units = MU.random_units(20261020 + int(domain), frames * 2, domain)
    want = composed(ctx, chans, units)
    pcm = [torch.from_numpy(x).cuda() for x in chans]
    d_units = torch.from_numpy(units).cuda()
    t = _device_buffers(torch, frames * 2, G)
    _device_call(ctx, pcm, frames, d_units, t, G)
    ctx.synchronize()
    assert np.array_equal(d_units.cpu().numpy(), units) and all(np.array_equal(p.cpu().numpy(), x) for p, x in zip(pcm, chans))
    got = _to_host(t, frames * 2, G)
    report(got, want)
    assert same(got, want)
    assert np.isfinite(got['noise']).all() and (got['noise'] > 0).all(axis=1).any()
    assert same(measure(ctx, chans, units), got)


def test_a_corrupted_stream(ctx, mat):
    """one bit flipped in ten units: only the rows of that frame and the next of the same channel change, and the outputs are
    the composition's"""
    chans, units = body(mat, 'pink'), mat['units']['pink', 'measured'][HALO * 2:]
    clean = measure(ctx, chans, units)
    rs = np.random.RandomState(9)
    hit = np.sort(rs.permutation(units.shape[0] - 2)[:10])
    bad = units.copy()
    for u in hit:
        bit = int(rs.randint(16, 600))                           # amount, word lengths, scale factors, the first mantissas
        bad[u, bit >> 3] ^= 0x80 >> (bit & 7)
    got = measure(ctx, chans, bad)
    changed = set(np.flatnonzero((got['noise'] != clean['noise']).any(axis=1) | (got['totals'] != clean['totals']).any(axis=1)).tolist())
    allowed = set(hit.tolist()) | set((hit + 2).tolist())
    assert changed <= allowed and len(changed & set(hit.tolist())) >= 1, (sorted(changed), hit)
    assert MP.bitwise(got['signal'], clean['signal'])                                # the PCM's alone
    assert same(got, composed(ctx, chans, bad))


def test_the_decode_precision_setting_does_not_reach_the_meter(ctx, mat):
    chans, units = body(mat, 'pink'), mat['units']['pink', 'detect'][HALO * 2:]
    want = composed(ctx, chans, units)                                              # the exact decoder's composition
    c = c1.Context(0)
    try:
        c.set_decode_precision(True)
        got = measure(c, chans, units)
        assert same(got, want)
        assert not same(composed(c, chans, units), want)                            # that context's own decode() is the binary32 one
    finally:
        c.close()


# ---- 3. halos ----
@pytest.fixture(scope='module')
def whole(ctx, mat):
    """pink under detection: the rows of the FRAMES frames in a call over everything, the history's own units included, so
    that every one of them has its real past"""
    out = rows(measure(ctx, mat['pink'], mat['units']['pink', 'detect']), HALO, HALO + FRAMES, 2)
    for a in out.values():
        a.setflags(write=False)
    return out


@pytest.mark.parametrize('hf', [1, 2])
def test_a_tail_with_its_halos_equals_the_rows_of_the_whole(ctx, mat, whole, hf):
    """rows 40 .. of the 130-frame material equal a call on the tail with the unit halo and one or two frames of PCM halo"""
    units = mat['units']['pink', 'detect']
    start = HALO + 40
    got = measure(ctx, [c[(start - hf) * 512:] for c in mat['pink']], units[(start - 1) * 2:], hf=hf, hu=1)
    assert same(got, rows(dict(whole), 40, FRAMES, 2))


def test_tails_without_one_or_both_halos_against_the_model(ctx, mat, whole):
    units = mat['units']['pink', 'detect']
    start = HALO + 40
    tail_pcm = [c[start * 512:] for c in mat['pink']]
    # neither halo: the model of the tail from a zero state and zero history
    got = measure(ctx, tail_pcm, units[start * 2:])
    assert same(got, MP.model(tail_pcm, units[start * 2:]))
    assert not same(rows(got, 0, 1, 2), rows(dict(whole), 40, 41, 2))
    # the unit halo alone: the decoder continues, the first 266 samples are compared with zero
    got = measure(ctx, tail_pcm, units[(start - 1) * 2:], hu=1)
    assert same(got, MP.model(tail_pcm, units[(start - 1) * 2:], halo_units=1))
    assert (got['signal'][0, :8] == 0).all() and got['signal'][0, 8] > 0
    # the PCM halo alone: the history is there, the decoder starts fresh
    with_pcm = [c[(start - 1) * 512:] for c in mat['pink']]
    got = measure(ctx, with_pcm, units[start * 2:], hf=1)
    assert same(got, MP.model(with_pcm, units[start * 2:], halo_frames=1))
    assert MP.bitwise(got['signal'], whole['signal'][80:])


# ---- 4. edges, outputs, repeatability ----
def test_silence_gives_zeros(ctx, mat):
    silence = [np.zeros(FRAMES * 512, dtype=np.float32)] * 2
    got = measure(ctx, silence, ctx.encode(silence))
    for k in OUTPUTS:
        assert not got[k].view(np.uint64).any(), k                                   # +0.0 exactly
    # the units of a signal against silence: the noise is what the units decode to, the signal nothing
    got = measure(ctx, silence, mat['units']['pink', 'detect'][HALO * 2:])
    assert not got['signal'].view(np.uint64).any() and (got['noise'] > 0).any() and not got['totals'][:, 1].view(np.uint64).any()


def test_non_finite_pcm_falls_where_the_definition_says(ctx, mat):
    """a NaN at sample 3 * 512 + 17 of channel 1 is compared 266 samples later, in segment 8 of frame 3; an infinity at sample
    5 * 512 + 400 of channel 0 in segment 4 of frame 6; a NaN in the halo at sample -10 in segment 8 of frame 0"""
    chans = [np.array(c[(HALO - 1) * 512:(HALO + 8) * 512]) for c in mat['pink']]
    units = mat['units']['pink', 'detect'][HALO * 2:(HALO + 8) * 2]
    clean = measure(ctx, chans, units, hf=1)
    chans[1][512 + 3 * 512 + 17] = np.nan
    chans[0][512 + 5 * 512 + 400] = np.inf
    chans[0][512 - 10] = np.nan
    got = measure(ctx, chans, units, hf=1)
    want = np.zeros((16, 16), dtype=bool)
    want[3 * 2 + 1, 8] = want[6 * 2 + 0, 4] = want[0, 8] = True
    for k in ('noise', 'signal'):
        assert np.array_equal(~np.isfinite(got[k]), want), k
        assert np.array_equal(got[k][~want].view(np.uint64), clean[k][~want].view(np.uint64)), k
    assert np.array_equal(~np.isfinite(got['totals']), np.repeat(want.any(axis=1)[:, None], 2, axis=1))
    assert np.isnan(got['signal'][7, 8]) and np.isinf(got['signal'][12, 4])


def test_outputs_do_not_depend_on_which_are_asked_for_and_repeat(ctx, mat):
    chans, units = body(mat, 'pink'), mat['units']['pink', 'measured'][HALO * 2:]
    base = measure(ctx, chans, units)
    for ask in [s for k in (1, 2) for s in itertools.combinations(OUTPUTS, k)]:
        assert same(measure(ctx, chans, units, ask=ask), {k: base[k] for k in ask}), ask
    for _ in range(3):
        assert same(measure(ctx, chans, units), base)


def test_on_a_callers_stream(mat):
    """PCM and units are written by work queued just before the call and the outputs are read by work queued just after, with
    no host synchronisation in between; then inputs and outputs are overwritten behind it"""
    import torch
    S = torch.cuda.Stream()
    c = _context(stream=S.cuda_stream)
    try:
        chans, host_units = body(mat, 'pink'), mat['units']['pink', 'detect'][HALO * 2:]
        want = model_of(mat, 'pink', 'detect')
        src = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in chans]
        src_units = torch.from_numpy(np.array(host_units)).cuda()
        pcm = [torch.zeros_like(x) for x in src]
        units = torch.zeros_like(src_units)
        n = FRAMES * 2
        t = _device_buffers(torch, n, 0)
        busy = torch.ones(1 << 26, dtype=torch.float32, device='cuda')
        torch.cuda.synchronize()
        with torch.cuda.stream(S):
            for _ in range(200):
                busy.mul_(-1.0)
            for p, x in zip(pcm, src):
                p.copy_(x)
            units.copy_(src_units)
            _device_call(c, pcm, FRAMES, units, t)
            snap = {k: v.clone() for k, v in t.items()}
            for p in pcm:
                p.zero_()
            units.zero_()
            for v in t.values():
                v.fill_(FILL)
            queued_behind_busy_stream = not S.query()
            S.synchronize()
        assert queued_behind_busy_stream
        assert same(_to_host(snap, n), want)
    finally:
        c.close()


# ---- 5. launch accounting, _batch against _device ----
@pytest.mark.parametrize('chunk', [None, 7])
def test_batch_equals_device_and_the_kernel_is_counted(mat, chunk):
    """the device call: one "meter_pcm" launch, no "decode" launch; the batch call: one per chunk (a context's chunk is at
    least 16 frames), the same bits"""
    import torch
    c = _context(**({} if chunk is None else {'C1_CHUNK_FRAMES': chunk}))
    try:
        chans, units = mat['pink'], mat['units']['pink', 'measured']
        n = FRAMES * 2
        pcm = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in chans]
        d_units = torch.from_numpy(np.array(units[2:])).cuda()               # from the halo units on
        t = _device_buffers(torch, n, 0)
        c.set_profiling(True)
        _device_call(c, pcm, FRAMES, d_units, t, hf=HALO, hu=1)
        c.synchronize()
        ms, launches = c.kernel_ms('meter_pcm')
        assert launches == 1 and ms > 0
        assert all(c.kernel_ms(k)[1] == 0 for k in ('decode', 'meter', 'analysis', 'decode_fields'))
        dev = _to_host(t, n)
        got = measure(c, chans, units[2:], hf=HALO, hu=1)
        assert same(got, dev)
        chunks = 1 if chunk is None else -(-FRAMES // 16)
        assert c.kernel_ms('meter_pcm')[1] == chunks and c.kernel_ms('decode')[1] == 0
        # and a subset of the outputs through the chunks
        assert same(measure(c, chans, units[2:], hf=HALO, hu=1, ask=('totals',)), {'totals': dev['totals']})
    finally:
        c.close()


# ---- 6. the rejections ----
def test_rejections_leave_the_outputs_untouched(ctx, mat):
    lib = capi.load()
    err = lambda: lib.c1_last_error().decode()
    chans, units = body(mat, 'pink'), np.array(mat['units']['pink', 'detect'][HALO * 2:])
    base = measure(ctx, chans, units)
    ptrs = capi.ptr_array([c.ctypes.data for c in chans])
    n = FRAMES * 2
    out = {k: np.full((n, WIDTH[k]), FILL) for k in OUTPUTS}
    outs = [out[k].ctypes.data for k in OUTPUTS]
    dptr = capi.ptr_array([0x1000, 0x2000])        # the device call decides on its arguments before it touches a pointer

    def call(fn, p, u, o=outs, nch=2, frames=FRAMES, hf=0, hu=0):
        return fn(ctx._h, p, nch, frames, hf, u, hu, *o)

    for fn, p, u in ((lib.c1_measure_pcm_batch, ptrs, units.ctypes.data), (lib.c1_measure_pcm_device, dptr, 0x3000)):
        assert call(fn, p, u, o=[None] * 3) == C1_ERR_ARG and 'all NULL' in err(), err()
        assert call(fn, p, None) == C1_ERR_ARG and 'units is NULL' in err(), err()
        assert call(fn, None, u) == C1_ERR_ARG and 'pcm is NULL' in err(), err()
        assert call(fn, p, u, nch=3) == C1_ERR_ARG and call(fn, p, u, nch=0) == C1_ERR_ARG
        assert call(fn, p, u, hf=3) == C1_ERR_ARG and call(fn, p, u, hf=-1) == C1_ERR_ARG
        assert call(fn, p, u, hu=2) == C1_ERR_ARG and call(fn, p, u, hu=-1) == C1_ERR_ARG
        assert call(fn, p, u, frames=-1) == C1_ERR_ARG and call(fn, p, u, frames=(1 << 22) + 1) == C1_ERR_ARG and '2^22' in err(), err()
        assert call(fn, p, u, frames=0) == C1_OK
    assert call(lib.c1_measure_pcm_device, dptr, 0x3001) == C1_ERR_ARG and '4-byte aligned' in err(), err()
    assert call(lib.c1_measure_pcm_device, capi.ptr_array([0x1000, 0x2004]), 0x3000) == C1_ERR_ARG and '16-byte aligned' in err(), err()
    assert all((out[k] == FILL).all() for k in OUTPUTS)
    with pytest.raises(ValueError, match='sound units'):
        ctx.measure_pcm(chans, units[:-1])
    # the next call is unharmed
    assert same(measure(ctx, chans, units), base)
