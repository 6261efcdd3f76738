"""GPU: contexts created on a caller's stream (c1_ctx_create(device, stream, ...), Context(0, stream=...)), ordered against
work that is not the library's.  A call is ordered after everything queued on the stream before it (a producer that writes
the input behind a long delay) and has finished with every buffer, inputs included, for everything queued after it (a
consumer that snapshots the output and then overwrites input and output), with no host synchronisation in between: on the
default path, the overlapped path (exact redo on the tail stream), the piped path (two internal streams forked from and
joined into the caller's), in call sequences, in whole chains over one and two contexts, on two streams at once, under the
host-synchronous entry points and when the context is closed.  Every expected byte is the oracle's.

The delay is a number of elementwise passes over a preallocated buffer, sized in the fixture from two measurements (printed):
the host time a warmed encode_device call takes to return, and the device time of the passes; it lasts at least 20 times the
former.  Every ordering case asserts `not S.query()` right after its last enqueue: the work really was queued behind a busy
stream.  A call that changes the options or grows the workspace drains the stream inside the library (upload_opts,
ensure_workspace), so every case is warmed first: the same call once, then S.synchronize()."""
import ctypes as C
import math
import os
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import geometry_lib as G
import oracle_lib as O
from test_gpu_geometry import (OPTSETS, POOL, SEQUENCE, enc_options, material, oracle_kw, oracle_pcm_window, oracle_window,
                               sequence_oracle)

pytestmark = pytest.mark.gpu

LABELS = ('long', 'short', 'detect', 'mixed_bias2')
OPTS = dict(OPTSETS)
FRAMES = 768                 # frames per channel of the ordering cases: twelve chunks of the chunked variants
CHUNK = 64
TONAL = (256, 512)           # frames of the real material replaced by stationary partials (forced speculation redoes most of
NOISE = (576, 768)           # them, about 4 % are packed again) and by white noise (about 5 % redone in every mode), which
                             # covers the last chunks: the last chunk's tail is the one that only the end of the call joins
VARIANTS = {'default': {'C1_OVERLAP': 0, 'C1_PIPELINE': 0, 'C1_CHUNK_FRAMES': 1 << 24},
            'overlap': {'C1_OVERLAP': 1, 'C1_PIPELINE': 0, 'C1_CHUNK_FRAMES': CHUNK},
            'piped': {'C1_OVERLAP': 0, 'C1_PIPELINE': 1, 'C1_CHUNK_FRAMES': CHUNK}}
SEQ_FRAMES = max(a + n for ch, n, a, l in SEQUENCE)
# The calls of test_call_sequence, (pass, index into SEQUENCE), that must be seen queued behind a busy stream.  A call that
# changes the options (upload_opts) or needs a larger workspace (ensure_workspace) drains the stream inside the library, the
# delay included; these three take the options of the call before them and are no larger than an earlier one.
SEQ_WITNESS = (('distinct', 4), ('shared', 0), ('shared', 4))
for _t, _i in SEQ_WITNESS:
    _k = _i + (len(SEQUENCE) if _t == 'shared' else 0)
    _twice = SEQUENCE + SEQUENCE
    assert _k > 0 and _twice[_k][3] == _twice[_k - 1][3] != 'detect', (_t, _i)
    assert _twice[_k][0] * _twice[_k][1] <= max(ch * n for ch, n, a, l in _twice[:_k]), (_t, _i)
BIG = 2 * 32768 + 300        # mono frames of the streamed host path (more than 65 536)
FILL = 0xA5
DELAY_CAP = 0.5              # seconds
assert FRAMES > CHUNK and FRAMES >= G.K_SPEC_MIN_UNITS


def modes_for(variant, label):
    """speculation modes of a variant's cases: the piped path is taken only where the call does not speculate"""
    return (0,) if variant == 'piped' and label in ('long', 'short') else (0, 1, 2)


def _context(stream, **env_vars):
    import carta1_amd as c1
    old = {k: os.environ.get(k) for k in env_vars}
    os.environ.update({k: str(v) for k, v in env_vars.items()})
    try:
        ctx = c1.Context(0, stream=stream.cuda_stream)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    assert ctx._h
    return ctx


def _partials(frames, seed):
    rng = np.random.RandomState(seed)
    t = np.arange(frames * 512, dtype=np.float64)
    x = sum(rng.uniform(0.05, 0.25) * np.sin(2 * np.pi * rng.uniform(100, 12000) * t / 44100 + rng.uniform(0, 6.28)) for _ in range(7))
    return x.astype(np.float32)


def real_material(seed):
    x = material(FRAMES, seed).copy()
    x[TONAL[0] * 512:TONAL[1] * 512] = _partials(TONAL[1] - TONAL[0], seed)
    x[NOISE[0] * 512:NOISE[1] * 512] = np.random.RandomState(seed + 1000).uniform(-0.5, 0.5, (NOISE[1] - NOISE[0]) * 512)
    return x


def decoy_material(seed):
    """another patchwork over a noise floor: never silent, so that no unit of it can equal a silent unit of the real one"""
    x = material(FRAMES, seed)
    return (x + np.random.RandomState(seed).uniform(-1e-3, 1e-3, x.size)).astype(np.float32)


def oracle_fields(units):
    f = [O.unpack_unit(u) for u in units]
    return {'nbfu': np.array([x.nbfu for x in f], np.int32), 'block_modes': np.array([x.modes[:] for x in f], np.int32),
            'sfi': np.array([x.sfi[:] for x in f], np.int32), 'wl': np.array([x.wl[:] for x in f], np.int32),
            'quantized': np.array([x.q[:] for x in f], np.int32)}


def oracle_coefs(pcm, modes):
    """the oracle's MDCT coefficients of a mono stream under fixed block modes"""
    st = O.EncState()
    m = np.array(modes, np.int32)
    out = np.zeros((len(pcm) // 512, 512), np.float32)
    bands = np.zeros(512, np.float32)
    for f in range(out.shape[0]):
        O.lib().c1o_qmf_analysis_frame(C.byref(st), O._fp(np.ascontiguousarray(pcm[f * 512:(f + 1) * 512])), O._fp(bands))
        O.lib().c1o_mdct_frame(C.byref(st), O._fp(bands), O._ip(m), O._fp(out[f]))
    return out


class Delay:
    """a bounded delay on the current stream: `passes` elementwise passes over a preallocated buffer"""

    def __init__(self, S, enqueue_s):
        import torch
        self.S = S
        self.buf = torch.ones(1 << 26, dtype=torch.float32, device='cuda')
        torch.cuda.synchronize()
        self.passes, self.cap = 64, 64
        per_pass = self.measure() / self.passes                     # the first measurement also warms the kernel
        per_pass = self.measure() / self.passes
        self.cap = max(1, int(DELAY_CAP / per_pass))
        self.passes = min(self.cap, max(1, math.ceil(40 * enqueue_s / per_pass)))      # twice the asserted 20 times: clocks vary
        self.seconds = self.measure()

    def __call__(self, scale=1):
        for _ in range(min(self.cap, self.passes * scale)):
            self.buf.mul_(-1.0)

    def measure(self):
        import torch
        with torch.cuda.stream(self.S):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            self()
            b.record()
            self.S.synchronize()
        return a.elapsed_time(b) * 1e-3


@pytest.fixture(scope='module')
def env():
    import torch
    S, S2 = torch.cuda.Stream(), torch.cuda.Stream()
    assert S.cuda_stream != 0 and S2.cuda_stream != 0 and S.cuda_stream != S2.cuda_stream
    real = [real_material(81), real_material(82)]
    decoy = [decoy_material(91), decoy_material(92)]
    seq_host = {0: material(SEQ_FRAMES, 71), 1: material(SEQ_FRAMES, 72)}      # test_gpu_geometry's streams: one oracle cache
    with ThreadPoolExecutor(POOL) as pool:
        enc = {(kind, l, ch): pool.submit(lambda src=src, l=l, ch=ch: O.encode_stream(src[:ch], **oracle_kw(OPTS[l]))[0])
               for kind, src in (('real', real), ('decoy', decoy)) for l in LABELS for ch in (1, 2)}
        enc = {k: v.result() for k, v in enc.items()}
        dec = {k: pool.submit(lambda u=u, ch=k[2]: O.decode_stream(u, ch)[0]) for k, u in enc.items()
               if k[1] == 'detect' or k in (('real', 'long', 2), ('decoy', 'mixed_bias2', 1))}
        dec = {k: v.result() for k, v in dec.items()}
    # a condition of the tests: the decoy's units differ from the real ones in every unit, its PCM in every frame
    for (kind, l, ch), u in enc.items():
        if kind == 'real':
            assert (u != enc['decoy', l, ch]).any(axis=1).all(), (l, ch)
    for ch in (1, 2):
        for c in range(ch):
            a, b = dec['real', 'detect', ch][c].view(np.uint32), dec['decoy', 'detect', ch][c].view(np.uint32)
            assert (a.reshape(-1, 512) != b.reshape(-1, 512)).any(axis=1).all(), (ch, c)
    e = {'S': S, 'S2': S2, 'real': real, 'decoy': decoy, 'host': seq_host, 'want': enc, 'want_pcm': dec,
         'real_dev': [torch.from_numpy(x).cuda() for x in real], 'decoy_dev': [torch.from_numpy(x).cuda() for x in decoy],
         'units_dev': {k: torch.from_numpy(u.reshape(-1)).cuda() for k, u in enc.items() if k[1] == 'detect'},
         'seq_dev': {c: torch.from_numpy(x).cuda() for c, x in seq_host.items()},
         'pcm': [torch.zeros(FRAMES * 512, dtype=torch.float32, device='cuda') for _ in range(2)],
         'units': torch.zeros(FRAMES * 2 * 212, dtype=torch.uint8, device='cuda'),
         'scratch': torch.zeros(FRAMES * 2 * 212, dtype=torch.uint8, device='cuda'),
         'copts': {l: enc_options(OPTS[l]).to_c() for l in LABELS}}
    torch.cuda.synchronize()
    e['ctx'] = {v: _context(S, **kw) for v, kw in VARIANTS.items()}
    e['ctx']['peer'] = _context(S, **VARIANTS['default'])               # a second context on the same stream
    e['ctx']['other'] = _context(S2, **VARIANTS['default'])             # and one on another stream
    # the host time a warmed encode_device call takes to return: the slowest of the variants and option sets
    ptrs = [x.data_ptr() for x in e['real_dev']]
    enqueue = 0.0
    for v in VARIANTS:
        for l in LABELS:
            ctx = e['ctx'][v]
            ctx.set_speculation(modes_for(v, l)[-1])
            took = []
            for _ in range(4):                                           # the first call warms: workspace, options
                t0 = time.perf_counter()
                ctx.encode_device(ptrs, FRAMES, e['scratch'].data_ptr(), c_options=e['copts'][l])
                took.append(time.perf_counter() - t0)
                S.synchronize()
            enqueue = max(enqueue, sorted(took[1:])[1])
    e['enqueue_s'] = enqueue
    e['delay'] = Delay(S, enqueue)
    print('\ncaller-stream fixture: warmed encode_device returns in %.1f us (slowest variant, %d stereo frames); the delay is %d passes, %.2f ms = %.0f times that'
          % (enqueue * 1e6, FRAMES, e['delay'].passes, e['delay'].seconds * 1e3, e['delay'].seconds / enqueue))
    assert e['delay'].seconds >= 20 * enqueue, ('the delay cannot cover 20 enqueue times under its cap', e['delay'].seconds, enqueue)
    yield e
    for ctx in e['ctx'].values():
        ctx.close()


def pcm_ptrs(e, ch):
    return [e['pcm'][c].data_ptr() for c in range(ch)]


def host_units(t, ch, frames=FRAMES):
    return t[:frames * ch * 212].cpu().numpy().reshape(-1, 212)


def first_bad(got, want):
    return np.flatnonzero((got != want).any(axis=1))[:4]


def late_path_stats(ctx):
    return ctx.speculation_stats()[1], ctx.quantization_stats()[1]


def check_late_paths(label, mode, before, after, where):
    """the exact redo (long / short) and the second packing pass (detect / mixed) ran in this very call"""
    if mode == 0:
        return
    if label in ('long', 'short'):
        assert after[0] - before[0] > 0, ('no unit was redone', where)
    else:
        assert after[1] - before[1] > 0, ('no unit was packed again', where)


# ---- 1. ordered after the caller's producer ---------------------------------------------------------------------------

@pytest.mark.parametrize('channels', [1, 2])
@pytest.mark.parametrize('variant', list(VARIANTS))
def test_encode_after_producer(env, variant, channels):
    """the PCM buffers hold the decoy; on S: delay, copy_ of the real PCM into them, encode_device.  The units are the oracle's
    for the real PCM"""
    import torch
    e, S, ctx = env, env['S'], env['ctx'][variant]
    for label in LABELS:
        for mode in modes_for(variant, label):
            where = (variant, channels, label, mode)
            ctx.set_speculation(mode)
            with torch.cuda.stream(S):
                ctx.encode_device(pcm_ptrs(e, channels), FRAMES, e['scratch'].data_ptr(), c_options=e['copts'][label])
                S.synchronize()                                          # warmed; no host synchronisation from here on
                for c in range(channels):
                    e['pcm'][c].copy_(e['decoy_dev'][c])
                e['units'].fill_(FILL)
                e['delay']()
                for c in range(channels):
                    e['pcm'][c].copy_(e['real_dev'][c])
                ctx.encode_device(pcm_ptrs(e, channels), FRAMES, e['units'].data_ptr(), c_options=e['copts'][label])
                busy = not S.query()
                S.synchronize()
            assert busy, ('not exercised: the stream was idle', where)
            got, want = host_units(e['units'], channels), e['want']['real', label, channels]
            assert np.array_equal(got, want), (where, first_bad(got, want))


@pytest.mark.parametrize('channels', [1, 2])
@pytest.mark.parametrize('variant', list(VARIANTS))
def test_decode_after_producer(env, variant, channels):
    """the units buffer holds the decoy's units; on S: delay, copy_ of the real units, decode_device"""
    import torch
    e, S, ctx, n = env, env['S'], env['ctx'][variant], FRAMES * channels * 212
    outs = [torch.zeros(FRAMES * 512, dtype=torch.float32, device='cuda') for _ in range(channels)]
    with torch.cuda.stream(S):
        ctx.decode_device(e['units'].data_ptr(), channels, FRAMES, [o.data_ptr() for o in outs])
        S.synchronize()
        e['units'][:n].copy_(e['units_dev']['decoy', 'detect', channels])
        for o in outs:
            o.fill_(float('nan'))
        e['delay']()
        e['units'][:n].copy_(e['units_dev']['real', 'detect', channels])
        ctx.decode_device(e['units'].data_ptr(), channels, FRAMES, [o.data_ptr() for o in outs])
        busy = not S.query()
        S.synchronize()
    assert busy, ('not exercised: the stream was idle', variant, channels)
    for c in range(channels):
        want = e['want_pcm']['real', 'detect', channels][c]
        assert np.array_equal(outs[c].cpu().numpy().view(np.uint32), want.view(np.uint32)), (variant, channels, c)


# ---- 2. ordered before the caller's consumer --------------------------------------------------------------------------

@pytest.mark.parametrize('channels', [1, 2])
@pytest.mark.parametrize('variant', list(VARIANTS))
def test_encode_before_consumer(env, variant, channels):
    """right behind encode_device on S: a clone of the units, then zeros over the units and the decoy over the PCM buffers.
    The clone holds the oracle's units, the units buffer stays zero, and the statistics show that the late paths (exact
    redo, second packing pass) ran"""
    import torch
    e, S, ctx, n = env, env['S'], env['ctx'][variant], FRAMES * channels * 212
    if variant == 'piped':
        assert FRAMES > CHUNK
    for label in LABELS:
        for mode in modes_for(variant, label):
            where = (variant, channels, label, mode)
            ctx.set_speculation(mode)
            with torch.cuda.stream(S):
                for c in range(channels):
                    e['pcm'][c].copy_(e['real_dev'][c])
                ctx.encode_device(pcm_ptrs(e, channels), FRAMES, e['scratch'].data_ptr(), c_options=e['copts'][label])
                warm = e['scratch'][:n].clone()                          # the allocator's block for the clone below
                S.synchronize()
                del warm
                before = late_path_stats(ctx)
                e['units'].fill_(FILL)
                e['delay']()
                ctx.encode_device(pcm_ptrs(e, channels), FRAMES, e['units'].data_ptr(), c_options=e['copts'][label])
                snap = e['units'][:n].clone()
                e['units'].zero_()                                       # the output first: a store that comes late lands on zeros
                for c in range(channels):
                    e['pcm'][c].copy_(e['decoy_dev'][c])
                busy = not S.query()
                S.synchronize()
            assert busy, ('not exercised: the stream was idle', where)
            got, want = host_units(snap, channels), e['want']['real', label, channels]
            assert np.array_equal(got, want), (where, first_bad(got, want))
            # The speculative packing pass stores every unit, the listed ones too, and most of those bytes are already the
            # exact ones: a redo that comes after the clone seldom shows in it.  It always shows in the buffer, which the
            # consumer has zeroed and which nothing may store into from then on (outside the window; the device-wide
            # synchronise also waits for an internal stream that was never joined)
            torch.cuda.synchronize()
            late = np.flatnonzero(host_units(e['units'], channels).any(axis=1))
            assert late.size == 0, ('units were stored after the consumer had zeroed the buffer', where, late[:4])
            after = late_path_stats(ctx)
            print('encode_before_consumer', where, 'redone %d packed again %d' % (after[0] - before[0], after[1] - before[1]))
            check_late_paths(label, mode, before, after, where)
            if variant == 'overlap' and mode and label in ('long', 'short'):
                # the tail of the last chunk is the one nothing inside the call waits for but the join at its end: that chunk
                # on its own (same context, same halo) must have units to redo.  halo_frames=2 is what the chunk loop of
                # encode_device_impl (c1_api.hip) gives every chunk past the second frame of a call: L.halo_frames =
                # min(2, f0 + halo_frames); the comparison with the oracle's window below fails if the two drift apart
                first = FRAMES - CHUNK
                assert first >= 2
                with torch.cuda.stream(S):
                    for c in range(channels):
                        e['pcm'][c].copy_(e['real_dev'][c])
                    ctx.encode_device([p + first * 2048 for p in pcm_ptrs(e, channels)], CHUNK, e['scratch'].data_ptr(),
                                      c_options=e['copts'][label], halo_frames=2)
                    S.synchronize()
                last = late_path_stats(ctx)
                print('encode_before_consumer', where, 'last chunk alone: redone %d' % (last[0] - after[0]))
                assert last[0] - after[0] > 0, ('no unit of the last chunk was redone', where)
                got = host_units(e['scratch'], channels, CHUNK)
                assert np.array_equal(got, want[first * channels:]), (where, 'last chunk alone')


@pytest.mark.parametrize('channels', [1, 2])
@pytest.mark.parametrize('variant', list(VARIANTS))
def test_decode_before_consumer(env, variant, channels):
    """right behind decode_device on S: clones of the PCM, then the decoy's units over the units buffer and NaN over the PCM"""
    import torch
    e, S, ctx, n = env, env['S'], env['ctx'][variant], FRAMES * channels * 212
    outs = [torch.zeros(FRAMES * 512, dtype=torch.float32, device='cuda') for _ in range(channels)]
    with torch.cuda.stream(S):
        e['units'][:n].copy_(e['units_dev']['real', 'detect', channels])
        ctx.decode_device(e['units'].data_ptr(), channels, FRAMES, [o.data_ptr() for o in outs])
        warm = [o.clone() for o in outs]
        S.synchronize()
        del warm
        for o in outs:
            o.fill_(float('nan'))
        e['delay']()
        ctx.decode_device(e['units'].data_ptr(), channels, FRAMES, [o.data_ptr() for o in outs])
        snaps = [o.clone() for o in outs]
        e['units'][:n].copy_(e['units_dev']['decoy', 'detect', channels])
        for o in outs:
            o.fill_(float('nan'))
        busy = not S.query()
        S.synchronize()
    assert busy, ('not exercised: the stream was idle', variant, channels)
    for c in range(channels):
        want = e['want_pcm']['real', 'detect', channels][c]
        assert np.array_equal(snaps[c].cpu().numpy().view(np.uint32), want.view(np.uint32)), (variant, channels, c)


# ---- 3. call sequences -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize('variant,mode', [('default', 1), ('overlap', 1), ('overlap', 2), ('piped', 0)])
def test_call_sequence(env, variant, mode):
    """test_gpu_geometry's SEQUENCE on a caller's stream, a delay in front of every call and a clone of its output right
    behind it, into distinct outputs and then all into one buffer: every clone equals its own oracle result.  A call that
    changes the options or grows the workspace drains the stream inside the library, delay included; the calls that do
    neither (SEQ_WITNESS) must be seen queued behind a busy stream"""
    import torch
    e, S, ctx = env, env['S'], env['ctx'][variant]
    want = sequence_oracle(e)
    assert SEQUENCE[3][0] * SEQUENCE[3][1] > max(ch * n for ch, n, a, l in SEQUENCE[:3])      # the fourth call grows the workspace
    ctx.set_speculation(mode)
    outs = [torch.zeros(n * ch * 212, dtype=torch.uint8, device='cuda') for ch, n, a, l in SEQUENCE]
    shared = torch.zeros(max(n * ch for ch, n, a, l in SEQUENCE) * 212, dtype=torch.uint8, device='cuda')
    copts = {l: enc_options(OPTS[l]).to_c() for l in set(l for ch, n, a, l in SEQUENCE)}
    torch.cuda.synchronize()
    before = late_path_stats(ctx)
    snaps, witnessed = [], []
    with torch.cuda.stream(S):
        for target in ('distinct', 'shared'):
            for i, (ch, n, a, l) in enumerate(SEQUENCE):
                out = outs[i] if target == 'distinct' else shared
                ptrs = [e['seq_dev'][c].data_ptr() + a * 512 * 4 for c in range(ch)]
                e['delay'](scale=-(-n // FRAMES))
                ctx.encode_device(ptrs, n, out.data_ptr(), c_options=copts[l])
                snaps.append(out[:n * ch * 212].clone())
                if (target, i) in SEQ_WITNESS:
                    witnessed.append((target, i, not S.query()))
        S.synchronize()
    assert len(witnessed) == len(SEQ_WITNESS) and all(w[2] for w in witnessed), ('not exercised: the stream was idle', witnessed)
    for k, snap in enumerate(snaps):
        ch, n, a, l = SEQUENCE[k % len(SEQUENCE)]
        got = snap.cpu().numpy().reshape(-1, 212)
        assert np.array_equal(got, want[k % len(SEQUENCE)]), (variant, mode, k, first_bad(got, want[k % len(SEQUENCE)]))
    ch, n, a, l = SEQUENCE[-1]
    assert np.array_equal(shared[:n * ch * 212].cpu().numpy().reshape(-1, 212), want[-1]), variant
    after = late_path_stats(ctx)
    if mode:
        assert after[0] > before[0], ('no unit was redone', variant, mode, before, after)


# ---- 4. a whole chain with one synchronise ---------------------------------------------------------------------------------

CHAIN_FRAMES = 512


@pytest.mark.parametrize('decoder', ['default', 'peer'], ids=['one_context', 'two_contexts'])
def test_chain_one_synchronise(env, decoder):
    """int16 interleaved bytes -> pcm_from_int_device -> encode_device -> decode_device -> pcm_to_int16_device on S, units and
    int16 samples cloned on the way, one synchronise at the end; the decoder in the same context or in a second one created
    on the same stream"""
    import torch
    e, S, enc, dec = env, env['S'], env['ctx']['default'], env['ctx'][decoder]
    n = CHAIN_FRAMES * 512
    pcm16 = np.clip(np.stack([c[:n] for c in e['real']], axis=1) * 8000.0, -32768, 32767).astype('<i2')
    raw_host = pcm16.reshape(-1).view(np.uint8).copy()
    f = O.pcm_from_int(raw_host, 16, 2)
    want_units, _ = O.encode_stream(f, **oracle_kw(OPTS['detect']))
    want_i16 = O.pcm_to_int16(O.decode_stream(want_units, 2)[0])
    raw = torch.from_numpy(raw_host).cuda()
    chans = [torch.zeros(n, dtype=torch.float32, device='cuda') for _ in range(2)]
    back = [torch.zeros(n, dtype=torch.float32, device='cuda') for _ in range(2)]
    units = torch.zeros(CHAIN_FRAMES * 2 * 212, dtype=torch.uint8, device='cuda')
    out = torch.zeros(2 * n, dtype=torch.int16, device='cuda')
    torch.cuda.synchronize()
    enc.set_speculation(1)

    def chain():
        enc.pcm_from_int_device(raw.data_ptr(), 16, 2, n, [c.data_ptr() for c in chans])
        enc.encode_device([c.data_ptr() for c in chans], CHAIN_FRAMES, units.data_ptr(), c_options=e['copts']['detect'])
        snap_u = units.clone()
        dec.decode_device(units.data_ptr(), 2, CHAIN_FRAMES, [b.data_ptr() for b in back])
        dec.pcm_to_int16_device([b.data_ptr() for b in back], n, out.data_ptr())
        return snap_u, out.clone()

    with torch.cuda.stream(S):
        warm = chain()
        S.synchronize()
        del warm
        for t in chans + back + [units, out]:
            t.zero_()
        e['delay']()
        snap_u, snap_i16 = chain()
        for t in chans + back + [units, out]:                            # the consumer reuses everything
            t.zero_()
        busy = not S.query()
        S.synchronize()
    assert busy, 'not exercised: the stream was idle'
    got = host_units(snap_u, 2, CHAIN_FRAMES)
    assert np.array_equal(got, want_units), first_bad(got, want_units)
    assert np.array_equal(snap_i16.cpu().numpy(), want_i16)


def test_chain_from_generator(env):
    """generate_device (host-synchronous: it drains the stream) feeding encode_device behind a delay, against O.gen_white"""
    import torch
    import carta1_amd as c1
    e, S, ctx = env, env['S'], env['ctx']['default']
    pcm = torch.zeros(CHAIN_FRAMES * 512, dtype=torch.float32, device='cuda')
    units = torch.zeros(CHAIN_FRAMES * 212, dtype=torch.uint8, device='cuda')
    torch.cuda.synchronize()
    white = O.gen_white(1, CHAIN_FRAMES * 512)
    want, _ = O.encode_stream([white], **oracle_kw(OPTS['detect']))
    ctx.set_speculation(1)
    with torch.cuda.stream(S):
        ctx.encode_device([pcm.data_ptr()], CHAIN_FRAMES, units.data_ptr(), c_options=e['copts']['detect'])
        warm = units.clone()
        S.synchronize()
        del warm
        units.fill_(FILL)
        e['delay']()
        ctx.generate_device(c1.SIGNAL_WHITE, 1, CHAIN_FRAMES, pcm.data_ptr())
        e['delay']()
        ctx.encode_device([pcm.data_ptr()], CHAIN_FRAMES, units.data_ptr(), c_options=e['copts']['detect'])
        snap_u, snap_p = units.clone(), pcm.clone()
        pcm.zero_()
        units.zero_()
        busy = not S.query()
        S.synchronize()
    assert busy, 'not exercised: the stream was idle'
    assert np.array_equal(snap_p.cpu().numpy().view(np.uint32), white.view(np.uint32))
    got = host_units(snap_u, 1, CHAIN_FRAMES)
    assert np.array_equal(got, want), first_bad(got, want)


# ---- 5. two caller streams -------------------------------------------------------------------------------------------

GUARD = 4096


def guarded(n, dtype, pattern):
    """an output of n elements with GUARD elements of a known pattern either side"""
    import torch
    t = torch.full((n + 2 * GUARD,), pattern, dtype=dtype, device='cuda')
    return t, t[GUARD:GUARD + n]


def guards_intact(t, pattern):
    import torch
    g = torch.cat([t[:GUARD], t[-GUARD:]])
    return bool((g == pattern).all())


def test_two_caller_streams(env):
    """contexts on S and S2, calls interleaved from one host thread: real stereo material with fixed long modes in mode 2 on S
    behind a delay, the mono decoy under mixed modes and bias 2 on S2 with no delay.  Each result equals its own oracle and
    the guard regions either side of every output keep their pattern"""
    import torch
    e, S, S2, A, B = env, env['S'], env['S2'], env['ctx']['default'], env['ctx']['other']
    ua_all, ua = guarded(FRAMES * 2 * 212, torch.uint8, 0x5C)
    ub_all, ub = guarded(FRAMES * 212, torch.uint8, 0x5C)
    pa = [guarded(FRAMES * 512, torch.float32, -12345.0) for _ in range(2)]
    pb = [guarded(FRAMES * 512, torch.float32, -12345.0)]
    torch.cuda.synchronize()
    A.set_speculation(2)
    B.set_speculation(1)
    a_in = [x.data_ptr() for x in e['real_dev']]
    b_in = [e['decoy_dev'][0].data_ptr()]

    def calls(delay):
        with torch.cuda.stream(S):
            if delay:
                e['delay']()
            A.encode_device(a_in, FRAMES, ua.data_ptr(), c_options=e['copts']['long'])
        with torch.cuda.stream(S2):
            B.encode_device(b_in, FRAMES, ub.data_ptr(), c_options=e['copts']['mixed_bias2'])
        with torch.cuda.stream(S):
            A.decode_device(ua.data_ptr(), 2, FRAMES, [p[1].data_ptr() for p in pa])
        with torch.cuda.stream(S2):
            B.decode_device(ub.data_ptr(), 1, FRAMES, [p[1].data_ptr() for p in pb])

    calls(False)
    S.synchronize()
    S2.synchronize()
    for t in (ua, ub):
        t.fill_(FILL)
    for p in pa + pb:
        p[1].fill_(float('nan'))
    torch.cuda.synchronize()
    before = late_path_stats(A)
    calls(True)
    busy = not S.query()
    S2.synchronize()
    got_b = host_units(ub, 1)
    S.synchronize()
    assert busy, 'not exercised: the stream was idle'
    assert late_path_stats(A)[0] > before[0], 'no unit was redone on S while the calls on S2 were interleaved'
    got_a = host_units(ua, 2)
    assert np.array_equal(got_a, e['want']['real', 'long', 2]), first_bad(got_a, e['want']['real', 'long', 2])
    assert np.array_equal(got_b, e['want']['decoy', 'mixed_bias2', 1]), first_bad(got_b, e['want']['decoy', 'mixed_bias2', 1])
    for c in range(2):
        assert np.array_equal(pa[c][1].cpu().numpy().view(np.uint32), e['want_pcm']['real', 'long', 2][c].view(np.uint32)), c
    assert np.array_equal(pb[0][1].cpu().numpy().view(np.uint32), e['want_pcm']['decoy', 'mixed_bias2', 1][0].view(np.uint32))
    assert guards_intact(ua_all, 0x5C) and guards_intact(ub_all, 0x5C)
    assert all(guards_intact(p[0], -12345.0) for p in pa + pb)


# ---- 6. host-synchronous entry points on a caller-stream context -------------------------------------------------------

class Queued:
    """the delay and one encode_device call behind it on the context's stream, into an output of its own"""

    def __init__(self, e, ctx, options):
        import torch
        self.e, self.ctx, self.S = e, ctx, e['S']
        self.copts = options.to_c()
        self.out = torch.zeros(FRAMES * 2 * 212, dtype=torch.uint8, device='cuda')
        torch.cuda.synchronize()

    def enqueue(self):
        import torch
        e, S = self.e, self.S
        ptrs = [x.data_ptr() for x in e['real_dev']]
        with torch.cuda.stream(S):
            self.ctx.encode_device(ptrs, FRAMES, self.out.data_ptr(), c_options=self.copts)
            S.synchronize()
            self.out.fill_(FILL)
            e['delay']()
            self.ctx.encode_device(ptrs, FRAMES, self.out.data_ptr(), c_options=self.copts)
            busy = not S.query()
        assert busy, 'not exercised: the stream was idle'

    def check(self, what):
        """after a host-synchronous call has returned: the stream is drained and the queued call's output complete"""
        import torch
        assert self.S.query(), ('the host call returned with work of the stream still pending', what)
        with torch.cuda.stream(self.S):
            got = self.out.cpu().numpy().reshape(-1, 212)
        want = self.e['want']['real', 'detect', 2]
        assert np.array_equal(got, want), (what, first_bad(got, want))


@pytest.fixture(scope='module')
def big():
    """material of the streamed host path and the oracle's windows around its chunk seams and ends"""
    pcm = material(BIG, 83)
    units = np.random.RandomState(31).randint(0, 256, size=(BIG, 212)).astype(np.uint8)
    wins = [(0, 3), (32768 - 3, 32768 + 3), (65536 - 3, 65536 + 3), (BIG - 3, BIG)]
    with ThreadPoolExecutor(POOL) as pool:
        wu = {w: pool.submit(oracle_window, [pcm], w[0], w[1], oracle_kw(OPTS['detect'])) for w in wins}
        wp = {w: pool.submit(oracle_pcm_window, units, 1, w[0], w[1]) for w in wins}
        return {'pcm': pcm, 'units': units, 'want_units': {w: f.result() for w, f in wu.items()},
                'want_pcm': {w: f.result() for w, f in wp.items()}}


@pytest.mark.parametrize('variant', ['default', 'overlap'])
def test_host_synchronous_entry_points(env, big, variant):
    """every host-synchronous entry point, called while the context's stream still holds the delay and a device call: it
    returns the oracle's bytes, and once it has returned the stream is drained and the queued call's output complete"""
    import carta1_amd as c1
    e, ctx = env, env['ctx'][variant]
    ctx.set_speculation(2 if variant == 'overlap' else 1)
    opts = enc_options(OPTS['detect'])
    q = Queued(e, ctx, opts)
    real2 = [x.copy() for x in e['real']]
    want_u, want_p = e['want']['real', 'detect', 2], e['want_pcm']['real', 'detect', 2]

    # encode / decode from pageable arrays
    q.enqueue()
    got = ctx.encode(real2, opts)
    q.check('encode')
    assert np.array_equal(got, want_u), first_bad(got, want_u)
    q.enqueue()
    pcm = ctx.decode(want_u, 2)
    q.check('decode')
    for c in range(2):
        assert np.array_equal(pcm[c].view(np.uint32), want_p[c].view(np.uint32)), c

    # the streamed path: page-locked arrays of more than 65 536 frames
    pin = c1.pinned_empty(BIG * 512, np.float32)
    pin[:] = big['pcm']
    pout = c1.pinned_empty((BIG, 212), np.uint8)
    pout[:] = 0
    q.enqueue()
    got = ctx.encode([pin], opts, out=pout)
    q.check('streamed encode')
    for (f0, f1), want in big['want_units'].items():
        assert np.array_equal(got[f0:f1], want), ('streamed encode', f0, f1)
    pu = c1.pinned_empty((BIG, 212), np.uint8)
    pu[:] = big['units']
    po = c1.pinned_empty(BIG * 512, np.float32)
    po[:] = 0
    q.enqueue()
    pcm = ctx.decode(pu, 1, out=[po])
    q.check('streamed decode')
    for (f0, f1), want in big['want_pcm'].items():
        assert np.array_equal(pcm[0][f0 * 512:f1 * 512].view(np.uint32), want[0].view(np.uint32)), ('streamed decode', f0, f1)
    del pin, pout, pu, po

    # a WAV body in, a WAV body out
    samples = FRAMES * 512 - 100
    pcm16 = np.clip(np.stack([c[:samples] for c in e['real']], axis=1) * 8000.0, -32768, 32767).astype('<i2')
    raw = pcm16.reshape(-1).view(np.uint8).copy()
    want_wav, _ = O.encode_stream([O.pad_frames(c) for c in O.pcm_from_int(raw, 16, 2)], **oracle_kw(OPTS['detect']))
    q.enqueue()
    got = ctx.encode_wav(raw, 16, 2, opts)
    q.check('encode_wav')
    assert np.array_equal(got, want_wav), first_bad(got, want_wav)
    q.enqueue()
    back = ctx.decode_wav16(want_u, 2)
    q.check('decode_wav16')
    assert np.array_equal(back.reshape(-1), O.pcm_to_int16(want_p))

    # stream pushes
    es, ds = c1.EncoderStream(ctx, 2, opts), c1.DecoderStream(ctx, 2)
    try:
        pos = 0
        for n in (100, 33, 200):
            q.enqueue()
            u = es.push([c[pos * 512:(pos + n) * 512] for c in real2])
            q.check('EncoderStream.push')
            assert np.array_equal(u, want_u[pos * 2:(pos + n) * 2]), ('EncoderStream.push', pos, n)
            q.enqueue()
            p = ds.push(want_u[pos * 2:(pos + n) * 2])
            q.check('DecoderStream.push')
            for c in range(2):
                assert np.array_equal(p[c].view(np.uint32), want_p[c][pos * 512:(pos + n) * 512].view(np.uint32)), ('DecoderStream.push', pos, c)
            pos += n
    finally:
        es.close()
        ds.close()

    # the stage functions: quantization of the oracle's coefficients, fields of the oracle's units, PCM of those fields
    frames = 96
    mono = e['real'][0][:frames * 512]
    long_units, _ = O.encode_stream([mono], **oracle_kw(OPTS['long']))
    fields = oracle_fields(long_units)
    q.enqueue()
    got = ctx.quantize_frames(oracle_coefs(mono, [0, 0, 0]), np.zeros((frames, 3), np.int32), enc_options(OPTS['long']))
    q.check('quantize_frames')
    for k in fields:
        assert np.array_equal(got[k], fields[k]), ('quantize_frames', k)
    q.enqueue()
    got = ctx.unpack_units(long_units)
    q.check('unpack_units')
    for k in fields:
        assert np.array_equal(got[k], fields[k]), ('unpack_units', k)
    q.enqueue()
    pcm = ctx.decode_fields(fields)
    q.check('decode_fields')
    assert np.array_equal(pcm[0].view(np.uint32), O.decode_stream(long_units, 1)[0][0].view(np.uint32))


# ---- 7. ownership -------------------------------------------------------------------------------------------------------

def test_close_joins_and_leaves_the_stream(env):
    """close() with a call still queued behind the delay returns once that call's output is complete; the stream is the
    caller's and goes on working, and another context can be created on it"""
    import torch
    e, S = env, env['S']
    ctx = _context(S, **VARIANTS['overlap'])
    ctx.set_speculation(2)
    ptrs = [x.data_ptr() for x in e['real_dev']]
    out = torch.zeros(FRAMES * 2 * 212, dtype=torch.uint8, device='cuda')
    out2 = torch.zeros_like(out)
    probe = torch.arange(1 << 16, dtype=torch.int64, device='cuda')
    torch.cuda.synchronize()
    try:
        with torch.cuda.stream(S):
            ctx.encode_device(ptrs, FRAMES, out.data_ptr(), c_options=e['copts']['long'])
            S.synchronize()
            out.fill_(FILL)
            e['delay']()
            ctx.encode_device(ptrs, FRAMES, out.data_ptr(), c_options=e['copts']['long'])
            busy = not S.query()
    finally:
        ctx.close()
    assert busy, 'not exercised: the stream was idle'
    assert S.query(), 'close() returned with the queued call still pending'
    want = e['want']['real', 'long', 2]
    with torch.cuda.stream(S):
        got = host_units(out, 2)
        doubled = (probe * 2 + 1).cpu().numpy()                          # the stream is still there and in order
    assert np.array_equal(got, want), first_bad(got, want)
    assert np.array_equal(doubled, np.arange(1 << 16, dtype=np.int64) * 2 + 1)
    again = _context(S, **VARIANTS['default'])
    try:
        with torch.cuda.stream(S):
            again.encode_device(ptrs, FRAMES, out2.data_ptr(), c_options=e['copts']['long'])
            snap = out2.clone()
            out2.zero_()
            S.synchronize()
    finally:
        again.close()
    assert np.array_equal(host_units(snap, 2), want)
    with torch.cuda.stream(S):                                           # and after the second close as well
        assert int((probe + 1).sum().item()) == (1 << 16) * ((1 << 16) + 1) // 2
