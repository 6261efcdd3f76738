"""GPU: encode and decode over the layouts of the work, which depend only on the size and order of calls (geometry_lib.py
restates the rules): every run length c1k_pick_run hands the frame-walking kernels, full and partial last runs, the
workgroup permutation of the speculative analysis over many grid sizes, the speculation cut-off of the default mode,
forced runs, chunk seams of the piped and overlapped paths, device calls issued back to back, and stream pushes of every
size around the run and cut-off boundaries.  Bytes and exact PCM equal the oracle's; binary32 PCM stays within
test_gpu_decode32's bounds.  Material: _patchwork (block switching, every scale-factor range, silence, clipping)."""
import hashlib
import json
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import geometry_lib as G
import oracle_lib as O
from test_gpu_parity import _patchwork

pytestmark = pytest.mark.gpu

OPTSETS = [('long', {'fixedBlockModes': [0, 0, 0]}), ('short', {'fixedBlockModes': [2, 2, 3]}), ('detect', {}),
           ('detect_low', {'transientThresholdLow': 0.3}), ('mixed_bias2', {'fixedBlockModes': [0, 2, 3], 'allocationBias': 2.0})]
RUNS = (5, 6, 7, 15, 16, 17, 31, 33, 63)
WHOLE_UNITS = 20000          # above this many units a batch is checked against the oracle on windows around run seams
POOL = 16


def oracle_kw(o):
    return {'fixed_modes': o.get('fixedBlockModes'), 'bias': o.get('allocationBias', 1.0),
            'threshold': o.get('transientThresholdLow', 1.0)}


def enc_options(o):
    import carta1_amd as c1
    return c1.EncoderOptions(o, biased_table=O.biased_table(o.get('allocationBias', 1.0)))


def rms(a, b):
    return float(np.sqrt(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)))


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def material(frames, seed):
    """patchwork in 4096-frame pieces (each piece its own segments): the same stream for every size, so every batch is
    a prefix of it and the oracle's units for a batch are a prefix of its units for the longest one"""
    return np.concatenate([_patchwork(4096, seed * 1000 + i) for i in range((frames + 4095) // 4096)])[:frames * 512]


def _ends(run, channels):
    lo, hi = G.frames_for_run(run, channels)
    a = lo + (1 - lo) % run                      # first frames count of the range with frames = 1 (mod run)
    b = hi - (hi - (run - 1)) % run              # last with frames = run - 1 (mod run)
    assert lo <= a <= hi and lo <= b <= hi and G.pick_run(a, channels) == run == G.pick_run(b, channels)
    return [a, b]


def sweep_sizes():
    mono = [1, 2, 63, 64, 65, 127, 8191, 8192, 8193] + [f for r in RUNS for f in _ends(r, 1)]
    stereo = [1, 31, 32, 33, 63, 64, 4095, 4096, 4097] + [f for r in RUNS for f in _ends(r, 2)]
    full = G.K_RUN_DEFAULT * G.SPLIT // 2 + 1                    # stereo, run 64, a last run of one frame
    assert G.pick_run(full, 2) == G.K_RUN_DEFAULT and full % G.K_RUN_DEFAULT == 1
    return [(f, 1) for f in mono] + [(f, 2) for f in stereo + [full]]


SIZES = sweep_sizes()
MAX_FRAMES = {ch: max(f for f, c in SIZES if c == ch) for ch in (1, 2)}
WHOLE_FRAMES = {ch: max(f for f, c in SIZES if c == ch and f * c <= WHOLE_UNITS) for ch in (1, 2)}


def windows(frames, channels):
    """[f0, f1) around the first, a middle and the last run seam of the encoder's and the decoders' runs, and both ends"""
    out = {(0, min(frames, 3)), (max(0, frames - 3), frames)}
    for run in {G.pick_run(frames, channels), G.pick_run(frames, 1)}:
        nr = -(-frames // run)
        for s in (run, (nr // 2) * run, (nr - 1) * run):
            if 0 < s < frames:
                out.add((max(0, s - 3), min(frames, s + 3)))
    return sorted(out)


def oracle_window(chans, f0, f1, kw):
    """the oracle's units for frames [f0, f1) of a stream, started fresh two frames before f0"""
    s = max(0, f0 - 2)
    u, _ = O.encode_stream([c[s * 512:f1 * 512] for c in chans], **kw)
    return u[(f0 - s) * len(chans):]


def oracle_pcm_window(units, channels, f0, f1):
    """the oracle's PCM for frames [f0, f1) of a unit stream, started fresh one unit before f0"""
    s = max(0, f0 - 1)
    pcm, _ = O.decode_stream(units[s * channels:f1 * channels], channels)
    return [p[(f0 - s) * 512:] for p in pcm]


@pytest.fixture(scope='module')
def env():
    import torch
    import carta1_amd as c1
    host = {0: material(MAX_FRAMES[1], 71), 1: material(MAX_FRAMES[2], 72)}
    dev = {c: torch.from_numpy(x).cuda() for c, x in host.items()}
    rng = np.random.RandomState(29)
    rand = {ch: rng.randint(0, 256, size=(MAX_FRAMES[ch] * ch, 212)).astype(np.uint8) for ch in (1, 2)}
    jobs = {}
    with ThreadPoolExecutor(POOL) as pool:
        for label, o in OPTSETS:
            for ch in (1, 2):
                chans = [host[c][:WHOLE_FRAMES[ch] * 512] for c in range(ch)]
                jobs[label, ch] = pool.submit(lambda chans=chans, o=o: O.encode_stream(chans, **oracle_kw(o))[0])
        want = {k: v.result() for k, v in jobs.items()}
        pcm_jobs = {(label, ch): pool.submit(lambda u=want[label, ch], ch=ch: O.decode_stream(u, ch)[0])
                    for label in ('detect', 'mixed_bias2') for ch in (1, 2)}
        for ch in (1, 2):
            pcm_jobs['random', ch] = pool.submit(lambda ch=ch: O.decode_stream(rand[ch][:WHOLE_FRAMES[ch] * ch], ch)[0])
        want_pcm = {k: v.result() for k, v in pcm_jobs.items()}
    ctx = c1.Context(0)
    torch.cuda.synchronize()
    yield {'ctx': ctx, 'host': host, 'dev': dev, 'want': want, 'want_pcm': want_pcm, 'rand': rand}
    ctx.set_speculation(1)
    ctx.set_decode_precision(False)
    ctx.close()


def encode_dev(ctx, dev, channels, frames, opts, out):
    ctx.encode_device([dev[c].data_ptr() for c in range(channels)], frames, out.data_ptr(), opts)


def check_units(e, label, o, channels, frames, got, pool):
    """got: the batch's units (host); against the oracle whole or on windows"""
    if frames * channels <= WHOLE_UNITS:
        want = e['want'][label, channels][:frames * channels]
        bad = np.flatnonzero((got != want).any(axis=1))
        assert bad.size == 0, (label, channels, frames, 'units differ from', bad[:4])
        return
    chans = [e['host'][c] for c in range(channels)]
    futs = {w: pool.submit(oracle_window, chans, w[0], w[1], oracle_kw(o)) for w in windows(frames, channels)}
    for (f0, f1), fut in futs.items():
        assert np.array_equal(got[f0 * channels:f1 * channels], fut.result()), (label, channels, frames, f0, f1)


def decode_all_ways(ctx, units, channels, frames):
    """exact: decode, decode_device, the decoder stage chain; binary32: whole and from a slice with one unit of halo"""
    import torch
    ctx.set_decode_precision(False)
    host = ctx.decode(units, channels)
    du = torch.from_numpy(np.ascontiguousarray(units).reshape(-1)).cuda()
    outs = [torch.full((frames * 512,), float('nan'), dtype=torch.float32, device='cuda') for _ in range(channels)]
    torch.cuda.synchronize()
    ctx.decode_device(du.data_ptr(), channels, frames, [o.data_ptr() for o in outs])
    ctx.synchronize()
    device = [o.cpu().numpy() for o in outs]
    u3 = units.reshape(frames, channels, 212)
    stages = []
    for c in range(channels):
        fields = ctx.unpack_units(np.ascontiguousarray(u3[:, c]))
        coefs = ctx.dequantize_frames(fields)
        bands = ctx.imdct(coefs, fields['block_modes'])
        stages.append(ctx.qmf_synthesis(bands).reshape(-1))
    ctx.set_decode_precision(True)
    b32 = ctx.decode(units, channels)
    cut = frames // 2 + 1 if frames > 2 else 0
    b32_part = ctx.decode(units[max(0, cut - 1) * channels:], channels, halo_units=min(1, cut)) if cut else None
    ctx.set_decode_precision(False)
    for c in range(channels):
        assert np.array_equal(device[c].view(np.uint32), host[c].view(np.uint32)), ('decode_device', frames, c)
        assert np.array_equal(stages[c].view(np.uint32), host[c].view(np.uint32)), ('stage chain', frames, c)
        if b32_part is not None:
            assert np.array_equal(b32_part[c], b32[c][cut * 512:], equal_nan=True), ('binary32 split', frames, c)
    return host, b32


def check_pcm(e, key, units, channels, frames, host, b32, pool, exact_only=False):
    """exact PCM bit for bit, binary32 PCM within test_gpu_decode32's bounds, against the oracle whole or on windows"""
    if frames * channels <= WHOLE_UNITS:
        parts = [((0, frames), [p[:frames * 512] for p in e['want_pcm'][key, channels]])]
    else:
        parts = [(w, pool.submit(oracle_pcm_window, units, channels, w[0], w[1])) for w in windows(frames, channels)]
    for (f0, f1), ref in parts:
        ref = ref if isinstance(ref, list) else ref.result()
        for c in range(channels):
            got = host[c][f0 * 512:f1 * 512]
            assert np.array_equal(got.view(np.uint32), ref[c].view(np.uint32)), (key, channels, frames, f0, f1, c)
            if not exact_only:
                g32 = b32[c][f0 * 512:f1 * 512]
                ok = np.isfinite(ref[c])
                scale = max(1.0, float(np.abs(ref[c][ok]).max(initial=0.0)))
                assert np.array_equal(ok, np.isfinite(g32)), (key, frames, c)
                assert rms(g32[ok], ref[c][ok]) < 1e-6 * scale, (key, channels, frames, f0, f1, c)


@pytest.mark.parametrize('channels', [1, 2])
def test_size_sweep_every_run_length(env, channels):
    """every size of SIZES in speculation modes 0, 1 and 2 and every option set: the modes agree bit for bit, mode 0
    equals the oracle; the units of two option sets and random unit bytes decode to the oracle's PCM in every decoder"""
    import torch
    e = env
    ctx, dev = e['ctx'], e['dev']
    sizes = [f for f, c in SIZES if c == channels]
    out = {m: torch.zeros(MAX_FRAMES[channels] * channels * 212, dtype=torch.uint8, device='cuda') for m in (0, 1, 2)}
    seen_runs = set()
    with ThreadPoolExecutor(POOL) as pool:
        for label, o in OPTSETS:
            opts = enc_options(o)
            for frames in sizes:
                n = frames * channels * 212
                for m in (0, 1, 2):                              # a unit a mode leaves unwritten keeps this fill
                    out[m][:n].fill_(0xA5 + m)
                torch.cuda.synchronize()
                for m in (0, 1, 2):
                    ctx.set_speculation(m)
                    encode_dev(ctx, dev, channels, frames, opts, out[m])
                ctx.synchronize()
                for m in (1, 2):
                    assert torch.equal(out[m][:n], out[0][:n]), (label, channels, frames, 'mode', m)
                got = out[0][:n].cpu().numpy().reshape(-1, 212)
                check_units(e, label, o, channels, frames, got, pool)
                seen_runs.add(G.pick_run(frames, channels))
                if label in ('detect', 'mixed_bias2'):
                    host, b32 = decode_all_ways(ctx, got, channels, frames)
                    check_pcm(e, label, got, channels, frames, host, b32, pool)
        ctx.set_speculation(1)
        for frames in sizes:
            units = e['rand'][channels][:frames * channels]
            host, b32 = decode_all_ways(ctx, units, channels, frames)
            check_pcm(e, 'random', units, channels, frames, host, b32, pool, exact_only=True)
    assert set(RUNS) <= seen_runs and G.RUN_FLOOR in seen_runs
    assert channels == 1 or G.K_RUN_DEFAULT in seen_runs


def test_speculation_cut_off(env):
    """mode 1 takes the exact kernels below kSpecMinUnits units and speculates from there on (the statistics say which
    path ran); the bytes equal the oracle's either way"""
    import carta1_amd as c1
    import torch
    e = env
    k = G.K_SPEC_MIN_UNITS
    ctx = c1.Context(0)
    out = torch.zeros((k + 2) * 2 * 212, dtype=torch.uint8, device='cuda')
    try:
        for channels, sizes in ((1, (k - 1, k, k + 1)), (2, (k // 2 - 1, k // 2, k // 2 + 1))):
            for frames in sizes:
                units = frames * channels
                for label, o in OPTSETS:
                    s0 = ctx.speculation_stats()[0], ctx.speculation_deferred(), ctx.quantization_stats()[0], ctx.detection_stats()[0]
                    out.fill_(0xA5)
                    torch.cuda.synchronize()
                    encode_dev(ctx, e['dev'], channels, frames, enc_options(o), out)
                    ctx.synchronize()
                    got = out[:units * 212].cpu().numpy().reshape(-1, 212)
                    assert np.array_equal(got, e['want'][label, channels][:units]), (label, channels, frames)
                    s1 = ctx.speculation_stats()[0], ctx.speculation_deferred(), ctx.quantization_stats()[0], ctx.detection_stats()[0]
                    spec, deferred, quant, det = (b - a for a, b in zip(s0, s1))
                    where = (label, channels, frames, spec, deferred, quant, det)
                    if units < k:
                        assert spec == deferred == quant == det == 0, where
                    elif label in ('long', 'short'):
                        assert spec + deferred == units and quant == deferred and det == 0, where
                    else:
                        assert spec == deferred == 0 and quant == units, where
                        assert det == (units if label.startswith('detect') else 0), where
    finally:
        ctx.close()


def _context(**env_vars):
    import carta1_amd as c1
    old = {k: os.environ.get(k) for k in env_vars}
    os.environ.update({k: str(v) for k, v in env_vars.items()})
    try:
        return c1.Context(0)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


@pytest.mark.parametrize('chunk', [16, 37, 64])
def test_chunk_seams(env, chunk):
    """contexts that cut a call into chunks of 16, 37 and 64 frames, with and without the two-stage pipeline (mode 0 and
    the exact option sets: `piped` halves) and the tail overlap (modes 1 and 2 on fixed long / short modes: `overlap`
    halves): the bytes equal a default context's and the oracle's"""
    e = env
    ctxs = [_context(C1_CHUNK_FRAMES=chunk), _context(C1_CHUNK_FRAMES=chunk, C1_PIPELINE=1, C1_OVERLAP=1)]
    try:
        for channels, frames in ((2, 700), (1, 301)):
            chans = [e['host'][c][:frames * 512] for c in range(channels)]
            for label, o in OPTSETS:
                opts = enc_options(o)
                want = e['want'][label, channels][:frames * channels]
                assert np.array_equal(e['ctx'].encode(chans, opts), want), (label, channels)
                for i, ctx in enumerate(ctxs):
                    for m in (0, 1, 2):
                        ctx.set_speculation(m)
                        got = ctx.encode(chans, opts)
                        assert np.array_equal(got, want), (chunk, i, label, channels, 'mode', m, np.flatnonzero((got != want).any(axis=1))[:4])
    finally:
        for ctx in ctxs:
            ctx.close()


# (channels, frames, first frame of the material, option set): different inputs and sizes, the fourth call grows the
# workspace, long-speculative calls next to each other, detection and short calls between them, an exact-only mono call
SEQUENCE = [(2, 2000, 0, 'long'), (2, 2000, 5000, 'detect'), (1, 3000, 3000, 'short'), (2, 4500, 1000, 'long'),
            (2, 2500, 11000, 'long'), (2, 1500, 700, 'mixed_bias2'), (1, 50, 8000, 'long'), (2, 2000, 20000, 'short'),
            (2, 1800, 30000, 'long')]
_sequence_oracle = []


def sequence_oracle(e):
    if not _sequence_oracle:
        opts = dict(OPTSETS)
        with ThreadPoolExecutor(POOL) as pool:
            futs = [pool.submit(lambda ch=ch, n=n, a=a, l=l: O.encode_stream([e['host'][c][a * 512:(a + n) * 512] for c in range(ch)], **oracle_kw(opts[l]))[0])
                    for ch, n, a, l in SEQUENCE]
            _sequence_oracle.extend(f.result() for f in futs)
    return _sequence_oracle


@pytest.mark.parametrize('overlap', [0, 1], ids=['inline', 'overlap'])
def test_back_to_back_device_calls(env, overlap):
    """encode_device calls on one context that owns its stream, enqueued without a synchronise in between: into distinct
    outputs (each equals its own oracle result) and all into one buffer at the same offset (it holds the last call's
    result: a late store of an earlier call's tail would show there)"""
    import torch
    e = env
    want = sequence_oracle(e)
    assert SEQUENCE[3][0] * SEQUENCE[3][1] > max(ch * n for ch, n, a, l in SEQUENCE[:3])      # the fourth call grows the workspace
    ctx = _context(C1_OVERLAP=overlap)
    try:
        outs = [torch.zeros(n * ch * 212, dtype=torch.uint8, device='cuda') for ch, n, a, l in SEQUENCE]
        shared = torch.zeros(max(n * ch for ch, n, a, l in SEQUENCE) * 212, dtype=torch.uint8, device='cuda')
        copts = {l: enc_options(o).to_c() for l, o in OPTSETS}
        torch.cuda.synchronize()
        for target in ('distinct', 'shared'):
            for i, (ch, n, a, l) in enumerate(SEQUENCE):
                ptrs = [e['dev'][c].data_ptr() + a * 512 * 4 for c in range(ch)]
                ctx.encode_device(ptrs, n, (outs[i] if target == 'distinct' else shared).data_ptr(), c_options=copts[l])
        ctx.synchronize()
        for i, (ch, n, a, l) in enumerate(SEQUENCE):
            assert np.array_equal(outs[i].cpu().numpy().reshape(-1, 212), want[i]), (overlap, i)
        ch, n, a, l = SEQUENCE[-1]
        assert np.array_equal(shared[:n * ch * 212].cpu().numpy().reshape(-1, 212), want[-1]), overlap
        if overlap:
            assert ctx.speculation_stats()[0] > 0
    finally:
        ctx.close()


PUSHES = (1, 31, 32, 33, 0, 63, 64, 65, 200, 4097)


@pytest.mark.parametrize('mode', [1, 2])
def test_stream_pushes(env, mode):
    """a stereo EncoderStream and DecoderStream pushed 1, 31, 32, 33, 0, 63, 64, 65, 200 and 4097 frames: the units equal
    a one-shot encode and the oracle; the exact PCM the oracle's, the binary32 PCM a whole-batch binary32 decode's; the
    empty push returns nothing and changes nothing"""
    import carta1_amd as c1
    e = env
    ctx = c1.Context(0)
    ctx.set_speculation(mode)
    total = sum(PUSHES)
    chans = [e['host'][c][:total * 512] for c in range(2)]
    try:
        for label, o in OPTSETS:
            opts = enc_options(o)
            want = e['want'][label, 2][:total * 2]
            assert np.array_equal(ctx.encode(chans, opts), want), label
            s = c1.EncoderStream(ctx, 2, opts)
            parts, pos = [], 0
            for n in PUSHES:
                u = s.push([c[pos * 512:(pos + n) * 512] for c in chans])
                assert u.shape == (n * 2, 212)
                parts.append(u)
                pos += n
            s.close()
            got = np.concatenate(parts)
            assert np.array_equal(got, want), (label, mode, np.flatnonzero((got != want).any(axis=1))[:4])
        units = want                                         # the last option set's
        ref, _ = O.decode_stream(units, 2)
        ctx.set_decode_precision(True)
        whole32 = ctx.decode(units, 2)
        for binary32 in (False, True):
            ctx.set_decode_precision(binary32)
            d = c1.DecoderStream(ctx, 2)
            outs, pos = [], 0
            for n in PUSHES:
                p = d.push(units[pos * 2:(pos + n) * 2])
                assert all(x.size == n * 512 for x in p)
                outs.append(p)
                pos += n
            d.close()
            for c in range(2):
                pcm = np.concatenate([p[c] for p in outs])
                want_pcm = whole32[c] if binary32 else ref[c]
                assert np.array_equal(pcm.view(np.uint32), want_pcm.view(np.uint32)), (binary32, c)
    finally:
        ctx.set_decode_precision(False)
        ctx.close()


# ---- forced runs: one fresh process per value of C1_RUN_FRAMES (read once per process) -------------------------

FORCED_RUNS = (4, 5, 7, 16, 17, 33, 63, 64)
CHILD_FRAMES = 2000


def _child_material():
    return [_patchwork(CHILD_FRAMES, 301), _patchwork(CHILD_FRAMES, 302)]


def child_main():
    """encode the fixed stereo patchwork in every option set and mode, decode mode 0's units exactly and in binary32;
    print the digests as one JSON line"""
    import carta1_amd as c1
    chans = _child_material()
    ctx = c1.Context(0)
    out = {}
    for label, o in OPTSETS:
        opts = enc_options(o)
        for m in (0, 1, 2):
            ctx.set_speculation(m)
            units = ctx.encode(chans, opts)
            out['%s/units/%d' % (label, m)] = digest(units)
        ctx.set_decode_precision(False)
        out['%s/pcm' % label] = digest(*ctx.decode(units, 2))
        ctx.set_decode_precision(True)
        out['%s/pcm32' % label] = digest(*ctx.decode(units, 2))
        ctx.set_decode_precision(False)
    ctx.close()
    print(json.dumps(out))


def _run_child(forced):
    env = {k: v for k, v in os.environ.items() if not k.startswith('C1_')}
    if forced is not None:
        env['C1_RUN_FRAMES'] = str(forced)
    cmd = [sys.executable] + (['-s'] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), 'child']
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, ('C1_RUN_FRAMES=%s' % forced, r.returncode, r.stderr[-3000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_forced_run_lengths():
    """C1_RUN_FRAMES = 4, 5, 7, 16, 17, 33, 63, 64, one fresh process each, one after the other (the sweep stops at the
    first failing one): units and exact PCM equal the oracle's, binary32 PCM equals a process without the variable"""
    chans = _child_material()
    want = {}
    with ThreadPoolExecutor(POOL) as pool:
        futs = {label: pool.submit(lambda o=o: O.encode_stream(chans, **oracle_kw(o))[0]) for label, o in OPTSETS}
        for label, _ in OPTSETS:
            u = futs[label].result()
            want['%s/units' % label] = digest(u)
            want['%s/pcm' % label] = digest(*O.decode_stream(u, 2)[0])
    plain = _run_child(None)
    for forced in (None,) + FORCED_RUNS:
        got = plain if forced is None else _run_child(forced)
        for label, _ in OPTSETS:
            for m in (0, 1, 2):
                assert got['%s/units/%d' % (label, m)] == want['%s/units' % label], (forced, label, m)
            assert got['%s/pcm' % label] == want['%s/pcm' % label], (forced, label)
            assert got['%s/pcm32' % label] == plain['%s/pcm32' % label], (forced, label)


if __name__ == '__main__' and sys.argv[1:] == ['child']:
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [os.path.dirname(here), here]
    child_main()
