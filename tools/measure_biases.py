"""Encode with a bias palette against what the library offered before it: python tools/measure_biases.py [--frames N] [--reps N]

Input: pink noise with bursts (C1_SIGNAL_PINK_BURSTS, seeds 3 and 4), 2^20 stereo frames, device-resident; the modes are those
the exact detector chooses for it (c1_detect_scores_device) and are given to every variant.  The palette is the first 1, 4 or 8
of the packaged biases 1, 0.5, 2, 0.25, 1.5, 3.3, 0, 5; the index is uniformly random per unit.
  A1 / A4 / A8  one c1_encode_biases_device call with 1, 4 and 8 entries
  B             one c1_encode_modes_device call under entry 0 on the same context: the path before, and the bytes of A1
  C             what a caller had to do before: per channel one stream, c1_enc_stream_set_options to the unit's bias wherever it
                changes and one c1_enc_stream_push_modes per run of equal bias, over the first --loop-frames frames of A8's
                schedule (host PCM, as the stream calls take it); A8_4k is variant A8 over the same frames, for the ratio
The bytes are compared once, before timing: A1 with B, and A4 / A8 with the per-unit selection among constant-bias calls of B's
kind.  Every figure is the host clock around the calls and a synchronise of the context, after warm-up rounds; the variants
alternate inside each round of one process; medians with the range.  Then the kernel breakdown of the A variants and B from
c1_ctx_kernel_ms."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import carta1_amd as c1

KINDS = ('analysis', 'allocate', 'pack', 'redo', 'total')
BIASES = (1, 0.5, 2, 0.25, 1.5, 3.3, 0, 5)


def timed(ctx, fn):
    ctx.synchronize()
    t0 = time.perf_counter()
    fn()
    ctx.synchronize()
    return (time.perf_counter() - t0) * 1e3


def stats(ms):
    return {'median_ms': float(np.median(ms)), 'min_ms': float(min(ms)), 'max_ms': float(max(ms)), 'calls': len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=1 << 20)
    ap.add_argument('--loop-frames', type=int, default=4096)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--loop-reps', type=int, default=2, help='rounds that also run the push-per-change loop')
    ap.add_argument('--warmup', type=int, default=2)
    a = ap.parse_args()
    frames, nch = a.frames, 2
    units_n = frames * nch
    k = min(a.loop_frames, frames)
    ctx = c1.Context(0)
    pcm = [torch.zeros(frames * 512, dtype=torch.float32, device='cuda:0') for _ in range(nch)]
    for c in range(nch):
        ctx.generate_device(c1.SIGNAL_PINK_BURSTS, 3 + c, frames, pcm[c].data_ptr())
    ptrs = [p.data_ptr() for p in pcm]
    scores = torch.zeros(units_n * 6, dtype=torch.float64, device='cuda:0')
    modes = torch.zeros(units_n, dtype=torch.uint8, device='cuda:0')
    opened = torch.zeros(1, dtype=torch.int32, device='cuda:0')
    units_a = torch.zeros(units_n * 212, dtype=torch.uint8, device='cuda:0')
    units_b = torch.zeros_like(units_a)
    torch.cuda.synchronize()
    ctx.detect_scores_device(ptrs, frames, scores.data_ptr(), modes.data_ptr(), opened.data_ptr(), c1.EncoderOptions({}), speculative=False)
    ctx.synchronize()
    del scores
    palette = [c1.EncoderOptions({'allocationBias': b}) for b in BIASES]
    rng = np.random.RandomState(20261018)
    index = {n: torch.from_numpy(rng.randint(0, n, size=units_n).astype(np.uint8)).cuda() for n in (1, 4, 8)}

    def enc_a(n, count=frames):
        return lambda: ctx.encode_biases_device(ptrs, count, palette[:n], index[n].data_ptr(), units_a.data_ptr(), modes.data_ptr())

    def enc_b(entry=0):
        return lambda: ctx.encode_modes_device(ptrs, frames, modes.data_ptr(), units_b.data_ptr(), palette[entry])

    # the bytes, before any timing
    enc_a(1)()
    enc_b()()
    ctx.synchronize()
    if not torch.equal(units_a, units_b):
        raise SystemExit('A1 and B disagree')
    want = torch.zeros_like(units_a).view(units_n, 212)
    for entry in range(8):
        enc_b(entry)()
        ctx.synchronize()
        sel = index[8] == entry
        want[sel] = units_b.view(units_n, 212)[sel]
    enc_a(8)()
    ctx.synchronize()
    if not torch.equal(units_a.view(units_n, 212), want):
        raise SystemExit('A8 disagrees with the per-unit selection among constant-bias encodes')
    for entry in range(4):
        enc_b(entry)()
        ctx.synchronize()
        sel = index[4] == entry
        want[sel] = units_b.view(units_n, 212)[sel]
    enc_a(4)()
    ctx.synchronize()
    if not torch.equal(units_a.view(units_n, 212), want):
        raise SystemExit('A4 disagrees with the per-unit selection among constant-bias encodes')
    del want

    # C: the first k frames from host memory, a mono stream per channel, one modes push per run of equal bias
    host_pcm = [p[:k * 512].cpu().numpy() for p in pcm]
    host_modes = modes.cpu().numpy().reshape(frames, nch)[:k]
    host_index = index[8].cpu().numpy().reshape(frames, nch)[:k]
    runs = []
    for c in range(nch):
        col = host_index[:, c]
        cuts = [0] + (np.flatnonzero(col[1:] != col[:-1]) + 1).tolist() + [k]
        runs.append([(x, y, palette[int(col[x])]) for x, y in zip(cuts[:-1], cuts[1:])])
    loop_out = [None, None]

    def enc_c():
        for c in range(nch):
            s = c1.EncoderStream(ctx, 1, runs[c][0][2])
            try:
                parts = []
                for x, y, o in runs[c]:
                    s.set_options(o)
                    parts.append(s.push([host_pcm[c][x * 512:y * 512]], modes=host_modes[x:y, c]))
                loop_out[c] = np.concatenate(parts)
            finally:
                s.close()

    enc_c()
    enc_a(8, k)()
    ctx.synchronize()
    head = units_a[:k * nch * 212].cpu().numpy().reshape(k, nch, 212)
    if not all(np.array_equal(head[:, c], loop_out[c]) for c in range(nch)):
        raise SystemExit('C disagrees with A8 over the first %d frames' % k)

    variants = [('A1', enc_a(1)), ('B', enc_b()), ('A4', enc_a(4)), ('A8', enc_a(8)), ('A8_4k', enc_a(8, k)), ('C', enc_c)]
    for _ in range(a.warmup):
        for name, fn in variants:
            if name != 'C':
                timed(ctx, fn)
    ms = {name: [] for name, _ in variants}
    for rep in range(a.reps):
        for name, fn in (variants if rep % 2 == 0 else [variants[1], variants[0], variants[3], variants[2]] + variants[4:]):
            if name == 'C' and rep >= a.loop_reps:
                continue
            ms[name].append(timed(ctx, fn))
    row = {'frames': frames, 'channels': nch, 'loop_frames': k, 'pushes_in_C': sum(len(r) for r in runs), **{name: stats(v) for name, v in ms.items()}}
    row['A1_over_B'] = row['A1']['median_ms'] / row['B']['median_ms']
    row['A4_over_A1'] = row['A4']['median_ms'] / row['A1']['median_ms']
    row['A8_over_A1'] = row['A8']['median_ms'] / row['A1']['median_ms']
    row['C_over_A8_4k'] = row['C']['median_ms'] / row['A8_4k']['median_ms']
    ctx.set_profiling(True)
    for name, fn in variants[:4]:
        fn()
        row[name + '_kernels_ms'] = {kind: ctx.kernel_ms(kind) for kind in KINDS}
    ctx.set_profiling(False)
    print('%d stereo frames; C: %d pushes over %d frames' % (frames, row['pushes_in_C'], k))
    print('  '.join('%s %.3f ms (%.3f - %.3f, %d)' % (n, row[n]['median_ms'], row[n]['min_ms'], row[n]['max_ms'], row[n]['calls']) for n in ms))
    print('A1/B %.3f  A4/A1 %.3f  A8/A1 %.3f  C/A8_4k %.0f' % (row['A1_over_B'], row['A4_over_A1'], row['A8_over_A1'], row['C_over_A8_4k']))
    for name, _ in variants[:4]:
        print('%s kernels: ' % name + ', '.join('%s %.3f ms x%d' % (n, v[0], v[1]) for n, v in row[name + '_kernels_ms'].items() if v[1]))
    print(json.dumps(row))
    ctx.close()


if __name__ == '__main__':
    main()
