"""Encode with given block modes against what the library offered before it: python tools/measure_modes.py [--frames N] [--reps N]

Input: pink noise with bursts (C1_SIGNAL_PINK_BURSTS, seeds 3 and 4), 2^20 stereo frames, device-resident; the modes are those
the exact detector chooses for it (c1_detect_scores_device).  Three ways to the same bytes:
  A  one c1_encode_modes_device call with those modes
  B  one c1_encode_device call under transient detection on the same context (the bytes are compared once, before timing)
  C  what a caller had to do before: per channel one stream, c1_enc_stream_set_options to the frame's fixed modes wherever
     they change and one c1_enc_stream_push per run of equal modes, over the first --loop-frames frames (host PCM, as the
     stream calls take it); A4k is variant A over the same frames, for the ratio
Every figure is the host clock around the calls and a synchronise of the context, after warm-up rounds; the variants alternate
inside each round of one process; medians with the range.  Then the kernel breakdown of A and B from c1_ctx_kernel_ms."""
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
    ap.add_argument('--loop-reps', type=int, default=3, help='rounds that also run the push-per-change loop')
    ap.add_argument('--warmup', type=int, default=2)
    a = ap.parse_args()
    frames, nch = a.frames, 2
    k = min(a.loop_frames, frames)
    ctx = c1.Context(0)
    pcm = [torch.zeros(frames * 512, dtype=torch.float32, device='cuda:0') for _ in range(nch)]
    for c in range(nch):
        ctx.generate_device(c1.SIGNAL_PINK_BURSTS, 3 + c, frames, pcm[c].data_ptr())
    ptrs = [p.data_ptr() for p in pcm]
    scores = torch.zeros(frames * nch * 6, dtype=torch.float64, device='cuda:0')
    modes = torch.zeros(frames * nch, dtype=torch.uint8, device='cuda:0')
    opened = torch.zeros(1, dtype=torch.int32, device='cuda:0')
    units_a = torch.zeros(frames * nch * 212, dtype=torch.uint8, device='cuda:0')
    units_b = torch.zeros_like(units_a)
    torch.cuda.synchronize()
    opts = c1.EncoderOptions({})
    ctx.detect_scores_device(ptrs, frames, scores.data_ptr(), modes.data_ptr(), opened.data_ptr(), opts, speculative=False)
    ctx.synchronize()
    del scores
    host_modes = modes.cpu().numpy().reshape(frames, nch)
    short = float(np.count_nonzero(host_modes)) / host_modes.size

    def enc_a():
        ctx.encode_modes_device(ptrs, frames, modes.data_ptr(), units_a.data_ptr(), opts)

    def enc_b():
        ctx.encode_device(ptrs, frames, units_b.data_ptr(), opts)

    def enc_a4k():
        ctx.encode_modes_device(ptrs, k, modes.data_ptr(), units_a.data_ptr(), opts)

    enc_a()
    enc_b()
    ctx.synchronize()
    if not torch.equal(units_a, units_b):
        raise SystemExit('A and B disagree: the modes path does not reproduce detection')

    # C: the first k frames from host memory, a mono stream per channel, one push per run of equal modes
    host_pcm = [p[:k * 512].cpu().numpy() for p in pcm]
    runs = []
    for c in range(nch):
        col = host_modes[:k, c]
        cuts = [0] + (np.flatnonzero(col[1:] != col[:-1]) + 1).tolist() + [k]
        runs.append([(x, y, c1.EncoderOptions({'fixedBlockModes': c1.unpack_block_modes(col[x])[0].tolist()})) for x, y in zip(cuts[:-1], cuts[1:])])
    loop_out = [None, None]

    def enc_c():
        for c in range(nch):
            s = c1.EncoderStream(ctx, 1, runs[c][0][2])
            try:
                parts = []
                for x, y, o in runs[c]:
                    s.set_options(o)
                    parts.append(s.push([host_pcm[c][x * 512:y * 512]]))
                loop_out[c] = np.concatenate(parts)
            finally:
                s.close()

    enc_c()
    enc_a4k()
    ctx.synchronize()
    head = units_a[:k * nch * 212].cpu().numpy().reshape(k, nch, 212)
    if not all(np.array_equal(head[:, c], loop_out[c]) for c in range(nch)):
        raise SystemExit('C disagrees with A over the first %d frames' % k)

    variants = [('A', enc_a), ('B', enc_b), ('A4k', enc_a4k), ('C', enc_c)]
    for _ in range(a.warmup):
        for name, fn in variants:
            if name != 'C':
                timed(ctx, fn)
    ms = {name: [] for name, _ in variants}
    for rep in range(a.reps):
        for name, fn in (variants if rep % 2 == 0 else [variants[1], variants[0]] + variants[2:]):
            if name == 'C' and rep >= a.loop_reps:
                continue
            ms[name].append(timed(ctx, fn))
    row = {'frames': frames, 'channels': nch, 'loop_frames': k, 'units_with_a_short_band': short,
           'pushes_in_C': sum(len(r) for r in runs), **{name: stats(v) for name, v in ms.items()}}
    row['A_over_B'] = row['A']['median_ms'] / row['B']['median_ms']
    row['C_over_A4k'] = row['C']['median_ms'] / row['A4k']['median_ms']
    ctx.set_profiling(True)
    enc_a()
    row['A_kernels_ms'] = {kind: ctx.kernel_ms(kind) for kind in KINDS}
    enc_b()
    row['B_kernels_ms'] = {kind: ctx.kernel_ms(kind) for kind in KINDS}
    ctx.set_profiling(False)
    print('%d stereo frames, %.2f %% of the units with a short band; C: %d pushes over %d frames' % (frames, 100 * short, row['pushes_in_C'], k))
    print('  '.join('%s %.3f ms (%.3f - %.3f, %d)' % (n, row[n]['median_ms'], row[n]['min_ms'], row[n]['max_ms'], row[n]['calls']) for n in ms)
          + '  A/B %.3f  C/A4k %.0f' % (row['A_over_B'], row['C_over_A4k']))
    print('A kernels: ' + ', '.join('%s %.3f ms x%d' % (n, v[0], v[1]) for n, v in row['A_kernels_ms'].items() if v[1])
          + ' | B: ' + ', '.join('%s %.3f ms x%d' % (n, v[0], v[1]) for n, v in row['B_kernels_ms'].items() if v[1]))
    print(json.dumps(row))
    ctx.close()


if __name__ == '__main__':
    main()
