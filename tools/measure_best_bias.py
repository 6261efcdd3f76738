"""The bias chosen per unit by least coding error against what a caller had to do before: python tools/measure_best_bias.py
[--frames N] [--reps N]

Input: 2^20 stereo frames, device-resident, of (white) BASELINE configs[1]'s white noise, seeds 1 and 2, and (mixed) the mixed
corpus of configs[3], both under fixedBlockModes [0,0,0].  The palette is the first 1, 4 or 8 of the packaged biases 1, 0.5, 2,
0.25, 1.5, 3.3, 0, 5.
  A1 / A4 / A8  one c1_encode_best_bias_device call with 1, 4 and 8 entries, all four outputs
  B1 / B4 / B8  one c1_encode_biases_device call with the same palette and a fixed index (the choice An returned): the path there
                was before, and the last step of the loop below
  H1 / H4 / H8  the loop An replaces, without its host work: n c1_encode_device calls, one per entry, then Bn
The bytes are compared once, before timing: An's units with Bn's.  Every figure is the host clock around the calls and a
synchronise of the context, after warm-up rounds; the variants alternate inside each round of one process; medians with the
range.  Then the kernel breakdown of the A variants and of B8 from c1_ctx_kernel_ms, in calls of their own."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import carta1_amd as c1

KINDS = ('analysis', 'allocate', 'choose', 'pack', 'redo', 'total')
BIASES = (1, 0.5, 2, 0.25, 1.5, 3.3, 0, 5)
SIZES = (1, 4, 8)


def timed(ctx, fn):
    ctx.synchronize()
    t0 = time.perf_counter()
    fn()
    ctx.synchronize()
    return (time.perf_counter() - t0) * 1e3


def stats(ms, frames):
    med = float(np.median(ms))
    return {'median_ms': med, 'min_ms': float(min(ms)), 'max_ms': float(max(ms)), 'calls': len(ms), 'frames_per_s': frames / med * 1e3}


def measure(ctx, signal, frames, reps, warmup):
    nch = 2
    units_n = frames * nch
    pcm = [torch.zeros(frames * 512, dtype=torch.float32, device='cuda:0') for _ in range(nch)]
    for c in range(nch):
        ctx.generate_device({'white': c1.SIGNAL_WHITE, 'mixed': c1.SIGNAL_MIXED}[signal], 1 + c, frames, pcm[c].data_ptr())
    ptrs = [p.data_ptr() for p in pcm]
    palette = [c1.EncoderOptions({'allocationBias': b, 'fixedBlockModes': [0, 0, 0]}) for b in BIASES]
    units_a = torch.zeros(units_n * 212, dtype=torch.uint8, device='cuda:0')
    units_b = torch.zeros_like(units_a)
    choice = {n: torch.zeros(units_n, dtype=torch.uint8, device='cuda:0') for n in SIZES}
    dist = torch.zeros(units_n * 8, dtype=torch.float64, device='cuda:0')
    energy = torch.zeros(units_n, dtype=torch.float64, device='cuda:0')
    scratch_choice = torch.zeros(units_n, dtype=torch.uint8, device='cuda:0')
    torch.cuda.synchronize()

    def enc_a(n, out_choice=None):
        ch = (out_choice if out_choice is not None else scratch_choice).data_ptr()
        return lambda: ctx.encode_best_bias_device(ptrs, frames, palette[:n], units_a.data_ptr(), ch, dist.data_ptr(), energy.data_ptr())

    def enc_b(n):
        return lambda: ctx.encode_biases_device(ptrs, frames, palette[:n], choice[n].data_ptr(), units_b.data_ptr())

    def enc_h(n):
        last = enc_b(n)

        def run():
            for k in range(n):
                ctx.encode_device(ptrs, frames, units_b.data_ptr(), palette[k])
            last()
        return run

    row = {'signal': signal, 'frames': frames, 'channels': nch}
    for n in SIZES:                                          # the bytes, before any timing
        enc_a(n, choice[n])()
        enc_b(n)()
        ctx.synchronize()
        if not torch.equal(units_a, units_b):
            raise SystemExit('%s: A%d and B%d disagree' % (signal, n, n))
        row['A%d_wins' % n] = torch.bincount(choice[n].to(torch.int64), minlength=n).cpu().tolist()
    variants = [(kind + str(n), fn(n)) for n in SIZES for kind, fn in (('A', enc_a), ('B', enc_b), ('H', enc_h))]
    for _ in range(warmup):
        for _, fn in variants:
            timed(ctx, fn)
    ms = {name: [] for name, _ in variants}
    for rep in range(reps):
        for name, fn in (variants if rep % 2 == 0 else variants[::-1]):
            ms[name].append(timed(ctx, fn))
    row.update({name: stats(v, frames) for name, v in ms.items()})
    for n in SIZES:
        row['A%d_over_B%d' % (n, n)] = row['A%d' % n]['median_ms'] / row['B%d' % n]['median_ms']
        row['H%d_over_A%d' % (n, n)] = row['H%d' % n]['median_ms'] / row['A%d' % n]['median_ms']
    ctx.set_profiling(True)
    for name, fn in [v for v in variants if v[0][0] == 'A'] + [('B8', enc_b(8))]:
        per = {kind: [] for kind in KINDS}
        for _ in range(3):
            fn()
            for kind in KINDS:
                per[kind].append(ctx.kernel_ms(kind))
        row[name + '_kernels_ms'] = {kind: [float(np.median([v[0] for v in per[kind]])), per[kind][0][1]] for kind in KINDS}
    ctx.set_profiling(False)
    print('%s: %d stereo frames' % (signal, frames))
    for n in SIZES:
        print('  ' + '  '.join('%s %.3f ms (%.3f - %.3f, %d; %.1f M frames/s)' % (k, row[k]['median_ms'], row[k]['min_ms'], row[k]['max_ms'], row[k]['calls'], row[k]['frames_per_s'] / 1e6)
                               for k in ('A%d' % n, 'B%d' % n, 'H%d' % n)) + '  A/B %.3f  H/A %.3f' % (row['A%d_over_B%d' % (n, n)], row['H%d_over_A%d' % (n, n)]))
    for name in ('A1', 'A4', 'A8', 'B8'):
        print('  %s kernels: ' % name + ', '.join('%s %.3f ms x%d' % (k, v[0], v[1]) for k, v in row[name + '_kernels_ms'].items() if v[1]))
    print('  entries chosen (A8): %s' % row['A8_wins'])
    print(json.dumps(row))
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=1 << 20)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--signals', default='white,mixed')
    a = ap.parse_args()
    ctx = c1.Context(0)
    try:
        for signal in a.signals.split(','):
            measure(ctx, signal, a.frames, a.reps, a.warmup)
    finally:
        ctx.close()


if __name__ == '__main__':
    main()
