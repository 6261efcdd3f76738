"""The block modes chosen per unit by least coding error against what a caller had to do before: python
tools/measure_best_modes.py [--frames N] [--reps N]

Input: 2^20 stereo frames, device-resident, of (white) BASELINE configs[1]'s white noise, seeds 1 and 2, and (mixed) the mixed
corpus of configs[3].  The candidates are the first 1, 2 or 8 of the mode bytes 58, 0, 10, 50, 2, 8, 48, 56, allocationBias 1.
  A1 / A2 / A8  one c1_encode_best_modes_device call with 1, 2 and 8 candidates, all five outputs
  H1 / H2 / H8  the loop An replaces, from the entry points there were before and without its host work: n measure-only
                c1_encode_best_bias_device calls with one entry and the candidate as constant modes, then one
                c1_encode_modes_device call (the minimum over the n unweighted reports is host work that is not counted,
                and is not comparable across modes: the loop is the cost of the attempt, not a replacement of its result)
  B             one c1_encode_modes_device call under the modes A8 chose
The bytes are compared once, before timing: An's units with c1_encode_modes_device fed An's modes.  Every figure is the host
clock around the calls and a synchronise of the context, after warm-up rounds; the variants alternate inside each round of one
process; medians with the range.  Then the kernel breakdown of the A variants and of B from c1_ctx_kernel_ms, in calls of their
own."""
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
CANDIDATES = (58, 0, 10, 50, 2, 8, 48, 56)
SIZES = (1, 2, 8)


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
    one = [c1.EncoderOptions()]
    units_a = torch.zeros(units_n * 212, dtype=torch.uint8, device='cuda:0')
    units_b = torch.zeros_like(units_a)
    choice = torch.zeros(units_n, dtype=torch.uint8, device='cuda:0')
    modes = {n: torch.zeros(units_n, dtype=torch.uint8, device='cuda:0') for n in SIZES}
    scratch_modes = torch.zeros(units_n, dtype=torch.uint8, device='cuda:0')
    dist = torch.zeros(units_n * 8, dtype=torch.float64, device='cuda:0')
    energy = torch.zeros(units_n * 8, dtype=torch.float64, device='cuda:0')
    const = {b: torch.full((units_n,), b, dtype=torch.uint8, device='cuda:0') for b in CANDIDATES}
    torch.cuda.synchronize()

    def enc_a(n, out_modes=None):
        m = (out_modes if out_modes is not None else scratch_modes).data_ptr()
        return lambda: ctx.encode_best_modes_device(ptrs, frames, CANDIDATES[:n], units_a.data_ptr(), choice.data_ptr(), m, dist.data_ptr(),
                                                    energy.data_ptr())

    def enc_b(n):
        return lambda: ctx.encode_modes_device(ptrs, frames, modes[n].data_ptr(), units_b.data_ptr())

    def enc_h(n):
        last = enc_b(n)

        def run():
            for b in CANDIDATES[:n]:
                ctx.encode_best_bias_device(ptrs, frames, one, None, None, dist.data_ptr(), None, modes_ptr=const[b].data_ptr())
            last()
        return run

    row = {'signal': signal, 'frames': frames, 'channels': nch}
    for n in SIZES:                                          # the bytes, before any timing
        enc_a(n, modes[n])()
        enc_b(n)()
        ctx.synchronize()
        if not torch.equal(units_a, units_b):
            raise SystemExit('%s: A%d and c1_encode_modes_device under its modes disagree' % (signal, n))
        row['A%d_wins' % n] = {str(b): int((modes[n] == b).sum().item()) for b in CANDIDATES[:n]}
    variants = [(kind + str(n), fn(n)) for n in SIZES for kind, fn in (('A', enc_a), ('H', enc_h))] + [('B', enc_b(8))]
    for _ in range(warmup):
        for _, fn in variants:
            timed(ctx, fn)
    ms = {name: [] for name, _ in variants}
    for rep in range(reps):
        for name, fn in (variants if rep % 2 == 0 else variants[::-1]):
            ms[name].append(timed(ctx, fn))
    row.update({name: stats(v, frames) for name, v in ms.items()})
    for n in SIZES:
        row['A%d_over_B' % n] = row['A%d' % n]['median_ms'] / row['B']['median_ms']
        row['H%d_over_A%d' % (n, n)] = row['H%d' % n]['median_ms'] / row['A%d' % n]['median_ms']
    ctx.set_profiling(True)
    for name, fn in [v for v in variants if v[0][0] in 'AB']:
        per = {kind: [] for kind in KINDS}
        for _ in range(3):
            fn()
            for kind in KINDS:
                per[kind].append(ctx.kernel_ms(kind))
        row[name + '_kernels_ms'] = {kind: [float(np.median([v[0] for v in per[kind]])), per[kind][0][1]] for kind in KINDS}
    ctx.set_profiling(False)
    print('%s: %d stereo frames' % (signal, frames))
    fmt = lambda k: '%s %.3f ms (%.3f - %.3f, %d; %.1f M frames/s)' % (k, row[k]['median_ms'], row[k]['min_ms'], row[k]['max_ms'], row[k]['calls'], row[k]['frames_per_s'] / 1e6)
    print('  ' + fmt('B'))
    for n in SIZES:
        print('  ' + '  '.join(fmt(k) for k in ('A%d' % n, 'H%d' % n)) + '  A/B %.3f  H/A %.3f' % (row['A%d_over_B' % n], row['H%d_over_A%d' % (n, n)]))
    for name in ('A1', 'A2', 'A8', 'B'):
        print('  %s kernels: ' % name + ', '.join('%s %.3f ms x%d' % (k, v[0], v[1]) for k, v in row[name + '_kernels_ms'].items() if v[1]))
    print('  candidates chosen (A8): %s' % row['A8_wins'])
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
