"""The word lengths allocated by the measured coding error against the encodes there were before: python
tools/measure_measured.py [--frames N] [--reps N] [--modes BYTE|random]

Input: 2^20 stereo frames, device-resident, of (white) BASELINE configs[1]'s white noise, seeds 1 and 2, and (mixed) the mixed
corpus of configs[3].  The block modes are given: one constant byte (default 0, all long), or a schedule over the whole domain
in runs of 1 to 9 frames per channel (seed 20261019).
  A  one c1_encode_measured_device call, all four outputs
  B  one c1_encode_modes_device call under the same modes: the open-loop encode
  C  one c1_encode_best_bias_device call with the eight packaged biases under the same modes: the best closed loop before
The bytes are checked once, before timing: A's units are B's wherever taken is 0 and differ wherever it is 1, T(n*) < T_ref
exactly where taken is 1.  Reported with them: the share of units taken and the aggregate gain of T_final against T_ref and,
under all-long modes, against C's least D (c1_encode_best_bias_device's D is not weighted: only then are the sums comparable).  Every figure is the host clock around the call
and a synchronise of the context, after warm-up rounds; the variants alternate inside each round of one process; medians with
the range.  Then the kernel breakdown of the three from c1_ctx_kernel_ms, in calls of their own.  C's "choose" is eight passes of
the quantizer and dequantizer over a unit, the table phase of A's "measure" fifteen: choose / 8 * 15 estimates the table
phase, the rest of "measure" is the greedy phase."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import carta1_amd as c1

KINDS = ('analysis', 'allocate', 'measure', 'choose', 'pack', 'redo', 'total')
BIASES = (1, 0.5, 2, 0.25, 1.5, 3.3, 0, 5)            # the packaged biases, as tools/measure_best_bias.py
DOMAIN = [a | b << 2 | c << 4 for a in (0, 2) for b in (0, 2) for c in (0, 3)]


def schedule(frames, nch, seed=20261019):
    rng = np.random.RandomState(seed)
    m = np.zeros((frames, nch), dtype=np.uint8)
    for c in range(nch):
        runs = rng.randint(1, 10, size=frames)
        bytes_ = np.asarray(DOMAIN, dtype=np.uint8)[rng.randint(0, 8, size=frames)]
        m[:, c] = np.repeat(bytes_, runs)[:frames]
    return m


def timed(ctx, fn):
    ctx.synchronize()
    t0 = time.perf_counter()
    fn()
    ctx.synchronize()
    return (time.perf_counter() - t0) * 1e3


def stats(ms, frames):
    med = float(np.median(ms))
    return {'median_ms': med, 'min_ms': float(min(ms)), 'max_ms': float(max(ms)), 'calls': len(ms), 'frames_per_s': frames / med * 1e3}


def measure(ctx, signal, frames, reps, warmup, modes_arg):
    nch = 2
    units_n = frames * nch
    pcm = [torch.zeros(frames * 512, dtype=torch.float32, device='cuda:0') for _ in range(nch)]
    for c in range(nch):
        ctx.generate_device({'white': c1.SIGNAL_WHITE, 'mixed': c1.SIGNAL_MIXED}[signal], 1 + c, frames, pcm[c].data_ptr())
    ptrs = [p.data_ptr() for p in pcm]
    host_modes = schedule(frames, nch) if modes_arg == 'random' else np.full((frames, nch), int(modes_arg, 0), dtype=np.uint8)
    modes = torch.from_numpy(host_modes.reshape(-1).copy()).to('cuda:0')
    palette = [c1.EncoderOptions({'allocationBias': b}) for b in BIASES]
    units_a = torch.zeros(units_n * 212, dtype=torch.uint8, device='cuda:0')
    units_b = torch.zeros_like(units_a)
    units_c = torch.zeros_like(units_a)
    taken = torch.zeros(units_n, dtype=torch.uint8, device='cuda:0')
    choice = torch.zeros(units_n, dtype=torch.uint8, device='cuda:0')
    dist = torch.zeros(units_n * 2, dtype=torch.float64, device='cuda:0')
    energy = torch.zeros(units_n, dtype=torch.float64, device='cuda:0')
    dist_c = torch.zeros(units_n * 8, dtype=torch.float64, device='cuda:0')
    energy_c = torch.zeros(units_n, dtype=torch.float64, device='cuda:0')
    torch.cuda.synchronize()

    enc_a = lambda: ctx.encode_measured_device(ptrs, frames, units_a.data_ptr(), taken.data_ptr(), dist.data_ptr(), energy.data_ptr(),
                                               modes_ptr=modes.data_ptr())
    enc_b = lambda: ctx.encode_modes_device(ptrs, frames, modes.data_ptr(), units_b.data_ptr())
    enc_c = lambda: ctx.encode_best_bias_device(ptrs, frames, palette, units_c.data_ptr(), choice.data_ptr(), dist_c.data_ptr(),
                                                energy_c.data_ptr(), modes_ptr=modes.data_ptr())
    row = {'signal': signal, 'frames': frames, 'channels': nch, 'modes': modes_arg}
    for fn in (enc_a, enc_b, enc_c):                         # the bytes, before any timing
        fn()
    ctx.synchronize()
    differ = (units_a.view(units_n, 212) != units_b.view(units_n, 212)).any(dim=1)
    d = dist.view(units_n, 2)
    if not torch.equal(differ, taken != 0):
        raise SystemExit('%s: A differs from c1_encode_modes_device in other units than the taken ones' % signal)
    if not torch.equal(d[:, 1] < d[:, 0], taken != 0):
        raise SystemExit('%s: taken is not T(n*) < T_ref' % signal)
    final = torch.where(taken != 0, d[:, 1], d[:, 0])
    best_c = dist_c.view(units_n, 8).min(dim=1).values
    row['taken_share'] = float((taken != 0).double().mean().item())
    row['gain_db_against_B'] = float(10 * torch.log10(d[:, 0].sum() / final.sum()).item())
    comparable = not host_modes.any()
    row['gain_db_against_C'] = float(10 * torch.log10(best_c.sum() / final.sum()).item()) if comparable else None
    row['gain_db_C_against_B'] = float(10 * torch.log10(d[:, 0].sum() / best_c.sum()).item()) if comparable else None
    row['snr_db_A'] = float(10 * torch.log10(energy.sum() / final.sum()).item())
    variants = [('A', enc_a), ('B', enc_b), ('C', enc_c)]
    for _ in range(warmup):
        for _, fn in variants:
            timed(ctx, fn)
    ms = {name: [] for name, _ in variants}
    for rep in range(reps):
        for name, fn in (variants if rep % 2 == 0 else variants[::-1]):
            ms[name].append(timed(ctx, fn))
    row.update({name: stats(v, frames) for name, v in ms.items()})
    row['A_over_B'] = row['A']['median_ms'] / row['B']['median_ms']
    row['A_over_C'] = row['A']['median_ms'] / row['C']['median_ms']
    ctx.set_profiling(True)
    for name, fn in variants:
        per = {kind: [] for kind in KINDS}
        for _ in range(3):
            fn()
            for kind in KINDS:
                per[kind].append(ctx.kernel_ms(kind))
        row[name + '_kernels_ms'] = {kind: [float(np.median([v[0] for v in per[kind]])), per[kind][0][1]] for kind in KINDS}
    ctx.set_profiling(False)
    table = row['C_kernels_ms']['choose'][0] / 8 * 15
    row['table_phase_estimate_ms'] = table
    row['greedy_phase_estimate_ms'] = row['A_kernels_ms']['measure'][0] - table
    print('%s: %d stereo frames, modes %s' % (signal, frames, modes_arg))
    fmt = lambda k: '%s %.3f ms (%.3f - %.3f, %d; %.1f M frames/s)' % (k, row[k]['median_ms'], row[k]['min_ms'], row[k]['max_ms'], row[k]['calls'], row[k]['frames_per_s'] / 1e6)
    print('  ' + '  '.join(fmt(k) for k in 'ABC') + '  A/B %.2f  A/C %.2f' % (row['A_over_B'], row['A_over_C']))
    for name in 'ABC':
        print('  %s kernels: ' % name + ', '.join('%s %.3f ms x%d' % (k, v[0], v[1]) for k, v in row[name + '_kernels_ms'].items() if v[1]))
    print('  measure: table phase about %.1f ms (choose / 8 * 15), greedy phase about %.1f ms' % (table, row['greedy_phase_estimate_ms']))
    print('  taken %.1f %% of the units; error energy of A: %.2f dB under B; A codes at %.2f dB' % (100 * row['taken_share'], row['gain_db_against_B'], row['snr_db_A']))
    if comparable:
        print('  error energy of A: %.2f dB under C (C: %.2f dB under B)' % (row['gain_db_against_C'], row['gain_db_C_against_B']))
    print(json.dumps(row))
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=1 << 20)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--signals', default='white,mixed')
    ap.add_argument('--modes', default='0')
    a = ap.parse_args()
    ctx = c1.Context(0)
    try:
        for signal in a.signals.split(','):
            measure(ctx, signal, a.frames, a.reps, a.warmup, a.modes)
    finally:
        ctx.close()


if __name__ == '__main__':
    main()
