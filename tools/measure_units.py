"""The meter of given sound units (c1_measure_units_device): its kernel's time against the measuring kernel of
c1_encode_best_modes_device, and every encoder of the library on one scale.  python tools/measure_units.py [--frames N] [--reps N]
[--skip-scoreboard] [--out FILE]

Kernel time.  2^20 stereo frames (2^21 units) of the mixed corpus of BASELINE configs[3], device-resident.  The units are those of
c1_encode_modes_device under a constant byte 0 (all long), and under a schedule over the whole domain in runs of 1 to 9 frames.
  M  c1_measure_units_device, totals only, no tables: "meter" of c1_ctx_kernel_ms
  C  c1_encode_best_modes_device, measure only (units NULL), one candidate (byte 0), distortion and energy: "choose".  That
     kernel quantizes by the trial allocation and makes the same two sums over the same coefficients
  M4 the meter with all four outputs under the packaged tables
2 warm-up rounds, then `reps` rounds alternating the variants in one process; median (min - max) in ms.
Scoreboard.  2^20 stereo frames of white noise (seeds 1 and 2) and of the mixed corpus; the units of c1_encode_device at bias
0.5, 1 and 2, of c1_encode_best_bias_device (the eight packaged biases), c1_encode_best_modes_device (the eight bytes of the
domain) and c1_encode_measured_device, _sf_ (offsets 0, -1, 1, -2, -3) and _masked_ (those offsets, the packaged tables), all
under transient detection; each measured flat and under the packaged tables: 10 log10(sum totals[:, 1] / sum totals[:, 0])."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import carta1_amd as c1

BIASES = (1, 0.5, 2, 0.25, 1.5, 3.3, 0, 5)            # the packaged biases, as tools/measure_measured.py
DOMAIN = [a | b << 2 | c << 4 for a in (0, 2) for b in (0, 2) for c in (0, 3)]
SIGNALS = {'white': c1.SIGNAL_WHITE, 'mixed': c1.SIGNAL_MIXED}


def schedule(frames, nch, seed=20261019):
    rng = np.random.RandomState(seed)
    m = np.zeros((frames, nch), dtype=np.uint8)
    for c in range(nch):
        runs = rng.randint(1, 10, size=frames)
        bytes_ = np.asarray(DOMAIN, dtype=np.uint8)[rng.randint(0, 8, size=frames)]
        m[:, c] = np.repeat(bytes_, runs)[:frames]
    return m


def generate(ctx, signal, frames):
    pcm = [torch.zeros(frames * 512, dtype=torch.float32, device='cuda:0') for _ in range(2)]
    for c in range(2):
        ctx.generate_device(SIGNALS[signal], 1 + c, frames, pcm[c].data_ptr())
    return pcm


def stat(v):
    return {'median_ms': float(np.median(v)), 'min_ms': float(min(v)), 'max_ms': float(max(v)), 'calls': len(v)}


def kernel_time(ctx, frames, reps, warmup, modes_name):
    n = frames * 2
    pcm = generate(ctx, 'mixed', frames)
    ptrs = [p.data_ptr() for p in pcm]
    host_modes = schedule(frames, 2) if modes_name == 'schedule' else np.zeros((frames, 2), dtype=np.uint8)
    modes = torch.from_numpy(host_modes.reshape(-1).copy()).to('cuda:0')
    units = torch.zeros(n * 212, dtype=torch.uint8, device='cuda:0')
    ctx.encode_modes_device(ptrs, frames, modes.data_ptr(), units.data_ptr())
    out = {k: torch.zeros(n * w, dtype=torch.float64, device='cuda:0') for k, w in (('noise', 52), ('signal', 52), ('totals', 2), ('weights', 52))}
    dist = torch.zeros(n, dtype=torch.float64, device='cuda:0')
    energy = torch.zeros(n, dtype=torch.float64, device='cuda:0')
    ctx.synchronize()

    def meter():
        ctx.measure_units_device(ptrs, frames, units.data_ptr(), totals_ptr=out['totals'].data_ptr())
        return ctx.kernel_ms('meter')[0]

    def meter4():
        ctx.measure_units_device(ptrs, frames, units.data_ptr(), out['noise'].data_ptr(), out['signal'].data_ptr(), out['totals'].data_ptr(),
                                 out['weights'].data_ptr(), masking=True)
        return ctx.kernel_ms('meter')[0]

    def choose():
        ctx.encode_best_modes_device(ptrs, frames, [0], distortion_ptr=dist.data_ptr(), energy_ptr=energy.data_ptr())
        return ctx.kernel_ms('choose')[0]

    variants = [('M', meter), ('C', choose), ('M4', meter4)]
    ctx.set_profiling(True)
    for _ in range(warmup):
        for _, fn in variants:
            fn()
    ms = {name: [] for name, _ in variants}
    for rep in range(reps):
        for name, fn in (variants if rep % 2 == 0 else variants[::-1]):
            ms[name].append(fn())
    meter()
    analysis = ctx.kernel_ms('analysis')[0]
    ctx.set_profiling(False)
    row = {'modes': modes_name, 'frames': frames, 'units': n, 'analysis_ms_of_M': analysis}
    row.update({name: stat(v) for name, v in ms.items()})
    row['M_over_C'] = row['M']['median_ms'] / row['C']['median_ms']
    row['M_bytes_per_s'] = n * (2048 + 212 + 16) / row['M']['median_ms'] * 1e3
    if modes_name == 'all long':                                 # the same sums by both kernels, within rounding
        t = out['totals'].view(n, 2)
        ctx.measure_units_device(ptrs, frames, units.data_ptr(), totals_ptr=out['totals'].data_ptr())
        ctx.synchronize()
        row['max_rel_difference_to_choose'] = float(max(((t[:, 0] - dist).abs() / dist.clamp_min(1e-300)).max().item(),
                                                        ((t[:, 1] - energy).abs() / energy.clamp_min(1e-300)).max().item()))
    fmt = lambda k: '%s %.3f (%.3f - %.3f)' % (k, row[k]['median_ms'], row[k]['min_ms'], row[k]['max_ms'])
    print('kernel time, mixed, %s, %d units: ' % (modes_name, n) + '  '.join(fmt(k) for k in ('M', 'C', 'M4')) +
          '  M/C %.2f  analysis %.3f ms  M moves %.0f GB/s' % (row['M_over_C'], analysis, row['M_bytes_per_s'] / 1e9))
    return row


def scoreboard(ctx, signal, frames):
    n = frames * 2
    pcm = generate(ctx, signal, frames)
    ptrs = [p.data_ptr() for p in pcm]
    units = torch.zeros(n * 212, dtype=torch.uint8, device='cuda:0')
    totals = torch.zeros(n * 2, dtype=torch.float64, device='cuda:0')
    palette = [c1.EncoderOptions({'allocationBias': b}) for b in BIASES]
    rows = [('c1_encode_device, bias 0.5', lambda: ctx.encode_device(ptrs, frames, units.data_ptr(), c1.EncoderOptions({'allocationBias': 0.5}))),
            ('c1_encode_device, bias 1', lambda: ctx.encode_device(ptrs, frames, units.data_ptr(), c1.EncoderOptions())),
            ('c1_encode_device, bias 2', lambda: ctx.encode_device(ptrs, frames, units.data_ptr(), c1.EncoderOptions({'allocationBias': 2.0}))),
            ('c1_encode_best_bias_device', lambda: ctx.encode_best_bias_device(ptrs, frames, palette, units.data_ptr())),
            ('c1_encode_best_modes_device', lambda: ctx.encode_best_modes_device(ptrs, frames, DOMAIN, units.data_ptr())),
            ('c1_encode_measured_device', lambda: ctx.encode_measured_device(ptrs, frames, units.data_ptr())),
            ('c1_encode_measured_sf_device', lambda: ctx.encode_measured_device(ptrs, frames, units.data_ptr(), scale_factor_offsets=c1.SCALE_FACTOR_OFFSETS)),
            ('c1_encode_measured_masked_device', lambda: ctx.encode_measured_device(ptrs, frames, units.data_ptr(), scale_factor_offsets=c1.SCALE_FACTOR_OFFSETS,
                                                                                    masking=True))]
    out = []
    for name, encode in rows:
        units.zero_()
        encode()
        db = {}
        for tables, masking in (('flat', None), ('packaged', True)):
            ctx.measure_units_device(ptrs, frames, units.data_ptr(), totals_ptr=totals.data_ptr(), masking=masking)
            ctx.synchronize()
            t = totals.view(n, 2)
            db[tables] = float(10 * torch.log10(t[:, 1].sum() / t[:, 0].sum()).item())
        print('%s  %-34s flat %.2f dB  packaged tables %.2f dB' % (signal, name, db['flat'], db['packaged']))
        out.append({'signal': signal, 'units_of': name, 'frames': frames, 'db': db})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=1 << 20)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--skip-scoreboard', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    ctx = c1.Context(0)
    result = {'kernel_time': [], 'scoreboard': []}
    try:
        for modes_name in ('all long', 'schedule'):
            result['kernel_time'].append(kernel_time(ctx, a.frames, a.reps, a.warmup, modes_name))
        if not a.skip_scoreboard:
            for signal in ('white', 'mixed'):
                result['scoreboard'] += scoreboard(ctx, signal, a.frames)
    finally:
        ctx.close()
    print(json.dumps(result))
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(result, f, indent=1)


if __name__ == '__main__':
    main()
