"""The meter of given sound units under the all-long threshold (c1_measure_units_shared_device): its kernel's time against
c1_measure_units_device's, every encoder of the library on the shared scale, and the gain DESIGN.md 6v quotes, from the device's
own totals.  python tools/measure_units_shared.py [--frames N] [--reps N] [--skip-scoreboard] [--out FILE]

Kernel time.  2^20 stereo frames (2^21 units) of the mixed corpus of BASELINE configs[3], device-resident.  The units are those of
c1_encode_modes_device under a constant byte 0 (all long), and under tools/measure_units.py's schedule over the whole domain.
  M4 c1_measure_units_device with all four outputs under the packaged tables: "meter" of c1_ctx_kernel_ms
  S4 c1_measure_units_shared_device with the same outputs and tables: "meter"
and "analysis" of both.  2 warm-up rounds, then `reps` rounds alternating the variants in one process; median (min - max) in ms.
Scoreboard.  tools/measure_units.py's rows and the two block-mode searches by the measured allocation (the eight bytes of the
domain, the five offsets; plain and under the packaged tables), all under transient detection; each measured flat, under the
packaged tables with the unit's own-mode threshold and under them with the all-long threshold: 10 log10(sum totals[:, 1] / sum
totals[:, 0]).
The claim of 6v.  On the pink material of the tests (130 stereo frames), the eight candidates, offset 0 and the five offsets: how
far the search's units lie below the masked allocation's under the detector's modes, sum totals[:, 0] of this call for both."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import numpy as np
import torch
import carta1_amd as c1
import measure_units as MU

DOMAIN = MU.DOMAIN
OUTPUTS = (('noise', 52), ('signal', 52), ('totals', 2), ('weights', 52))


def kernel_time(ctx, frames, reps, warmup, modes_name):
    n = frames * 2
    pcm = MU.generate(ctx, 'mixed', frames)
    ptrs = [p.data_ptr() for p in pcm]
    host_modes = MU.schedule(frames, 2) if modes_name == 'schedule' else np.zeros((frames, 2), dtype=np.uint8)
    modes = torch.from_numpy(host_modes.reshape(-1).copy()).to('cuda:0')
    units = torch.zeros(n * 212, dtype=torch.uint8, device='cuda:0')
    ctx.encode_modes_device(ptrs, frames, modes.data_ptr(), units.data_ptr())
    out = {k: torch.zeros(n * w, dtype=torch.float64, device='cuda:0') for k, w in OUTPUTS}
    ctx.synchronize()

    def run(threshold):
        ctx.measure_units_device(ptrs, frames, units.data_ptr(), out['noise'].data_ptr(), out['signal'].data_ptr(), out['totals'].data_ptr(),
                                 out['weights'].data_ptr(), masking=True, threshold_from=threshold)
        return ctx.kernel_ms('meter')[0], ctx.kernel_ms('analysis')[0]

    variants = [('M4', 'own'), ('S4', 'long')]
    ctx.set_profiling(True)
    for _ in range(warmup):
        for _, threshold in variants:
            run(threshold)
    ms = {name: [] for name, _ in variants}
    ana = {name: [] for name, _ in variants}
    for rep in range(reps):
        for name, threshold in (variants if rep % 2 == 0 else variants[::-1]):
            m, a = run(threshold)
            ms[name].append(m)
            ana[name].append(a)
    ctx.set_profiling(False)
    row = {'modes': modes_name, 'frames': frames, 'units': n}
    row.update({name: MU.stat(v) for name, v in ms.items()})
    row.update({name + '_analysis': MU.stat(v) for name, v in ana.items()})
    row['S4_over_M4'] = row['S4']['median_ms'] / row['M4']['median_ms']
    row['bar'] = 5572.0 / 3524.0
    fmt = lambda k: '%s %.3f (%.3f - %.3f)' % (k, row[k]['median_ms'], row[k]['min_ms'], row[k]['max_ms'])
    print('kernel time, mixed, %s, %d units: ' % (modes_name, n) + '  '.join(fmt(k) for k in ('M4', 'S4')) +
          '  S4/M4 %.3f (bar %.2f)  analysis %.3f and %.3f ms' % (row['S4_over_M4'], row['bar'], row['M4_analysis']['median_ms'],
                                                                   row['S4_analysis']['median_ms']))
    return row


def score(ctx, ptrs, frames, units, totals):
    """the three columns of one row -> dict of dB, and the sums of totals[:, 0] under the all-long threshold"""
    n = frames * 2
    db = {}
    for column, masking, threshold in (('flat', None, 'own'), ('packaged, own', True, 'own'), ('packaged, long', True, 'long')):
        ctx.measure_units_device(ptrs, frames, units.data_ptr(), totals_ptr=totals.data_ptr(), masking=masking, threshold_from=threshold)
        ctx.synchronize()
        t = totals.view(n, 2)
        db[column] = float(10 * torch.log10(t[:, 1].sum() / t[:, 0].sum()).item())
    return db, float(t[:, 0].sum().item())


def scoreboard(ctx, signal, frames):
    n = frames * 2
    pcm = MU.generate(ctx, signal, frames)
    ptrs = [p.data_ptr() for p in pcm]
    units = torch.zeros(n * 212, dtype=torch.uint8, device='cuda:0')
    totals = torch.zeros(n * 2, dtype=torch.float64, device='cuda:0')
    palette = [c1.EncoderOptions({'allocationBias': b}) for b in MU.BIASES]
    five = c1.SCALE_FACTOR_OFFSETS
    rows = [('c1_encode_device, bias 0.5', lambda: ctx.encode_device(ptrs, frames, units.data_ptr(), c1.EncoderOptions({'allocationBias': 0.5}))),
            ('c1_encode_device, bias 1', lambda: ctx.encode_device(ptrs, frames, units.data_ptr(), c1.EncoderOptions())),
            ('c1_encode_device, bias 2', lambda: ctx.encode_device(ptrs, frames, units.data_ptr(), c1.EncoderOptions({'allocationBias': 2.0}))),
            ('c1_encode_best_bias_device', lambda: ctx.encode_best_bias_device(ptrs, frames, palette, units.data_ptr())),
            ('c1_encode_best_modes_device', lambda: ctx.encode_best_modes_device(ptrs, frames, DOMAIN, units.data_ptr())),
            ('c1_encode_measured_device', lambda: ctx.encode_measured_device(ptrs, frames, units.data_ptr())),
            ('c1_encode_measured_sf_device', lambda: ctx.encode_measured_device(ptrs, frames, units.data_ptr(), scale_factor_offsets=five)),
            ('c1_encode_measured_masked_device', lambda: ctx.encode_measured_device(ptrs, frames, units.data_ptr(), scale_factor_offsets=five, masking=True)),
            ('c1_encode_measured_modes_device', lambda: ctx.encode_measured_modes_device(ptrs, frames, DOMAIN, units.data_ptr(), scale_factor_offsets=five)),
            ('c1_encode_measured_modes_masked_device', lambda: ctx.encode_measured_modes_device(ptrs, frames, DOMAIN, units.data_ptr(),
                                                                                                scale_factor_offsets=five, masking=True))]
    out = []
    for name, encode in rows:
        units.zero_()
        encode()
        db, _ = score(ctx, ptrs, frames, units, totals)
        print('%s  %-40s ' % (signal, name) + '  '.join('%s %.2f dB' % kv for kv in db.items()))
        out.append({'signal': signal, 'units_of': name, 'frames': frames, 'db': db})
    return out


def claim_of_6v(ctx):
    """the pink material of the tests, from the device's own totals"""
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import best_bias_lib as BB
    body = BB.material()[1]
    frames = len(body[0]) // 512
    n = frames * 2
    pcm = [torch.from_numpy(np.ascontiguousarray(c, dtype=np.float32)).to('cuda:0') for c in body]
    ptrs = [p.data_ptr() for p in pcm]
    units = torch.zeros(n * 212, dtype=torch.uint8, device='cuda:0')
    totals = torch.zeros(n * 2, dtype=torch.float64, device='cuda:0')
    out = []
    for name, offsets in (('offset 0', None), ('five offsets', c1.SCALE_FACTOR_OFFSETS)):
        ctx.encode_measured_device(ptrs, frames, units.data_ptr(), scale_factor_offsets=offsets, masking=True)
        base = score(ctx, ptrs, frames, units, totals)[1]
        ctx.encode_measured_modes_device(ptrs, frames, DOMAIN, units.data_ptr(), scale_factor_offsets=offsets, masking=True)
        ours = score(ctx, ptrs, frames, units, totals)[1]
        gain = float(10 * np.log10(base / ours))
        print('pink, %s: the masked search lies %.2f dB below the masked allocation under the detector\'s modes' % (name, gain))
        out.append({'offsets': name, 'gain_db': gain, 'detector_total': base, 'search_total': ours})
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
    result = {'kernel_time': [], 'scoreboard': [], 'claim_of_6v': []}
    try:
        for modes_name in ('all long', 'schedule'):
            result['kernel_time'].append(kernel_time(ctx, a.frames, a.reps, a.warmup, modes_name))
        result['claim_of_6v'] = claim_of_6v(ctx)
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
