"""The block modes chosen by the error of the measured allocation (c1_encode_measured_modes_device) against the loop over the
existing calls that it replaces: python tools/measure_measured_modes.py [--frames N] [--reps N] [--warmup N] [--signals white,mixed]
[--counts 2,8] [--small 128,4096] [--skip-scoreboard] [--out FILE]

Input: 2^20 stereo frames, device-resident, of (white) BASELINE configs[1]'s white noise, seeds 1 and 2, and (mixed) the mixed
corpus of configs[3].  Candidates: the first n of 58, 0, 10, 50, 2, 8, 48, 56; plain (offsets 0) and with the suggested offsets.
  An  one c1_encode_measured_modes_device call, all seven outputs
  Hn  the loop it replaces: n measure-only c1_encode_measured_sf_device calls under constant modes (distortion and energy), then
      one c1_encode_measured_sf_device call with units, taken and shifts under An's modes_out
The bytes are checked once, before timing: column k of An's distortion and energy is call k's bit for bit, the choice is the
first least T_final of those columns, modes_out = cand[choice], and units, taken and shifts are the final call's.  Every figure is
the host clock around the call(s) and a synchronise of the context, after warm-up rounds; An and Hn alternate inside each round of
one process; medians with the range.  Then the kernel breakdown of both from c1_ctx_kernel_ms, in calls of their own.
--small: the same pair at a few stereo frames (the loop's calls then take the workgroup-per-unit kernel).
Scoreboard: DESIGN.md 6m's and 6n's row for the new call with all eight candidates, plain and with the offsets -- the
coefficient-domain figure of c1_measure_units_device and the PCM-domain figure of c1_measure_pcm_device without the first two
frames, 10 log10(sum totals[:, 1] / sum totals[:, 0]) -- and the share of units per winning candidate."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch
import carta1_amd as c1
from measure_measured import timed, stats

CANDIDATES = (58, 0, 10, 50, 2, 8, 48, 56)
KINDS = ('analysis', 'allocate', 'choose', 'measure', 'pack', 'total')
SKIP = 2


def generate(ctx, signal, frames):
    pcm = [torch.zeros(frames * 512, dtype=torch.float32, device='cuda:0') for _ in range(2)]
    for c in range(2):
        ctx.generate_device({'white': c1.SIGNAL_WHITE, 'mixed': c1.SIGNAL_MIXED}[signal], 1 + c, frames, pcm[c].data_ptr())
    return pcm


def buffers(units_n, n):
    new = lambda dtype, count: torch.zeros(count, dtype=dtype, device='cuda:0')
    return {'units': new(torch.uint8, units_n * 212), 'choice': new(torch.uint8, units_n), 'modes': new(torch.uint8, units_n),
            'taken': new(torch.uint8, units_n), 'shifts': new(torch.int8, units_n * 52), 'dist': new(torch.float64, units_n * n * 2),
            'energy': new(torch.float64, units_n * n)}


def pair(ctx, ptrs, frames, cand, offsets):
    """-> (A, H, run_a, run_h): the new call's outputs, the loop's, and the two as functions"""
    units_n, n = frames * 2, len(cand)
    A = buffers(units_n, n)
    H = {'units': torch.zeros_like(A['units']), 'taken': torch.zeros_like(A['taken']), 'shifts': torch.zeros_like(A['shifts']),
         'dist': [torch.zeros(units_n * 2, dtype=torch.float64, device='cuda:0') for _ in cand],
         'energy': [torch.zeros(units_n, dtype=torch.float64, device='cuda:0') for _ in cand]}
    const = [torch.full((units_n,), b, dtype=torch.uint8, device='cuda:0') for b in cand]

    def run_a():
        ctx.encode_measured_modes_device(ptrs, frames, cand, A['units'].data_ptr(), A['choice'].data_ptr(), A['modes'].data_ptr(),
                                         A['taken'].data_ptr(), A['shifts'].data_ptr(), A['dist'].data_ptr(), A['energy'].data_ptr(),
                                         scale_factor_offsets=offsets)

    def run_h():
        for k in range(n):
            ctx.encode_measured_device(ptrs, frames, None, None, H['dist'][k].data_ptr(), H['energy'][k].data_ptr(), modes_ptr=const[k].data_ptr(),
                                       scale_factor_offsets=offsets)
        ctx.encode_measured_device(ptrs, frames, H['units'].data_ptr(), H['taken'].data_ptr(), modes_ptr=A['modes'].data_ptr(),
                                   scale_factor_offsets=offsets, shifts_ptr=H['shifts'].data_ptr())
    return A, H, run_a, run_h


def check_bytes(ctx, A, H, run_a, run_h, cand, units_n, what):
    n = len(cand)
    run_a()
    ctx.synchronize()
    run_h()
    ctx.synchronize()
    d, e = A['dist'].view(units_n, n, 2), A['energy'].view(units_n, n)
    for k in range(n):
        if not torch.equal(d[:, k].contiguous().view(torch.int64), H['dist'][k].view(units_n, 2).view(torch.int64)):
            raise SystemExit('%s: distortion of candidate %d is not the measure-only call\'s' % (what, k))
        if not torch.equal(e[:, k].contiguous().view(torch.int64), H['energy'][k].view(torch.int64)):
            raise SystemExit('%s: energy of candidate %d is not the measure-only call\'s' % (what, k))
    final = torch.where(d[:, :, 1] < d[:, :, 0], d[:, :, 1], d[:, :, 0])
    least = final.min(dim=1, keepdim=True).values
    first = (final == least).to(torch.uint8).argmax(dim=1)
    if not torch.equal(first.to(torch.uint8), A['choice']):
        raise SystemExit('%s: choice is not the first least T_final' % what)
    if not torch.equal(torch.tensor(cand, dtype=torch.uint8, device='cuda:0')[A['choice'].long()], A['modes']):
        raise SystemExit('%s: modes_out is not cand[choice]' % what)
    for k in ('units', 'taken', 'shifts'):
        if not torch.equal(A[k], H[k]):
            raise SystemExit('%s: %s is not the call\'s under the chosen modes' % (what, k))
    return final


def measure(ctx, signal, frames, n, offsets, reps, warmup, pcm=None):
    pcm = pcm or generate(ctx, signal, frames)
    ptrs = [p.data_ptr() for p in pcm]
    cand, units_n = list(CANDIDATES[:n]), frames * 2
    what = '%s, %d frames, n = %d, offsets %s' % (signal, frames, n, list(offsets))
    A, H, run_a, run_h = pair(ctx, ptrs, frames, cand, offsets)
    final = check_bytes(ctx, A, H, run_a, run_h, cand, units_n, what)
    row = {'signal': signal, 'frames': frames, 'n_cand': n, 'candidates': cand, 'offsets': list(offsets)}
    row['winner_share'] = [float((A['choice'] == k).double().mean().item()) for k in range(n)]
    row['taken_share'] = float((A['taken'] != 0).double().mean().item())
    row['snr_db'] = float(10 * torch.log10(A['energy'].view(units_n, n)[:, 0].sum() / final.min(dim=1).values.sum()).item())
    variants = [('A', run_a), ('H', run_h)]
    for _ in range(warmup):
        for _, fn in variants:
            timed(ctx, fn)
    ms = {name: [] for name, _ in variants}
    for rep in range(reps):
        for name, fn in (variants if rep % 2 == 0 else variants[::-1]):
            ms[name].append(timed(ctx, fn))
    row.update({name: stats(v, frames) for name, v in ms.items()})
    row['A_over_H'] = row['A']['median_ms'] / row['H']['median_ms']
    ctx.set_profiling(True)
    run_a()
    row['A_kernels_ms'] = {kind: list(ctx.kernel_ms(kind)) for kind in KINDS}
    per = {kind: [0.0, 0] for kind in KINDS}
    const = [torch.full((units_n,), b, dtype=torch.uint8, device='cuda:0') for b in cand]
    for k in range(n + 1):                                  # the loop's calls one by one: the timings are kept per call
        if k < n:
            ctx.encode_measured_device(ptrs, frames, None, None, H['dist'][k].data_ptr(), H['energy'][k].data_ptr(), modes_ptr=const[k].data_ptr(),
                                       scale_factor_offsets=offsets)
        else:
            ctx.encode_measured_device(ptrs, frames, H['units'].data_ptr(), H['taken'].data_ptr(), modes_ptr=A['modes'].data_ptr(),
                                       scale_factor_offsets=offsets, shifts_ptr=H['shifts'].data_ptr())
        for kind in KINDS:
            t, c = ctx.kernel_ms(kind)
            per[kind][0] += t
            per[kind][1] += c
    row['H_kernels_ms'] = per
    ctx.set_profiling(False)
    fmt = lambda k: '%s %.2f ms (%.2f - %.2f, %d)' % (k, row[k]['median_ms'], row[k]['min_ms'], row[k]['max_ms'], row[k]['calls'])
    print(what)
    print('  ' + '  '.join(fmt(k) for k in 'AH') + '  A/H %.3f' % row['A_over_H'])
    for name in 'AH':
        print('  %s kernels: ' % name + ', '.join('%s %.2f ms x%d' % (k, v[0], v[1]) for k, v in row[name + '_kernels_ms'].items() if v[1]))
    print('  winners ' + ', '.join('%d: %.1f %%' % (cand[k], 100 * s) for k, s in enumerate(row['winner_share'])) +
          '; taken %.1f %%; codes at %.2f dB' % (100 * row['taken_share'], row['snr_db']))
    print(json.dumps(row), flush=True)
    return row


def snr_db(totals, n, skip):
    t = totals.view(n, 2)[skip * 2:]
    return float(10 * torch.log10(t[:, 1].sum() / t[:, 0].sum()).item())


def scoreboard(ctx, signal, frames, pcm=None):
    pcm = pcm or generate(ctx, signal, frames)
    ptrs = [p.data_ptr() for p in pcm]
    n = frames * 2
    units = torch.zeros(n * 212, dtype=torch.uint8, device='cuda:0')
    choice = torch.zeros(n, dtype=torch.uint8, device='cuda:0')
    totals = torch.zeros(n * 2, dtype=torch.float64, device='cuda:0')
    out = []
    for name, offsets in (('c1_encode_measured_modes_device, offsets 0', (0,)),
                          ('c1_encode_measured_modes_device, offsets 0, -1, 1, -2, -3', c1.SCALE_FACTOR_OFFSETS)):
        ctx.encode_measured_modes_device(ptrs, frames, list(CANDIDATES), units.data_ptr(), choice.data_ptr(), scale_factor_offsets=offsets)
        ctx.measure_units_device(ptrs, frames, units.data_ptr(), totals_ptr=totals.data_ptr())
        ctx.synchronize()
        db = {'coefficients': snr_db(totals, n, 0)}
        ctx.measure_pcm_device(ptrs, frames, units.data_ptr(), totals_ptr=totals.data_ptr())
        ctx.synchronize()
        db['pcm_skip2'] = snr_db(totals, n, SKIP)
        share = [float((choice == k).double().mean().item()) for k in range(len(CANDIDATES))]
        print('%s  %-58s coefficients %.2f dB  PCM %.2f dB  winners %s' % (signal, name, db['coefficients'], db['pcm_skip2'],
              ', '.join('%d: %.1f %%' % (b, 100 * s) for b, s in zip(CANDIDATES, share))), flush=True)
        out.append({'signal': signal, 'units_of': name, 'frames': frames, 'db': db, 'winner_share': share})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=1 << 20)
    ap.add_argument('--reps', type=int, default=4)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--signals', default='white,mixed')
    ap.add_argument('--counts', default='2,8')
    ap.add_argument('--small', default='128,4096')
    ap.add_argument('--skip-scoreboard', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    ctx = c1.Context(0)
    rows = []
    try:
        for signal in a.signals.split(','):
            pcm = generate(ctx, signal, a.frames)
            for offsets in ((0,), c1.SCALE_FACTOR_OFFSETS):
                for n in [int(v) for v in a.counts.split(',') if v]:
                    rows.append(measure(ctx, signal, a.frames, n, offsets, a.reps, a.warmup, pcm))
            for frames in [int(v) for v in a.small.split(',') if v]:
                rows.append(measure(ctx, signal, frames, 8, c1.SCALE_FACTOR_OFFSETS, max(a.reps, 10), a.warmup))
            if not a.skip_scoreboard:
                rows += scoreboard(ctx, signal, a.frames, pcm)
    finally:
        ctx.close()
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(rows, f)


if __name__ == '__main__':
    main()
