"""The measured allocation with the scale-factor index of every BFU chosen by the same error against the measured allocation
there was before: python tools/measure_scale_factors.py [--frames N] [--reps N] [--modes BYTE|random] [--offsets 0,-1,1,-2,-3]

Input: 2^20 stereo frames, device-resident, of (white) BASELINE configs[1]'s white noise, seeds 1 and 2, and (mixed) the mixed
corpus of configs[3].  The block modes are given: one constant byte (default 0, all long), or a schedule over the whole domain
in runs of 1 to 9 frames per channel (tools/measure_measured.py's).
  S  one c1_encode_measured_sf_device call with the offsets (default: the suggested five), all five outputs
  Z  the same call with the one offset 0
  P  one c1_encode_measured_device call: the measured allocation at findScaleFactor's indices
The bytes are checked once, before timing: every output of Z is P's bit for bit and its shifts are zero; S's T_ref is P's bit
for bit, T(n*) < T_ref exactly where taken is 1, shifts are zero in every unit not taken, and S's units are the plain encode's
(c1_encode_modes_device) wherever taken is 0 and differ wherever it is 1.  Reported with them: the share of units taken, the
aggregate gain of S's T_final against T_ref and against P's T_final, the share of units whose T(n*) exceeds P's, and the
histogram of the offsets written for coded BFUs.  Every figure is the host clock around the call and a synchronise of the context,
after warm-up rounds; the variants alternate inside each round of one process; medians with the range.  Then the kernel
breakdown of the three from c1_ctx_kernel_ms, in calls of their own: S's "measure" less Z's is the extra table passes."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch
import carta1_amd as c1
from measure_measured import schedule, timed, stats

KINDS = ('analysis', 'allocate', 'measure', 'pack', 'redo', 'total')
AMOUNTS = (20, 28, 32, 36, 40, 44, 48, 52)


def coded_mask(units, units_n):
    """bool [units_n, 52]: BFU b of the unit is below its nBfu and has a word length above 0, from the bytes"""
    u = units.view(units_n, 212)
    nbfu = torch.tensor(AMOUNTS, device=u.device)[(u[:, 1] >> 5).long()]
    wl = torch.stack([(u[:, 2 + b // 2] >> (4 if b % 2 == 0 else 0)) & 15 for b in range(52)], dim=1)
    return (torch.arange(52, device=u.device)[None, :] < nbfu[:, None]) & (wl > 0)


def measure(ctx, signal, frames, reps, warmup, modes_arg, offsets):
    nch = 2
    units_n = frames * nch
    pcm = [torch.zeros(frames * 512, dtype=torch.float32, device='cuda:0') for _ in range(nch)]
    for c in range(nch):
        ctx.generate_device({'white': c1.SIGNAL_WHITE, 'mixed': c1.SIGNAL_MIXED}[signal], 1 + c, frames, pcm[c].data_ptr())
    ptrs = [p.data_ptr() for p in pcm]
    host_modes = schedule(frames, nch) if modes_arg == 'random' else np.full((frames, nch), int(modes_arg, 0), dtype=np.uint8)
    modes = torch.from_numpy(host_modes.reshape(-1).copy()).to('cuda:0')
    new = lambda dtype, n: torch.zeros(n, dtype=dtype, device='cuda:0')
    out = {v: {'units': new(torch.uint8, units_n * 212), 'taken': new(torch.uint8, units_n), 'shifts': new(torch.int8, units_n * 52),
               'dist': new(torch.float64, units_n * 2), 'energy': new(torch.float64, units_n)} for v in 'SZP'}
    plain = new(torch.uint8, units_n * 212)
    torch.cuda.synchronize()

    def call(v, offs):
        o = out[v]
        return lambda: ctx.encode_measured_device(ptrs, frames, o['units'].data_ptr(), o['taken'].data_ptr(), o['dist'].data_ptr(),
                                                  o['energy'].data_ptr(), modes_ptr=modes.data_ptr(), scale_factor_offsets=offs,
                                                  shifts_ptr=o['shifts'].data_ptr() if offs is not None else None)
    variants = [('S', call('S', offsets)), ('Z', call('Z', (0,))), ('P', call('P', None))]
    row = {'signal': signal, 'frames': frames, 'channels': nch, 'modes': modes_arg, 'offsets': list(offsets)}
    for _, fn in variants:                                   # the bytes, before any timing
        fn()
    ctx.encode_modes_device(ptrs, frames, modes.data_ptr(), plain.data_ptr())
    ctx.synchronize()
    S, Z, P = out['S'], out['Z'], out['P']
    for k in ('units', 'taken', 'dist', 'energy'):
        if not torch.equal(Z[k].view(torch.uint8), P[k].view(torch.uint8)):
            raise SystemExit('%s: %s of the call with the one offset 0 is not c1_encode_measured_device\'s' % (signal, k))
    if Z['shifts'].any():
        raise SystemExit('%s: shifts of the call with the one offset 0 are not zero' % signal)
    d, dp = S['dist'].view(units_n, 2), P['dist'].view(units_n, 2)
    took = S['taken'] != 0
    if not torch.equal(d[:, 0].view(torch.int64), dp[:, 0].view(torch.int64)):
        raise SystemExit('%s: T_ref differs from c1_encode_measured_device\'s' % signal)
    if not torch.equal(d[:, 1] < d[:, 0], took):
        raise SystemExit('%s: taken is not T(n*) < T_ref' % signal)
    differ = (S['units'].view(units_n, 212) != plain.view(units_n, 212)).any(dim=1)
    if not torch.equal(differ, took):
        raise SystemExit('%s: S differs from c1_encode_modes_device in other units than the taken ones' % signal)
    shifts = S['shifts'].view(units_n, 52)
    if shifts[~took].any():
        raise SystemExit('%s: a unit not taken has shifts' % signal)
    final = torch.where(took, d[:, 1], d[:, 0])
    final_p = torch.where(P['taken'] != 0, dp[:, 1], dp[:, 0])
    row['taken_share'] = float(took.double().mean().item())
    row['taken_share_P'] = float((P['taken'] != 0).double().mean().item())
    row['gain_db_against_T_ref'] = float(10 * torch.log10(d[:, 0].sum() / final.sum()).item())
    row['gain_db_P_against_T_ref'] = float(10 * torch.log10(d[:, 0].sum() / final_p.sum()).item())
    row['gain_db_against_P'] = float(10 * torch.log10(final_p.sum() / final.sum()).item())
    row['share_worse_than_P'] = float((final > final_p).double().mean().item())
    row['snr_db_S'] = float(10 * torch.log10(S['energy'].sum() / final.sum()).item())
    written = shifts[coded_mask(S['units'], units_n) & took[:, None]]
    row['offsets_written_share'] = {str(int(v)): float((written == int(v)).double().mean().item()) for v in offsets}
    for _ in range(warmup):
        for _, fn in variants:
            timed(ctx, fn)
    ms = {name: [] for name, _ in variants}
    for rep in range(reps):
        for name, fn in (variants if rep % 2 == 0 else variants[::-1]):
            ms[name].append(timed(ctx, fn))
    row.update({name: stats(v, frames) for name, v in ms.items()})
    row['S_over_P'] = row['S']['median_ms'] / row['P']['median_ms']
    ctx.set_profiling(True)
    for name, fn in variants:
        per = {kind: [] for kind in KINDS}
        for _ in range(3):
            fn()
            for kind in KINDS:
                per[kind].append(ctx.kernel_ms(kind))
        row[name + '_kernels_ms'] = {kind: [float(np.median([v[0] for v in per[kind]])), per[kind][0][1]] for kind in KINDS}
    ctx.set_profiling(False)
    row['extra_table_passes_ms'] = row['S_kernels_ms']['measure'][0] - row['Z_kernels_ms']['measure'][0]
    print('%s: %d stereo frames, modes %s, offsets %s' % (signal, frames, modes_arg, list(offsets)))
    fmt = lambda k: '%s %.3f ms (%.3f - %.3f, %d; %.2f M frames/s)' % (k, row[k]['median_ms'], row[k]['min_ms'], row[k]['max_ms'], row[k]['calls'], row[k]['frames_per_s'] / 1e6)
    print('  ' + '  '.join(fmt(k) for k in 'SZP') + '  S/P %.2f' % row['S_over_P'])
    for name in 'SZP':
        print('  %s kernels: ' % name + ', '.join('%s %.3f ms x%d' % (k, v[0], v[1]) for k, v in row[name + '_kernels_ms'].items() if v[1]))
    print('  measure: S - Z = %.1f ms for the extra table passes' % row['extra_table_passes_ms'])
    print('  taken %.1f %% of the units (P: %.1f %%); error energy of S: %.2f dB under T_ref (P: %.2f dB), %.2f dB under P; S codes at %.2f dB; '
          'T_final above P\'s in %.3f %% of the units' % (100 * row['taken_share'], 100 * row['taken_share_P'], row['gain_db_against_T_ref'],
                                                        row['gain_db_P_against_T_ref'], row['gain_db_against_P'], row['snr_db_S'],
                                                        100 * row['share_worse_than_P']))
    print('  offsets written for coded BFUs: ' + ', '.join('%s: %.1f %%' % (k, 100 * v) for k, v in row['offsets_written_share'].items()))
    print(json.dumps(row))
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=1 << 20)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--signals', default='white,mixed')
    ap.add_argument('--modes', default='0')
    ap.add_argument('--offsets', default=','.join(str(v) for v in c1.SCALE_FACTOR_OFFSETS))
    a = ap.parse_args()
    offsets = tuple(int(v) for v in a.offsets.split(','))
    ctx = c1.Context(0)
    try:
        for signal in a.signals.split(','):
            measure(ctx, signal, a.frames, a.reps, a.warmup, a.modes, offsets)
    finally:
        ctx.close()


if __name__ == '__main__':
    main()
