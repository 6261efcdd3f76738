"""The measured allocation under a masking threshold against the measured allocation with chosen scale factors, which it leaves
unchanged: python tools/measure_masked.py [--frames N] [--reps N] [--modes BYTE|random] [--offsets 0,-1,1,-2,-3] [--judge N]

Input: 2^20 stereo frames, device-resident, of (white) BASELINE configs[1]'s white noise, seeds 1 and 2, and (mixed) the mixed
corpus of configs[3].  The block modes are given: one constant byte (default 0, all long), or a schedule over the whole domain
in runs of 1 to 9 frames per channel (tools/measure_measured.py's).
  M  one c1_encode_measured_masked_device call with the packaged tables and the offsets (default: the suggested five), all six
     outputs
  F  the same call with flat tables (floor 1.0, no spread)
  S  one c1_encode_measured_sf_device call with the same offsets: the path there was before, which this work does not touch
The bytes are checked once, before timing: units, taken, shifts, distortion and energy of F are S's bit for bit and its weights
are 1.0; in M, T(n*) < T_ref exactly where taken is 1, shifts are zero in every unit not taken, and the units are the plain
encode's (c1_encode_modes_device) wherever taken is 0 and differ wherever it is 1.  Reported with them: the share of units taken,
the share of BFUs whose threshold is the floor, the aggregate gain of M's weighted T_final against its T_ref, and -- on the first
--judge frames of the call, on the CPU from the bytes (tests/masked_alloc_lib.py; the encoder is causal) -- the weighted error of
S's units against that of M's units, both judged with M's weights.  Every time is the host clock around the call and a
synchronise of the context, after warm-up rounds; the variants alternate inside each round of one process; medians with the
range.  Then the kernel breakdown of the three from c1_ctx_kernel_ms, in calls of their own."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch
import carta1_amd as c1
from measure_measured import schedule, timed, stats

KINDS = ('analysis', 'allocate', 'measure', 'pack', 'redo', 'total')
FLAT = (np.ones(52), None)


def judge(pcm, host_modes, plain, S_units, M_units, M_weights, n):
    """the first n frames on the CPU: (weighted error of S's units, of M's units) under M's weights, from the bytes"""
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import best_bias_lib as BB
    import masked_alloc_lib as MK
    chans = [p[:n * 512].cpu().numpy() for p in pcm]
    u = 2 * n
    coefs = BB.coefficients(chans, plain.view(-1, 212)[:u].cpu().numpy())
    P = M_weights.view(-1, 52)[:u].cpu().numpy()
    return (float(MK.weighted_errors(S_units.view(-1, 212)[:u].cpu().numpy(), coefs, P).sum()),
            float(MK.weighted_errors(M_units.view(-1, 212)[:u].cpu().numpy(), coefs, P).sum()))


def measure(ctx, signal, frames, reps, warmup, modes_arg, offsets, judge_frames):
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
               'dist': new(torch.float64, units_n * 2), 'energy': new(torch.float64, units_n)} for v in 'MFS'}
    for v in 'MF':
        out[v]['weights'] = new(torch.float64, units_n * 52)
    plain = new(torch.uint8, units_n * 212)
    torch.cuda.synchronize()

    def call(v, masking):
        o = out[v]
        return lambda: ctx.encode_measured_device(ptrs, frames, o['units'].data_ptr(), o['taken'].data_ptr(), o['dist'].data_ptr(),
                                                  o['energy'].data_ptr(), modes_ptr=modes.data_ptr(), scale_factor_offsets=offsets,
                                                  shifts_ptr=o['shifts'].data_ptr(), masking=masking,
                                                  weights_ptr=o['weights'].data_ptr() if masking is not None else None)
    variants = [('M', call('M', True)), ('F', call('F', FLAT)), ('S', call('S', None))]
    row = {'signal': signal, 'frames': frames, 'channels': nch, 'modes': modes_arg, 'offsets': list(offsets)}
    for _, fn in variants:                                   # the bytes, before any timing
        fn()
    ctx.encode_modes_device(ptrs, frames, modes.data_ptr(), plain.data_ptr())
    ctx.synchronize()
    M, F, S = out['M'], out['F'], out['S']
    for k in ('units', 'taken', 'shifts', 'dist', 'energy'):
        if not torch.equal(F[k].view(torch.uint8), S[k].view(torch.uint8)):
            raise SystemExit('%s: %s of the call with flat tables is not c1_encode_measured_sf_device\'s' % (signal, k))
    if not bool((F['weights'] == 1.0).all()):
        raise SystemExit('%s: the weights of the call with flat tables are not 1.0' % signal)
    d = M['dist'].view(units_n, 2)
    took = M['taken'] != 0
    if not torch.equal(d[:, 1] < d[:, 0], took):
        raise SystemExit('%s: taken is not T(n*) < T_ref' % signal)
    differ = (M['units'].view(units_n, 212) != plain.view(units_n, 212)).any(dim=1)
    if not torch.equal(differ, took):
        raise SystemExit('%s: M differs from c1_encode_modes_device in other units than the taken ones' % signal)
    if M['shifts'].view(units_n, 52)[~took].any():
        raise SystemExit('%s: a unit not taken has shifts' % signal)
    final = torch.where(took, d[:, 1], d[:, 0])
    at_floor = M['weights'].view(units_n, 52) == torch.from_numpy(1.0 / np.asarray(c1.MASKING_DEFAULT[0])).to('cuda:0')[None, :]
    row['taken_share'] = float(took.double().mean().item())
    row['taken_share_S'] = float((S['taken'] != 0).double().mean().item())
    row['floor_share'] = float(at_floor.double().mean().item())
    row['gain_db_against_T_ref'] = float(10 * torch.log10(d[:, 0].sum() / final.sum()).item())
    row['units_differing_from_S'] = float((M['units'].view(units_n, 212) != S['units'].view(units_n, 212)).any(dim=1).double().mean().item())
    n = min(judge_frames, frames)
    if n > 0:
        e_s, e_m = judge(pcm, host_modes, plain, S['units'], M['units'], M['weights'], n)
        row['judged_frames'] = n
        row['weighted_error_S_units'], row['weighted_error_M_units'] = e_s, e_m
        row['gain_db_against_S_units'] = float(10 * np.log10(e_s / e_m))
    for _ in range(warmup):
        for _, fn in variants:
            timed(ctx, fn)
    ms = {name: [] for name, _ in variants}
    for rep in range(reps):
        for name, fn in (variants if rep % 2 == 0 else variants[::-1]):
            ms[name].append(timed(ctx, fn))
    row.update({name: stats(v, frames) for name, v in ms.items()})
    row['M_over_S'] = row['M']['median_ms'] / row['S']['median_ms']
    row['F_over_S'] = row['F']['median_ms'] / row['S']['median_ms']
    ctx.set_profiling(True)
    for name, fn in variants:
        per = {kind: [] for kind in KINDS}
        for _ in range(3):
            fn()
            for kind in KINDS:
                per[kind].append(ctx.kernel_ms(kind))
        row[name + '_kernels_ms'] = {kind: [float(np.median([v[0] for v in per[kind]])), per[kind][0][1]] for kind in KINDS}
    ctx.set_profiling(False)
    print('%s: %d stereo frames, modes %s, offsets %s' % (signal, frames, modes_arg, list(offsets)))
    fmt = lambda k: '%s %.3f ms (%.3f - %.3f, %d; %.2f M frames/s)' % (k, row[k]['median_ms'], row[k]['min_ms'], row[k]['max_ms'], row[k]['calls'], row[k]['frames_per_s'] / 1e6)
    print('  ' + '  '.join(fmt(k) for k in 'MFS') + '  M/S %.3f  F/S %.3f' % (row['M_over_S'], row['F_over_S']))
    for name in 'MFS':
        print('  %s kernels: ' % name + ', '.join('%s %.3f ms x%d' % (k, v[0], v[1]) for k, v in row[name + '_kernels_ms'].items() if v[1]))
    print('  taken %.1f %% of the units (S: %.1f %%); %.1f %% of the units differ from S\'s; %.1f %% of the thresholds are the floor; '
          'weighted error of M: %.2f dB under its T_ref' % (100 * row['taken_share'], 100 * row['taken_share_S'], 100 * row['units_differing_from_S'],
                                                           100 * row['floor_share'], row['gain_db_against_T_ref']))
    if n > 0:
        print('  first %d frames, under M\'s weights: S\'s units %.6g, M\'s units %.6g: %.2f dB' % (n, e_s, e_m, row['gain_db_against_S_units']))
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
    ap.add_argument('--judge', type=int, default=2048, help='frames judged on the CPU from the bytes (0: none)')
    a = ap.parse_args()
    offsets = tuple(int(v) for v in a.offsets.split(','))
    ctx = c1.Context(0)
    try:
        for signal in a.signals.split(','):
            measure(ctx, signal, a.frames, a.reps, a.warmup, a.modes, offsets, a.judge)
    finally:
        ctx.close()


if __name__ == '__main__':
    main()
