"""The measured block-mode search under one masking threshold per unit (c1_encode_measured_modes_masked_device) against the
composition of existing calls a masking caller has without it: python tools/measure_measured_modes_masked.py [--frames N]
[--reps N] [--warmup N] [--signals white,mixed] [--counts 2,8] [--pushes 1,8,64] [--out FILE]

Input: 2^20 stereo frames, device-resident, of (white) BASELINE configs[1]'s white noise, seeds 1 and 2, and (mixed) the mixed
corpus of configs[3].  Candidates: the first n of 58, 0, 10, 50, 2, 8, 48, 56; the suggested offsets; the packaged tables.
  An  one c1_encode_measured_modes_masked_device call, all eight outputs
  Hn  the composition: c1_encode_measured_modes_device asked for modes_out only, then c1_encode_measured_masked_device under
      those modes with all its outputs
  Un  the same build's unweighted c1_encode_measured_modes_device with all seven outputs (no bar: what the weights cost)
The bytes are checked once, before timing: An's weights are c1_encode_measured_masked_device's under constant modes 0, bit for
bit, and so is the column of byte 0 of distortion and energy; choice is the first least T_final of the columns; modes_out =
cand[choice].  Every figure is the host clock around the call(s) and a synchronise of the context, after warm-up rounds; the
variants alternate inside each round of one process; medians with the range.  Then the kernel breakdown of An from
c1_ctx_kernel_ms, and "measure" of one c1_encode_measured_masked_device and one c1_encode_measured_sf_device call under the
detector's modes (what the weight phase costs where it was introduced).
--pushes: a stereo push of that many frames, c1_enc_stream_push_measured_modes_masked against c1_enc_stream_push_measured_modes,
eight candidates, the offsets, alternating on two streams of one context."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch
import carta1_amd as c1
from measure_measured import timed, stats
from measure_measured_modes import CANDIDATES, generate, buffers

KINDS = ('analysis', 'allocate', 'choose', 'measure', 'pack', 'total')
OFFSETS = c1.SCALE_FACTOR_OFFSETS


def measure(ctx, signal, frames, n, reps, warmup, pcm):
    ptrs = [p.data_ptr() for p in pcm]
    cand, units_n = list(CANDIDATES[:n]), frames * 2
    new = lambda dtype, count: torch.zeros(count, dtype=dtype, device='cuda:0')
    A = buffers(units_n, n)
    A['weights'] = new(torch.float64, units_n * 52)
    U = buffers(units_n, n)
    H = {'modes': new(torch.uint8, units_n), 'units': new(torch.uint8, units_n * 212), 'taken': new(torch.uint8, units_n),
         'shifts': new(torch.int8, units_n * 52), 'dist': new(torch.float64, units_n * 2), 'energy': new(torch.float64, units_n),
         'weights': new(torch.float64, units_n * 52)}
    zero = new(torch.uint8, units_n)

    def run_a():
        ctx.encode_measured_modes_device(ptrs, frames, cand, A['units'].data_ptr(), A['choice'].data_ptr(), A['modes'].data_ptr(),
                                         A['taken'].data_ptr(), A['shifts'].data_ptr(), A['dist'].data_ptr(), A['energy'].data_ptr(),
                                         scale_factor_offsets=OFFSETS, masking=True, weights_ptr=A['weights'].data_ptr())

    def run_u():
        ctx.encode_measured_modes_device(ptrs, frames, cand, U['units'].data_ptr(), U['choice'].data_ptr(), U['modes'].data_ptr(),
                                         U['taken'].data_ptr(), U['shifts'].data_ptr(), U['dist'].data_ptr(), U['energy'].data_ptr(),
                                         scale_factor_offsets=OFFSETS)

    def masked(modes, out):
        ctx.encode_measured_device(ptrs, frames, out['units'].data_ptr(), out['taken'].data_ptr(), out['dist'].data_ptr(), out['energy'].data_ptr(),
                                   modes_ptr=modes.data_ptr(), scale_factor_offsets=OFFSETS, shifts_ptr=out['shifts'].data_ptr(), masking=True,
                                   weights_ptr=out['weights'].data_ptr())

    def run_h():
        ctx.encode_measured_modes_device(ptrs, frames, cand, modes_ptr=H['modes'].data_ptr(), scale_factor_offsets=OFFSETS)
        masked(H['modes'], H)

    what = '%s, %d frames, n = %d' % (signal, frames, n)
    # ---- the bytes, before any timing ----
    run_a()
    masked(zero, H)
    ctx.synchronize()
    bits = lambda t: t.contiguous().view(torch.int64)
    if not torch.equal(bits(A['weights']), bits(H['weights'])):
        raise SystemExit('%s: weights are not the masked call\'s under constant modes 0' % what)
    d, e = A['dist'].view(units_n, n, 2), A['energy'].view(units_n, n)
    if 0 in cand:
        k0 = cand.index(0)
        if not torch.equal(bits(d[:, k0]), bits(H['dist'].view(units_n, 2))) or not torch.equal(bits(e[:, k0]), bits(H['energy'])):
            raise SystemExit('%s: the column of byte 0 is not the masked call\'s under constant modes 0' % what)
    final = torch.where(d[:, :, 1] < d[:, :, 0], d[:, :, 1], d[:, :, 0])
    first = (final == final.min(dim=1, keepdim=True).values).to(torch.uint8).argmax(dim=1)
    if not torch.equal(first.to(torch.uint8), A['choice']):
        raise SystemExit('%s: choice is not the first least T_final' % what)
    if not torch.equal(torch.tensor(cand, dtype=torch.uint8, device='cuda:0')[A['choice'].long()], A['modes']):
        raise SystemExit('%s: modes_out is not cand[choice]' % what)
    run_u()
    ctx.synchronize()
    row = {'signal': signal, 'frames': frames, 'n_cand': n, 'candidates': cand, 'offsets': list(OFFSETS)}
    row['winner_share'] = [float((A['choice'] == k).double().mean().item()) for k in range(n)]
    row['differs_from_unweighted'] = float((A['choice'] != U['choice']).double().mean().item())
    # ---- the time ----
    variants = [('A', run_a), ('H', run_h), ('U', run_u)]
    for _ in range(warmup):
        for _, fn in variants:
            timed(ctx, fn)
    ms = {name: [] for name, _ in variants}
    for rep in range(reps):
        for name, fn in (variants if rep % 2 == 0 else variants[::-1]):
            ms[name].append(timed(ctx, fn))
    row.update({name: stats(v, frames) for name, v in ms.items()})
    row['A_over_H'] = row['A']['median_ms'] / row['H']['median_ms']
    row['A_over_U'] = row['A']['median_ms'] / row['U']['median_ms']
    ctx.set_profiling(True)
    run_a()
    row['A_kernels_ms'] = {kind: list(ctx.kernel_ms(kind)) for kind in KINDS}
    run_u()
    row['U_kernels_ms'] = {kind: list(ctx.kernel_ms(kind)) for kind in KINDS}
    ctx.set_profiling(False)
    fmt = lambda k: '%s %.2f ms (%.2f - %.2f, %d)' % (k, row[k]['median_ms'], row[k]['min_ms'], row[k]['max_ms'], row[k]['calls'])
    print(what)
    print('  ' + '  '.join(fmt(k) for k in 'AHU') + '  A/H %.3f  A/U %.3f' % (row['A_over_H'], row['A_over_U']))
    for name in 'AU':
        print('  %s kernels: ' % name + ', '.join('%s %.2f ms x%d' % (k, v[0], v[1]) for k, v in row[name + '_kernels_ms'].items() if v[1]))
    print('  winners ' + ', '.join('%d: %.1f %%' % (cand[k], 100 * s) for k, s in enumerate(row['winner_share'])) +
          '; not the unweighted search\'s winner in %.1f %%' % (100 * row['differs_from_unweighted']))
    print(json.dumps(row), flush=True)
    return row


def weight_phase(ctx, signal, frames, pcm):
    """"measure" of c1_encode_measured_masked_device over that of c1_encode_measured_sf_device, the detector's modes, measure only"""
    ptrs = [p.data_ptr() for p in pcm]
    dist = torch.zeros(frames * 4, dtype=torch.float64, device='cuda:0')
    ctx.set_profiling(True)
    out = {}
    for name, masking in (('k_measured_masked', True), ('k_measured_sf', None)):
        for _ in range(2):
            ctx.encode_measured_device(ptrs, frames, None, None, dist.data_ptr(), scale_factor_offsets=OFFSETS, masking=masking)
            out[name] = ctx.kernel_ms('measure')[0]
    ctx.set_profiling(False)
    row = {'signal': signal, 'frames': frames, 'measure_ms': out, 'masked_over_sf': out['k_measured_masked'] / out['k_measured_sf']}
    print('%s: k_measured_masked %.2f ms, k_measured_sf %.2f ms, ratio %.3f' % (signal, out['k_measured_masked'], out['k_measured_sf'], row['masked_over_sf']))
    print(json.dumps(row), flush=True)
    return row


def pushes(ctx, signal, frames, reps, pcm):
    chans = [p[:frames * 512].cpu().numpy() for p in pcm]
    a, b = c1.EncoderStream(ctx, 2), c1.EncoderStream(ctx, 2)
    try:
        run = {'masked': lambda: a.push_measured_modes(chans, list(CANDIDATES), scale_factor_offsets=OFFSETS, masking=True),
               'unweighted': lambda: b.push_measured_modes(chans, list(CANDIDATES), scale_factor_offsets=OFFSETS)}
        ms = {k: [] for k in run}
        for rep in range(reps + 3):
            for name in (list(run) if rep % 2 == 0 else list(run)[::-1]):
                t = time.perf_counter()
                run[name]()
                if rep >= 3:
                    ms[name].append((time.perf_counter() - t) * 1e3)
    finally:
        a.close(), b.close()
    row = {'signal': signal, 'push_frames': frames, 'masked_ms': float(np.median(ms['masked'])), 'unweighted_ms': float(np.median(ms['unweighted'])),
           'masked_range': [min(ms['masked']), max(ms['masked'])], 'unweighted_range': [min(ms['unweighted']), max(ms['unweighted'])]}
    print('%s: a stereo push of %d frames: masked %.3f ms (%.3f - %.3f), unweighted %.3f ms (%.3f - %.3f)' % (
        signal, frames, row['masked_ms'], *row['masked_range'], row['unweighted_ms'], *row['unweighted_range']))
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=1 << 20)
    ap.add_argument('--reps', type=int, default=4)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--signals', default='white,mixed')
    ap.add_argument('--counts', default='2,8')
    ap.add_argument('--pushes', default='1,8,64')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    ctx = c1.Context(0)
    rows = []
    try:
        for signal in a.signals.split(','):
            pcm = generate(ctx, signal, a.frames)
            for n in [int(v) for v in a.counts.split(',') if v]:
                rows.append(measure(ctx, signal, a.frames, n, a.reps, a.warmup, pcm))
            rows.append(weight_phase(ctx, signal, a.frames, pcm))
            for frames in [int(v) for v in a.pushes.split(',') if v]:
                rows.append(pushes(ctx, signal, frames, 20, pcm))
    finally:
        ctx.close()
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(rows, f)


if __name__ == '__main__':
    main()
