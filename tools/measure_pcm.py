"""The PCM-domain meter of given sound units (c1_measure_pcm_device): its kernel's time against the decoder's, every encoder of
the library on the PCM scale next to the coefficient scale, and a first pre-echo figure.  python tools/measure_pcm.py [--frames N]
[--reps N] [--warmup N] [--skip-scoreboard] [--out FILE]

Kernel time.  2^20 stereo frames (2^21 units) of the mixed corpus of BASELINE configs[3], device-resident; the units of
c1_encode_device under transient detection.
  P  c1_measure_pcm_device, all three outputs: "meter_pcm" of c1_ctx_kernel_ms
  Pt the same, totals only
  D  c1_decode_device of the same units (the exact decoder): "decode"
2 warm-up rounds, then `reps` rounds alternating the variants in one process; median (min - max) in ms.
Scoreboard.  2^20 stereo frames of white noise (seeds 1 and 2) and of the mixed corpus; the units of the eight encoders of
tools/measure_units.py under transient detection.  Per encoder the coefficient-domain figure of c1_measure_units_device (flat, all
frames: DESIGN.md 6m's column), the same without the first two frames, and the PCM-domain figure without the first two frames:
10 log10(sum totals[:, 1] / sum totals[:, 0]).
Pre-echo.  The mixed corpus.  In the units where c1_encode_device under detection coded at least one band with short blocks: the
noise in the four 32-sample segments ahead of the unit's loudest segment of `signal` (they may lie in the frame before), summed
over those units, against the signal of the loudest segments, for c1_encode_device under detection, at fixed [0,0,0] and for
c1_encode_best_modes_device.  Figures of the meter: nobody has listened to anything."""
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
SKIP = 2                                              # frames left out at the start of every signal


def generate(ctx, signal, frames):
    pcm = [torch.zeros(frames * 512, dtype=torch.float32, device='cuda:0') for _ in range(2)]
    for c in range(2):
        ctx.generate_device(SIGNALS[signal], 1 + c, frames, pcm[c].data_ptr())
    return pcm


def stat(v):
    return {'median_ms': float(np.median(v)), 'min_ms': float(min(v)), 'max_ms': float(max(v)), 'calls': len(v)}


def kernel_time(ctx, frames, reps, warmup):
    n = frames * 2
    pcm = generate(ctx, 'mixed', frames)
    ptrs = [p.data_ptr() for p in pcm]
    units = torch.zeros(n * 212, dtype=torch.uint8, device='cuda:0')
    ctx.encode_device(ptrs, frames, units.data_ptr())
    out = {k: torch.zeros(n * w, dtype=torch.float64, device='cuda:0') for k, w in (('noise', 16), ('signal', 16), ('totals', 2))}
    dec = [torch.zeros(frames * 512, dtype=torch.float32, device='cuda:0') for _ in range(2)]
    ctx.synchronize()

    def meter():
        ctx.measure_pcm_device(ptrs, frames, units.data_ptr(), out['noise'].data_ptr(), out['signal'].data_ptr(), out['totals'].data_ptr())
        return ctx.kernel_ms('meter_pcm')[0]

    def meter_totals():
        ctx.measure_pcm_device(ptrs, frames, units.data_ptr(), totals_ptr=out['totals'].data_ptr())
        return ctx.kernel_ms('meter_pcm')[0]

    def decode():
        ctx.decode_device(units.data_ptr(), 2, frames, [d.data_ptr() for d in dec])
        return ctx.kernel_ms('decode')[0]

    variants = [('P', meter), ('D', decode), ('Pt', meter_totals)]
    ctx.set_profiling(True)
    for _ in range(warmup):
        for _, fn in variants:
            fn()
    ms = {name: [] for name, _ in variants}
    for rep in range(reps):
        for name, fn in (variants if rep % 2 == 0 else variants[::-1]):
            ms[name].append(fn())
    ctx.set_profiling(False)
    row = {'frames': frames, 'units': n}
    row.update({name: stat(v) for name, v in ms.items()})
    row['P_over_D'] = row['P']['median_ms'] / row['D']['median_ms']
    row['Pt_over_D'] = row['Pt']['median_ms'] / row['D']['median_ms']
    row['P_bytes_per_s'] = n * (2048 + 212 + 34 * 8) / row['P']['median_ms'] * 1e3
    # the meter against its own definition applied to the decoder's PCM, on the device (float64 sums in another order: a
    # figure, not a check -- tests/test_gpu_measure_pcm.py compares bit for bit)
    meter()
    decode()
    ctx.synchronize()
    worst = 0.0
    for c in range(2):
        x = torch.zeros_like(pcm[c])
        x[c1.PCM_DELAY:] = pcm[c][:-c1.PCM_DELAY]
        e = dec[c].double() - x.double()
        want = (e * e).view(frames, 16, 32).sum(dim=2)
        got = out['noise'].view(frames, 2, 16)[:, c]
        worst = max(worst, float(((got - want).abs() / want.clamp_min(1e-300)).max().item()))
    row['max_rel_difference_to_decode'] = worst
    fmt = lambda k: '%s %.3f (%.3f - %.3f)' % (k, row[k]['median_ms'], row[k]['min_ms'], row[k]['max_ms'])
    print('kernel time, mixed, detection, %d units: ' % n + '  '.join(fmt(k) for k in ('P', 'Pt', 'D')) +
          '  P/D %.2f  Pt/D %.2f  P moves %.0f GB/s  |noise - recomputed| <= %.1e relative' %
          (row['P_over_D'], row['Pt_over_D'], row['P_bytes_per_s'] / 1e9, worst))
    return row


def encoders(ctx, ptrs, frames, units):
    palette = [c1.EncoderOptions({'allocationBias': b}) for b in BIASES]
    return [('c1_encode_device, bias 0.5', lambda: ctx.encode_device(ptrs, frames, units.data_ptr(), c1.EncoderOptions({'allocationBias': 0.5}))),
            ('c1_encode_device, bias 1', lambda: ctx.encode_device(ptrs, frames, units.data_ptr(), c1.EncoderOptions())),
            ('c1_encode_device, bias 2', lambda: ctx.encode_device(ptrs, frames, units.data_ptr(), c1.EncoderOptions({'allocationBias': 2.0}))),
            ('c1_encode_best_bias_device', lambda: ctx.encode_best_bias_device(ptrs, frames, palette, units.data_ptr())),
            ('c1_encode_best_modes_device', lambda: ctx.encode_best_modes_device(ptrs, frames, DOMAIN, units.data_ptr())),
            ('c1_encode_measured_device', lambda: ctx.encode_measured_device(ptrs, frames, units.data_ptr())),
            ('c1_encode_measured_sf_device', lambda: ctx.encode_measured_device(ptrs, frames, units.data_ptr(), scale_factor_offsets=c1.SCALE_FACTOR_OFFSETS)),
            ('c1_encode_measured_masked_device', lambda: ctx.encode_measured_device(ptrs, frames, units.data_ptr(), scale_factor_offsets=c1.SCALE_FACTOR_OFFSETS,
                                                                                    masking=True))]


def snr_db(totals, n, skip):
    t = totals.view(n, 2)[skip * 2:]
    return float(10 * torch.log10(t[:, 1].sum() / t[:, 0].sum()).item())


def scoreboard(ctx, signal, frames):
    n = frames * 2
    pcm = generate(ctx, signal, frames)
    ptrs = [p.data_ptr() for p in pcm]
    units = torch.zeros(n * 212, dtype=torch.uint8, device='cuda:0')
    totals = torch.zeros(n * 2, dtype=torch.float64, device='cuda:0')
    out = []
    for name, encode in encoders(ctx, ptrs, frames, units):
        units.zero_()
        encode()
        ctx.measure_units_device(ptrs, frames, units.data_ptr(), totals_ptr=totals.data_ptr())
        ctx.synchronize()
        db = {'coefficients': snr_db(totals, n, 0), 'coefficients_skip2': snr_db(totals, n, SKIP)}
        ctx.measure_pcm_device(ptrs, frames, units.data_ptr(), totals_ptr=totals.data_ptr())
        ctx.synchronize()
        db['pcm_skip2'] = snr_db(totals, n, SKIP)
        print('%s  %-34s coefficients %.2f dB (without the first two frames %.2f)  PCM %.2f dB  gap %+.2f' %
              (signal, name, db['coefficients'], db['coefficients_skip2'], db['pcm_skip2'], db['pcm_skip2'] - db['coefficients']))
        out.append({'signal': signal, 'units_of': name, 'frames': frames, 'db': db})
    return out


def pre_echo(ctx, frames):
    n = frames * 2
    pcm = generate(ctx, 'mixed', frames)
    ptrs = [p.data_ptr() for p in pcm]
    units = torch.zeros(n * 212, dtype=torch.uint8, device='cuda:0')
    noise = torch.zeros(n * 16, dtype=torch.float64, device='cuda:0')
    signal = torch.zeros(n * 16, dtype=torch.float64, device='cuda:0')
    rows = [('c1_encode_device, detection', lambda: ctx.encode_device(ptrs, frames, units.data_ptr(), c1.EncoderOptions())),
            ('c1_encode_device, fixed [0,0,0]', lambda: ctx.encode_device(ptrs, frames, units.data_ptr(), c1.EncoderOptions({'fixedBlockModes': [0, 0, 0]}))),
            ('c1_encode_best_modes_device', lambda: ctx.encode_best_modes_device(ptrs, frames, DOMAIN, units.data_ptr()))]
    out, short, ahead, peak = [], None, None, None
    for name, encode in rows:
        units.zero_()
        encode()
        ctx.measure_pcm_device(ptrs, frames, units.data_ptr(), noise.data_ptr(), signal.data_ptr())
        ctx.synchronize()
        if short is None:
            # deserializeFrame: the block modes are 2, 2 and 3 minus the three 2-bit fields of the first byte; all long is 0xAC
            first = units.view(n, 212)[:, 0]
            short = ((first & 0xFC) != 0xAC).view(frames, 2)
            short[:SKIP] = False
            sig = signal.view(frames, 2, 16)
            loudest = sig.argmax(dim=2)                                            # [frames, 2]
            peak = sig.gather(2, loudest.unsqueeze(2)).squeeze(2)
            # positions of the four segments ahead in the channel's sequence of frames * 16 segments
            at = (torch.arange(frames, device='cuda:0').unsqueeze(1) * 16 + loudest).unsqueeze(2) - torch.arange(1, 5, device='cuda:0')
            ahead = at.clamp_min(0)                                                # [frames, 2, 4]; frame 0 is left out anyway
        seq = noise.view(frames, 2, 16).permute(1, 0, 2).reshape(2, frames * 16)
        pre = torch.stack([seq[c][ahead[:, c]] for c in range(2)], dim=1).sum(dim=2)   # [frames, 2]
        row = {'units_of': name, 'frames': frames, 'units_with_short_blocks': int(short.sum().item()),
               'noise_ahead': float(pre[short].sum().item()), 'signal_loudest': float(peak[short].sum().item())}
        row['db_below_loudest'] = float(10 * np.log10(row['signal_loudest'] / row['noise_ahead']))
        print('pre-echo, mixed, %-32s %d units with short blocks under detection: noise in the four segments ahead %.4g, %.2f dB below the '
              'loudest segments' % (name, row['units_with_short_blocks'], row['noise_ahead'], row['db_below_loudest']))
        out.append(row)
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
    result = {'kernel_time': [], 'scoreboard': [], 'pre_echo': []}
    try:
        result['kernel_time'].append(kernel_time(ctx, a.frames, a.reps, a.warmup))
        if not a.skip_scoreboard:
            for signal in ('white', 'mixed'):
                result['scoreboard'] += scoreboard(ctx, signal, a.frames)
            result['pre_echo'] = pre_echo(ctx, a.frames)
    finally:
        ctx.close()
    print(json.dumps(result))
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(result, f, indent=1)


if __name__ == '__main__':
    main()
