"""The measured allocation for n signals in one call against what the library offered before it:
python tools/measure_signals_measured.py [--reps N] [--shapes clips,ticks,songs]

Three shapes of n mono signals of white noise: 4 096 x 86 frames (one-second clips), 65 536 x 4 (server ticks), 256 x 15 504
(three-minute songs); fixed modes [0,0,0] and transient detection; device-resident buffers; the masked definition with the
packaged tables and the offsets 0, -1, 1, -2, -3, every output asked for.  Four ways:
  A1  one c1_encode_signals_measured_device call on a context under C1_SIGNAL_STARTS=1 (the fused signal starts)
  A0  the same call on a second context under C1_SIGNAL_STARTS=0 (two passes)
  B   a loop of c1_encode_measured_masked_device, one call per signal
  C   one c1_encode_measured_masked_device over the same total frames as a single stream: the floor
Every figure is the host clock around the calls and a synchronise of the context, after warm-up rounds; the variants alternate
inside each round of one process; medians with the range.  A1, A0 and B must agree bit for bit on every output (checked once per
row).  Then the kernel breakdown of A1 and A0 from c1_ctx_kernel_ms."""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import carta1_amd as c1
from carta1_amd import capi

SHAPES = {'clips': (4096, 86), 'ticks': (65536, 4), 'songs': (256, 15504)}
OPTIONS = {'long': {'fixedBlockModes': [0, 0, 0]}, 'detect': {}}
KINDS = ('analysis', 'allocate', 'measure', 'pack', 'redo', 'signal_starts', 'total')
OUTPUTS = (('units', 212, torch.uint8), ('taken', 1, torch.uint8), ('shifts', 52, torch.int8), ('distortion', 2, torch.float64),
           ('energy', 1, torch.float64), ('weights', 52, torch.float64))


def context(starts):
    old = os.environ.get('C1_SIGNAL_STARTS')
    os.environ['C1_SIGNAL_STARTS'] = str(starts)
    try:
        return c1.Context(0)
    finally:
        if old is None:
            del os.environ['C1_SIGNAL_STARTS']
        else:
            os.environ['C1_SIGNAL_STARTS'] = old


def timed(ctx, fn):
    ctx.synchronize()
    t0 = time.perf_counter()
    fn()
    ctx.synchronize()
    return (time.perf_counter() - t0) * 1e3


def stats(ms):
    return {'median_ms': float(np.median(ms)), 'min_ms': float(min(ms)), 'max_ms': float(max(ms)), 'calls': len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--loop-reps', type=int, default=3, help='rounds of the per-signal loop on shapes of more than 10 000 signals')
    ap.add_argument('--shapes', default='clips,ticks,songs')
    ap.add_argument('--warmup', type=int, default=2)
    a = ap.parse_args()
    lib = capi.load()
    fused, twopass = context(1), context(0)
    I64P, VP = C.POINTER(C.c_int64), C.c_void_p
    floor, spread = (np.ascontiguousarray(x, dtype=np.float64) for x in c1.check_masking(True))
    offs = np.ascontiguousarray(c1.SCALE_FACTOR_OFFSETS, dtype=np.int8)
    results = []
    for shape in a.shapes.split(','):
        n, m = SHAPES[shape]
        total = n * m
        off = np.arange(n + 1, dtype=np.int64) * m
        offp = off.ctypes.data_as(I64P)
        pcm = (torch.rand(total * 512, device='cuda:0') - 0.5) * 0.6
        sets = [{k: torch.zeros(total * w, dtype=d, device='cuda:0') for k, w, d in OUTPUTS} for _ in range(2)]
        est = torch.zeros(n * capi.ENC_STATE_FLOATS, dtype=torch.float32, device='cuda:0')
        torch.cuda.synchronize()
        P = pcm.data_ptr()
        loop_reps = a.loop_reps if n > 10000 else a.reps
        for oname, oset in OPTIONS.items():
            o = c1.EncoderOptions(oset).to_c()
            ob = C.byref(o)
            one = [capi.ptr_array([P + i * m * 2048]) for i in range(n)]
            whole = capi.ptr_array([P])

            def signals(ctx, s):
                capi.check(lib.c1_encode_signals_measured_device(
                    ctx._h, n, offp, VP(P), None, ob, None, offs.ctypes.data, len(offs), floor.ctypes.data, spread.ctypes.data,
                    VP(s['units'].data_ptr()), VP(est.data_ptr()), VP(s['taken'].data_ptr()), VP(s['shifts'].data_ptr()),
                    VP(s['distortion'].data_ptr()), VP(s['energy'].data_ptr()), VP(s['weights'].data_ptr())))

            def masked(ctx, s, chan, frames, at):
                return lib.c1_encode_measured_masked_device(
                    ctx._h, chan, 1, frames, 0, ob, None, offs.ctypes.data, len(offs), floor.ctypes.data, spread.ctypes.data,
                    VP(s['units'].data_ptr() + at * 212), VP(s['taken'].data_ptr() + at), VP(s['shifts'].data_ptr() + at * 52),
                    VP(s['distortion'].data_ptr() + at * 16), VP(s['energy'].data_ptr() + at * 8), VP(s['weights'].data_ptr() + at * 416))

            def a1():
                signals(fused, sets[0])

            def a0():
                signals(twopass, sets[1])

            def b():
                for i in range(n):
                    masked(fused, sets[1], one[i], m, i * m)

            def c():
                capi.check(masked(fused, sets[1], whole, total, 0))

            variants = [('A1', fused, a1), ('A0', twopass, a0), ('B', fused, b), ('C', fused, c)]
            for _ in range(a.warmup):
                for name, ctx, fn in variants:
                    if name != 'B' or n <= 10000:
                        timed(ctx, fn)
            ms = {name: [] for name, _, _ in variants}
            for rep in range(a.reps):
                for name, ctx, fn in variants:
                    if name == 'B' and rep >= loop_reps:
                        continue
                    ms[name].append(timed(ctx, fn))
            row = {'shape': shape, 'signals': n, 'frames_each': m, 'options': oname, **{name: stats(v) for name, v in ms.items()}}
            row['A1_over_A0'] = row['A1']['median_ms'] / row['A0']['median_ms']
            row['A1_range_below_A0'] = row['A1']['max_ms'] < row['A0']['min_ms']
            row['B_over_A1'] = row['B']['median_ms'] / row['A1']['median_ms']
            row['A1_over_C'] = row['A1']['median_ms'] / row['C']['median_ms']
            row['A0_over_C'] = row['A0']['median_ms'] / row['C']['median_ms']
            # the same bits from the three ways that encode n signals
            timed(fused, a1)
            timed(twopass, a0)
            row['A0_equals_A1'] = all(torch.equal(sets[0][k], sets[1][k]) for k, _, _ in OUTPUTS)
            timed(fused, b)
            row['B_equals_A1'] = all(torch.equal(sets[0][k], sets[1][k]) for k, _, _ in OUTPUTS)
            for name, ctx, fn in variants[:2]:
                ctx.set_profiling(True)
                fn()
                row[name + '_kernels_ms'] = {k: ctx.kernel_ms(k) for k in KINDS}
                ctx.set_profiling(False)
            results.append(row)
            print('%-6s %-7s ' % (shape, oname) + '  '.join(
                '%s %.3f ms (%.3f - %.3f, %d)' % (k, row[k]['median_ms'], row[k]['min_ms'], row[k]['max_ms'], row[k]['calls']) for k in ms)
                + '  A1/A0 %.3f (range below: %s)  B/A1 %.1f  A1/C %.3f  A0/C %.3f  bits A0==A1 %s B==A1 %s' % (
                    row['A1_over_A0'], row['A1_range_below_A0'], row['B_over_A1'], row['A1_over_C'], row['A0_over_C'], row['A0_equals_A1'],
                    row['B_equals_A1']), flush=True)
            for name in ('A1', 'A0'):
                print('       %s kernels: ' % name + ', '.join('%s %.3f ms x%d' % (k, v[0], v[1]) for k, v in row[name + '_kernels_ms'].items() if v[1]),
                      flush=True)
        del pcm, sets, est
        torch.cuda.empty_cache()
    print(json.dumps(results))
    fused.close()
    twopass.close()


if __name__ == '__main__':
    main()
