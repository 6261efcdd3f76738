"""One signals call against what the library offered before it: python tools/measure_signals.py [--reps N] [--shapes clips,ticks,songs]

Three shapes of n mono signals of white noise: 4 096 x 86 frames (one-second clips), 65 536 x 4 (server ticks), 256 x 15 504
(three-minute songs); fixed modes [0,0,0] and transient detection; encode and decode; device-resident buffers.  Three ways:
  A  one c1_*_signals_device call (fresh pools in, pools out)
  B  a loop of c1_encode_device / c1_decode_device, one call per signal, on the same context; for the ticks also B4: four
     c1_*_frames_from_states_device calls, one per frame index, in place on the pools (PCM frame-major for that one)
  C  one c1_encode_device / c1_decode_device over the same total frames as a single stream: the floor
Every figure is the host clock around the calls and a synchronise of the context, after warm-up calls; the variants alternate
inside each repetition of one process; medians with the range.  Then the kernel breakdown of A from c1_ctx_kernel_ms."""
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
KINDS = ('analysis', 'allocate', 'pack', 'redo', 'decode', 'signal_starts', 'total')


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
    ap.add_argument('--loop-reps', type=int, default=0, help='repetitions of the per-signal loops of more than 10 000 calls (default: --reps)')
    ap.add_argument('--shapes', default='clips,ticks,songs')
    ap.add_argument('--warmup', type=int, default=2)
    a = ap.parse_args()
    lib = capi.load()
    ctx = c1.Context(0)
    h = ctx._h
    I64P, VP = C.POINTER(C.c_int64), C.c_void_p
    results = []
    for shape in a.shapes.split(','):
        n, m = SHAPES[shape]
        total = n * m
        off = np.arange(n + 1, dtype=np.int64) * m
        offp = off.ctypes.data_as(I64P)
        pcm = (torch.rand(total * 512, device='cuda:0') - 0.5) * 0.6
        out = torch.zeros(total * 512, dtype=torch.float32, device='cuda:0')
        units = torch.zeros(total * 212, dtype=torch.uint8, device='cuda:0')
        est = torch.zeros(n * capi.ENC_STATE_FLOATS, dtype=torch.float32, device='cuda:0')
        dst = torch.zeros(n * capi.DEC_STATE_FLOATS, dtype=torch.float32, device='cuda:0')
        torch.cuda.synchronize()
        P, U, O_ = pcm.data_ptr(), units.data_ptr(), out.data_ptr()
        loop_reps = a.loop_reps if (a.loop_reps and n > 10000) else a.reps
        for oname, oset in OPTIONS.items():
            o = c1.EncoderOptions(oset).to_c()
            ob = C.byref(o)
            one = [capi.ptr_array([P + i * m * 2048]) for i in range(n)]      # c1_encode_device's pcm[channels] per signal
            one_out = [capi.ptr_array([O_ + i * m * 2048]) for i in range(n)]
            whole, whole_out = capi.ptr_array([P]), capi.ptr_array([O_])

            def enc_a():
                capi.check(lib.c1_encode_signals_device(h, n, offp, VP(P), None, ob, VP(U), VP(est.data_ptr())))

            def enc_b():
                for i in range(n):
                    lib.c1_encode_device(h, one[i], 1, m, 0, ob, VP(U + i * m * 212))

            def enc_b4():
                for k in range(m):
                    lib.c1_encode_frames_from_states_device(h, n, VP(P + k * n * 2048), VP(est.data_ptr()), ob, VP(U + k * n * 212), VP(est.data_ptr()))

            def enc_c():
                capi.check(lib.c1_encode_device(h, whole, 1, total, 0, ob, VP(U)))

            def dec_a():
                capi.check(lib.c1_decode_signals_device(h, n, offp, VP(U), None, VP(O_), VP(dst.data_ptr())))

            def dec_b():
                for i in range(n):
                    lib.c1_decode_device(h, VP(U + i * m * 212), 1, m, 0, one_out[i])

            def dec_b4():
                for k in range(m):
                    lib.c1_decode_frames_from_states_device(h, n, VP(U + k * n * 212), VP(dst.data_ptr()), VP(O_ + k * n * 2048), VP(dst.data_ptr()))

            def dec_c():
                capi.check(lib.c1_decode_device(h, VP(U), 1, total, 0, whole_out))

            for direction, variants in (('encode', [('A', enc_a), ('B', enc_b), ('C', enc_c)] + ([('B4', enc_b4)] if shape == 'ticks' else [])),
                                        ('decode', [('A', dec_a), ('B', dec_b), ('C', dec_c)] + ([('B4', dec_b4)] if shape == 'ticks' else []))):
                if direction == 'decode':
                    enc_c()                                                   # valid units to decode
                for _ in range(a.warmup):
                    for name, fn in variants:
                        if name != 'B' or n <= 10000:
                            timed(ctx, fn)
                ms = {name: [] for name, _ in variants}
                for rep in range(a.reps):
                    for name, fn in variants:
                        if name == 'B' and rep >= loop_reps:
                            continue
                        ms[name].append(timed(ctx, fn))
                row = {'shape': shape, 'signals': n, 'frames_each': m, 'options': oname, 'direction': direction,
                       **{name: stats(v) for name, v in ms.items()}}
                row['A_over_C'] = row['A']['median_ms'] / row['C']['median_ms']
                row['B_over_A'] = row['B']['median_ms'] / row['A']['median_ms']
                ctx.set_profiling(True)
                (enc_a if direction == 'encode' else dec_a)()
                row['A_kernels_ms'] = {k: ctx.kernel_ms(k) for k in KINDS}
                (enc_c if direction == 'encode' else dec_c)()
                row['C_kernels_ms'] = {k: ctx.kernel_ms(k) for k in KINDS}
                ctx.set_profiling(False)
                results.append(row)
                print('%-6s %-7s %-7s ' % (shape, oname, direction) + '  '.join(
                    '%s %.3f ms (%.3f - %.3f, %d)' % (k, row[k]['median_ms'], row[k]['min_ms'], row[k]['max_ms'], row[k]['calls']) for k in ms)
                    + '  A/C %.3f  B/A %.1f' % (row['A_over_C'], row['B_over_A']), flush=True)
                print('       A kernels: ' + ', '.join('%s %.3f ms x%d' % (k, v[0], v[1]) for k, v in row['A_kernels_ms'].items() if v[1])
                      + ' | C: ' + ', '.join('%s %.3f ms x%d' % (k, v[0], v[1]) for k, v in row['C_kernels_ms'].items() if v[1]), flush=True)
        del pcm, out, units, est, dst
        torch.cuda.empty_cache()
    print(json.dumps(results))
    ctx.close()


if __name__ == '__main__':
    main()
