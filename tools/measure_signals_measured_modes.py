"""The measured block-mode search for n signals in one call against what the library offered before it:
python tools/measure_signals_measured_modes.py [--shapes clips,ticks,songs] [--options long,detect]

Three shapes of n mono signals of white noise: 4 096 x 86 frames (one-second clips), 16 384 x 4 (four frames for each of many live
streams), 256 x 15 504 (three-minute songs); fixed modes [0,0,0] and transient detection (the search reads neither); the eight
candidates of the domain, the offsets 0, -1, 1, -2, -3, every output asked for.  Three ways:
  A  one c1_encode_signals_measured_modes_device call, device-resident buffers
  B  what the library offered before: per signal one EncoderStream, restored with c1_enc_stream_set_state and pushed once with
     c1_enc_stream_push_measured_modes (host buffers, as that call takes them; the streams are created before the clock starts)
  C  one c1_encode_measured_modes_device over the same total frames as a single stream: the floor
Every figure is the host clock around the calls and a synchronise of the context; the variants alternate inside each round of one
process: 2 warm-up rounds, then 10 timed rounds, or 3 where a round of the loop takes over ten seconds; medians with the range.
A and B are compared bit for bit on every output and on the states before anything is timed.  Then the kernel breakdown of one
profiled A call from c1_ctx_kernel_ms."""
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

SHAPES = {'clips': (4096, 86), 'ticks': (16384, 4), 'songs': (256, 15504)}
OPTIONS = {'long': {'fixedBlockModes': [0, 0, 0]}, 'detect': {}}
KINDS = ('analysis', 'allocate', 'measure', 'pack', 'redo', 'signal_starts', 'total')
CANDIDATES = (0x00, 0x02, 0x08, 0x0a, 0x30, 0x32, 0x38, 0x3a)
NC = len(CANDIDATES)
OUTPUTS = (('units', 212, np.uint8), ('choice', 1, np.uint8), ('modes', 1, np.uint8), ('taken', 1, np.uint8), ('shifts', 52, np.int8),
           ('distortion', 2 * NC, np.float64), ('energy', NC, np.float64))
TORCH = {np.uint8: torch.uint8, np.int8: torch.int8, np.float64: torch.float64}


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
    ap.add_argument('--slow-reps', type=int, default=3, help='timed rounds where a round of the per-signal loop takes over ten seconds')
    ap.add_argument('--shapes', default='clips,ticks,songs')
    ap.add_argument('--options', default='long,detect')
    ap.add_argument('--warmup', type=int, default=2)
    a = ap.parse_args()
    lib = capi.load()
    ctx = c1.Context(0)
    I64P, VP = C.POINTER(C.c_int64), C.c_void_p
    cand = np.ascontiguousarray(CANDIDATES, dtype=np.uint8)
    offs = np.ascontiguousarray(c1.SCALE_FACTOR_OFFSETS, dtype=np.int8)
    results = []
    for shape in a.shapes.split(','):
        n, m = SHAPES[shape]
        total = n * m
        off = np.arange(n + 1, dtype=np.int64) * m
        offp = off.ctypes.data_as(I64P)
        pcm = (torch.rand(total * 512, device='cuda:0') - 0.5) * 0.6
        host_pcm = pcm.cpu().numpy()
        dev = {k: torch.zeros(total * w, dtype=TORCH[d], device='cuda:0') for k, w, d in OUTPUTS}
        floor = {k: torch.zeros(total * w, dtype=TORCH[d], device='cuda:0') for k, w, d in OUTPUTS}
        host = {k: np.zeros(total * w, dtype=d) for k, w, d in OUTPUTS}
        st_in = torch.zeros(n * capi.ENC_STATE_FLOATS, dtype=torch.float32, device='cuda:0')
        st_out = torch.zeros(n * capi.ENC_STATE_FLOATS, dtype=torch.float32, device='cuda:0')
        zero_state = np.zeros(capi.ENC_STATE_FLOATS, dtype=np.float32)
        host_states = np.zeros((n, capi.ENC_STATE_FLOATS), dtype=np.float32)
        torch.cuda.synchronize()
        P = pcm.data_ptr()
        for oname in a.options.split(','):
            o = c1.EncoderOptions(OPTIONS[oname]).to_c()
            ob = C.byref(o)
            streams = [c1.EncoderStream(ctx, 1, c1.EncoderOptions(OPTIONS[oname])) for _ in range(n)]
            chans = [capi.ptr_array([host_pcm.ctypes.data + i * m * 2048]) for i in range(n)]
            size = {k: w * np.dtype(d).itemsize for k, w, d in OUTPUTS}
            whole = capi.ptr_array([P])

            def va():
                capi.check(lib.c1_encode_signals_measured_modes_device(
                    ctx._h, n, offp, VP(P), VP(st_in.data_ptr()), ob, cand.ctypes.data, NC, offs.ctypes.data, len(offs),
                    VP(dev['units'].data_ptr()), VP(st_out.data_ptr()), *[VP(dev[k].data_ptr()) for k, _, _ in OUTPUTS[1:]]))

            def vb(states=False):
                for i, s in enumerate(streams):
                    at = i * m
                    rc = lib.c1_enc_stream_set_state(s._h, zero_state.ctypes.data)
                    rc = rc or lib.c1_enc_stream_push_measured_modes(
                        s._h, chans[i], m, cand.ctypes.data, NC, offs.ctypes.data, len(offs),
                        *[VP(host[k].ctypes.data + at * size[k]) for k, _, _ in OUTPUTS])
                    if states:
                        rc = rc or lib.c1_enc_stream_get_state(s._h, host_states[i].ctypes.data)
                    if rc:
                        capi.check(rc)

            def vc():
                capi.check(lib.c1_encode_measured_modes_device(
                    ctx._h, whole, 1, total, 0, ob, cand.ctypes.data, NC, offs.ctypes.data, len(offs),
                    *[VP(floor[k].data_ptr()) for k, _, _ in OUTPUTS]))

            # the same bits from the two ways that encode n signals, before anything is timed
            t_first_b = timed(ctx, lambda: vb(states=True))
            timed(ctx, va)
            equal = {k: bool(np.array_equal(dev[k].cpu().numpy().view(np.uint8), host[k].view(np.uint8))) for k, _, _ in OUTPUTS}
            equal['states'] = bool(np.array_equal(st_out.cpu().numpy().view(np.uint32), host_states.reshape(-1).view(np.uint32)))
            variants = [('A', va), ('B', vb), ('C', vc)]
            warm = {'B': [t_first_b]}
            for r in range(a.warmup):
                for name, fn in variants:
                    if name == 'B' and r == 0:
                        continue                                        # the bit check's round was B's first
                    warm.setdefault(name, []).append(timed(ctx, fn))
            reps = a.slow_reps if max(warm['B']) > 10000.0 else a.reps
            ms = {name: [] for name, _ in variants}
            for rep in range(reps):
                for name, fn in variants:
                    ms[name].append(timed(ctx, fn))
            row = {'shape': shape, 'signals': n, 'frames_each': m, 'options': oname, 'A_equals_B': equal,
                   **{name: stats(v) for name, v in ms.items()}}
            row['A_range_below_B'] = row['A']['max_ms'] < row['B']['min_ms']
            row['B_over_A'] = row['B']['median_ms'] / row['A']['median_ms']
            row['A_over_C'] = row['A']['median_ms'] / row['C']['median_ms']
            ctx.set_profiling(True)
            va()
            row['A_kernels_ms'] = {k: ctx.kernel_ms(k) for k in KINDS}
            vc()
            row['C_kernels_ms'] = {k: ctx.kernel_ms(k) for k in KINDS}
            ctx.set_profiling(False)
            results.append(row)
            print('%-6s %-7s ' % (shape, oname) + '  '.join(
                '%s %.3f ms (%.3f - %.3f, %d)' % (k, row[k]['median_ms'], row[k]['min_ms'], row[k]['max_ms'], row[k]['calls']) for k in ms)
                + '  B/A %.1f  A/C %.3f  A range below B: %s  bits A==B %s' % (
                    row['B_over_A'], row['A_over_C'], row['A_range_below_B'], 'all' if all(equal.values()) else equal), flush=True)
            for name in ('A', 'C'):
                print('       %s kernels: ' % name + ', '.join('%s %.3f ms x%d' % (k, v[0], v[1]) for k, v in row[name + '_kernels_ms'].items() if v[1]),
                      flush=True)
            for s in streams:
                s.close()
        del pcm, dev, floor, st_in, st_out
        torch.cuda.empty_cache()
    print(json.dumps(results))
    ctx.close()
    bad = [r for r in results if not all(r['A_equals_B'].values())]
    sys.exit(1 if bad else 0)


if __name__ == '__main__':
    main()
