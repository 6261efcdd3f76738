"""tools/bench_decode_model.py (GPU) -- the decode entries that run from frame fields and from decoder states, timed under the
decode models given (default 2 = binary32 throughout and 0 = exact), alternated in one process after a warm-up: median and range
of the rounds, and the c1_ctx_kernel_ms split of one profiled call.
  fields   c1_decode_fields_device at 2^20 mono frames (65 536 encoded frames of white noise unpacked, tiled on the device)
  signals  c1_decode_signals_device at 2^18 signals of 4 frames
  push     a 1-frame DecoderStream.push_fields (host call, synchronous)
--root DIR imports carta1_amd from another tree, e.g. the parent commit's with --models 0, for the figures of its library."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ap = argparse.ArgumentParser()
ap.add_argument('--root', default=os.getcwd())
ap.add_argument('--models', default='2,0')
ap.add_argument('--rounds', type=int, default=9)
ap.add_argument('--calls', type=int, default=5)
args = ap.parse_args()
sys.path[:0] = [os.path.abspath(args.root)]
import carta1_amd as c1  # noqa: E402

MODELS = [int(m) for m in args.models.split(',')]
FRAMES, BASE, SIGNALS, PER = 1 << 20, 1 << 16, 1 << 18, 4
KEYS = ('nbfu', 'block_modes', 'sfi', 'wl', 'quantized')
ctx = c1.Context(0)


def set_model(m):
    if hasattr(ctx, 'set_decode_model'):
        ctx.set_decode_model(m)
    elif m:
        raise SystemExit('this tree has no decode model %d' % m)


pcm = torch.empty(FRAMES * 512, dtype=torch.float32, device='cuda')
ctx.generate_device(c1.SIGNAL_WHITE, 1, FRAMES, pcm.data_ptr())
units = torch.empty(FRAMES * 212, dtype=torch.uint8, device='cuda')
ctx.encode_device([pcm.data_ptr()], FRAMES, units.data_ptr(), c1.EncoderOptions())
ctx.synchronize()
host_units = units[:BASE * 212].cpu().numpy().reshape(-1, 212)
fields = ctx.unpack_units(host_units)
dev = {k: torch.from_numpy(np.ascontiguousarray(fields[k]).reshape(BASE, -1)).to('cuda').repeat(FRAMES // BASE, 1).contiguous() for k in KEYS}
out = torch.empty(FRAMES * 512, dtype=torch.float32, device='cuda')
offsets = np.arange(SIGNALS + 1, dtype=np.int64) * PER
one = {k: np.ascontiguousarray(fields[k][100:101]) for k in KEYS}
stream = c1.DecoderStream(ctx, 1)
stream.push_fields({k: np.ascontiguousarray(fields[k][:100]) for k in KEYS})


def run_fields():
    ctx.decode_fields_device([dev[k].data_ptr() for k in KEYS], 1, FRAMES, [out.data_ptr()])


def run_signals():
    ctx.decode_signals_device(offsets, units.data_ptr(), out.data_ptr())


def run_push():
    stream.push_fields(one)


CASES = (('fields', run_fields, ('decode_fields',), args.calls), ('signals', run_signals, ('decode', 'signal_starts', 'from_state'), args.calls),
         ('push', run_push, ('decode_fields', 'from_state'), 200))
result = {}
for name, fn, kinds, calls in CASES:
    ms = {m: [] for m in MODELS}
    for m in MODELS:                                         # warm-up: both models, buffers and code objects in place
        set_model(m)
        for _ in range(3):
            fn()
    ctx.synchronize()
    for _ in range(args.rounds):
        for m in MODELS:
            set_model(m)
            fn()
            ctx.synchronize()
            t = time.perf_counter()
            for _ in range(calls):
                fn()
            ctx.synchronize()
            ms[m].append((time.perf_counter() - t) / calls * 1e3)
    for m in MODELS:
        set_model(m)
        ctx.set_profiling(True)
        fn()
        ctx.synchronize()
        split = {k: round(ctx.kernel_ms(k)[0], 4) for k in kinds}
        ctx.set_profiling(False)
        v = sorted(ms[m])
        result['%s_model%d' % (name, m)] = {'median_ms': round(v[len(v) // 2], 4), 'min_ms': round(v[0], 4), 'max_ms': round(v[-1], 4),
                                           'kernel_ms': split}
    if len(MODELS) == 2:
        a, b = (result['%s_model%d' % (name, m)]['median_ms'] for m in MODELS)
        result['%s_ratio_model%d_over_model%d' % (name, MODELS[1], MODELS[0])] = round(b / a, 3)
stream.close()
set_model(0)
ctx.close()
print(json.dumps(result))
