"""tools/bench_pack_units.py (GPU) -- rate of c1_pack_units (serializeFrame, host pointers, synchronous) on 1 M mono frames, host
to host, and the time of its kernel from c1_ctx_kernel_ms("pack_units").  The fields are c1_unpack_units of channel 0 of the
eleven KAT files, tiled; the result is checked against the units they came from.  Each call moves 2 480 bytes of fields in
and 212 bytes of units out per frame."""
import glob
import os
import sys
import time

import numpy as np
R = os.getcwd(); sys.path[:0] = [R, os.path.join(R, 'tests')]
import carta1_amd as c1
from carta1_amd import capi

frames = int(sys.argv[1]) if len(sys.argv) > 1 else 1 << 20
reps = 3
kat = np.concatenate([np.fromfile(p, dtype=np.uint8).reshape(-1, 2, 212)[:, 0] for p in sorted(glob.glob('tests/golden/kat64_*.units.bin'))])
units = np.ascontiguousarray(np.resize(kat, (frames, 212)))
ctx = c1.Context(0)
lib, h = capi.load(), ctx._h
f = ctx.unpack_units(units)
out = np.zeros((frames, 212), np.uint8)
P = lambda a: a.ctypes.data
args = [P(f[k]) for k, _ in ctx.FIELD_SHAPES]


def call():
    t = time.perf_counter()
    capi.check(lib.c1_pack_units(h, frames, *args, P(out)))
    return time.perf_counter() - t


call()
host = min(call() for _ in range(reps))
assert np.array_equal(out, units), 'c1_pack_units differs from the units the fields came from'
ctx.set_profiling(True)
kms = []
for _ in range(reps):
    call()
    kms.append(ctx.kernel_ms('pack_units')[0])
ctx.set_profiling(False)
rate = lambda s: frames / s / 1e6
print('frames %d mono (best of %d)' % (frames, reps))
print('c1_pack_units (host to host) %8.1f ms  %7.2f M frames/s' % (host * 1e3, rate(host)))
print('k_pack_units (kernel)        %8.3f ms  %7.1f M frames/s' % (min(kms), rate(min(kms) / 1e3)))
ctx.close()
