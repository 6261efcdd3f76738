"""Latency of the measured allocation on a live stream, and the threshold between its two kernels:
python tools/measure_stream_measured.py [--what sweep,pushes,node] [--reps 200] [--warmup 20] [--parent-lib PATH]

sweep   The "measure" time (c1_ctx_kernel_ms) of the one-wave-per-unit kernels and of the workgroup-per-unit kernel
        (k_measured_wide), forced by C1_MEASURED_WIDE = 0 and 1 on two contexts of one process, for the masked whole-buffer call
        with the packaged tables and the offsets 0, -1, 1, -2, -3 over 1, 2, 8, 32, 128, 256, 512, 1 024, 2 048 and 8 192 mono
        units of pink noise with transients.  The contexts alternate; medians of --sweep-reps calls after 3 warm-up calls.  The
        threshold kMeasuredWideUnits (csrc/c1_internal.h) is the largest of these counts at which the wide kernel is faster.
pushes  A stereo stream of pink noise with transients, packaged tables, five offsets, pushes of 1, 8 and 64 frames.  Host clock
        around the call (it synchronises); --warmup pushes, then the median (min - max) of --reps.  Variants, alternating inside
        every round: c1_enc_stream_push_measured on contexts made with C1_MEASURED_WIDE unset, 0 and 1; the plain
        c1_enc_stream_push of the same frames; and what a caller had to do before the streaming entry point existed:
        c1_encode_measured_masked_batch over the same frames with a two-frame halo, on this build and -- with --parent-lib, the
        shared library of the commit before -- on that build, in a child process run right after the others.
node    The mono frame closure through Node, frame by frame, with and without the third argument (tools: node and the addon)."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np

OFFSETS = (0, -1, 1, -2, -3)
COUNTS = (1, 2, 8, 32, 128, 256, 512, 1024, 2048, 8192)
PUSHES = (1, 8, 64)
SEEDS = (11, 12)


def material(nch, frames):
    import oracle_lib as O
    return [O.gen_pinkT(SEEDS[c], frames * 512) for c in range(nch)]


def context(c1, wide):
    old = os.environ.pop('C1_MEASURED_WIDE', None)
    if wide is not None:
        os.environ['C1_MEASURED_WIDE'] = str(wide)
    try:
        return c1.Context(0)
    finally:
        os.environ.pop('C1_MEASURED_WIDE', None)
        if old is not None:
            os.environ['C1_MEASURED_WIDE'] = old


def spread(ms):
    return {'median_ms': float(np.median(ms)), 'min_ms': float(np.min(ms)), 'max_ms': float(np.max(ms)), 'calls': len(ms)}


def sweep(reps):
    import carta1_amd as c1
    pcm = material(1, max(COUNTS))
    ctxs = {'narrow': context(c1, 0), 'wide': context(c1, 1)}
    rows = []
    try:
        for c in ctxs.values():
            c.set_profiling(True)
        for units in COUNTS:
            chans = [pcm[0][:units * 512]]
            ms = {k: [] for k in ctxs}
            outs = {}
            for rep in range(3 + reps):
                for k in (list(ctxs) if rep % 2 == 0 else list(ctxs)[::-1]):
                    outs[k] = ctxs[k].encode_measured(chans, masking=True, scale_factor_offsets=OFFSETS, return_distortion=True)
                    t, launches = ctxs[k].kernel_ms('measure')
                    if launches != 1:
                        raise SystemExit('%s, %d units: %d measure launches' % (k, units, launches))
                    if rep >= 3:
                        ms[k].append(t)
            if not all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(outs['narrow'], outs['wide'])):
                raise SystemExit('%d units: the two kernels differ' % units)
            row = {'units': units, 'narrow': spread(ms['narrow']), 'wide': spread(ms['wide'])}
            row['wide_over_narrow'] = row['wide']['median_ms'] / row['narrow']['median_ms']
            rows.append(row)
            print('%5d units: narrow %.4f ms (%.4f - %.4f)  wide %.4f ms (%.4f - %.4f)  wide/narrow %.3f' % (
                units, row['narrow']['median_ms'], row['narrow']['min_ms'], row['narrow']['max_ms'], row['wide']['median_ms'],
                row['wide']['min_ms'], row['wide']['max_ms'], row['wide_over_narrow']))
    finally:
        for c in ctxs.values():
            c.close()
    faster = [r['units'] for r in rows if r['wide']['median_ms'] < r['narrow']['median_ms']]
    print('the wide kernel is faster at: %s -> threshold %d' % (faster or 'no count', max(faster) if faster else 0))
    print(json.dumps({'sweep': rows, 'threshold': max(faster) if faster else 0}))


def halo_calls(lib_path, frames_list, warmup, reps):
    """c1_encode_measured_masked_batch over n frames with a two-frame halo, from the library at lib_path with nothing but ctypes
    (an older build has no newer symbols to bind) -> {n: [ms, ...]}"""
    import carta1_amd as c1
    from carta1_amd import capi
    lib = C.CDLL(lib_path)
    for name in ('c1_ctx_create', 'c1_ctx_destroy', 'c1_encode_measured_masked_batch'):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = capi.SIGNATURES[name]
    ctx = C.c_void_p()
    if lib.c1_ctx_create(0, None, C.byref(ctx)) != 0:
        raise SystemExit('c1_ctx_create failed')
    opts = c1.EncoderOptions().to_c()
    floor, spread_ = (np.ascontiguousarray(a) for a in c1.MASKING_DEFAULT)
    off = np.array(OFFSETS, dtype=np.int8)
    out = {}
    try:
        for n in frames_list:
            total = (warmup + reps) * n + 2
            pcm = material(2, min(total, 4096 + n + 2))
            units = np.zeros((n * 2, 212), dtype=np.uint8)
            ms = []
            for i in range(warmup + reps):
                at = 2 + (i * n) % 4096
                ptrs = capi.ptr_array([c.ctypes.data + at * 2048 for c in pcm])
                t0 = time.perf_counter()
                rc = lib.c1_encode_measured_masked_batch(ctx, ptrs, 2, n, 2, C.byref(opts), None, off.ctypes.data, len(off), floor.ctypes.data,
                                                         spread_.ctypes.data, units.ctypes.data, None, None, None, None, None)
                t1 = time.perf_counter()
                if rc != 0:
                    raise SystemExit('c1_encode_measured_masked_batch failed: %d' % rc)
                if i >= warmup:
                    ms.append((t1 - t0) * 1e3)
            out[n] = ms
    finally:
        lib.c1_ctx_destroy(ctx)
    return out


def pushes(warmup, reps, parent_lib):
    import carta1_amd as c1
    from carta1_amd import capi
    ctxs = {'unset': context(c1, None), 'narrow': context(c1, 0), 'wide': context(c1, 1)}
    rows = []
    try:
        for n in PUSHES:
            pcm = material(2, 4096 + n)
            streams = {k: c1.EncoderStream(c, 2) for k, c in ctxs.items()}
            streams['plain'] = c1.EncoderStream(ctxs['unset'], 2)
            ms = {k: [] for k in streams}
            try:
                for i in range(warmup + reps):
                    at = (i * n) % 4096
                    part = [c[at * 512:(at + n) * 512] for c in pcm]
                    order = list(streams) if i % 2 == 0 else list(streams)[::-1]
                    for k in order:
                        t0 = time.perf_counter()
                        if k == 'plain':
                            streams[k].push(part)
                        else:
                            streams[k].push_measured(part, scale_factor_offsets=OFFSETS, masking=True)
                        t1 = time.perf_counter()
                        if i >= warmup:
                            ms[k].append((t1 - t0) * 1e3)
            finally:
                for s in streams.values():
                    s.close()
            row = {'frames': n, 'channels': 2}
            row.update({k: spread(v) for k, v in ms.items()})
            row['halo_batch'] = spread(halo_calls(capi.LIB_PATH, [n], warmup, reps)[n])
            rows.append(row)
    finally:
        for c in ctxs.values():
            c.close()
    if parent_lib:                                          # a process of its own: one library of that name per process
        child = subprocess.run([sys.executable, os.path.abspath(__file__), '--what', 'halo-child', '--lib', parent_lib, '--warmup', str(warmup),
                                '--reps', str(reps)], stdout=subprocess.PIPE, universal_newlines=True, timeout=600)
        if child.returncode != 0:
            raise SystemExit('the child on the parent build failed:\n' + child.stdout)
        parent = json.loads(child.stdout.strip().splitlines()[-1])
        for row in rows:
            row['halo_batch_parent_build'] = spread(parent[str(row['frames'])])
    for row in rows:
        fmt = lambda k: '%s %.3f ms (%.3f - %.3f)' % (k, row[k]['median_ms'], row[k]['min_ms'], row[k]['max_ms'])
        keys = [k for k in ('plain', 'unset', 'narrow', 'wide', 'halo_batch', 'halo_batch_parent_build') if k in row]
        print('%2d stereo frames a push: ' % row['frames'] + '  '.join(fmt(k) for k in keys))
        print('   measured over plain %.2fx; wide over narrow %.3f' % (row['unset']['median_ms'] / row['plain']['median_ms'],
                                                                       row['wide']['median_ms'] / row['narrow']['median_ms']))
    print(json.dumps({'pushes': rows}))


NODE_SCRIPT = """
import { encode, EncoderOptions, BufferPool, SCALE_FACTOR_OFFSETS } from '%s/carta1_amd/js/index.js'
const [warmup, reps] = [%d, %d]
const pcm = new Float32Array(512 * 64)
let s = 12345
for (let i = 0, p = 0; i < pcm.length; i++) { s = (s * 1103515245 + 12345) >>> 0; p = 0.98 * p + 0.05 * (s / 2147483648 - 1); pcm[i] = p }
const out = {}
for (const [tag, how] of [['plain', undefined], ['measured', { measuredAllocation: true, scaleFactorOffsets: SCALE_FACTOR_OFFSETS, masking: true }]]) {
  const enc = encode(new EncoderOptions(), new BufferPool(), how)
  const ms = []
  for (let i = 0; i < warmup + reps; i++) {
    const x = pcm.subarray((i %% 64) * 512, (i %% 64 + 1) * 512).slice()
    const t0 = process.hrtime.bigint()
    enc(x)
    const t1 = process.hrtime.bigint()
    if (i >= warmup) ms.push(Number(t1 - t0) / 1e6)
  }
  out[tag] = ms
}
console.log(JSON.stringify(out))
"""


def node(warmup, reps):
    import shutil
    import tempfile
    from carta1_amd import build
    exe = shutil.which('node')
    if exe is None or build.build_addon() is None:
        print('node: not measured (node or the addon is missing)')
        return
    with tempfile.NamedTemporaryFile('w', suffix='.mjs', delete=False) as f:
        f.write(NODE_SCRIPT % (ROOT, warmup, reps))
    try:
        p = subprocess.run([exe, f.name], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=600)
    finally:
        os.unlink(f.name)
    if p.returncode != 0:
        raise SystemExit('node failed:\n' + p.stdout)
    got = {k: spread(v) for k, v in json.loads(p.stdout.strip().splitlines()[-1]).items()}
    print('the mono frame closure through Node: ' + '  '.join('%s %.3f ms (%.3f - %.3f)' % (k, v['median_ms'], v['min_ms'], v['max_ms'])
                                                            for k, v in got.items()))
    print(json.dumps({'node': got}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--what', default='sweep,pushes,node')
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--sweep-reps', type=int, default=15)
    ap.add_argument('--parent-lib', default=None, help='libcarta1_hip.so of the commit before, for the halo workaround on that build')
    ap.add_argument('--lib', default=None)
    a = ap.parse_args()
    if a.what == 'halo-child':
        print(json.dumps({str(k): v for k, v in halo_calls(a.lib, PUSHES, a.warmup, a.reps).items()}))
        return
    for what in a.what.split(','):
        if what == 'sweep':
            sweep(a.sweep_reps)
        elif what == 'pushes':
            pushes(a.warmup, a.reps, a.parent_lib)
        elif what == 'node':
            node(a.warmup, a.reps)
        else:
            raise SystemExit('unknown --what ' + what)


if __name__ == '__main__':
    main()
