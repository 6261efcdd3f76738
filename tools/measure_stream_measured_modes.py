"""The mode search of the measured allocation: its two kernels, the call against the loop it replaces, and a live stream:
python tools/measure_stream_measured_modes.py [--what sweep,loop,pushes,node] [--reps 200] [--warmup 20] [--parent-lib PATH]

sweep   The "measure" time (c1_ctx_kernel_ms) of k_measured_modes (a wave per unit) and of k_measured_modes_wide (a workgroup per
        unit), forced by C1_MEASURED_WIDE = 0 and 1 on two contexts of one process, for c1_encode_measured_modes_batch over 1, 2, 8,
        32, 128, 256, 512, 1 024, 2 048 and 8 192 mono units of pink noise with transients, in two configurations: two candidates
        at offsets {0}, and eight candidates at the five offsets.  The outputs are compared bit for bit at every count before
        anything is timed.  The contexts alternate; medians of --sweep-reps calls after 3 warm-up calls.  The threshold
        kMeasuredModesWideUnits (csrc/c1_internal.h) is the largest count such that the wide kernel's median is below the narrow
        one's at that count and at every smaller count, in both configurations.
loop    At 256 mono units, eight candidates, five offsets: the whole call (host clock, synchronous) on contexts with the variable
        unset, 0 and 1, against the loop it replaces -- eight measure-only c1_encode_measured_sf_batch calls under the constant
        bytes, the minimum on the host, one final call under the chosen modes -- alternating, medians of --reps after --warmup.
pushes  A stereo stream of pink noise with transients, eight candidates, five offsets, pushes of 1, 8 and 64 frames.  Host clock
        around the call (it synchronises); --warmup pushes, then the median (min - max) of --reps.  Variants, alternating inside
        every round: c1_enc_stream_push_measured_modes on contexts made with C1_MEASURED_WIDE unset, 0 and 1; the plain
        c1_enc_stream_push and c1_enc_stream_push_measured (five offsets) of the same frames; and what a caller had to do before
        the streaming entry point existed: c1_encode_measured_modes_batch over the same frames with a two-frame halo -- with
        --parent-lib, the shared library of the commit before, on that build, in a child process run right after the others.
node    The mono frame closure through Node, frame by frame, with and without measuredModeCandidates."""
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
CAND8 = (0, 48, 8, 56, 2, 50, 10, 58)
CONFIGS = {'two-offset0': ((10, 58), (0,)), 'eight-offsets': (CAND8, OFFSETS)}
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


def fmt(tag, s):
    return '%s %.4f ms (%.4f - %.4f)' % (tag, s['median_ms'], s['min_ms'], s['max_ms'])


def sweep(reps):
    import carta1_amd as c1
    pcm = material(1, max(COUNTS))
    ctxs = {'narrow': context(c1, 0), 'wide': context(c1, 1)}
    result = {}
    try:
        for c in ctxs.values():
            c.set_profiling(True)
        for name, (cand, offsets) in CONFIGS.items():
            rows = []
            for units in COUNTS:
                chans = [pcm[0][:units * 512]]
                ms = {k: [] for k in ctxs}
                outs = {}
                for rep in range(3 + reps):
                    for k in (list(ctxs) if rep % 2 == 0 else list(ctxs)[::-1]):
                        outs[k] = ctxs[k].encode_measured_modes(chans, cand, scale_factor_offsets=offsets, return_distortion=True, return_shifts=True)
                        t, launches = ctxs[k].kernel_ms('measure')
                        if launches != 1:
                            raise SystemExit('%s, %d units: %d measure launches' % (k, units, launches))
                        if rep == 0 and k == list(ctxs)[-1] and not all(
                                np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(outs['narrow'], outs['wide'])):
                            raise SystemExit('%s, %d units: the two kernels differ' % (name, units))
                        if rep >= 3:
                            ms[k].append(t)
                row = {'units': units, 'narrow': spread(ms['narrow']), 'wide': spread(ms['wide'])}
                row['wide_over_narrow'] = row['wide']['median_ms'] / row['narrow']['median_ms']
                rows.append(row)
                print('%-13s %5d units: %s  %s  wide/narrow %.3f' % (name, units, fmt('narrow', row['narrow']), fmt('wide', row['wide']),
                                                                     row['wide_over_narrow']))
            result[name] = rows
    finally:
        for c in ctxs.values():
            c.close()
    threshold = 0
    for i, units in enumerate(COUNTS):                          # the largest count with every smaller one, in both configurations
        if all(rows[i]['wide']['median_ms'] < rows[i]['narrow']['median_ms'] for rows in result.values()):
            threshold = units
        else:
            break
    print('the wide kernel is faster at every count up to %d in both configurations' % threshold)
    print(json.dumps({'sweep': result, 'threshold': threshold}))


def loop(warmup, reps):
    import carta1_amd as c1
    chans = [np.ascontiguousarray(c, dtype=np.float32) for c in material(1, 256)]
    ctxs = {'unset': context(c1, None), 'narrow': context(c1, 0), 'wide': context(c1, 1)}
    from carta1_amd import capi
    lib = capi.load()
    cand, off = np.array(CAND8, dtype=np.uint8), np.array(OFFSETS, dtype=np.int8)
    modes, dist = np.zeros(256, dtype=np.uint8), np.zeros((256, 2), dtype=np.float64)
    opts = c1.EncoderOptions().to_c()
    ptrs = capi.ptr_array([chans[0].ctypes.data])

    def hn(c):
        """eight measure-only calls, the minimum on the host, the final call"""
        fins = []
        for b in CAND8:
            modes.fill(b)
            capi.check(lib.c1_encode_measured_sf_batch(c._h, ptrs, 1, 256, 0, C.byref(opts), modes.ctypes.data, off.ctypes.data, len(off), None,
                                                       None, None, dist.ctypes.data, None))
            fins.append(np.where(dist[:, 1] < dist[:, 0], dist[:, 1], dist[:, 0]))
        modes[:] = cand[np.argmin(np.stack(fins, axis=1), axis=1)]
        return c.encode_measured(chans, modes=modes.reshape(-1, 1), scale_factor_offsets=OFFSETS)[0]

    ms = {k: [] for k in list(ctxs) + ['loop']}
    try:
        want = hn(ctxs['unset'])
        for k, c in ctxs.items():
            if not np.array_equal(c.encode_measured_modes(chans, CAND8, scale_factor_offsets=OFFSETS)[0], want):
                raise SystemExit('%s: the call and the loop give different units' % k)
        for i in range(warmup + reps):
            order = list(ms) if i % 2 == 0 else list(ms)[::-1]
            for k in order:
                t0 = time.perf_counter()
                if k == 'loop':
                    hn(ctxs['unset'])
                else:
                    ctxs[k].encode_measured_modes(chans, CAND8, scale_factor_offsets=OFFSETS)
                t1 = time.perf_counter()
                if i >= warmup:
                    ms[k].append((t1 - t0) * 1e3)
    finally:
        for c in ctxs.values():
            c.close()
    row = {k: spread(v) for k, v in ms.items()}
    print('256 mono units, eight candidates, five offsets, whole call: ' + '  '.join(fmt(k, row[k]) for k in row))
    print(json.dumps({'loop': row}))


def halo_calls(lib_path, frames_list, warmup, reps):
    """c1_encode_measured_modes_batch over n frames with a two-frame halo, from the library at lib_path with nothing but ctypes
    (an older build has no newer symbols to bind) -> {n: [ms, ...]}"""
    import carta1_amd as c1
    from carta1_amd import capi
    lib = C.CDLL(lib_path)
    for name in ('c1_ctx_create', 'c1_ctx_destroy', 'c1_encode_measured_modes_batch'):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = capi.SIGNATURES[name]
    ctx = C.c_void_p()
    if lib.c1_ctx_create(0, None, C.byref(ctx)) != 0:
        raise SystemExit('c1_ctx_create failed')
    opts = c1.EncoderOptions().to_c()
    off, cand = np.array(OFFSETS, dtype=np.int8), np.array(CAND8, dtype=np.uint8)
    out = {}
    try:
        for n in frames_list:
            pcm = material(2, min((warmup + reps) * n + 2, 4096 + n + 2))
            units = np.zeros((n * 2, 212), dtype=np.uint8)
            ms = []
            for i in range(warmup + reps):
                at = 2 + (i * n) % 4096
                ptrs = capi.ptr_array([c.ctypes.data + at * 2048 for c in pcm])
                t0 = time.perf_counter()
                rc = lib.c1_encode_measured_modes_batch(ctx, ptrs, 2, n, 2, C.byref(opts), cand.ctypes.data, len(cand), off.ctypes.data, len(off),
                                                        units.ctypes.data, None, None, None, None, None, None)
                t1 = time.perf_counter()
                if rc != 0:
                    raise SystemExit('c1_encode_measured_modes_batch failed: %d' % rc)
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
            streams['measured'] = c1.EncoderStream(ctxs['unset'], 2)
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
                        elif k == 'measured':
                            streams[k].push_measured(part, scale_factor_offsets=OFFSETS)
                        else:
                            streams[k].push_measured_modes(part, CAND8, scale_factor_offsets=OFFSETS)
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
        keys = [k for k in ('plain', 'measured', 'unset', 'narrow', 'wide', 'halo_batch', 'halo_batch_parent_build') if k in row]
        print('%2d stereo frames a push: ' % row['frames'] + '  '.join(fmt(k, row[k]) for k in keys))
    print(json.dumps({'pushes': rows}))


NODE_SCRIPT = """
import { encode, EncoderOptions, BufferPool, SCALE_FACTOR_OFFSETS } from '%s/carta1_amd/js/index.js'
const [warmup, reps] = [%d, %d]
const pcm = new Float32Array(512 * 64)
let s = 12345
for (let i = 0, p = 0; i < pcm.length; i++) { s = (s * 1103515245 + 12345) >>> 0; p = 0.98 * p + 0.05 * (s / 2147483648 - 1); pcm[i] = p }
const out = {}
const measured = { measuredAllocation: true, scaleFactorOffsets: SCALE_FACTOR_OFFSETS }
for (const [tag, how] of [['plain', undefined], ['measured', measured], ['searched', { ...measured, measuredModeCandidates: [0, 48, 8, 56, 2, 50, 10, 58] }]]) {
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
    print('the mono frame closure through Node: ' + '  '.join(fmt(k, v) for k, v in got.items()))
    print(json.dumps({'node': got}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--what', default='sweep,loop,pushes,node')
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
        elif what == 'loop':
            loop(a.warmup, a.reps)
        elif what == 'pushes':
            pushes(a.warmup, a.reps, a.parent_lib)
        elif what == 'node':
            node(a.warmup, a.reps)
        else:
            raise SystemExit('unknown --what ' + what)


if __name__ == '__main__':
    main()
