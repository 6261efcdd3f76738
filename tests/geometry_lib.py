"""How the frame-walking kernels lay out their work, restated from the sources for the tests (test_geometry_cpu.py,
test_gpu_geometry.py): the run length of c1k_pick_run (c1_internal.h), the workgroup permutation spread_block
(c1_k_spec.hip) and the slot arrays the speculative path keeps in d_redo (c1_api.hip: ensure_workspace, bind_lists,
bind_defer, the open_masks placement).  The constants are read from the sources, not copied."""
import hashlib
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'carta1_amd', 'csrc')
INTERNAL_H = os.path.join(CSRC, 'c1_internal.h')
API = os.path.join(CSRC, 'c1_api.hip')
SPEC = os.path.join(CSRC, 'c1_k_spec.hip')


def _src(path):
    with open(path) as f:
        return f.read()


def _const(path, name):
    m = re.search(r'constexpr\s+(?:int|int64_t)\s+%s\s*=\s*(\d+)\s*;' % name, _src(path))
    assert m, '%s not found in %s' % (name, path)
    return int(m.group(1))


K_RUN_DEFAULT = _const(INTERNAL_H, 'kRunDefault')
K_LIST_HEAD = _const(API, 'kListHead')
K_SPEC_MIN_UNITS = _const(API, 'kSpecMinUnits')


def pick_run_source():
    """the text of c1k_pick_run"""
    m = re.search(r'inline int c1k_pick_run\(int64_t frames, int channels, int slots\) \{\n.*?\n\}\n', _src(INTERNAL_H), re.S)
    assert m, 'c1k_pick_run not found'
    return m.group(0)


def _split_and_floor():
    body = pick_run_source()
    m = re.search(r'units >= \(int64_t\)kRunDefault \* (\d+)\) return kRunDefault;', body)
    n = re.search(r'const int run = \(int\)\(\(units \+ (\d+)\) / (\d+)\);\n\s*return run < (\d+) \? (\d+) : run;', body)
    assert m and n and int(n.group(1)) + 1 == int(n.group(2)) == int(m.group(1)) and n.group(3) == n.group(4), body
    return int(m.group(1)), int(n.group(3))


SPLIT, RUN_FLOOR = _split_and_floor()


def pick_run(frames, channels, forced=0):
    """c1k_pick_run: frames * channels units; `forced` = C1_RUN_FRAMES (0 = unset), clamped to RUN_FLOOR"""
    if forced > 0:
        return max(RUN_FLOOR, forced)
    units = np.asarray(frames, dtype=np.int64) * channels
    run = np.maximum(RUN_FLOOR, -(-units // SPLIT))
    out = np.where(units >= K_RUN_DEFAULT * SPLIT, K_RUN_DEFAULT, run)
    return int(out) if out.ndim == 0 else out


def frames_for_run(run, channels):
    """the frames counts whose batch c1k_pick_run gives `run` (RUN_FLOOR < run < K_RUN_DEFAULT): (first, last)"""
    lo_units, hi_units = SPLIT * (run - 1) + 1, SPLIT * run
    return -(-lo_units // channels), hi_units // channels


# ---- d_redo (c1_api.hip) ---------------------------------------------------------------------------------------

def _redo_layout_constants():
    api = _src(API)
    m = re.search(r'hipMalloc\(&ctx->d_redo\[p\], \(\(size_t\)units \* (\d+) \+ kListHead \+ (\d+)\) \* sizeof\(uint32_t\)\)', api)
    d = re.search(r'L->defer_list = ctx->d_redo\[p\] \+ kListHead \+ (\d+) \* \(size_t\)ctx->ws_units;', api)
    o = re.search(r'ctx->d_redo\[p\] \+ kListHead \+ (\d+) \* \(size_t\)ctx->ws_units \+ \(size_t\)ctx->ws_units / (\d+) \+ (\d+)\) \+ 7\) & ~\(uintptr_t\)7\)', api)
    assert m and d and o, 'd_redo layout changed: restate it here'
    assert d.group(1) == o.group(1)
    return {'per_unit': int(m.group(1)), 'slack': int(m.group(2)), 'defer_at': int(d.group(1)),
            'mask_div': int(o.group(2)), 'mask_pad': int(o.group(3))}


REDO = _redo_layout_constants()


def redo_layout(frames, channels, ws_units, run):
    """uint32 offsets in one d_redo half for a chunk of `frames` frames (numpy arrays broadcast): the deferred-run slots
    [defer_lo, defer_hi), the open-scale-factor masks (one uint64 per slot, 8-byte aligned; hipMalloc's base is) and the
    words allocated.  Returns (fits, defer_hi, mask_lo, mask_hi, words)."""
    f = np.asarray(frames, dtype=np.int64)
    u = np.asarray(ws_units, dtype=np.int64)
    r = np.asarray(run, dtype=np.int64)
    slots = -(-f // r) * channels
    defer_lo = K_LIST_HEAD + REDO['defer_at'] * u
    defer_hi = defer_lo + slots
    mask_lo = defer_lo + u // REDO['mask_div'] + REDO['mask_pad']
    mask_lo = mask_lo + (mask_lo & 1)
    mask_hi = mask_lo + 2 * slots
    words = REDO['per_unit'] * u + K_LIST_HEAD + REDO['slack']
    fits = (defer_hi <= mask_lo) & (mask_hi <= words) & (u >= f * channels)
    return fits, defer_hi, mask_lo, mask_hi, words


# ---- spread_block (c1_k_spec.hip) ------------------------------------------------------------------------------

def _spread_constants():
    m = re.search(r'uint32_t spread_block\(uint32_t b, uint32_t n, int bits\) \{\n(.*?)\n\}\n', _src(SPEC), re.S)
    assert m, 'spread_block not found'
    body = m.group(1)
    mul = re.findall(r'x = \(x \* (0x[0-9A-Fa-f]+)u\) & mask;', body)
    assert 'if (bits < 4) return b;' in body and 'const int sh = (bits >> 1) + 1;' in body and len(mul) == 2, body
    assert body.count('x ^= x >> sh;') == 2 and 'while (x >= n);' in body, body
    return [int(v, 16) for v in mul]


SPREAD_MUL = _spread_constants()


def spread_round(x, bits):
    """one step of spread_block's cycle walk: a permutation of [0, 2^bits) (uint32 arithmetic)"""
    mask = np.uint32((1 << bits) - 1)
    sh = np.uint32((bits >> 1) + 1)
    x = np.asarray(x, dtype=np.uint32)
    x = (x * np.uint32(SPREAD_MUL[0])) & mask
    x ^= x >> sh
    x = (x * np.uint32(SPREAD_MUL[1])) & mask
    x ^= x >> sh
    return x


def spread_block(b, n, bits, table=None):
    """spread_block(b, n, bits) for an array of b < n; `table`: spread_round over [0, 2^bits), if at hand"""
    b = np.asarray(b, dtype=np.uint32)
    if bits < 4:
        return b.copy()
    step = (lambda v: table[v]) if table is not None else (lambda v: spread_round(v, bits))
    x = step(b)
    todo = np.flatnonzero(x >= n)
    while todo.size:
        x[todo] = step(x[todo])
        todo = todo[x[todo] >= n]
    return x


def spread_bits(workgroups):
    """c1k_launch_analysis_spec: ceil(log2(workgroups))"""
    bits = 0
    while (1 << bits) < workgroups:
        bits += 1
    return bits


# ---- the compiled rule ---------------------------------------------------------------------------------------

def pick_run_tool():
    """c1k_pick_run as the sources have it, compiled for the host: `tool <max_units>` writes, for channels 1 then 2 and
    every frames count with frames * channels <= max_units, the run as one byte; C1_RUN_FRAMES is read as in the library"""
    src = pick_run_source()
    k = re.search(r'constexpr int kRunDefault = \d+;', _src(INTERNAL_H)).group(0)
    prog = ('#include <stdint.h>\n#include <stdio.h>\n#include <stdlib.h>\n%s\n%s\n'
            'int main(int argc, char **argv) {\n'
            '  const int64_t max_units = atoll(argv[1]);\n'
            '  for (int ch = 1; ch <= 2; ch++)\n'
            '    for (int64_t f = 1; f * ch <= max_units; f++) { const int r = c1k_pick_run(f, ch, 0); putchar(r < 0 || r > 255 ? 255 : r); }\n'
            '  return 0;\n}\n') % (k, src)
    tag = hashlib.sha256(prog.encode()).hexdigest()[:16]
    out_dir = os.path.join(ROOT, 'oracle', '_build')
    exe = os.path.join(out_dir, 'pick_run_%s' % tag)
    if not os.path.exists(exe):
        os.makedirs(out_dir, exist_ok=True)
        c, tmp = exe + '.cpp', '%s.%d' % (exe, os.getpid())
        with open(c, 'w') as f:
            f.write(prog)
        subprocess.check_call(['g++', '-O1', '-std=c++17', '-o', tmp, c])
        os.replace(tmp, exe)
    return exe


def compiled_runs(max_units, forced=None):
    """{channels: uint8 runs for frames 1 ..} from the compiled c1k_pick_run, with C1_RUN_FRAMES = forced (None: unset)"""
    env = dict(os.environ)
    env.pop('C1_RUN_FRAMES', None)
    if forced is not None:
        env['C1_RUN_FRAMES'] = str(forced)
    raw = np.frombuffer(subprocess.run([pick_run_tool(), str(max_units)], env=env, check=True, capture_output=True).stdout, dtype=np.uint8)
    n1 = max_units
    assert raw.size == n1 + max_units // 2
    return {1: raw[:n1], 2: raw[n1:]}
