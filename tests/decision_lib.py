"""Reader of tests/golden/decision.json / decision.bin (made by tests/golden/gen/gen_decision.mjs from the reference's own
performFFT, detectTransient, findScaleFactor, allocateBits and Math.log2), and the ctypes binding of tests/model/decision_model.c,
the CPU model of those functions over their general domain.  Test infrastructure; the model is built on demand with gcc into
oracle/_build/."""
import ctypes as C
import json
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, 'tests', 'golden')
SRC = os.path.join(ROOT, 'tests', 'model', 'decision_model.c')
SO = os.path.join(ROOT, 'oracle', '_build', 'libdecision_model.so')
SPECS = np.array([8] * 4 + [4] * 4 + [8] * 4 + [6] * 12 + [7] * 4 + [9] * 4 + [10] * 4 + [12] * 8 + [20] * 8, dtype=np.int32)
START_LONG = np.concatenate([[0], np.cumsum(SPECS)[:-1]]).astype(np.int32)
START_SHORT = np.array([0, 32, 64, 96, 8, 40, 72, 104, 12, 44, 76, 108, 20, 52, 84, 116, 26, 58, 90, 122, 128, 160, 192, 224,
                        134, 166, 198, 230, 141, 173, 205, 237, 150, 182, 214, 246, 256, 288, 320, 352, 384, 416, 448, 480,
                        268, 300, 332, 364, 396, 428, 460, 492], dtype=np.int32)
BAND_OF_BFU = np.array([0] * 20 + [1] * 16 + [2] * 16, dtype=np.int32)

_fixture = None
_lib = None


def fixture():
    """(index, words): the JSON index and the float64 words its [offset, length] pairs point into"""
    global _fixture
    if _fixture is None:
        index = json.load(open(os.path.join(G, 'decision.json')))
        words = np.fromfile(os.path.join(G, 'decision.bin'), dtype='<f8')
        _fixture = (index, words)
    return _fixture


def span(words, r):
    return words[r[0]:r[0] + r[1]]


def table(index, words, bias):
    """the biased scale-factor table the reference built for `bias` (its engine's Math.pow)"""
    at = index['tables'][str(bias)]
    return words[at:at + 64]


def lib(rebuild=False):
    global _lib
    if _lib is None:
        if rebuild or not os.path.exists(SO) or os.path.getmtime(SRC) > os.path.getmtime(SO):
            os.makedirs(os.path.dirname(SO), exist_ok=True)
            subprocess.check_call(['gcc', '-O2', '-fPIC', '-shared', '-std=c11', '-ffp-contract=off', '-fno-fast-math',
                                   '-o', SO, SRC, '-lm'])
        L = C.CDLL(SO)
        dp, fp, i32p, i64p, u8p = (C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_int64),
                                   C.POINTER(C.c_uint8))
        L.dm_log2.argtypes, L.dm_log2.restype = [C.c_double], C.c_double
        L.dm_find_scale_factor.argtypes, L.dm_find_scale_factor.restype = [dp, C.c_int64], C.c_int
        L.dm_perform_fft.argtypes = [dp, C.c_int64, C.c_int, dp, fp, fp, fp]
        L.dm_detect.argtypes, L.dm_detect.restype = [dp, C.c_int64, dp, C.c_int64, C.c_int, C.c_double, C.c_double, dp], C.c_int
        L.dm_allocate.argtypes = [dp, i64p, i32p, i32p, C.c_int, dp, i32p, i32p, i32p, u8p]
        _lib = L
    return _lib


def broken(mode):
    C.c_int.in_dll(lib(), 'dm_broken').value = mode


def _d(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    return a, a.ctypes.data_as(C.POINTER(C.c_double))


LOG1P_10 = 2.3978952727983707      # Math.log1p(10) in V8 (the default tables' log1p_10)


def log2(x):
    return lib().dm_log2(float(x))


def find_scale_factor(values, length=None):
    v, p = _d(values)
    n = v.size if length is None else max(0, min(int(length), v.size))
    return lib().dm_find_scale_factor(p, n)


def perform_fft(x, n, w):
    xv, xp = _d(x if len(x) else [0.0])
    wv, wp = _d(w if len(w) else [0.0])
    re, im, mag = np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros(max(n // 2, 1), np.float32)
    fp = C.POINTER(C.c_float)
    lib().dm_perform_fft(xp, len(x), n, wp, re.ctypes.data_as(fp), im.ctypes.data_as(fp), mag.ctypes.data_as(fp))
    return mag[:n // 2]


def detect(cur, prev, threshold, log1p10=LOG1P_10):
    """(decision, score); prev None = a falsy prevCoeffs"""
    cv, cp = _d(cur if len(cur) else [0.0])
    pv, pp = _d(prev if prev is not None and len(prev) else [0.0])
    score = C.c_double()
    r = lib().dm_detect(cp, len(cur), pp, 0 if prev is None else len(prev), prev is not None, float(threshold), log1p10,
                        C.byref(score))
    return bool(r), score.value


def allocate(bfus, sizes, mb, bsf):
    """bfus: list of 1-D arrays (BFU i's values); sizes: int32 per BFU (| 0 applied) -> (count, wl[52], sfi[52], fallback)"""
    arrs = [np.ascontiguousarray(b, dtype=np.float64).reshape(-1) for b in bfus][:52]
    data = np.concatenate(arrs + [np.zeros(1)])
    off = np.zeros(52, np.int64)
    ln = np.zeros(52, np.int32)
    pos = 0
    for i, a in enumerate(arrs):
        off[i], ln[i] = pos, a.size
        pos += a.size
    sz = np.zeros(52, np.int32)
    sz[:min(len(sizes), 52)] = np.asarray(sizes, dtype=np.int64)[:52].astype(np.int32)
    t, tp = _d(bsf)
    count, fb = C.c_int32(), C.c_uint8()
    wl, sfi = np.zeros(52, np.int32), np.zeros(52, np.int32)
    i32p = C.POINTER(C.c_int32)
    lib().dm_allocate(data.ctypes.data_as(C.POINTER(C.c_double)), off.ctypes.data_as(C.POINTER(C.c_int64)), ln.ctypes.data_as(i32p),
                      sz.ctypes.data_as(i32p), int(mb), tp, C.byref(count), wl.ctypes.data_as(i32p), sfi.ctypes.data_as(i32p),
                      C.byref(fb))
    return count.value, wl, sfi, bool(fb.value)


def alloc_record(index, words, rec):
    """(bfus, sizes, maxBfuCount, table) of one allocateBits record"""
    return [span(words, d) for d in rec['data']], rec['sizes'], rec['mb'], table(index, words, rec['bias'])


def group_into_bfus(coefs, modes):
    """groupIntoBFUs (quantization.js:106-149) of one frame: 52 arrays of SPECS_PER_BFU values (every BFU of the codec lies
    inside its band, so no clipping occurs)"""
    out = []
    for b in range(52):
        start = (START_LONG if modes[BAND_OF_BFU[b]] == 0 else START_SHORT)[b]
        with np.errstate(invalid='ignore'):                      # signalling NaN coefficients stay NaN
            out.append(np.asarray(coefs[start:start + SPECS[b]], dtype=np.float64))
    return out


def same(a, b):
    """bitwise equality of float arrays, every NaN equal to every NaN"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    nan = np.isnan(a) & np.isnan(b)
    return bool(np.all(nan | (a.view(np.uint64) == b.view(np.uint64))))
