"""The option-domain fixture (tests/golden/option_domain.json, written by tests/golden/gen/gen_option_domain.mjs from the
reference encoder) and a numpy restatement of its input generator.

Inputs and coefficient frames are xorshift32 of a counter and single Float32 roundings, so they are the same bits on
every machine; the fixture records the SHA-256 of each and test_option_domain_cpu.py checks that this module reproduces
all of them."""
import hashlib
import json
import os
import struct

import numpy as np

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
_fixture = None


def fixture():
    """the JSON, with each case's 2-byte unit digests (option_domain_digests.bin) attached as `digests`"""
    global _fixture
    if _fixture is None:
        fx = json.load(open(os.path.join(G, 'option_domain.json')))
        dig = np.fromfile(os.path.join(G, 'option_domain_digests.bin'), dtype=np.uint8).reshape(-1, 2)
        at = 0
        for c in fx['cases']:
            n = c['frames'] * c['channels']
            c['digests'] = dig[at:at + n]
            at += n
        assert at == dig.shape[0]
        _fixture = fx
    return _fixture


def biased(bias):
    """allocationBias's table as the reference built it (64 binary64 values): from the fixture, or for the eight biases
    the package carries, from tests/golden/tables.json"""
    import oracle_lib as O
    for k, v in list(fixture()['biased'].items()) + list(O.golden_tables()['biased_scale_factors_f64'].items()):
        if float(k) == float(bias):
            return np.array([struct.unpack('>d', bytes.fromhex(h))[0] for h in v], dtype=np.float64)
    raise KeyError(bias)


def wave():
    """one period of a piecewise parabola, +-4t(1-t) over each half: the partials' oscillator"""
    k = np.arange(4096)
    t = (k & 2047).astype(np.float32) / np.float32(2048)
    return np.where(k < 2048, np.float32(1), np.float32(-1)) * ((np.float32(4) * t) * (np.float32(1) - t))


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


# ---- gen_option_domain.mjs: hash32, base, key, uni, material (keep in step) ----

M32 = 0xFFFFFFFF


def hash32(x):
    x = np.asarray(x, dtype=np.uint32).copy()
    x ^= x << np.uint32(13)
    x ^= x >> np.uint32(17)
    x ^= x << np.uint32(5)
    x = (x.astype(np.uint64) * 0x2C1B3C6D & M32).astype(np.uint32)
    x ^= x << np.uint32(13)
    x ^= x >> np.uint32(17)
    x ^= x << np.uint32(5)
    return x


def base(seed, stream):
    return int(hash32(((seed * 0x9E3779B1) + (stream * 0x85EBCA77)) & M32))


def key(b, i):
    return hash32((np.asarray(i, dtype=np.uint64) + b) & M32)


def uni(v):
    return ((v >> np.uint32(8)).astype(np.int32) - 8388608).astype(np.float32) * np.float32(2.0 ** -23)


PATCH = [{'kind': 'white', 'exp': -140}, {'kind': 'white', 'exp': -100}, {'kind': 'white', 'exp': -20},
         {'kind': 'white', 'exp': -1}, {'kind': 'white', 'exp': 3}, {'kind': 'pink', 'exp': 0},
         {'kind': 'partials', 'exp': 0}, {'kind': 'partials', 'exp': -30}, {'kind': 'square', 'exp': -2},
         {'kind': 'impulses', 'exp': 0}, {'kind': 'silence'}, {'kind': 'zeros'}]


def material(spec, seed, i0, n):
    """one material over the global sample indices [i0, i0 + n): float32 [n]"""
    i = np.arange(i0, i0 + n, dtype=np.uint64)
    g = np.float32(2.0 ** spec.get('exp', 0))
    kind = spec['kind']
    f32 = np.float32
    if kind == 'white':
        return uni(key(base(seed, 1), i)) * g
    if kind == 'pink':
        acc = np.zeros(n, f32)
        for k in range(8):
            acc = acc + uni(key(base(seed, 2 + k), i >> np.uint64(k))) * f32(0.125)
        burst = ((i >> np.uint64(9)) % 8 == 5) & ((i & np.uint64(511)) >= 256)
        acc = np.where(burst, acc + uni(key(base(seed, 10), i)) * f32(0.75), acc)
        return acc * g
    if kind == 'partials':
        w = wave()
        acc = np.zeros(n, f32)
        for k in range(6):
            inc = int(key(base(seed, 20), k)) % 858993459 + 100000
            ph = int(key(base(seed, 21), k))
            idx = ((ph + i * np.uint64(inc)) & np.uint64(M32)) >> np.uint64(20)
            acc = acc + w[idx.astype(np.int64)] * f32(2.0 ** (-1 - k))
        return acc * g
    if kind == 'square':
        inc = int(key(base(seed, 30), 0)) % 107374182 + 1073742
        ph = int(key(base(seed, 31), 0))
        hi = ((ph + i * np.uint64(inc)) & np.uint64(M32)) >= 0x80000000
        return np.where(hi, -g, g).astype(f32)
    if kind == 'impulses':
        on = (key(base(seed, 40), i) & np.uint32(1023)) < 3
        return np.where(on, uni(key(base(seed, 41), i)) * g, f32(0)).astype(f32)
    if kind == 'silence':
        return np.zeros(n, f32)
    if kind == 'zeros':
        neg = (key(base(seed, 50), i) & np.uint32(1)) != 0
        return np.where(neg, f32(-0.0), f32(0.0)).astype(f32)
    if kind == 'patch':
        bl, bm, bs = base(seed, 60), base(seed, 61), base(seed, 62)
        out = np.zeros(n, f32)
        at, k = 0, 0
        while at < i0 + n:
            ln = (1 + int(key(bl, k)) % 24) * 512
            lo, hi = max(at, i0), min(at + ln, i0 + n)
            if hi > lo:
                out[lo - i0:hi - i0] = material(PATCH[int(key(bm, k)) % len(PATCH)], int(key(bs, k)), lo, hi - lo)
            at += ln
            k += 1
        return out
    raise ValueError(kind)


def inputs(case):
    """the case's channels, float32 [frames * 512] each"""
    return [material(case['material'], case['seed'] + 7919 * c, 0, case['frames'] * 512) for c in range(case['channels'])]


def options(case):
    """(fixed_modes, threshold) as oracle_lib.encode_stream takes them"""
    o = case['options']
    return o.get('fixedBlockModes'), float(o.get('transientThresholdLow', 1.0))


def first_wrong_unit(units, case):
    """index of the first unit whose digest differs from the fixture's, or None"""
    u = np.ascontiguousarray(units, dtype=np.uint8).reshape(-1, 212)
    want = case['digests']
    for k in range(min(len(u), len(want))):
        if hashlib.sha256(u[k].tobytes()).digest()[:2] != want[k].tobytes():
            return k
    return None if len(u) == len(want) else min(len(u), len(want))


def pcm_sha(pcm):
    """decoded PCM hashed as the fixture does: per frame L then R"""
    nch = len(pcm)
    frames = len(pcm[0]) // 512
    return sha(np.stack([np.asarray(p, np.float32).reshape(frames, 512) for p in pcm], axis=1))


# ---- quantizationStage vectors ----

def stage_coefs():
    """the coefficient frames and block modes the fixture gave quantizationStage (gen_option_domain.mjs, keep in step)"""
    import oracle_lib as O
    st = fixture()['stage']
    sf = np.array([O.h2d(h) for h in O.golden_tables()['scale_factors_f64']]).astype(np.float32)
    i = np.arange(512, dtype=np.uint64)
    f32 = np.float32
    out = np.zeros((st['frames'], 512), f32)
    for fr in range(st['frames']):
        b, kind = base(fr, 70), [0, 1, 2, 5, 6, 7][fr % 6]
        u = uni(key(b, i))
        if kind == 0:                                   # one scale factor in every BFU
            out[fr] = u * sf[10 + fr % 50]
        elif kind == 1:                                 # three shared scale factors
            out[fr] = u * sf[np.array([5 + fr % 20, 30 + fr % 20, 55 + fr % 8])[(i >> np.uint64(6)) % 3]]
        elif kind == 2:                                 # a falling spectrum
            out[fr] = u * np.exp2(-(i >> np.uint64(5)).astype(np.float64)).astype(f32)
        elif kind == 5:                                 # every coefficient one scale factor exactly
            out[fr] = np.where(key(b, i) & np.uint32(1), f32(-1), f32(1)) * sf[20 + fr % 40]
        elif kind == 6:                                 # a few BFUs of the low band: budgets saturate
            lo = i[:128]
            out[fr, :128] = np.where(key(b, lo >> np.uint64(3)) & np.uint32(3) == 0, u[:128] * f32(0.5), f32(0))
        else:                                           # two or three coefficients anywhere
            out[fr] = np.where(key(b, i) & np.uint32(255) == 0, uni(key(b, i + np.uint64(512))) * f32(0.25), f32(0))
    return out, np.array(st['block_modes'], dtype=np.int32)


def stage_rows(fields):
    """quantize_frames' (or the oracle's) fields in the fixture's form: nbfu and a digest of every frame"""
    rows = {'nbfu': [int(n) for n in fields['nbfu']], 'fields': []}
    for f in range(len(fields['nbfu'])):
        v = np.concatenate([[fields['nbfu'][f]], fields['sfi'][f], fields['wl'][f], fields['quantized'][f]]).astype(np.int32)
        rows['fields'].append(sha(v)[:8])
    return rows
