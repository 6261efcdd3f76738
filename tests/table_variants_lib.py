"""The table-variant fixture (tests/golden/table_variants.json and table_variants_<variant>.bin, written by
tests/golden/gen/gen_table_variants.mjs): the reference run with Math.sin / cos / pow wrapped so that it builds other tables,
as another engine's c1_set_tables() would install them.  One dict of numpy arrays per variant."""
import ctypes as C
import hashlib
import json
import os

import numpy as np

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
FRAMES = 64
_fixture = None


def fixture():
    global _fixture
    if _fixture is None:
        _fixture = json.load(open(os.path.join(G, 'table_variants.json')))
    return _fixture


def names():
    return sorted(fixture()['variants'])


def _h2d(h):
    return np.frombuffer(bytes.fromhex(h), dtype='>f8')[0]


def variant(name):
    """tables (945 float64 in c1_tables order), biased (bias 1), gates, kat {case: meta + units [128, 212] + pcm8 [128, 8]},
    quant (coefs [F, 512], modes [F, 3], nbfu, sfi, wl, quantized) and points (x, sfi, bits, q)"""
    v = dict(fixture()['variants'][name])
    raw = open(os.path.join(G, 'table_variants_%s.bin' % name), 'rb').read()

    def part(key, dtype):
        at, n = v['offsets'][key]
        return np.frombuffer(raw[at:at + n], dtype=dtype).copy()
    v['tables'] = np.array([_h2d(h) for h in v['tables_f64']], dtype=np.float64)
    v['biased'] = np.array([_h2d(h) for h in v['biased_b1_f64']], dtype=np.float64)
    kat = {}
    for case, meta in v['kat'].items():
        kat[case] = dict(meta, units=part('kat_%s_units' % case, np.uint8).reshape(-1, 212),
                         pcm8=part('kat_%s_pcm8' % case, np.uint8).reshape(-1, 8))
    v['kat'] = kat
    F = v['quant_frames']
    flds = part('quant_fields', np.int32).reshape(F, 617)
    v['quant'] = {'coefs': part('quant_coefs', np.float32).reshape(F, 512), 'modes': part('quant_modes', np.int32).reshape(F, 3),
                  'nbfu': flds[:, 0].copy(), 'sfi': flds[:, 1:53].copy(), 'wl': flds[:, 53:105].copy(), 'quantized': flds[:, 105:].copy()}
    v['points'] = {k: part('quantize_' + k, np.float32 if k == 'x' else np.int32) for k in ('x', 'sfi', 'bits', 'q')}
    fx = fixture()
    fft, at = [], 0
    flat = part('stage_fft', np.float32)
    for n, seed in fx['fft_cases']:
        fft.append({'n': n, 'seed': seed, 'real': flat[at:at + n], 'imag': flat[at + n:at + 2 * n]})
        at += 2 * n
    nf = fx['fields_frames']
    v['stages'] = {'mags': part('stage_mags', np.float32).reshape(8, 256), 'fft': fft,
                   'mdct_modes': fx['mdct_modes'], 'mdct': part('stage_mdct', np.float32).reshape(len(fx['mdct_modes']), 4, 512),
                   'decoder_d8': part('stage_decoder_d8', np.uint8).reshape(nf, 3, 8)}
    return v


def fft_w(tables, n):
    """the (cos, sin)(-2 pi / stride) pairs of strides 2 .. n from the c1_tables layout: log2(n) pairs, flattened"""
    w = np.asarray(tables[928:944], dtype=np.float64)
    return np.ascontiguousarray(w[:2 * (int(n).bit_length() - 1)])


def d8(a):
    """the first 8 bytes of the SHA-256 of an array's bytes"""
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest()[:8], np.uint8)


def kat_inputs(case):
    """the case's two channels, float32 [64 * 512] each: gen_golden.mjs's xorshift32 signals (as the oracle makes them)"""
    import oracle_lib as O
    n = FRAMES * 512
    return [O.gen_white(1, n), O.gen_white(2, n)] if case['signal'] == 'white' else [O.gen_pinkT(3, n), O.gen_pinkT(4, n)]


def kat_options(case):
    """(fixed_modes, threshold) as oracle_lib.encode_stream takes them"""
    o = case['options']
    return o.get('fixedBlockModes'), float(o.get('transientThresholdLow', 1.0))


def frame_digests(channels):
    """the first 8 bytes of the SHA-256 of every 512-sample frame, frame by frame, L then R: [frames * channels, 8]"""
    frames = len(channels[0]) // 512
    out = np.zeros((frames * len(channels), 8), np.uint8)
    for f in range(frames):
        for c, x in enumerate(channels):
            out[f * len(channels) + c] = np.frombuffer(hashlib.sha256(np.ascontiguousarray(x[f * 512:(f + 1) * 512], dtype=np.float32).tobytes()).digest()[:8], np.uint8)
    return out


def c_tables(tables):
    """a carta1_amd.capi.Tables holding the 945 doubles"""
    from carta1_amd import capi
    t = capi.Tables()
    C.memmove(C.addressof(t), np.ascontiguousarray(tables, dtype=np.float64).ctypes.data, 945 * 8)
    return t
