"""Reader of tests/golden/export_domain.json + export_domain.bin (made by tests/golden/gen/gen_export_domain.mjs from the
reference's own quantize, dequantize, FFT.fft, qmfAnalysisStage and mdctStage over the whole domain their C entry points
accept), and the input generator it names."""
import hashlib
import json
import os

import numpy as np

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def load():
    index = json.load(open(os.path.join(G, 'export_domain.json')))
    raw = open(os.path.join(G, 'export_domain.bin'), 'rb').read()
    assert hashlib.sha256(raw).hexdigest() == index['bin_sha256'] and len(raw) == 4 * index['bin_words']
    return index, np.frombuffer(raw, dtype='<u4')


def words(bin_, off, n, dtype):
    return bin_[off:off + n].view(np.dtype(dtype).newbyteorder('<')).astype(dtype)


def hash_noise(seed, n, amp):
    """hashNoise of the generator: fround(((h / 2^32) * 2 - 1) * amp), h a murmur3-style mix of i ^ seed (uint32 arithmetic)"""
    h = np.arange(n, dtype=np.uint32) ^ np.uint32(seed)
    h = h * np.uint32(0x9e3779b1)
    h ^= h >> np.uint32(15)
    h = h * np.uint32(0x85ebca77)
    h ^= h >> np.uint32(13)
    return (((h.astype(np.float64) / 4294967296.0) * 2 - 1) * amp).astype(np.float32)


def quantize_cases(index, bin_):
    """(sfi, bits, x, q, mantissas, dequantized) per record"""
    noise = words(bin_, index['dequantize_noise']['words'], index['dequantize_noise']['n'], np.int32)
    for c in index['quantize']:
        m = np.concatenate([words(bin_, c['m'], c['nm'] - noise.size, np.int32), noise])
        yield (c['sfi'], c['bits'], words(bin_, c['x'], c['n'], np.float32), words(bin_, c['q'], c['n'], np.int32), m,
               words(bin_, c['d'], c['nm'], np.float32))


def twiddles(index, n):
    """V8's (cos, sin)(-2 pi / stride) for stride = 2, 4, .., n, as c1_fft takes them"""
    w = []
    for stride, c, s in index['fft_twiddles']:
        if stride <= n:
            w += [np.frombuffer(bytes.fromhex(c), '<f8')[0], np.frombuffer(bytes.fromhex(s), '<f8')[0]]
    return np.array(w, dtype=np.float64)


def stage_pcm(stream):
    x = hash_noise(stream['seed'], stream['frames'] * 512, stream['amp'])
    x[:stream['zero_frames'] * 512] = -0.0
    return x


def h16(a):
    return hashlib.sha256(np.ascontiguousarray(a).astype('<f4').tobytes()).hexdigest()[:16]


def same_f32(got, want):
    """bit for bit, NaN for NaN with any payload"""
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    return (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))
