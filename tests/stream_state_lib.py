"""Stream state in the reference's BufferPool layout (tests/golden/stream_state.json + .bin, gen_stream_state.mjs): the
fixture's blobs, its signals, the foreign-pool recipe, and the CPU oracle run from explicit states (the model the GPU tests
compare against).  States travel as float32 arrays of shape (channels, 483) / (channels, 179): the fields of c1_enc_state /
c1_dec_state (include/carta1_hip.h) back to back, which is also the oracle's struct layout."""
import ctypes as C
import hashlib
import json
import os

import numpy as np

import oracle_lib as O

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'stream_state.json')
BLOBS = os.path.join(HERE, 'golden', 'stream_state.bin')
ENC_FLOATS, DEC_FLOATS = 483, 179
# float offsets of the fields of one state
ENC_FIELDS = {'qmf_low': (0, 46), 'qmf_mid': (46, 46), 'qmf_high': (92, 39), 'mdct_overlap': (131, 96), 'transient_mags': (227, 256)}
DEC_FIELDS = {'qmf_low': (0, 46), 'qmf_mid': (46, 46), 'qmf_high': (92, 39), 'imdct_tail': (131, 48)}
_GEN = {'white': O.gen_white, 'pinkT': O.gen_pinkT}

_fix = None
_bin = None


def fixture():
    global _fix, _bin
    if _fix is None:
        with open(GOLDEN) as f:
            _fix = json.load(f)
        with open(BLOBS, 'rb') as f:
            _bin = f.read()
    return _fix


def blob(ref, dtype=np.uint8):
    fixture()
    return np.frombuffer(_bin[ref[0]:ref[0] + ref[1]], dtype=dtype).copy()


def states(ref, floats):
    return blob(ref, np.float32).reshape(-1, floats)


def units(ref):
    return blob(ref).reshape(-1, 212)


def signal(spec, frames):
    return [_GEN[g](seed, frames * 512) for g, seed in spec]


def oracle_kwargs(oset):
    modes = oset.get('fixedBlockModes')
    return dict(fixed_modes=tuple(modes) if modes is not None else None, bias=oset.get('allocationBias', 1.0),
                threshold=oset.get('transientThresholdLow', 1.0))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- oracle <-> arrays ----
def enc_states_to_oracle(arr):
    arr = np.ascontiguousarray(arr, dtype=np.float32).reshape(-1, ENC_FLOATS)
    st = (O.EncState * arr.shape[0])()
    assert C.sizeof(st) == arr.nbytes
    C.memmove(st, arr.ctypes.data, arr.nbytes)
    return st


def enc_states_from_oracle(st):
    return np.frombuffer(st, dtype=np.float32).reshape(-1, ENC_FLOATS).copy()


def dec_states_to_oracle(arr):
    arr = np.ascontiguousarray(arr, dtype=np.float32).reshape(-1, DEC_FLOATS)
    st = (O.DecState * arr.shape[0])()
    assert C.sizeof(st) == arr.nbytes
    C.memmove(st, arr.ctypes.data, arr.nbytes)
    return st


def dec_states_from_oracle(st):
    return np.frombuffer(st, dtype=np.float32).reshape(-1, DEC_FLOATS).copy()


def oracle_encode(chans, oset, start=None):
    """the oracle's encode_stream from explicit states (None: fresh pools) -> (units, states after)"""
    st = enc_states_to_oracle(start) if start is not None else None
    u, st = O.encode_stream(chans, states=st, **oracle_kwargs(oset))
    return u, enc_states_from_oracle(st)


def oracle_decode(un, nch, start=None):
    st = dec_states_to_oracle(start) if start is not None else None
    pcm, st = O.decode_stream(un, nch, states=st)
    return pcm, dec_states_from_oracle(st)


def oracle_encode_pools(pcm, pools, oset):
    """n independent pools, one frame each (c1o_encode_frame per pool): pcm (n, 512), pools (n, 483)"""
    n = pcm.shape[0]
    u = np.zeros((n, 212), dtype=np.uint8)
    out = np.zeros((n, ENC_FLOATS), dtype=np.float32)
    for i in range(n):
        ui, si = oracle_encode([pcm[i]], oset, pools[i:i + 1])
        u[i] = ui[0]
        out[i] = si[0]
    return u, out


def oracle_decode_pools(un, pools):
    n = un.shape[0]
    pcm = np.zeros((n, 512), dtype=np.float32)
    out = np.zeros((n, DEC_FLOATS), dtype=np.float32)
    for i in range(n):
        p, s = oracle_decode(un[i:i + 1], 1, pools[i:i + 1])
        pcm[i] = p[0]
        out[i] = s[0]
    return pcm, out


def pcm_sha(chans, first_frame, frames):
    """the fixture's pcm_sha256: per frame channel 0 then channel 1, 512 little-endian binary32 each"""
    h = hashlib.sha256()
    for f in range(first_frame, first_frame + frames):
        for c in chans:
            h.update(np.ascontiguousarray(c[f * 512:(f + 1) * 512], dtype='<f4').tobytes())
    return h.hexdigest()


# ---- xorshift32 values in [-1, 1), as the fixture's recipe and the KAT generators draw them ----
def xorshift_values(seed, n):
    s = seed & 0xffffffff
    out = np.empty(n, dtype=np.float64)
    for i in range(n):
        s ^= (s << 13) & 0xffffffff
        s ^= s >> 17
        s ^= (s << 5) & 0xffffffff
        out[i] = s / 4294967296.0 * 2 - 1
    return out.astype(np.float32)


def foreign_enc_state(seed):
    """one c1_enc_state filled in the recipe's order, which is the struct's order"""
    return xorshift_values(seed, ENC_FLOATS).reshape(1, ENC_FLOATS)


def foreign_dec_state(seed):
    """the recipe fills qmfDelays and then EVERY entry of imdctOverlap (256 | 256 | 512); the state keeps the last 16 of each"""
    v = xorshift_values(seed, 131 + 1024)
    ov = v[131:]
    return np.concatenate([v[:131], ov[240:256], ov[496:512], ov[1008:1024]]).reshape(1, DEC_FLOATS)


def random_pools(seed, n, floats):
    """n pools drawn from xorshift32 in [-1, 1), with a denormal and a -0 planted in each field of pool 0"""
    p = xorshift_values(seed, n * floats).reshape(n, floats)
    if n:
        for first, count in (ENC_FIELDS if floats == ENC_FLOATS else DEC_FIELDS).values():
            p[0, first + 1] = np.float32(1e-41)          # a denormal
            p[0, first + count - 2] = np.float32(-0.0)
    return p
