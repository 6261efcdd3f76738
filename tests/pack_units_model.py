"""A NumPy model of c1_pack_units, written from the semantics include/carta1_hip.h states for it (serializeFrame,
serialization.js:41-98), and the readers of tests/golden/pack_units.json.

Frame fields are the library's layout: nbfu [F], block_modes [F, 3], sfi / wl [F, 52], quantized [F, 512], int32, any
values (nbfu 0..52).  The model lists every field a frame writes as (bit position, width, value), places the fields' bits
into a bit plane of the whole stream, drops what lies past bit 1696 and zeroes bytes 209..211."""
import json
import os

import numpy as np

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
SPECS = np.array([8, 8, 8, 8, 4, 4, 4, 4, 8, 8, 8, 8] + [6] * 12 + [7] * 4 + [9] * 4 + [10] * 4 + [12] * 8 + [20] * 8, np.int64)
FIRST = np.concatenate([[0], np.cumsum(SPECS)])
BFU_OF_SLOT = np.repeat(np.arange(52), SPECS)
BFU_AMOUNTS = (20, 28, 32, 36, 40, 44, 48, 52)
UNIT_BITS = 212 * 8
KEPT_BITS = 209 * 8                      # bytes 209..211 are zeroed after packing
FIELDS = ('nbfu', 'block_modes', 'sfi', 'wl', 'quantized')
N_FIELDS = 1 + 52 + 52 + 512             # header, word lengths, scale factors, mantissas


def header(nbfu, modes):
    """the 16-bit header: ((2 - m0) << 14) | ((2 - m1) << 12) | ((3 - m2) << 10) | (idx << 5) in wrapping uint32 arithmetic"""
    n = np.asarray(nbfu, np.int64)
    m = np.asarray(modes, np.int64).astype(np.uint32).astype(np.uint64)
    idx = np.full(n.shape, -1, np.int64)
    for i, a in enumerate(BFU_AMOUNTS):
        idx[n == a] = i
    w = lambda x: x & 0xffffffff
    h = (w((2 - m[:, 0]) << 14) | w((2 - m[:, 1]) << 12) | w((3 - m[:, 2]) << 10) | w(idx.astype(np.uint32).astype(np.uint64) << 5))
    return (h & 0xffff).astype(np.int64)


def mantissa_bits(nbfu, wl):
    """WORD_LENGTH_BITS[wl] per BFU, for the BFUs below nbfu; 0 for wl 0, outside 0..15 and at or above nbfu"""
    wl = np.asarray(wl, np.int64)
    live = (np.arange(52)[None, :] < np.asarray(nbfu, np.int64)[:, None]) & (wl >= 1) & (wl <= 15)
    return np.where(live, wl + 1, 0)


def field_table(f):
    """(pos, width, value) [F, N_FIELDS] of every field a frame writes; width 0 for the fields it does not write"""
    n = np.asarray(f['nbfu'], np.int64).reshape(-1)
    F = n.size
    wl = np.asarray(f['wl'], np.int64).reshape(F, 52)
    sfi = np.asarray(f['sfi'], np.int64).reshape(F, 52)
    q = np.asarray(f['quantized'], np.int64).reshape(F, 512)
    assert ((n >= 0) & (n <= 52)).all()
    b = np.arange(52)[None, :]
    below = b < n[:, None]
    bits = mantissa_bits(n, wl)
    start = 16 + 10 * n[:, None] + np.concatenate([np.zeros((F, 1), np.int64), np.cumsum(bits * SPECS, axis=1)[:, :-1]], axis=1)
    sb = bits[:, BFU_OF_SLOT]
    pos = np.concatenate([np.zeros((F, 1), np.int64), 16 + 4 * b + 0 * n[:, None], 16 + 4 * n[:, None] + 6 * b,
                          start[:, BFU_OF_SLOT] + (np.arange(512) - FIRST[BFU_OF_SLOT])[None, :] * sb], axis=1)
    width = np.concatenate([np.full((F, 1), 16), np.where(below, 4, 0), np.where(below, 6, 0), sb], axis=1)
    value = np.concatenate([header(n, f['block_modes']).reshape(F, 1), wl & 15, sfi & 63, q & ((1 << sb) - 1)], axis=1)
    return pos, width, value


def stream_bits(f):
    """length in bits of the stream a frame writes, before truncation"""
    pos, width, _ = field_table(f)
    return (pos + width).max(axis=1)


def pack(f, chunk=2048):
    """uint8 [F, 212]: the units serializeFrame makes of the frame fields"""
    F = int(np.asarray(f['nbfu']).size)
    out = np.zeros((F, 212), np.uint8)
    for a in range(0, F, chunk):
        sub = {k: np.asarray(f[k]).reshape(F, -1)[a:a + chunk] for k in FIELDS}
        pos, width, value = field_table(sub)
        k = np.arange(16)[None, None, :]
        bit = (value[:, :, None] >> np.maximum(width[:, :, None] - 1 - k, 0)) & 1
        at = pos[:, :, None] + k
        keep = (k < width[:, :, None]) & (at < KEPT_BITS) & (bit == 1)
        rows = np.broadcast_to(np.arange(pos.shape[0])[:, None, None], at.shape)
        plane = np.zeros((pos.shape[0], UNIT_BITS), np.uint8)
        plane[rows[keep], at[keep]] = 1
        out[a:a + chunk] = np.packbits(plane, axis=1)
    return out


def canonical_mask(units):
    """uint8 [F, 212]: the bits of each unit that deserializeFrame reads and serializeFrame writes back -- the header's mode
    and BFU-amount bits (value bits 5..7 and 10..15; bits 0..4 and 8..9 are never written), the stream up to its end as the
    unit's own header and word lengths give it, nothing from bit 1672 on"""
    u = np.asarray(units, np.uint8).reshape(-1, 212)
    F = u.shape[0]
    h = (u[:, 0].astype(np.int64) << 8) | u[:, 1]
    n = np.array(BFU_AMOUNTS)[(h >> 5) & 7]
    plane = np.unpackbits(u, axis=1).astype(np.int64)
    wl_pos = 16 + 4 * np.arange(52)
    wl = np.zeros((F, 52), np.int64)
    for j in range(4):
        wl = (wl << 1) | plane[:, wl_pos + j]
    bits = mantissa_bits(n, wl)
    end = np.minimum(16 + 10 * n + (bits * SPECS).sum(axis=1), KEPT_BITS)
    mask = (np.arange(UNIT_BITS)[None, :] < end[:, None]).astype(np.uint8)
    mask[:, :16] = np.array([1 if (15 - i) in (5, 6, 7, 10, 11, 12, 13, 14, 15) else 0 for i in range(16)], np.uint8)
    return np.packbits(mask, axis=1)


def cases():
    """tests/golden/pack_units.json: {name: dict of arrays (the frame fields, units) plus 'meta'}"""
    index = json.load(open(os.path.join(G, 'pack_units.json')))
    out = {}
    for case in index['cases']:
        raw = open(os.path.join(G, case['file']), 'rb').read()
        at, arrays = 0, {}
        for a in case['arrays']:
            dt = np.dtype(a['dtype']).newbyteorder('<')
            n = int(np.prod(a['shape']))
            arrays[a['name']] = np.frombuffer(raw, dtype=dt, count=n, offset=at).reshape(a['shape']).astype(a['dtype'])
            at += n * dt.itemsize
        assert at == len(raw), case['file']
        arrays['meta'] = case
        out[case['name']] = arrays
    return out


def fields_of(case, start=0, stop=None):
    return {k: np.ascontiguousarray(case[k][start:stop]) for k in FIELDS}


EDGES = np.array([0, 1, -1, 2, 3, 5, 7, 15, 16, 19, 20, 21, 31, 52, 53, 63, 64, 127, 32767, -32768, 65535, 65536, -65536,
                  2 ** 31 - 1, -2 ** 31, 2 ** 31 - 2, -2 ** 31 + 1], np.int64)


def random_fields(frames, seed):
    """frame fields from the whole int32 domain, mixed with edge values and with values of the canonical ranges"""
    r = np.random.default_rng(seed)

    def mix(shape, lo, hi):
        full = r.integers(-2 ** 31, 2 ** 31, size=shape, dtype=np.int64)
        edge = EDGES[r.integers(0, EDGES.size, size=shape)]
        small = r.integers(lo, hi, size=shape, dtype=np.int64)
        k = r.integers(0, 4, size=shape)
        return np.where(k == 0, full, np.where(k == 1, edge, small)).astype(np.int32)

    nbfu = np.where(r.integers(0, 3, frames) == 0, np.array(BFU_AMOUNTS)[r.integers(0, 8, frames)], r.integers(0, 53, frames))
    return {'nbfu': nbfu.astype(np.int32), 'block_modes': mix((frames, 3), -1, 4), 'sfi': mix((frames, 52), 0, 64),
            'wl': mix((frames, 52), 0, 16), 'quantized': mix((frames, 512), -32768, 32768)}
