"""Material, metrics and bounds that pin the binary32 decoder (k_decode<float>, c1_ctx_set_decode_precision(ctx, 1)).

The decoder is linear in the dequantized coefficients for given block modes, so it is pinned by its response to every
basis vector: one sound unit per coefficient slot, followed by two silent units, under each of the eight mode triples, at
three levels, with the silent units under the same or the complementary triple.  Beside that: arbitrary bytes and crafted
units whose mantissas run past the 212 bytes (the slow dequantize branch), random frame fields, and encoded pink noise
from full scale down to 1e-6 of it.

The yardstick is the binary32 twin of the oracle's decoder (oracle/atrac1_oracle_f32.c): what binary32 costs this decoder
in the reference's own operation order.  TWIN holds the twin's measured ceilings against the oracle on exactly this
material, in units of u = 2^-24; tests/test_decode32_model_cpu.py re-measures them.  The device bound is GPU_FACTOR x TWIN:
the kernel sums in another order (radix-4, packed, FMA), so its single errors differ from the twin's though not in size.
No bound here comes from the kernel's own output."""
import ctypes as C
import os
import subprocess

import numpy as np

import oracle_lib as O

U = 2.0 ** -24
# the twin's ceilings against the oracle, in u: per basis response (max / peak, relative RMS), per stream (frame max /
# local peak, relative RMS)
TWIN = {'basis_max': 35, 'basis_rms': 19, 'frame_max': 18, 'stream_rms': 6}
GPU_FACTOR = 4
GPU = {k: GPU_FACTOR * v for k, v in TWIN.items()}          # 140 u, 76 u, 72 u, 24 u

TRIPLES = [(a, b, c) for a in (0, 2) for b in (0, 2) for c in (0, 3)]
LEVELS = [(1, 1, 1), (30, 7, 100), (63, 15, -32767)]       # (scale factor index, word length index, mantissa)
FOLLOWERS = ('same', 'complement')
SLOTS = 512
SPECS = np.array([8, 8, 8, 8, 4, 4, 4, 4, 8, 8, 8, 8, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6, 7, 7, 7, 7, 9, 9, 9, 9, 10, 10, 10, 10,
                  12, 12, 12, 12, 12, 12, 12, 12, 20, 20, 20, 20, 20, 20, 20, 20])
WL_BITS = np.array([0, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16])
BFU_AMOUNTS = np.array([20, 28, 32, 36, 40, 44, 48, 52])
BFU_OF_SLOT = np.repeat(np.arange(52), SPECS)              # slot = index of the mantissa in bit-stream order
UNIT_BITS = 212 * 8
FIELD_INTS = 620                                            # c1o_fields: nbfu, modes[3], wl[52], sfi[52], q[512]

TWIN_SO = os.path.join(O.ODIR, '_build', 'libatrac1_oracle_f32.so')
_twin = None


def twin():
    """the binary32 twin of the oracle.  Only c1o_pack_unit, c1o_unpack_unit, c1o_decode_frame and c1o_decode_stream keep
    their ABI in it (no double in their arguments); the stream decoder is all that is used, so it is all that is bound."""
    global _twin
    if _twin is None:
        srcs = [os.path.join(O.ODIR, f) for f in ('atrac1_oracle_f32.c', 'atrac1_oracle.c', 'atrac1_oracle.h', 'c1o_tables.inc', 'Makefile')]
        if not os.path.exists(TWIN_SO) or any(os.path.getmtime(s) > os.path.getmtime(TWIN_SO) for s in srcs):
            subprocess.check_call(['make', '-s', '-C', O.ODIR])
        _twin = C.CDLL(TWIN_SO)
        fp = C.POINTER(C.c_float)
        _twin.c1o_decode_stream.argtypes = [C.POINTER(C.c_uint8), C.c_int, C.c_long, C.POINTER(O.DecState), C.POINTER(fp)]
    return _twin


def decode(lib, units, nch=1):
    """c1o_decode_stream of `lib` (O.lib() or twin()) from a zero state: a list of float32 arrays"""
    units = np.ascontiguousarray(units, dtype=np.uint8).reshape(-1, 212)
    frames = units.shape[0] // nch
    st = (O.DecState * nch)()
    outs = [np.zeros(frames * 512, dtype=np.float32) for _ in range(nch)]
    ptrs = (C.POINTER(C.c_float) * nch)(*[o.ctypes.data_as(C.POINTER(C.c_float)) for o in outs])
    lib.c1o_decode_stream(units.ctypes.data_as(C.POINTER(C.c_uint8)), nch, frames, st, ptrs)
    return outs


# ---- material ---------------------------------------------------------------------------------------------------------

def pack_rows(rows):
    """rows: int32 [n, 620] laid out as c1o_fields -> units uint8 [n, 212], packed by the oracle"""
    rows = np.ascontiguousarray(rows, dtype=np.int32)
    assert rows.ndim == 2 and rows.shape[1] == FIELD_INTS and FIELD_INTS * 4 == C.sizeof(O.Fields)
    units = np.zeros((rows.shape[0], 212), dtype=np.uint8)
    lib, src, dst = O.lib(), rows.ctypes.data, units.ctypes.data
    for i in range(rows.shape[0]):
        lib.c1o_pack_unit(C.cast(src + i * FIELD_INTS * 4, C.POINTER(O.Fields)), C.cast(dst + i * 212, C.POINTER(C.c_uint8)))
    return units


def complement(triple):
    """each band's mode flipped between long and short"""
    return (2 - triple[0], 2 - triple[1], 3 - triple[2])


def silent_unit(triple):
    row = np.zeros((1, FIELD_INTS), dtype=np.int32)
    row[0, 0] = 20
    row[0, 1:4] = triple
    return pack_rows(row)[0]


_batches = {}


def basis_batch(triple, level, follower='same', order=None):
    """units uint8 [3 * 512, 212]: for every slot (in `order`, ascending by default) one unit of 52 BFUs in which only the
    slot's BFU has a word length and a scale factor and only the slot a mantissa, then two silent units (nBfu 20, every word
    length 0) under the same or the complementary triple.  Response k is frames 3k and 3k + 1; frame 3k + 2 is silence."""
    key = (tuple(triple), tuple(level), follower)
    if key not in _batches:
        sfi, wl, q = level
        rows = np.zeros((SLOTS, FIELD_INTS), dtype=np.int32)
        s = np.arange(SLOTS)
        rows[:, 0] = 52
        rows[:, 1:4] = triple
        rows[s, 4 + BFU_OF_SLOT] = wl
        rows[s, 56 + BFU_OF_SLOT] = sfi
        rows[s, 108 + s] = q
        units = np.zeros((SLOTS, 3, 212), dtype=np.uint8)
        units[:, 0] = pack_rows(rows)
        units[:, 1:] = silent_unit(triple if follower == 'same' else complement(triple))
        units.setflags(write=False)
        _batches[key] = units
    units = _batches[key]
    if order is not None:
        units = units[np.asarray(order)]
    return np.ascontiguousarray(units.reshape(-1, 212))


def basis_cases():
    """the 48 batches: (triple, level, follower)"""
    return [(t, l, f) for t in TRIPLES for l in LEVELS for f in FOLLOWERS]


def random_units(count=4096, seed=20):
    """arbitrary bytes.  Uniform bytes leave one unit in seven within its 1696 bits (most of those with 20 BFUs), so the three
    bits of the BFU amount are the larger of two draws: more than nine in ten then ask for more mantissa bits than they hold"""
    rng = np.random.default_rng(seed)
    units = rng.integers(0, 256, (count, 212), dtype=np.uint8)
    amount = np.maximum(units[:, 1] >> 5, rng.integers(0, 8, count, dtype=np.uint8))
    units[:, 1] = (units[:, 1] & 0x1f) | (amount << 5)
    return units


def overrun_units(seed=21):
    """crafted overruns: 52 BFUs, every word length 15, random mantissa bytes (the last three included, which no packer
    writes); unit 64 t + s carries scale factor index s in every BFU under triple t.  [512, 212]"""
    rng = np.random.default_rng(seed)
    rows = np.zeros((8 * 64, FIELD_INTS), dtype=np.int32)
    rows[:, 0] = 52
    rows[:, 1:4] = np.repeat(np.array(TRIPLES, dtype=np.int32), 64, axis=0)
    rows[:, 56:108] = np.tile(np.arange(64, dtype=np.int32), 8)[:, None]
    units = pack_rows(rows)                                   # the oracle's packer writes without bounds: word lengths by hand
    units[:, 2:28] = 0xff                                     # 52 four-bit word lengths from bit 16
    first = (16 + 52 * 10) // 8                               # the mantissas start at bit 536 = byte 67
    units[:, first:] = rng.integers(0, 256, (units.shape[0], 212 - first), dtype=np.uint8)
    return units


def random_field_units(frames=1024, seed=22):
    """frame fields drawn as the stage tests' random_fields draws them, restricted to what a sound unit can carry (nBfu of
    the eight amounts, mode codes 0..3 per band, at most 1672 bits), packed by the oracle: wide word lengths, any scale factor,
    extreme mantissas"""
    rng = np.random.default_rng(seed)
    rows = np.zeros((frames, FIELD_INTS), dtype=np.int32)
    nbfu = rng.choice(BFU_AMOUNTS, frames)
    rows[:, 0] = nbfu
    rows[:, 1:3] = rng.choice(np.array([0, 0, 0, 1, 2, -1], dtype=np.int32), (frames, 2))     # 2 - code
    rows[:, 3] = rng.choice(np.array([0, 0, 0, 1, 2, 3], dtype=np.int32), frames)             # 3 - code
    wl = rng.integers(0, 16, (frames, 52))
    wl[rng.random((frames, 52)) < 0.25] = 0
    sfi = rng.integers(0, 64, (frames, 52))
    unread = np.arange(52)[None, :] >= nbfu[:, None]
    wl[unread] = 0
    sfi[unread] = 0
    for b in range(51, -1, -1):                               # the oracle's packer writes without bounds: drop word lengths from
        over = 16 + 10 * nbfu + (WL_BITS[wl] * SPECS).sum(axis=1) > UNIT_BITS - 24         # the top until the unit fits
        wl[over, b] = 0
    rows[:, 4:56] = wl
    rows[:, 56:108] = sfi
    q = rng.integers(-(1 << 31), 1 << 31, (frames, 512), dtype=np.int64)
    small = rng.random((frames, 512)) < 0.6
    q[small] = rng.integers(-40000, 40000, int(small.sum()))
    rows[:, 108:] = q.astype(np.int32)
    return pack_rows(rows)


def unit_fields(units):
    """(nbfu [n], modes [n, 3], bits asked for [n]) as the oracle unpacks the units; a unit holds 1696 bits"""
    units = np.ascontiguousarray(units, dtype=np.uint8).reshape(-1, 212)
    nbfu, modes, bits = np.zeros(len(units), np.int64), np.zeros((len(units), 3), np.int64), np.zeros(len(units), np.int64)
    f = O.Fields()
    lib = O.lib()
    for i in range(len(units)):
        lib.c1o_unpack_unit(C.cast(units.ctypes.data + i * 212, C.POINTER(C.c_uint8)), C.byref(f))
        n = f.nbfu
        wl = np.frombuffer(f.wl, dtype=np.int32, count=52)[:n]
        nbfu[i], modes[i] = n, (f.modes[0], f.modes[1], f.modes[2])
        bits[i] = 16 + 10 * n + int((WL_BITS[wl] * SPECS[:n]).sum())
    return nbfu, modes, bits


LEVEL_SCALES = (1.0, 1e-2, 1e-4, 1e-6)
LEVEL_FRAMES = 256
LEVEL_SETTINGS = {'detect': dict(threshold=0.3), 'short': dict(fixed_modes=(2, 2, 3))}
_levels = None


def level_signal(seed, frames=LEVEL_FRAMES):
    """gen_pinkT, its last 48 frames replaced by three steady tones (1, 8 and 15 kHz: one per QMF band) of which every fourth
    frame one, or the lower two, is four times as loud for 128 samples.  At threshold 0.3 the detector switches the pink
    noise's bands together, nearly always all three; the tail supplies the triples in which one band alone is short."""
    x = O.gen_pinkT(seed, frames * 512).astype(np.float64)
    t = np.arange(TAIL_FRAMES * 512)
    tones = [a * np.sin(2 * np.pi * hz / 44100.0 * t) for a, hz in TAIL_TONES]
    for k, f in enumerate(range(4, TAIL_FRAMES, 4)):
        at = f * 512 + 200
        for band in TAIL_STEPS[k % len(TAIL_STEPS)]:
            tones[band][at:at + 128] *= 4.0
    x[(frames - TAIL_FRAMES) * 512:] = sum(tones)
    return x


TAIL_FRAMES = 48
TAIL_TONES = ((0.2, 1000.0), (0.05, 8000.0), (0.05, 15000.0))
TAIL_STEPS = ((1,), (2,), (0,), (0, 1))


def level_streams():
    """{(scale, setting, channels): units}: level_signal at each scale, encoded by the oracle under detection at threshold 0.3
    and under fixed short blocks, mono (seed 3) and stereo (seeds 3 and 4).  A scale that encodes to silence is dropped."""
    global _levels
    if _levels is None:
        _levels = {}
        base = [level_signal(3), level_signal(4)]
        for scale in LEVEL_SCALES:
            chs = [(x * scale).astype(np.float32) for x in base]
            for name, kw in LEVEL_SETTINGS.items():
                for nch in (1, 2):
                    units, _ = O.encode_stream(chs[:nch], **kw)
                    if any(np.any(p) for p in decode(O.lib(), units, nch)):
                        units.setflags(write=False)
                        _levels[(scale, name, nch)] = units
    return _levels


# ---- metrics, in units of u ---------------------------------------------------------------------------------------------

def basis_metrics(got, ref):
    """got, ref: the decoded PCM of a basis batch, float32 [3 * 512 * 512].  Returns per response (max|got - ref| / peak(ref),
    relative RMS over the response's two frames), both in u, peak(ref), and the largest |sample| of each third frame of got"""
    g = np.asarray(got, dtype=np.float64).reshape(SLOTS, 3, 512)
    r = np.asarray(ref, dtype=np.float64).reshape(SLOTS, 3, 512)
    d = (g - r)[:, :2].reshape(SLOTS, -1)
    rr = r[:, :2].reshape(SLOTS, -1)
    peak = np.abs(rr).max(axis=1)
    energy = (rr * rr).sum(axis=1)
    with np.errstate(divide='ignore', invalid='ignore'):
        m = np.abs(d).max(axis=1) / peak / U
        e = np.sqrt((d * d).sum(axis=1) / energy) / U
    return m, e, peak, np.abs(g[:, 2]).max(axis=1)


def stream_metrics(got, ref):
    """got, ref: one channel of decoded PCM.  Returns (per frame f: max|got - ref| over f / the larger of ref's peaks in f
    and f - 1, in u, 0 where both peaks are zero; the stream's relative RMS in u; the number of samples of got that are not
    exactly zero in frames where both peaks are zero)"""
    g = np.asarray(got, dtype=np.float64).reshape(-1, 512)
    r = np.asarray(ref, dtype=np.float64).reshape(-1, 512)
    d = g - r
    peak = np.abs(r).max(axis=1)
    local = np.maximum(peak, np.concatenate([[0.0], peak[:-1]]))
    quiet = local == 0
    per = np.zeros(len(g))
    per[~quiet] = np.abs(d[~quiet]).max(axis=1) / local[~quiet] / U
    energy = (r * r).sum()
    rel = float(np.sqrt((d * d).sum() / energy) / U) if energy > 0 else 0.0
    return per, rel, int(np.count_nonzero(g[quiet]))
