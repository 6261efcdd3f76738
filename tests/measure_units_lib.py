"""The coding error of given sound units against their PCM (c1_measure_units_*): the CPU model, built from the oracle alone.

The fields of a unit come from oracle_lib.unpack_unit, the coefficients from best_bias_lib.coefficients under the unit's own block
modes, the dequantized values from c1o_dequantize_bfu (zero where the BFU is at or above nBfu or has word length or index 0).
Per BFU the two sums run with j ascending (cumsum), the weights are masked_alloc_lib.weights over the signal, and the totals run
in BFU order (cumsum) over the rounded products: include/carta1_hip.h's definition, line by line."""
import ctypes as C

import numpy as np

import best_bias_lib as BB
import masked_alloc_lib as MK
import measured_alloc_lib as MA
import oracle_lib as O
import pack_model_lib as PM

REL = MA.REL
DOMAIN_BYTES = [lo | mid << 2 | hi << 4 for lo in (0, 2) for mid in (0, 2) for hi in (0, 3)]


def mode_in_domain(b):
    """what the device entry points make of any mode byte (an int of any sign)"""
    return (b & 0x02) | (b & 0x08) | (0x30 if (b & 0x30) == 0x30 else 0)


def mode_byte(fields):
    """low | mid << 2 | high << 4 of the block modes deserializeFrame reports; negative where a field the encoder never writes
    makes a mode negative"""
    return int(fields.modes[0]) | (int(fields.modes[1]) << 2) | (int(fields.modes[2]) << 4)


def triple(byte):
    return [byte & 3, (byte >> 2) & 3, (byte >> 4) & 3]


def with_modes(units, bytes_):
    """the units with the six mode bits of their first byte rewritten to the block modes of these (in-domain) mode bytes"""
    out = np.array(units, dtype=np.uint8).reshape(-1, 212)
    for u, b in enumerate(np.asarray(bytes_).reshape(-1).tolist()):
        lo, mid, hi = triple(int(b))
        out[u, 0] = ((2 - lo) << 6) | ((2 - mid) << 4) | ((3 - hi) << 2) | (int(out[u, 0]) & 3)
    return out


def model(chans, units, floor=None, spread=None, device=False):
    """chans: the PCM from a zero state; units uint8 [frames * nch, 212] -> dict: 'noise', 'signal', 'weights' float64 [U, 52],
    'totals' float64 [U, 2], 'bytes' int [U] (the mode byte every unit is measured under).  device: a byte outside the domain of
    c1_encode_modes_* is brought into it as the device call does; else it is an error"""
    lib = O.lib()
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int)
    units = np.ascontiguousarray(units, dtype=np.uint8).reshape(-1, 212)
    U = units.shape[0]
    fields = [O.unpack_unit(u) for u in units]
    bytes_ = np.array([mode_byte(f) for f in fields], dtype=np.int64)
    if device:
        bytes_ = np.array([mode_in_domain(int(b)) for b in bytes_], dtype=np.int64)
    assert set(bytes_.tolist()) <= set(DOMAIN_BYTES), 'a unit outside the domain of c1_encode_modes_*'
    coefs = BB.coefficients(chans, with_modes(units, bytes_))      # reads the units' modes and nothing else
    noise, signal = np.zeros((U, 52)), np.zeros((U, 52))
    d = np.zeros(20, dtype=np.float32)
    for u in range(U):
        f, modes = fields[u], triple(int(bytes_[u]))
        slots = MA.bfu_coefficients(coefs[u], modes).astype(np.float64)
        W = MA.weights_of_modes(modes)
        for b in range(52):
            first, n = int(PM.FIRST[b]), int(PM.SPECS[b])
            xb = slots[first:first + n]
            d[:] = 0.0
            if b < f.nbfu and f.wl[b] != 0 and f.sfi[b] != 0:
                q = np.ascontiguousarray(np.array(f.q[first:first + n], dtype=np.int32))
                lib.c1o_dequantize_bfu(q.ctypes.data_as(ip), n, int(f.sfi[b]), int(f.wl[b]) + 1, d.ctypes.data_as(fp))
            t = xb - d[:n].astype(np.float64)
            noise[u, b] = W[b] * np.cumsum(t * t)[-1]
            signal[u, b] = W[b] * np.cumsum(xb * xb)[-1]
    return with_tables({'noise': noise, 'signal': signal, 'bytes': bytes_}, floor, spread)


def with_tables(m, floor=None, spread=None):
    """the model `m` (any tables) of the same units under these tables: noise and signal do not depend on them"""
    noise, signal = m['noise'], m['signal']
    P = np.ones(noise.shape) if floor is None else MK.weights(signal, floor, spread)[0]
    totals = np.stack([np.cumsum(P * noise, axis=1)[:, -1], np.cumsum(P * signal, axis=1)[:, -1]], axis=1)
    return {'noise': noise, 'signal': signal, 'weights': P, 'totals': totals, 'bytes': m['bytes']}


def bitwise(a, b):
    return MK.bitwise(a, b)


def close(got, want):
    """|got - want| <= REL * want everywhere, exact zeros zero, a NaN only where the model has one"""
    got, want = np.asarray(got), np.asarray(want)
    nan = np.isnan(want)
    return (got.shape == want.shape and np.array_equal(np.isnan(got), nan) and bool((np.abs(got - want)[~nan] <= REL * want[~nan]).all())
            and not ((want == 0) & (got != 0)).any())


def check_outputs(m, got):
    """the GPU's outputs (dict of any of noise, signal, totals, weights) against the model `m`: None, or what is wrong"""
    for k, v in got.items():
        if not close(v, m[k]):
            bad = np.argwhere(~(np.abs(v - m[k]) <= REL * m[k]))
            at = tuple(bad[0]) if len(bad) else ()
            return '%s at %r: %r against the model %r' % (k, at, v[at] if at else None, m[k][at] if at else None)
    return None


def random_units(seed, n, domain=True):
    """n units of random bytes; domain: the six mode bits rewritten to a random byte of the domain of c1_encode_modes_*"""
    rs = np.random.RandomState(seed)
    units = rs.randint(0, 256, size=(n, 212)).astype(np.uint8)
    if domain:
        units = with_modes(units, rs.choice(DOMAIN_BYTES, size=n))
    return units
