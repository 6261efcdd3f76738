"""The coding error of given sound units under the all-long threshold (c1_measure_units_shared_*): the CPU model, composed of
two existing ones, neither of which it changes.

noise, signal and the mode byte every unit is measured under are measure_units_lib.model's.  The weights are
masked_alloc_lib.weights over E0[u, c], the ascending sum of squares (W = 1) of the frame's coefficients under mode byte 0:
best_bias_lib.coefficients under the units rewritten to byte 0, taken in slot order by measured_alloc_lib.bfu_coefficients.  They
do not depend on the unit's bytes.  The totals run in BFU order (cumsum) over the rounded products: include/carta1_hip.h's
definition, line by line."""
import numpy as np

import best_bias_lib as BB
import masked_alloc_lib as MK
import measure_units_lib as MU
import measured_alloc_lib as MA
import pack_model_lib as PM

REL = MU.REL


def all_long_energies(chans, n_units):
    """E0 float64 [n_units, 52]: per BFU the ascending sum of x0[j]^2 over the all-long coefficients of every unit's frame"""
    zero = MU.with_modes(np.zeros((n_units, 212), dtype=np.uint8), np.zeros(n_units, dtype=np.int64))
    coefs = BB.coefficients(chans, zero)                              # reads the units' modes and nothing else
    E0 = np.zeros((n_units, 52))
    for u in range(n_units):
        slots = MA.bfu_coefficients(coefs[u], [0, 0, 0]).astype(np.float64)
        for b in range(52):
            first, n = int(PM.FIRST[b]), int(PM.SPECS[b])
            E0[u, b] = np.cumsum(slots[first:first + n] * slots[first:first + n])[-1]
    return E0


def sums(chans, units, device=False):
    """what does not depend on the tables: measure_units_lib.model's 'noise', 'signal' and 'bytes', and 'E0'"""
    m = MU.model(chans, units, device=device)
    return {'noise': m['noise'], 'signal': m['signal'], 'bytes': m['bytes'], 'E0': all_long_energies(chans, m['noise'].shape[0])}


def with_tables(s, floor, spread):
    """the model over the sums `s` under these tables (the floor is required) -> 'noise', 'signal', 'weights' [U, 52], 'totals'
    [U, 2], 'bytes' [U]"""
    noise, signal = s['noise'], s['signal']
    with np.errstate(all='ignore'):
        P = MK.weights(s['E0'], floor, spread)[0]
        totals = np.stack([np.cumsum(P * noise, axis=1)[:, -1], np.cumsum(P * signal, axis=1)[:, -1]], axis=1)
    return {'noise': noise, 'signal': signal, 'weights': P, 'totals': totals, 'bytes': s['bytes']}


def model(chans, units, floor, spread, device=False):
    return with_tables(sums(chans, units, device), floor, spread)


def gap_db(shared, own):
    """how far the two weights of a BFU lie apart, in dB -> float64, the shape of the inputs"""
    return np.abs(10.0 * np.log10(shared / own))


bitwise = MU.bitwise
close = MU.close
check_outputs = MU.check_outputs
