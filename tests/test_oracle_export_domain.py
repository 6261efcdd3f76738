"""CPU: the oracle's quantize / dequantize (c1o_quantize_bfu, c1o_dequantize_bfu) against the reference's own outputs over
the whole word-length domain (tests/golden/export_domain.json, made by tests/golden/gen/gen_export_domain.mjs): every bit
count 0..32 and the ones outside it the reference gives a meaning (shift count mod 32), specials, half-way points of the
rounding and the ToInt32 wrap.  GPU tests compare kernels with the oracle as a stand-in for the reference, so it must
agree on everything it accepts."""
import ctypes as C

import numpy as np

import export_domain_golden as X
import oracle_lib as O


def test_oracle_quantize_and_dequantize_over_the_domain():
    index, bin_ = X.load()
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int)
    bad = []
    n = 0
    for sfi, bits, x, q, m, d in X.quantize_cases(index, bin_):
        got_q = np.zeros(x.size, dtype=np.int32)
        O.lib().c1o_quantize_bfu(x.ctypes.data_as(fp), x.size, sfi, bits, got_q.ctypes.data_as(ip))
        got_d = np.zeros(m.size, dtype=np.float32)
        O.lib().c1o_dequantize_bfu(m.ctypes.data_as(ip), m.size, sfi, bits, got_d.ctypes.data_as(fp))
        if not np.array_equal(got_q, q):
            bad.append(('quantize', sfi, bits, x[got_q != q][:3], got_q[got_q != q][:3], q[got_q != q][:3]))
        if not X.same_f32(got_d, d).all():
            bad.append(('dequantize', sfi, bits))
        n += 1
    assert n == len(index['quantize']) and {32, 33, -1, 1} <= {c['bits'] for c in index['quantize']}
    assert not bad, (len(bad), bad[:6])
