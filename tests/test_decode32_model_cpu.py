"""CPU: the yardstick of the binary32 decoder's tests.  The binary32 twin of the oracle's decoder (oracle/atrac1_oracle_f32.c)
is measured against the oracle on the material of decode32_lib; the four ceilings decode32_lib.TWIN, of which the device bounds
are four times, must hold and must not have become loose; and the material must be what the device tests take it for: every
slot answers under every triple, responses do not overlap, the overrun units overrun, the encoded streams do not, and the level
streams carry all eight mode triples.

Measured (u = 2^-24), twin against oracle: basis responses 34.93 u per sample and 19.02 u RMS (long-block triples; all-short is
9.6 u and 4.2 u); random bytes 17.4 u per frame and 5.77 u RMS; the level sweep at most 17.2 u and 4.29 u.  The figures are
compared with the ceilings at the 0.1 u to which the ceilings were set (19.02 u stands against a ceiling of 19).  The crafted
overruns (16.1 u, 6.77 u: half their bands are long) and the random fields (21.2 u, 6.68 u) are not what the stream ceilings
were set on; the twin must stay within twice the ceilings there, which leaves the device bound a factor of two."""
import numpy as np
import pytest

import decode32_lib as D
import oracle_lib as O


def _both(units, nch=1):
    return D.decode(O.lib(), units, nch), D.decode(D.twin(), units, nch)


@pytest.fixture(scope='module')
def basis():
    """per batch (triple, level, follower): the twin's two metrics per slot, the oracle's peaks and third-frame maxima"""
    out = {}
    for case in D.basis_cases():
        ref, got = _both(D.basis_batch(*case))
        m, e, peak, _ = D.basis_metrics(got[0], ref[0])
        out[case] = (m, e, peak, D.basis_metrics(ref[0], ref[0])[3])
    return out


@pytest.fixture(scope='module')
def streams():
    """{name: [(frame metric, relative RMS, non-zero samples in silence, finite) per channel]} of the twin"""
    out = {}
    material = [('random', D.random_units(), 1), ('overrun', D.overrun_units(), 1), ('fields', D.random_field_units(), 1)]
    material += [('level %g %s %d' % k, u, k[2]) for k, u in D.level_streams().items()]
    for name, units, nch in material:
        ref, got = _both(units, nch)
        out[name] = [D.stream_metrics(got[c], ref[c]) + (bool(np.isfinite(got[c]).all()),) for c in range(nch)]
    return out


def _within(measured, key):
    """the ceiling holds at the 0.1 u it was set to, and is no more than four times what is measured"""
    print('twin %s: %.2f u (ceiling %d u)' % (key, measured, D.TWIN[key]))
    assert round(measured, 1) <= D.TWIN[key], (key, measured)
    assert measured > D.TWIN[key] / 4.0, (key, measured, 'the ceiling has become loose')


def test_the_twin_is_another_arithmetic_and_leaves_the_oracle_alone():
    units = D.basis_batch((0, 2, 3), D.LEVELS[1])
    before = D.decode(O.lib(), units)[0]
    got = D.decode(D.twin(), units)[0]
    after = D.decode(O.lib(), units)[0]
    assert np.array_equal(before.view(np.uint32), after.view(np.uint32))
    assert not np.array_equal(before.view(np.uint32), got.view(np.uint32))
    assert np.array_equal(O.decode_stream(units, 1)[0][0].view(np.uint32), before.view(np.uint32))


def test_basis_material(basis):
    assert len(basis) == 48
    for case, (m, e, peak, third) in basis.items():
        assert peak.shape == (D.SLOTS,) and (peak > 0).all(), (case, 'slots without a response', np.nonzero(peak == 0)[0])
        assert (third == 0).all(), (case, 'responses overlap at slots', np.nonzero(third)[0])


def test_basis_ceilings(basis):
    for t in D.TRIPLES:
        print('triple %s: %.1f u per sample, %.1f u RMS' % (t, max(v[0].max() for k, v in basis.items() if k[0] == t),
                                                           max(v[1].max() for k, v in basis.items() if k[0] == t)))
    _within(max(v[0].max() for v in basis.values()), 'basis_max')
    _within(max(v[1].max() for v in basis.values()), 'basis_rms')


def test_stream_material():
    for name, units, least in (('random', D.random_units(), 0.9), ('overrun', D.overrun_units(), 1.0)):
        _, _, bits = D.unit_fields(units)
        assert (bits > D.UNIT_BITS).mean() >= least, (name, (bits > D.UNIT_BITS).mean())
    assert len(D.random_units()) == 4096
    _, _, bits = D.unit_fields(D.random_field_units())
    assert bits.max() <= D.UNIT_BITS and bits.max() > D.UNIT_BITS - 64
    levels = D.level_streams()
    assert len({k[0] for k in levels}) >= 3, sorted(levels)
    seen = set()
    for k, units in levels.items():
        _, modes, bits = D.unit_fields(units)
        assert bits.max() <= D.UNIT_BITS, k
        seen |= {tuple(int(x != 0) for x in m) for m in modes}
    assert len(seen) == 8, sorted(seen)


def test_stream_ceilings(streams):
    for name, chans in streams.items():
        for c, (per, rel, loud, finite) in enumerate(chans):
            print('%s ch %d: %.1f u per frame, %.2f u RMS' % (name, c, per.max(), rel))
            assert finite and loud == 0, (name, c)
    on = [v for name, chans in streams.items() if name not in ('overrun', 'fields') for v in chans]
    _within(max(v[0].max() for v in on), 'frame_max')
    _within(max(v[1] for v in on), 'stream_rms')
    for name in ('overrun', 'fields'):
        per, rel = streams[name][0][:2]
        assert per.max() <= 2 * D.TWIN['frame_max'] and rel <= 2 * D.TWIN['stream_rms'], (name, per.max(), rel)
