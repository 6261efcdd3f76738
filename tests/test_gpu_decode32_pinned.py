"""GPU: the binary32 decoder (k_decode<float>) pinned per coefficient, block mode and level.

The decoder is linear in the dequantized coefficients for given block modes, so it is compared with the exact decoder on the
response to every basis vector (decode32_lib: 512 slots x 8 mode triples x 3 levels x 2 followers), at bounds relative to the
response; then on arbitrary bytes and crafted units that take the slow dequantize branch, on random frame fields, and on encoded
material from full scale down to -80 dB, per frame against the local peak.  Every bound is decode32_lib.GPU = 4 x the ceiling of
the oracle's binary32 twin on the same material (tests/test_decode32_model_cpu.py measures those on the CPU): 140 u per sample
and 76 u RMS per response, 72 u per frame and 24 u RMS per stream, u = 2^-24.  None comes from the kernel's own output.  The
exact context must give the oracle's bits on all of it.  Seams (halo, stream pushes, stereo against mono) are bit for bit."""
import ctypes as C

import numpy as np
import pytest

import decode32_lib as D
import oracle_lib as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ctxs():
    """(the exact context, the binary32 context)"""
    import carta1_amd as c1
    exact, b32 = c1.Context(0), c1.Context(0)
    b32.set_decode_precision(True)
    yield exact, b32
    b32.close()
    exact.close()


_ref = {}


def oracle_pcm(key, units, nch=1):
    """the oracle's PCM, computed once per piece of material"""
    if key not in _ref:
        _ref[key] = D.decode(O.lib(), units, nch)
        for p in _ref[key]:
            p.setflags(write=False)
    return _ref[key]


def same(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def check_basis(exact, b32, cases, ref_of, label):
    """the exact context gives the oracle's bits; the binary32 context stays within GPU['basis_max'] and GPU['basis_rms'] of
    every response and leaves every third frame exactly zero.  Returns the worst (per sample, RMS) in u."""
    worst_m, worst_e = (0.0, None), (0.0, None)
    for case in cases:
        units = D.basis_batch(*case)
        ref = ref_of(case, units)
        assert same(exact.decode(units, 1)[0], ref), (label, case, 'the exact decoder differs from the oracle')
        got = b32.decode(units, 1)[0]
        assert np.isfinite(got).all(), (label, case)
        m, e, _, third = D.basis_metrics(got, ref)
        assert (third == 0).all(), (label, case, 'third frame not silent at slots', np.nonzero(third)[0][:8])
        if m.max() > worst_m[0]:
            worst_m = (float(m.max()), (case, 'slot %d' % int(m.argmax())))
        if e.max() > worst_e[0]:
            worst_e = (float(e.max()), (case, 'slot %d' % int(e.argmax())))
    print('%s: %.1f u per sample, %.1f u RMS' % (label, worst_m[0], worst_e[0]))
    assert worst_m[0] <= D.GPU['basis_max'], (label, 'per sample, in u', worst_m)
    assert worst_e[0] <= D.GPU['basis_rms'], (label, 'RMS, in u', worst_e)
    return worst_m[0], worst_e[0]


@pytest.mark.parametrize('triple', D.TRIPLES, ids=['%d%d%d' % t for t in D.TRIPLES])
def test_basis_responses(ctxs, triple):
    exact, b32 = ctxs
    cases = [(triple, level, follower) for level in D.LEVELS for follower in D.FOLLOWERS]
    m, e = check_basis(exact, b32, cases, lambda case, units: oracle_pcm(('basis',) + case, units)[0], 'triple %s' % (triple,))
    assert m > 0 and e > 0                                   # this really is another arithmetic


def test_stereo_channels_equal_their_mono_decodes(ctxs):
    """channel 0: a batch in ascending slot order; channel 1: a batch under another triple in descending order"""
    _, b32 = ctxs
    down = np.arange(D.SLOTS)[::-1]
    for i, t in enumerate(D.TRIPLES):
        level, follower = D.LEVELS[i % 3], D.FOLLOWERS[i % 2]
        left = D.basis_batch(t, level, follower)
        right = D.basis_batch(D.TRIPLES[(i + 3) % 8], D.LEVELS[(i + 1) % 3], D.FOLLOWERS[(i + 1) % 2], order=down)
        stereo = np.ascontiguousarray(np.stack([left, right], axis=1).reshape(-1, 212))
        got = b32.decode(stereo, 2)
        assert same(got[0], b32.decode(left, 1)[0]), (t, 'channel 0')
        assert same(got[1], b32.decode(right, 1)[0]), (t, 'channel 1')


@pytest.mark.parametrize('triple', [(2, 2, 3), (2, 0, 3)], ids=['223', '203'])
def test_seams_are_bit_for_bit_in_binary32(ctxs, triple):
    import carta1_amd as c1
    _, b32 = ctxs
    units = D.basis_batch(triple, D.LEVELS[2], 'complement')
    whole = b32.decode(units, 1)[0]
    for k in (1, 3, 31, 64, 100, 767, len(units) - 1):       # at a basis unit, behind one, and behind a silent unit
        two = np.concatenate([b32.decode(units[:k], 1)[0], b32.decode(units[k - 1:], 1, halo_units=1)[0]])
        assert same(two, whole), (triple, 'two calls split at unit %d' % k)
    stream = c1.DecoderStream(b32, 1)
    try:
        parts, at = [], 0
        for n in (1, 31, 33, len(units) - 65):
            parts.append(stream.push(units[at:at + n])[0])
            at += n
        assert at == len(units)
    finally:
        stream.close()
    assert same(np.concatenate(parts), whole), (triple, 'stream pushes')


def check_stream(exact, b32, name, units, nch=1):
    """the exact context gives the oracle's bits; the binary32 context is finite, silent where the oracle has been silent for
    two frames, within GPU['frame_max'] of the local peak in every frame and within GPU['stream_rms'] over the stream.
    Returns the binary32 PCM."""
    ref = oracle_pcm(name, units, nch)
    ex = exact.decode(units, nch)
    got = b32.decode(units, nch)
    for c in range(nch):
        assert same(ex[c], ref[c]), (name, c, 'the exact decoder differs from the oracle')
        assert np.isfinite(got[c]).all(), (name, c)
        per, rel, loud = D.stream_metrics(got[c], ref[c])
        print('%s ch %d: %.1f u per frame, %.2f u RMS' % (name, c, per.max(), rel))
        assert loud == 0, (name, c, '%d samples where the oracle is silent' % loud)
        assert per.max() <= D.GPU['frame_max'], (name, c, 'frame %d' % int(per.argmax()), float(per.max()))
        assert rel <= D.GPU['stream_rms'], (name, c, rel)
        assert rel > 0, (name, c)
    return got, ref


@pytest.mark.parametrize('name', ['random', 'overrun', 'fields'])
def test_arbitrary_bytes_overruns_and_random_fields(ctxs, name):
    exact, b32 = ctxs
    units = {'random': D.random_units, 'overrun': D.overrun_units, 'fields': D.random_field_units}[name]()
    if name != 'fields':                                     # these take the slow dequantize branch
        assert (D.unit_fields(units)[2] > D.UNIT_BITS).mean() >= 0.9
    check_stream(exact, b32, name, units)


def test_levels(ctxs):
    exact, b32 = ctxs
    levels = D.level_streams()
    assert len({k[0] for k in levels}) >= 3
    for key, units in levels.items():
        got, ref = check_stream(exact, b32, 'level %g %s %d' % key, units, key[2])
        for c in range(key[2]):                              # the absolute limits of test_gpu_decode32, at every level
            d = got[c].astype(np.float64) - ref[c]
            assert np.sqrt(np.mean(d * d)) < 1e-6 and np.abs(d).max() < 1e-5, key


def test_installed_tables(ctxs):
    """the all-long and all-short batches on contexts created under another engine's tables (the `twiddle` variant of
    table_variants_lib: other MDCT tables and window), the oracle set to the same tables: the same bounds"""
    import carta1_amd as c1
    from carta1_amd import capi
    import table_variants_lib as TV
    v = TV.variant('twiddle')
    lib = capi.load()
    t = TV.c_tables(v['tables'])
    exact = b32 = None
    try:
        assert lib.c1_set_tables(C.byref(t)) == 0
        O.set_tables(v['tables'])
        exact, b32 = c1.Context(0), c1.Context(0)
        b32.set_decode_precision(True)
        cases = [(tr, level, 'same') for tr in ((0, 0, 0), (2, 2, 3)) for level in D.LEVELS]
        refs = {case: D.decode(O.lib(), D.basis_batch(*case))[0] for case in cases}
        check_basis(exact, b32, cases, lambda case, units: refs[case], 'twiddle tables')
    finally:
        for c in (exact, b32):
            if c is not None:
                c.close()
        lib.c1_set_tables(None)
        O.set_tables(None)
    units = D.basis_batch(*cases[1])
    assert not same(refs[cases[1]], D.decode(O.lib(), units)[0])     # the variant's tables were really in use
