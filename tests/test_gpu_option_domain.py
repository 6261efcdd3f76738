"""GPU: the library against the reference over the encoder's option domain (tests/golden/option_domain.json, written by
the reference at allocation biases 0 to 5, detection thresholds 0.01 to 2 and four fixed block-mode sets).  Every case is
encoded with the fixture's own biased table in speculation modes 0, 1 and 2, as a whole and as a tail from its halo,
and decoded; the coefficient frames go through quantize_frames at every bias.  Units, PCM and fields are compared with
the reference's hashes; a mismatch names the case and its first wrong unit or frame."""
import ctypes as C

import numpy as np
import pytest

import option_domain_lib as L

pytestmark = pytest.mark.gpu
FX = L.fixture()
BIASES = FX['biases']


@pytest.fixture(scope='module')
def ctx():
    import carta1_amd as c1
    c = c1.Context(0)
    yield c
    c.close()


def options(case):
    import carta1_amd as c1
    return c1.EncoderOptions(case['options'], biased_table=[float(x) for x in L.biased(case['bias'])])


@pytest.mark.parametrize('mode', [0, 1, 2])
@pytest.mark.parametrize('bias', BIASES)
def test_encode_reproduces_every_case(ctx, bias, mode):
    ctx.set_speculation(mode)
    try:
        for c in (c for c in FX['cases'] if c['bias'] == bias):
            xs = L.inputs(c)
            eo = options(c)
            nch = c['channels']
            units = ctx.encode(xs, eo)
            assert L.sha(units) == c['units_sha256'], ('case', c['id'], c['options'], c['material'], c['frames'], nch,
                                                       'first wrong unit', L.first_wrong_unit(units, c))
            if c['cut']:
                h, cut = c['halo'], c['cut']
                tail = ctx.encode([x[(cut - h) * 512:] for x in xs], eo, halo_frames=h)
                assert np.array_equal(tail, units.reshape(-1, nch, 212)[cut:].reshape(-1, 212)), ('halo', c['id'], cut, h)
            pcm = ctx.decode(units, nch)
            assert L.pcm_sha(pcm) == c['pcm_sha256'], ('pcm', c['id'])
    finally:
        ctx.set_speculation(1)


@pytest.mark.parametrize('bias', BIASES)
def test_quantize_frames_reproduces_the_stage_vectors(ctx, bias):
    import carta1_amd as c1
    coefs, modes = L.stage_coefs()
    eo = c1.EncoderOptions({'allocationBias': float(bias)}, biased_table=[float(x) for x in L.biased(bias)])
    got = L.stage_rows(ctx.quantize_frames(coefs, modes, eo))
    want = FX['stage']['by_bias'][bias]
    for k in ('nbfu', 'fields'):
        bad = [f for f in range(len(want[k])) if got[k][f] != want[k][f]]
        assert not bad, (bias, k, 'first wrong frame', bad[0], got[k][bad[0]], want[k][bad[0]])


def test_both_rank_forms_are_exercised(ctx):
    """the heap orders priorities by an integer form of (sfi, wl) where the host finds one, else by the rank table
    (c1_k_allocate.hip rank_of); the corpus above must run both"""
    import carta1_amd as c1
    from carta1_amd import capi
    lib = capi.load()
    form = {}
    for bias in BIASES:
        o = c1.EncoderOptions({'allocationBias': float(bias)}, biased_table=[float(x) for x in L.biased(bias)]).to_c()
        affine, coef = C.c_int(-1), (C.c_int * 4)()
        capi.check(lib.c1_alloc_rank_form(C.byref(o), C.byref(affine), coef))
        form[bias] = (affine.value, tuple(coef))
    print('rank form per bias (affine, (A, B, C, offset)):', form)
    assert form['0'][0] == 0                           # every priority of one word length ties: no form in sfi
    assert form['1'][0] == 1                           # 2^(s/3-21) * {0.875 | 2^-(wl+2)}
    assert {a for a, _ in form.values()} == {0, 1}
