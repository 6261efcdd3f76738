"""GPU: every kernel of the measured allocation against the CPU models, on two contexts of the module: `narrow` (C1_MEASURED_WIDE=0:
k_measured, k_measured_sf, k_measured_masked, a wave per unit) and `wide` (C1_MEASURED_WIDE=1: k_measured_wide, a workgroup per
unit).  Launches of at most 8 192 units take the wide kernel by default, so the model comparisons of test_gpu_measured_alloc.py,
test_gpu_scale_factor_choice.py and test_gpu_masked_alloc.py run on it alone; here their cases run on the narrow kernels too, bit
for bit against the wide one.  Then the all-long variants (fixedBlockModes [0, 0, 0], modes NULL) of all three entry points on both
contexts; the hard material of tests/hard_material_lib.py -- the level-15 cap, scale-factor indices 0 .. 3 and 63, 20-BFU units,
the reference's all-zero fallback record, exact ties, silence between coded frames -- through the three entry points and
c1_encode_measured_modes_batch (k_measured_modes); c1_measure_units_batch on the units those calls wrote; NaN and +Inf in the PCM.
No call is larger than 260 units.  tests/test_hard_material_cpu.py shows what the material reaches and how few units are close."""
import numpy as np
import pytest

import best_bias_lib as BB
import hard_material_lib as H
import masked_alloc_lib as MK
import measure_units_lib as MU
import measured_alloc_lib as MA
import measured_modes_lib as MM
import scale_factor_choice_lib as SF
import test_gpu_masked_alloc as TK
import test_gpu_measure_units as TU
import test_gpu_measured_alloc as TA
import test_gpu_measured_modes as TM
import test_gpu_scale_factor_choice as TS

pytestmark = pytest.mark.gpu

ENTRIES = ('measured', 'sf', 'masked')
MODEL_OF = {'measured': 'plain', 'sf': 'sf', 'masked': 'masked'}
KINDS = ('narrow', 'wide')
ALL_LONG = {'fixedBlockModes': [0, 0, 0]}
HARD_CASES = [(name, byte) for name in H.NAMES for byte in H.BYTES] + [('impulse', 'detect')]


@pytest.fixture(scope='module')
def two():
    ctxs = {'narrow': TA._context(C1_MEASURED_WIDE=0), 'wide': TA._context(C1_MEASURED_WIDE=1)}
    yield ctxs
    _hard.clear()
    for c in ctxs.values():
        c.close()


def run(ctx, entry, chans, options=None, modes=None, offsets=SF.OFFSETS, tables='packaged'):
    """c1_encode_measured_batch, _sf_batch or _masked_batch, every output asked for -> dict"""
    if entry == 'measured':
        return TA.batch(ctx, chans, options, modes)
    if entry == 'sf':
        return TS.batch(ctx, chans, options, modes, offsets=offsets)
    return TK.batch(ctx, chans, options, modes, offsets=offsets, tables=tables)


def same(a, b):
    return a.keys() == b.keys() and all(a[k].shape == b[k].shape and np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) for k in a)


def outputs_wrong(entry, m, got, keep=None):
    """the lib's check_outputs of this entry point over the units `keep` (all of them when None): None, or what is wrong"""
    if keep is not None:
        m, got = H.rows(m, keep), H.rows(got, keep)
    if entry == 'measured':
        return MA.check_outputs(m, got['units'], got['taken'], got['distortion'], got['energy'])
    if entry == 'sf':
        return SF.check_outputs(m, got['units'], got['taken'], got['shifts'], got['distortion'], got['energy'])
    return MK.check_outputs(m, got['units'], got['taken'], got['shifts'], got['distortion'], got['energy'], got['weights'])


def units_wrong(entry, m, got, offsets=SF.OFFSETS, keep=None):
    """the lib's check_valid of this entry point, from the bytes alone: None, or what is wrong"""
    nch = 2
    if keep is not None:
        m, got, nch = H.rows(m, keep), H.rows(got, keep), 1
    if entry == 'measured':
        return MA.check_valid(got['units'], m['coefs'], got['taken'], got['distortion'], nch=nch)
    if entry == 'sf':
        return SF.check_valid(got['units'], m['coefs'], got['taken'], got['distortion'], offsets, nch=nch)
    return MK.check_valid(got['units'], m['coefs'], got['taken'], got['distortion'], got['weights'], offsets, nch=nch)


def final_of(got):
    return np.where(got['taken'] != 0, got['distortion'][:, 1], got['distortion'][:, 0])


def measure_launches(ctx, call):
    """the number of launches c1_ctx_kernel_ms counts under "measure" for one call"""
    ctx.set_profiling(True)
    try:
        call()
        ms, launches = ctx.kernel_ms('measure')
        assert ms > 0
        return launches
    finally:
        ctx.set_profiling(False)


# ---- a. the shared material on the narrow kernels ----
SHARED = ([('measured', material, kind, None, 'packaged', SF.OFFSETS) for material, kind in
           [('pink', 0), ('pink', 10), ('pink', 58), ('white', 0), ('white', 58), ('pink', 'modes'), ('pink', 'detect'), ('pink', 'fixed')]] +
          [('sf', material, kind, frames, 'packaged', SF.OFFSETS) for material, kind, frames in
           [('pink', 10, None), ('white', 58, None), ('pink', 'detect', None), ('pink', 'modes', TS.SHORT), ('pink', 'fixed', TS.SHORT)]] +
          [('masked', material, kind, frames, tables, offsets) for material, kind, frames, tables, offsets in
           [('pink', 10, None, 'packaged', SF.OFFSETS), ('white', 58, None, 'packaged', SF.OFFSETS), ('pink', 'detect', TK.SHORT, 'packaged', SF.OFFSETS),
            ('pink', 'modes', TK.SHORT, 'packaged', SF.OFFSETS), ('pink', 'fixed', TK.SHORT, 'packaged', SF.OFFSETS),
            ('pink', 10, None, 'specs', (0,)), ('pink', 'modes', TK.SHORT, 'specs', SF.OFFSETS), ('pink', 10, 65, 'self', (0,))]])


@pytest.fixture(scope='module')
def mat():
    return {'modes': BB.given_modes()}


@pytest.mark.parametrize('entry,material,kind,frames,tables,offsets', SHARED)
def test_shared_material_on_the_narrow_kernels(two, mat, entry, material, kind, frames, tables, offsets):
    """the cases of test_gpu_measured_alloc.py, test_gpu_scale_factor_choice.py and test_gpu_masked_alloc.py against the same
    models with the same checks, on the context that never takes the wide kernel; the wide context gives the same bits"""
    chans, o, modes = TK.call_of(kind, mat, material, frames)
    if entry == 'measured':
        m = MA.case(kind, material)
    elif entry == 'sf':
        m = SF.case(kind, material, frames=frames)
    else:
        m = MK.case(kind, material, tables, offsets, frames)
    got = run(two['narrow'], entry, chans, o, modes, offsets, tables)
    print(entry, material, kind, 'taken %d of %d' % (int(got['taken'].sum()), len(got['taken'])))
    assert outputs_wrong(entry, m, got) is None
    assert units_wrong(entry, m, got, offsets) is None
    assert (final_of(got) <= got['distortion'][:, 0]).all()
    assert same(got, run(two['wide'], entry, chans, o, modes, offsets, tables))
    assert measure_launches(two['narrow'], lambda: run(two['narrow'], entry, chans, o, modes, offsets, tables)) == 1


# ---- c. the hard material (b and d below read its calls) ----
_hard = {}


def hard_call(two, which, entry, name, kind):
    """the call of one entry point on one hard material on one context, made once per module"""
    key = (which, entry, name, kind)
    if key not in _hard:
        got = run(two[which], entry, H.material(name), None, H.modes_of(kind))
        for a in got.values():
            a.setflags(write=False)
        _hard[key] = got
    return _hard[key]


@pytest.mark.parametrize('entry', ENTRIES)
@pytest.mark.parametrize('name,kind', HARD_CASES)
def test_hard_material_against_the_model(two, entry, name, kind):
    """decided and tied units: units, taken, shifts, word lengths, T_ref, T(n*), E (and the weights) against the model exactly as
    the pink material is compared, exact zeros zero.  All units, close ones included: ordinary sound units from their bytes
    alone, T_ref and E within REL, T_final <= T_ref.  Narrow and wide the same bits."""
    m = H.model(MODEL_OF[entry], name, kind)
    decided, tied, close = H.classes(m)
    for which in KINDS:
        got = hard_call(two, which, entry, name, kind)
        print(which, entry, name, kind, 'decided %d tied %d close %d; taken %d, the model %d' % (
            decided.sum(), tied.sum(), close.sum(), int(got['taken'].sum()), int(m['taken'].sum())))
        assert outputs_wrong(entry, m, got, decided | tied) is None, which
        assert units_wrong(entry, m, got) is None, which
        for name_, g, want in (('T_ref', got['distortion'][:, 0], m['D'][:, 0]), ('E', got['energy'], m['E'])):
            assert (np.abs(g - want) <= MA.REL * want).all() and not g[want == 0].view(np.uint64).any(), (which, name_)
        if entry == 'masked':
            assert (np.abs(got['weights'] - m['P']) <= MA.REL * m['P']).all(), which
        assert set(got['taken'].tolist()) <= {0, 1} and (final_of(got) <= got['distortion'][:, 0]).all(), which
        assert (got['distortion'][:, 1][got['taken'] != 0] < got['distortion'][:, 0][got['taken'] != 0]).all(), which
    assert same(hard_call(two, 'narrow', entry, name, kind), hard_call(two, 'wide', entry, name, kind))
    plain = two['narrow'].encode(H.material(name)) if kind == 'detect' else two['narrow'].encode_modes(H.material(name), H.modes_of(kind))
    assert np.array_equal(plain, m['ref'])


# ---- b. the all-long variants ----
@pytest.mark.parametrize('which', KINDS)
@pytest.mark.parametrize('entry', ENTRIES)
def test_all_long_variants(two, which, entry):
    """fixedBlockModes [0, 0, 0] with modes NULL (the kernels' all-long variants: no mode bytes are read) against modes given as
    all zeros (the general variants) bit for bit, against the byte-0 model, and one measure launch per call"""
    ctx = two[which]
    o = TA.opts(ALL_LONG)
    for name in H.NAMES:
        chans = H.material(name)
        got = run(ctx, entry, chans, o, None)
        assert same(got, hard_call(two, which, entry, name, 0)), name
        m = H.model(MODEL_OF[entry], name, 0)
        decided, tied, _ = H.classes(m)
        assert outputs_wrong(entry, m, got, decided | tied) is None, name
        assert units_wrong(entry, m, got) is None, name
    white = MM.BMO.material('white')
    got = run(ctx, entry, white, o, None)
    assert same(got, run(ctx, entry, white, None, np.zeros((len(white[0]) // 512, 2), dtype=np.uint8)))
    if entry == 'measured':
        assert outputs_wrong(entry, MA.case(0, 'white'), got) is None
    assert measure_launches(ctx, lambda: run(ctx, entry, white, o, None)) == 1
    assert measure_launches(ctx, lambda: run(ctx, entry, H.material('tone'), o, None)) == 1


# ---- c, continued: the joint choice of block modes ----
@pytest.mark.parametrize('sf', [False, True], ids=['offset0', 'offsets'])
@pytest.mark.parametrize('name', H.NAMES)
def test_hard_material_joint_modes(two, name, sf):
    """c1_encode_measured_modes_batch: per (unit, candidate) the figures bit for bit those of the measure-only calls under that
    byte, the choice the first least T_final of them, units, taken and shifts those of encode_measured under the chosen modes
    (all units); against the composed model where the unit is not close; silent units choose candidate 0 with +0.0 figures"""
    chans, cand = H.material(name), H.modes_candidates(sf)
    offsets = H.OFFSETS if sf else (0,)
    m = H.modes_model(name, sf)
    firm, tied, close, silent = H.modes_classes(name, sf)
    got = TM.batch(two['narrow'], chans, cand, offsets)
    print(name, 'sf' if sf else 'plain', 'firm %d tied %d close %d silent %d' % (firm.sum(), tied.sum(), close.sum(), silent.sum()),
          'winners', np.bincount(got['choice'], minlength=len(cand)).tolist())
    assert TM.composed(two['narrow'], chans, got, cand, offsets if sf else None) is None
    assert MM.check_case(H.rows(m, ~close), H.rows(got, ~close)) is None
    for g, want in ((got['distortion'][:, :, 0], m['D'][:, :, 0]), (got['energy'], m['E'])):          # T_ref and E: every unit
        assert (np.abs(g - want) <= MM.REL * want).all()
    ar = np.arange(len(got['choice']))
    assert SF.check_valid(got['units'], coefs_of(chans, got['units']), got['taken'], got['distortion'][ar, got['choice']], offsets) is None
    assert not got['choice'][silent].any() and not got['taken'][silent].any()
    assert not got['distortion'][silent].view(np.uint64).any() and not got['energy'][silent].view(np.uint64).any()
    if name == 'dc_gap':
        assert silent.sum() == 4
    assert TM.same(got, TM.batch(two['wide'], chans, cand, offsets))      # k_measured_modes either way: the switch changes nothing


def coefs_of(chans, units):
    """the coefficients under the modes the units themselves record (close units included, whatever the device chose)"""
    return BB.coefficients(chans, units)


# ---- d. the meter on the units those calls wrote ----
@pytest.mark.parametrize('entry', ENTRIES)
@pytest.mark.parametrize('name,kind', HARD_CASES)
def test_meter_reports_what_the_hard_units_hold(two, entry, name, kind):
    """c1_measure_units_batch on the units of each hard-material call: totals bit for bit that call's T_final and E (and the
    weights its weights), the header's promise"""
    got = hard_call(two, 'narrow', entry, name, kind)
    tables = 'packaged' if entry == 'masked' else None
    meter = TU.measure(two['wide'], H.material(name), got['units'], tables)
    assert MU.bitwise(meter['totals'][:, 0], final_of(got))
    assert MU.bitwise(meter['totals'][:, 1], got['energy'])
    if entry == 'masked':
        assert MU.bitwise(meter['weights'], got['weights'])


# ---- e. non-finite PCM ----
def clean_frames():
    """bool [U]: the units of frames before the first bad sample of their channel"""
    u = np.arange(2 * H.NONFINITE_FRAMES)
    first = np.array([H.NONFINITE_AT[c][0] for c in (0, 1)])
    return u // 2 < first[u % 2]


@pytest.mark.parametrize('which', KINDS)
@pytest.mark.parametrize('entry', ENTRIES)
def test_non_finite_pcm(two, which, entry):
    """one NaN in channel 1 of frame 3 and one +Inf in channel 0 of frame 6 of pink noise, under given modes.  The call returns
    C1_OK; a unit whose T are all NaN in the model is not taken and is byte for byte encode_modes' unit of the same PCM; no unit
    is taken with a NaN T(n*); the units before the first bad sample are bit for bit those of the clean run; the units the model
    says the bad samples do not reach are compared with the model as ever."""
    ctx = two[which]
    chans, modes = H.nonfinite_material(), H.NONFINITE_MODES
    m = H.nonfinite_model(MODEL_OF[entry])
    got = run(ctx, entry, chans, None, modes)                                # capi.check: C1_OK
    lost = np.isnan(m['D'][:, 1])
    sound = H.untouched(m)
    print(which, entry, 'all T NaN in units', np.flatnonzero(lost).tolist(), 'finite in', int(sound.sum()), 'of', len(sound))
    assert lost.any() and not (lost & clean_frames()).any() and sound[clean_frames()].all()
    assert set(got['taken'].tolist()) <= {0, 1}
    assert not got['taken'][lost].any()
    assert np.array_equal(got['units'][lost], ctx.encode_modes(chans, modes)[lost])
    assert not np.isnan(got['distortion'][:, 1][got['taken'] != 0]).any()
    assert np.array_equal(np.isnan(got['distortion'][:, 1]), lost)
    clean = run(ctx, entry, H.nonfinite_material(clean=True), None, modes)
    assert same(H.rows(got, clean_frames()), H.rows(clean, clean_frames()))
    decided, tied, _ = H.classes(H.rows(m, sound))
    assert (decided | tied).all()                                            # pink: no unit is close
    assert outputs_wrong(entry, m, got, sound) is None
    assert units_wrong(entry, m, got, keep=sound) is None


@pytest.mark.parametrize('which', KINDS)
def test_non_finite_pcm_joint_modes(two, which):
    """the same PCM through c1_encode_measured_modes_batch: a unit whose T_final is NaN under every candidate chooses candidate 0,
    is not taken and is encode_modes' unit under modes_out; a NaN never wins elsewhere"""
    ctx = two[which]
    chans, cand = H.nonfinite_material(), H.NONFINITE_CANDIDATES
    m = H.nonfinite_modes_model()
    got = TM.batch(ctx, chans, cand, H.OFFSETS)                              # capi.check: C1_OK
    lost = np.isnan(m['final']).all(axis=1)
    sound = np.isfinite(m['D']).all(axis=(1, 2)) & np.isfinite(m['E']).all(axis=1)
    assert lost.any() and not (lost & clean_frames()).any() and sound[clean_frames()].all()
    assert not got['choice'][lost].any() and not got['taken'][lost].any() and (got['modes'][lost] == cand[0]).all()
    assert np.array_equal(got['units'][lost], ctx.encode_modes(chans, got['modes'].reshape(-1, 2))[lost])
    ar = np.arange(len(lost))
    won = got['distortion'][ar, got['choice']]
    assert not np.isnan(won[:, 1][got['taken'] != 0]).any()
    fin = np.where(got['distortion'][:, :, 1] < got['distortion'][:, :, 0], got['distortion'][:, :, 1], got['distortion'][:, :, 0])
    assert not np.isnan(fin[ar, got['choice']])[~np.isnan(fin).all(axis=1)].any()
    clean = TM.batch(ctx, H.nonfinite_material(clean=True), cand, H.OFFSETS)
    assert TM.same(H.rows(got, clean_frames()), H.rows(clean, clean_frames()))
    assert MM.check_case(H.rows(m, sound), H.rows(got, sound)) is None
