"""GPU: the coding error of given sound units under the all-long threshold (c1_measure_units_shared_device / _batch,
k_measure_units_shared).  Library against library, bit for bit: units that are all long give c1_measure_units_*'s outputs; noise
and signal are that call's whatever the modes; weights are c1_encode_measured_modes_masked_*'s whatever units are passed; for the
search's own units, whole-buffer and from a live stream, the totals are its distortion and energy of the winner; flat tables;
scaling both tables by 4.  Then the CPU model of tests/measure_units_shared_lib.py for plain units, foreign bytes through the
device entry point between guard words and a corrupted stream; the geometry of the kernel (one wave per unit, four per workgroup,
a grid bounded at 2 048 workgroups); independence of chunking, pipeline, overlap, speculation, halo and of which outputs are asked
for; NaN and +Inf; a caller's stream; tables back to back; the calls around it unharmed; the rejections; the launch counts.
tests/test_measure_units_shared_cpu.py shows the model to agree bit for bit with the model of the masked search."""
import itertools

import numpy as np
import pytest

import carta1_amd as c1
from carta1_amd import capi
import best_bias_lib as BB
import best_modes_lib as BMO
import masked_alloc_lib as MK
import masked_modes_lib as X
import measure_units_lib as MU
import measure_units_shared_lib as MS
import measured_alloc_lib as MA
import test_gpu_measure_units as TU
import test_gpu_measured_modes_masked as TX

pytestmark = pytest.mark.gpu

C1_OK, C1_ERR_ARG = 0, 1   # include/carta1_hip.h
FRAMES = BB.FRAMES
OUTPUTS, WIDTH, FILL, SHORT, COUNTS = TU.OUTPUTS, TU.WIDTH, TU.FILL, TU.SHORT, TU.COUNTS
CAND8, OFFSETS = X.CANDIDATES, X.OFFSETS
same, rows, _env, _context = TU.same, TU.rows, TU._env, TU._context


@pytest.fixture(scope='module')
def ctx():
    c = c1.Context(0)
    yield c
    c.close()


def tables_of(tables):
    floor, spread = MK.named(tables) if isinstance(tables, str) else tables
    return np.ascontiguousarray(floor, dtype=np.float64), None if spread is None else np.ascontiguousarray(spread, dtype=np.float64)


def measure(ctx, chans, units, tables='packaged', halo=0, ask=OUTPUTS):
    """c1_measure_units_shared_batch with any subset of the outputs; the others are passed as NULL -> dict of the ones asked
    for.  tables: a name of masked_alloc_lib.named, or a (floor, spread | None) pair"""
    chans = [np.ascontiguousarray(c, dtype=np.float32) for c in chans]
    nch, frames = len(chans), len(chans[0]) // 512 - halo
    n = frames * nch
    u = np.ascontiguousarray(units, dtype=np.uint8).reshape(-1, 212)
    assert u.shape[0] == n
    floor, spread = tables_of(tables)
    out = {k: np.full((n, WIDTH[k]), FILL) for k in OUTPUTS}
    ptrs = capi.ptr_array([c.ctypes.data + halo * 2048 for c in chans])
    capi.check(capi.load().c1_measure_units_shared_batch(
        ctx._h, ptrs, nch, frames, halo, u.ctypes.data, floor.ctypes.data, None if spread is None else spread.ctypes.data,
        *[out[k].ctypes.data if k in ask else None for k in OUTPUTS]))
    assert all((out[k] == FILL).all() for k in OUTPUTS if k not in ask)
    return {k: out[k] for k in ask}


@pytest.fixture(scope='module')
def mat(ctx):
    with_halo, body = BB.material()
    modes = BB.given_modes()
    m = {'with_halo': with_halo, 'body': body, 'pink': body, 'modes': modes, 'white': BMO.material('white'),
         'silence': [np.zeros(FRAMES * 512, dtype=np.float32)] * 2}
    m['units'] = ctx.encode_modes(body, modes)                 # plain units over the whole domain of the modes
    m['units_halo'] = ctx.encode_modes(with_halo, np.concatenate([np.zeros((2, 2), dtype=np.uint8), modes]))
    m['long'] = ctx.encode_modes(body, np.zeros_like(modes))
    m['units'].setflags(write=False)
    return m


@pytest.fixture(scope='module')
def baseline(ctx, mat):
    out = measure(ctx, mat['body'], mat['units'])
    for a in out.values():
        a.setflags(write=False)
    return out


def against(m, got):
    print('bit-equal: ' + ', '.join('%s %s' % (k, MS.bitwise(got[k], m[k])) for k in got))
    assert MS.check_outputs(m, got) is None


# ---- library against library, bit for bit ----
@pytest.mark.parametrize('nch', [1, 2])
@pytest.mark.parametrize('tables', ['packaged', 'packaged*4', 'flat', 'self', 'no-spread'])
def test_all_long_units_are_measured_as_before(ctx, mat, tables, nch):
    """1. the unit's own spectrum is the all-long one: every output is c1_measure_units_*'s"""
    t = (MK.packaged()[0], None) if tables == 'no-spread' else tables
    frames = len(mat['white'][0]) // 512
    for name, units in (('body', mat['long']), ('white', ctx.encode_modes(mat['white'], np.zeros((frames, 2), dtype=np.uint8)))):
        chans = mat[name][:nch]
        u = np.ascontiguousarray(units.reshape(-1, 2, 212)[:, :nch]).reshape(-1, 212)
        got = measure(ctx, chans, u, t)
        assert same(got, TU.measure(ctx, chans, u, t)), name
        assert (got['noise'] > 0).any() and (got['totals'] > 0).any()


def test_noise_and_signal_are_the_own_mode_meters(ctx, mat):
    """2. whatever the modes"""
    for name, units in (('modes', mat['units']), ('detect', ctx.encode(mat['body'])), ('random', MU.random_units(77, FRAMES * 2))):
        got, own = measure(ctx, mat['body'], units), TU.measure(ctx, mat['body'], units, 'packaged')
        assert MS.bitwise(got['noise'], own['noise']) and MS.bitwise(got['signal'], own['signal']), name
        if name != 'detect':                                     # units with a short band: the new call is not the old one renamed
            assert MS.gap_db(got['weights'], own['weights']).max() > 6.0, name


@pytest.mark.parametrize('tables', ['packaged', 'self'])
def test_weights_are_the_masked_searchs_whatever_the_units(ctx, mat, tables):
    """3. the same bits for the search's units, the same units under every byte of the domain, and random bytes"""
    found = TX.batch(ctx, mat['body'], CAND8, (0,), tables)
    n = FRAMES * 2
    cycle = np.array(MU.DOMAIN_BYTES)[np.arange(n) % 8]
    for units in (found['units'], MU.with_modes(found['units'], cycle), MU.random_units(3, n), mat['long']):
        got = measure(ctx, mat['body'], units, tables, ask=('weights',))
        assert MS.bitwise(got['weights'], found['weights'])
    assert len(set(found['modes'].tolist())) > 2


@pytest.mark.parametrize('offsets', [(0,), OFFSETS], ids=['plain', 'five-offsets'])
@pytest.mark.parametrize('cand', [CAND8, [0, 58]], ids=['eight', 'pair'])
@pytest.mark.parametrize('material', ['pink', 'white', 'silence'])
def test_the_masked_search_reports_what_its_units_hold(ctx, mat, material, cand, offsets):
    """4. totals[:, 0] == distortion[u, choice[u], taken[u]] and totals[:, 1] == energy[u, choice[u]] in every row, whole-buffer
    and for the units a live stream's pushes return"""
    chans = mat[material]
    n = len(chans[0]) // 512
    found = TX.batch(ctx, chans, cand, offsets)
    s = c1.EncoderStream(ctx, 2)
    try:
        parts = [s.push_measured_modes([c[a * 512:b * 512] for c in chans], cand, scale_factor_offsets=None if offsets == (0,) else offsets,
                                       return_distortion=True, return_shifts=True, masking=True, return_weights=True)
                 for a, b in ((0, 1), (1, 4), (4, 37), (37, n))]
    finally:
        s.close()
    pushed = {k: np.concatenate([p[i] for p in parts]) for i, k in enumerate(TX.OUTPUTS)}
    for out in (found, pushed):
        ar = np.arange(n * 2)
        got = measure(ctx, chans, out['units'])
        print('bit-equal: T %s, E %s' % (MS.bitwise(got['totals'][:, 0], out['distortion'][ar, out['choice'], out['taken']]),
                                         MS.bitwise(got['totals'][:, 1], out['energy'][ar, out['choice']])))
        assert MS.bitwise(got['totals'][:, 0], out['distortion'][ar, out['choice'], out['taken']])
        assert MS.bitwise(got['totals'][:, 1], out['energy'][ar, out['choice']])
        assert MS.bitwise(got['weights'], out['weights'])
    if material != 'silence':
        assert found['taken'].any() and len(set(found['choice'].tolist())) > 1


def test_flat_tables_and_scaling_by_four(ctx, mat, baseline):
    """5. floor all 1.0 and no spread: weights exactly 1.0, totals the table-less c1_measure_units_*'s; 6. both tables times 4.0:
    totals and weights times exactly 0.25"""
    flat = measure(ctx, mat['body'], mat['units'], 'flat')
    assert (flat.pop('weights') == 1.0).all() and same(flat, TU.measure(ctx, mat['body'], mat['units'], None))
    for tables in ('packaged', 'self', 'specs'):
        one = dict(baseline) if tables == 'packaged' else measure(ctx, mat['body'], mat['units'], tables)
        four = measure(ctx, mat['body'], mat['units'], tables + '*4')
        assert MS.bitwise(four['weights'], 0.25 * one['weights']) and MS.bitwise(four['totals'], 0.25 * one['totals'])
        assert MS.bitwise(four['noise'], one['noise']) and MS.bitwise(four['signal'], one['signal'])


# ---- against the CPU model ----
_sums = {}


def model_of(key, chans, units, tables='packaged', device=False):
    """the model of these units; the own-mode sums are test_gpu_measure_units' (computed once per key in the process), the
    all-long energies are added here"""
    if key not in _sums:
        if key not in TU._models:
            TU._models[key] = MU.model(chans, units, device=device)
        m = TU._models[key]
        _sums[key] = {'noise': m['noise'], 'signal': m['signal'], 'bytes': m['bytes'], 'E0': MS.all_long_energies(chans, m['noise'].shape[0])}
    return MS.with_tables(_sums[key], *tables_of(tables))


@pytest.mark.parametrize('kind', ['detect', 'fixed', 'modes'])
def test_plain_units_against_the_model(ctx, mat, kind):
    """noise, signal, totals and weights within measure_units_lib.REL of the model, exact zeros zero; bit-for-bit equality is
    expected and printed"""
    chans = [c[:SHORT * 512] for c in mat['body']]
    if kind == 'detect':
        units = ctx.encode(chans)
    elif kind == 'fixed':
        units = ctx.encode(chans, c1.EncoderOptions({'fixedBlockModes': MA.FIXED}))
    else:
        units = mat['units'][:SHORT * 2]
    for tables in ('packaged', 'self'):
        got = measure(ctx, chans, units, tables)
        against(model_of(('plain', kind), chans, units, tables), got)
        assert (got['signal'] > 0).any() and (got['noise'] > 0).any()
    # the Python host: the same call; 'own' and no keyword: the call that was there before
    res = ctx.measure_units(chans, units, masking=True, return_weights=True, threshold_from='long')
    assert same(dict(zip(OUTPUTS, res)), measure(ctx, chans, units))
    before = TU.measure(ctx, chans, units, 'packaged')
    assert same(dict(zip(OUTPUTS, ctx.measure_units(chans, units, masking=True, return_weights=True, threshold_from='own'))), before)
    assert same(dict(zip(OUTPUTS, ctx.measure_units(chans, units, masking=True, return_weights=True))), before)
    with pytest.raises(ValueError, match='needs masking'):
        ctx.measure_units(chans, units, threshold_from='long')


def _device_call(c, pcm, frames, units, t, tables, guard=0, threshold_from='long'):
    p = {k: t[k].data_ptr() + guard for k in OUTPUTS}
    c.measure_units_device([x.data_ptr() for x in pcm], frames, units.data_ptr(), p['noise'], p['signal'], p['totals'], p['weights'],
                           masking=tables, threshold_from=threshold_from)


@pytest.mark.parametrize('domain', [True, False])
def test_foreign_bytes_through_the_device_entry_point(ctx, mat, domain):
    """512 units of random bytes from torch tensors (domain: the mode bits rewritten to a random byte of the domain; else raw):
    every unit is measured, the outputs are the model's (under mode_in_domain for the raw bytes), the 4 096 bytes on either side
    of every output keep their fill and the inputs their bytes.  The host call agrees where it accepts the units and names the
    first it rejects"""
    import torch
    frames, G = 256, 4096
    chans = [np.tile(c, 2)[:frames * 512] for c in mat['body']]
    units = MU.random_units(20261019 + int(domain), frames * 2, domain)
    m = model_of(('foreign', domain), chans, units, 'packaged', device=not domain)
    assert len(set(m['bytes'].tolist())) == 8
    pcm = [torch.cat([torch.full((1024,), 7.0), torch.from_numpy(x), torch.full((1024,), 7.0)]).cuda() for x in chans]
    d_units = torch.cat([torch.full((G,), 0x5A, dtype=torch.uint8), torch.from_numpy(units).reshape(-1), torch.full((G,), 0x5A, dtype=torch.uint8)]).cuda()
    t = TU._device_buffers(torch, frames * 2, G)
    _device_call(ctx, [x[1024:] for x in pcm], frames, d_units[G:], t, True, G)
    ctx.synchronize()
    back = d_units.cpu().numpy()
    assert np.array_equal(back[G:-G].reshape(-1, 212), units) and (back[:G] == 0x5A).all() and (back[-G:] == 0x5A).all()
    assert all(np.array_equal(x.cpu().numpy()[1024:-1024], c) for x, c in zip(pcm, chans))
    got = TU._to_host(t, frames * 2, G)
    against(m, got)
    assert np.isfinite(got['noise']).all() and (got['noise'] > 0).all(axis=1).any()
    if domain:
        assert same(measure(ctx, chans, units), got)
    else:
        first = next(u for u in range(frames * 2) if MU.mode_byte(MU.O.unpack_unit(units[u])) not in MU.DOMAIN_BYTES)
        with pytest.raises(c1.Carta1Error, match='c1_measure_units_shared_batch: frame %d, channel %d: .* block mode of the unit' % (first // 2, first % 2)):
            measure(ctx, chans, units)


def test_a_corrupted_stream(ctx, mat):
    """one bit flipped in ten units of the masked search's stream (behind the mode bits): only those units' rows change, and the
    weights not at all"""
    units = np.array(TX.batch(ctx, mat['body'], [0, 58, 10], OFFSETS, ask=('units',))['units'])
    clean = measure(ctx, mat['body'], units)
    rs = np.random.RandomState(9)
    hit = np.sort(rs.permutation(units.shape[0])[:10])
    bad = units.copy()
    for u in hit:
        bit = int(rs.randint(16, 600))                           # amount, word lengths, scale factors, the first mantissas
        bad[u, bit >> 3] ^= 0x80 >> (bit & 7)
    got = measure(ctx, mat['body'], bad)
    changed = np.flatnonzero((got['noise'] != clean['noise']).any(axis=1) | (got['totals'] != clean['totals']).any(axis=1))
    assert set(changed.tolist()) <= set(hit.tolist()) and len(changed) >= 1
    keep = np.ones(units.shape[0], dtype=bool)
    keep[hit] = False
    assert same({k: v[keep] for k, v in got.items()}, {k: v[keep] for k, v in clean.items()})
    assert MS.bitwise(got['signal'], clean['signal']) and MS.bitwise(got['weights'], clean['weights'])   # the PCM's alone
    frames = int(hit[1]) // 2 + 1
    m = MS.model([c[:frames * 512] for c in mat['body']], bad[:frames * 2], *MK.packaged())
    against(m, rows(got, 0, frames, 2))


# ---- shapes and paths ----
@pytest.mark.parametrize('nch', [1, 2])
def test_frame_counts_and_the_stride_of_the_grid(ctx, mat, baseline, nch):
    """the rows of the whole call for every count, also when the grid is bounded at 1 or 3 workgroups, so that the waves stride
    over the units with and without a remainder"""
    chans = mat['body'][:nch]
    units = np.ascontiguousarray(mat['units'].reshape(FRAMES, 2, 212)[:, :nch]).reshape(-1, 212)
    whole = measure(ctx, chans, units)
    if nch == 2:
        assert same(whole, dict(baseline))
    else:
        assert same(whole, {k: v[0::2] for k, v in baseline.items()})
    for blocks in (None, 1, 3):
        with _env(**({} if blocks is None else {'C1_METER_BLOCKS': blocks})):
            for frames in COUNTS:
                got = measure(ctx, [c[:frames * 512] for c in chans], units[:frames * nch])
                assert same(got, rows(whole, 0, frames, nch)), (blocks, frames, nch)


def test_the_seam_of_the_bounded_grid(ctx, mat):
    """2 048 workgroups of four waves: 8 192 units per sweep.  One unit either side of the seam, against a grid that never strides"""
    n = 8193
    reps = -(-n // FRAMES)
    chan = np.tile(mat['body'][0], reps)[:n * 512]
    units = np.tile(mat['units'][0::2], (reps, 1))[:n]
    with _env(C1_METER_BLOCKS=4096):
        want = measure(ctx, [chan], units)
    for frames in (8191, 8192, 8193):
        got = measure(ctx, [chan[:frames * 512]], units[:frames])
        assert same(got, rows(want, 0, frames, 1)), frames
    assert (want['noise'][8192] > 0).any()


@pytest.mark.parametrize('halo', [1, 2])
def test_halo_with_the_same_real_history(ctx, mat, halo):
    part = [c[(2 - halo) * 512:] for c in mat['with_halo']]
    units = mat['units_halo'][(2 - halo) * 2:]
    whole = measure(ctx, part, units)
    got = measure(ctx, part, units[halo * 2:], halo=halo)
    assert same(got, rows(whole, halo, halo + FRAMES, 2))


@pytest.mark.parametrize('env', [{'C1_CHUNK_FRAMES': 7}, {'C1_CHUNK_FRAMES': 64}, {'C1_PIPELINE': 0}, {'C1_PIPELINE': 1},
                                 {'C1_CHUNK_FRAMES': 64, 'C1_PIPELINE': 1, 'C1_OVERLAP': 1}],
                         ids=['chunk7', 'chunk64', 'unpiped', 'piped', 'chunk64-piped-overlap'])
def test_outputs_do_not_depend_on_chunks_pipeline_or_speculation(mat, baseline, env):
    c = _context(**env)
    try:
        for mode in (0, 1, 2):
            c.set_speculation(mode)
            assert same(measure(c, mat['body'], mat['units']), dict(baseline)), (env, mode)
        # the timing kinds: one launch of the meter per chunk, the analysis beside it, nothing else
        c.set_profiling(True)
        measure(c, mat['body'], mat['units'])
        chunks = -(-FRAMES // max(env['C1_CHUNK_FRAMES'], 16)) if 'C1_CHUNK_FRAMES' in env else 1   # a context's chunk is at least 16 frames
        ms, launches = c.kernel_ms('meter')
        assert launches == chunks and ms > 0
        assert c.kernel_ms('analysis')[1] == chunks
        assert all(c.kernel_ms(k)[1] == 0 for k in ('allocate', 'pack', 'measure', 'choose'))
    finally:
        c.close()


def test_outputs_do_not_depend_on_which_are_asked_for(ctx, mat, baseline):
    """every single output and every set of all but one; the call twice"""
    for ask in [s for k in (1, 3) for s in itertools.combinations(OUTPUTS, k)]:
        assert same(measure(ctx, mat['body'], mat['units'], ask=ask), {k: baseline[k] for k in ask}), ask
    assert same(measure(ctx, mat['body'], mat['units']), dict(baseline))


def test_silence_gives_zeros(ctx, mat):
    units = ctx.encode(mat['silence'])
    got = measure(ctx, mat['silence'], units)
    for k in ('noise', 'signal', 'totals'):
        assert not got[k].view(np.uint64).any(), k                                   # +0.0 exactly
    assert MS.bitwise(got['weights'], np.broadcast_to(1.0 / MK.packaged()[0], got['weights'].shape))
    got = measure(ctx, mat['silence'], mat['units'])
    assert not got['signal'].view(np.uint64).any() and (got['noise'] > 0).any() and MS.bitwise(got['totals'][:, 1], np.zeros(FRAMES * 2))


@pytest.mark.parametrize('value', [np.nan, np.inf])
def test_non_finite_pcm(ctx, mat, baseline, value):
    """one NaN, one +Inf in channel 1 of frame 3: that unit's totals are not finite, the other channel and the frames before are
    the clean call's, and nothing faults"""
    chans = [np.array(c[:8 * 512]) for c in mat['body']]
    chans[1][3 * 512 + 17] = value
    got = measure(ctx, chans, mat['units'][:16])
    assert not np.isfinite(got['totals'][7]).any()
    clean = rows(baseline, 0, 8, 2)
    assert same({k: v[0::2] for k, v in got.items()}, {k: v[0::2] for k, v in clean.items()})
    assert same(rows(got, 0, 2, 2), rows(clean, 0, 2, 2))
    assert not np.isnan(got['weights'][0::2]).any() and (got['weights'][0::2] > 0).all()
    assert same(measure(ctx, chans, mat['units'][:16]), got)


def test_two_calls_with_different_tables_back_to_back(ctx, mat, baseline):
    """two device calls queued one behind the other with no host synchronisation between them, each with tables of its own that
    the host overwrites as soon as its call returns: each gives the bits of a call alone.  This pins the order of the upload on
    the stream.  A c1_measure_units_device call and a masked search afterwards give their usual bits"""
    import torch
    pcm = [torch.from_numpy(x).cuda() for x in mat['body']]
    units = torch.from_numpy(np.array(mat['units'])).cuda()
    n = FRAMES * 2
    first, second, third = (TU._device_buffers(torch, n, 0) for _ in range(3))
    want_self, want_own = measure(ctx, mat['body'], mat['units'], 'self'), TU.measure(ctx, mat['body'], mat['units'], 'packaged')
    want_search = TX.batch(ctx, mat['body'], [0, 58], (0,))
    _device_call(ctx, pcm, FRAMES, units, first, MK.FLAT)                    # warm: workspace, the tables' buffer
    ctx.synchronize()
    floor_a, spread_a = (np.array(a) for a in MK.packaged())
    floor_b, spread_b = np.array(MK.explicit('self')[0]), np.array(MK.explicit('self')[1])
    floor_c, spread_c = (np.array(a) for a in MK.packaged())
    _device_call(ctx, pcm, FRAMES, units, first, (floor_a, spread_a))
    floor_a[:] = 1.0
    spread_a[:] = 0.0
    _device_call(ctx, pcm, FRAMES, units, second, (floor_b, spread_b))
    floor_b[:] = 1.0
    spread_b[:] = 0.0
    _device_call(ctx, pcm, FRAMES, units, third, (floor_c, spread_c), threshold_from='own')
    floor_c[:] = 1.0
    ctx.synchronize()
    assert same(TU._to_host(first, n), dict(baseline))
    assert same(TU._to_host(second, n), want_self)
    assert same(TU._to_host(third, n), want_own)
    assert TX.same(TX.batch(ctx, mat['body'], [0, 58], (0,)), want_search)
    assert same(measure(ctx, mat['body'], mat['units']), dict(baseline))


def test_on_a_callers_stream(mat, baseline):
    """PCM and units are written by work queued just before the call and the outputs are read by work queued just after, with
    no host synchronisation in between; then inputs and outputs are overwritten behind it"""
    import torch
    S = torch.cuda.Stream()
    c = _context(stream=S.cuda_stream)
    try:
        src = [torch.from_numpy(x).cuda() for x in mat['body']]
        src_units = torch.from_numpy(np.array(mat['units'])).cuda()
        pcm = [torch.zeros_like(x) for x in src]
        units = torch.zeros_like(src_units)
        n = FRAMES * 2
        t = TU._device_buffers(torch, n, 0)
        busy = torch.ones(1 << 26, dtype=torch.float32, device='cuda')
        torch.cuda.synchronize()
        with torch.cuda.stream(S):
            _device_call(c, pcm, FRAMES, units, t, MK.FLAT)   # warm: workspace grown (this drains the stream)
            S.synchronize()
            for _ in range(200):
                busy.mul_(-1.0)
            for p, x in zip(pcm, src):
                p.copy_(x)
            units.copy_(src_units)
            _device_call(c, pcm, FRAMES, units, t, True)
            snap = {k: v.clone() for k, v in t.items()}
            for p in pcm:
                p.zero_()
            units.zero_()
            for v in t.values():
                v.fill_(FILL)
            queued_behind_busy_stream = not S.query()
            S.synchronize()
        assert queued_behind_busy_stream
        assert same(TU._to_host(snap, n), dict(baseline))
    finally:
        c.close()


def test_rejections_leave_the_outputs_untouched_and_the_next_call_unharmed(ctx, mat, baseline):
    lib = capi.load()
    err = lambda: lib.c1_last_error().decode()
    ptrs = capi.ptr_array([c.ctypes.data for c in mat['body']])
    floor, spread = (np.ascontiguousarray(a) for a in MK.packaged())
    n = FRAMES * 2
    out = {k: np.full((n, WIDTH[k]), FILL) for k in OUTPUTS}
    outs = [out[k].ctypes.data for k in OUTPUTS]
    units = np.array(mat['units'])
    dptr = capi.ptr_array([0x1000, 0x2000])        # the device call decides on its arguments before it touches a pointer

    def call(fn, p, f=floor, s=spread, u=units, o=outs, nch=2, frames=FRAMES, halo=0):
        f = None if f is None else np.ascontiguousarray(f)
        s = None if s is None else np.ascontiguousarray(s)
        return fn(ctx._h, p, nch, frames, halo, u if isinstance(u, int) or u is None else u.ctypes.data, None if f is None else f.ctypes.data,
                  None if s is None else s.ctypes.data, *o)

    for fn, p, u, name in ((lib.c1_measure_units_shared_batch, ptrs, units, 'c1_measure_units_shared_batch'),
                           (lib.c1_measure_units_shared_device, dptr, 0x3000, 'c1_measure_units_shared_device')):
        bad = floor.copy()
        bad[7] = 0.0
        assert call(fn, p, f=bad, u=u) == C1_ERR_ARG and name + ': mask_floor[7]' in err(), err()
        bad = spread.copy()
        bad[3, 9] = -1.0
        assert call(fn, p, s=bad, u=u) == C1_ERR_ARG and 'mask_spread[165]' in err(), err()
        assert call(fn, p, u=u, o=[None] * 4) == C1_ERR_ARG and 'all NULL' in err(), err()
        assert call(fn, p, f=None, u=u) == C1_ERR_ARG and 'mask_spread needs mask_floor' in err(), err()
        assert call(fn, p, f=None, s=None, u=u) == C1_ERR_ARG and name + ': mask_floor is NULL' in err(), err()
        assert call(fn, p, f=None, s=None, u=u, o=[None, None, outs[2], None]) == C1_ERR_ARG and 'mask_floor is NULL' in err(), err()
        assert call(fn, p, u=None) == C1_ERR_ARG and 'units is NULL' in err(), err()
        assert call(fn, p, u=u, nch=3) == C1_ERR_ARG and call(fn, p, u=u, halo=3) == C1_ERR_ARG and call(fn, p, u=u, frames=-1) == C1_ERR_ARG
        assert call(fn, None, u=u) == C1_ERR_ARG and 'pcm is NULL' in err(), err()
    assert call(lib.c1_measure_units_shared_device, dptr, u=0x3001) == C1_ERR_ARG and '4-byte aligned' in err(), err()
    assert call(lib.c1_measure_units_shared_device, capi.ptr_array([0x1000, 0x2004]), u=0x3000) == C1_ERR_ARG and '16-byte aligned' in err(), err()
    assert call(lib.c1_measure_units_shared_batch, ptrs, frames=(1 << 22) + 1) == C1_ERR_ARG and 'at most' in err(), err()
    bad = units.copy()
    bad[77, 0] = (bad[77, 0] & 0xF3) | 0x04                     # high field 1: block mode 2
    assert call(lib.c1_measure_units_shared_batch, ptrs, u=bad) == C1_ERR_ARG
    assert 'frame 38, channel 1: high block mode of the unit is 2, not 0 or 3' in err(), err()
    assert call(lib.c1_measure_units_shared_batch, ptrs, frames=0) == C1_OK
    assert call(lib.c1_measure_units_shared_device, dptr, u=0x3000, frames=0) == C1_OK
    assert all((out[k] == FILL).all() for k in OUTPUTS)
    with pytest.raises(ValueError, match='high block mode'):
        ctx.measure_units(mat['body'], bad, masking=True, threshold_from='long')
    with pytest.raises(c1.Carta1Error, match=r'c1_measure_units_shared_device: mask_floor\[0\]'):
        ctx.measure_units_device([0x1000, 0x2000], FRAMES, 0x3000, totals_ptr=0x4000, masking=(np.zeros(52), None), threshold_from='long')
    # the next calls are unharmed
    assert same(measure(ctx, mat['body'], mat['units']), dict(baseline))
    assert np.array_equal(ctx.encode_modes(mat['body'], mat['modes']), mat['units'])
