"""GPU twin of tests/test_pack_guard_cpu.py: the kernels take the decisions their CPU model takes, on inputs built to sit
on the edge of the guards.
 * k_pack<.., SPEC> through c1_pack_spec_tap_device on adversarial coefficients (the reference's, moved 0.95 of the bound
   towards the nearest truncation boundary; bounds from realistic to 1000 x looser): mantissas == model, redo /
   reallocation / re-analysis lists == the model's flags -- so what the CPU test proves of the model (every unit whose
   bytes would differ from the reference's is flagged) holds for the kernel.  Both instantiations: k_pack<true, true>
   (all long: coefficient order == slot order) and k_pack<false, true>, which gathers every band's slots through the long
   or short start table as the unit's own mode byte says, under all-long, all-short and mixed block modes, one mode set per
   launch and all six shuffled into one;
 * the scale-factor guard of k_analysis_spec through c1_spec_stages_device on twelve signal classes: indices and flag ==
   model on the kernel's own coefficients and bounds, in long blocks and (k_analysis_spec<true>) in short ones."""
import numpy as np
import pytest

import oracle_lib as O
import pack_model_lib as P
import spec_model_lib as M
from test_pack_guard_cpu import MODE_SETS, adversarial, material, mode_id, model_bounds, reference_units
from test_spec_bound import signals

pytestmark = pytest.mark.gpu
AMOUNTS = [20, 28, 32, 36, 40, 44, 48, 52]


@pytest.fixture(scope='module')
def ctx():
    import carta1_amd as c1
    c = c1.Context(0)
    yield c
    c.close()


def alloc_record(nbfu, wl):
    rec = np.zeros(32, dtype=np.uint8)
    for b in range(52):
        w = int(wl[b]) if b < nbfu else 0
        rec[b >> 1] |= w << (4 * (b & 1))
    rec[31] |= AMOUNTS.index(nbfu) << 4                       # dword 7 bits 28..30
    return rec


def run_tap(ctx, coefs, eps4, side, alloc, all_long=True):
    import torch
    n = coefs.shape[0]
    d = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (coefs, eps4, side, alloc)]
    out = torch.zeros(n * 212, dtype=torch.uint8, device='cuda')
    lists = torch.zeros(8 + 3 * n, dtype=torch.int32, device='cuda')
    torch.cuda.synchronize()
    ctx.pack_spec_tap_device(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), n, out.data_ptr(), lists.data_ptr(),
                             all_long=all_long)
    ctx.synchronize()
    ls = lists.cpu().numpy().astype(np.int64)
    sets = [set(ls[8 + k * n:8 + k * n + ls[k]].tolist()) for k in range(3)]
    assert all(len(sets[k]) == ls[k] for k in range(3))       # no unit listed twice
    return out.cpu().numpy().reshape(n, 212), sets


@pytest.mark.parametrize('scale', [1.0, 30.0, 1000.0], ids=['bound', 'bound_x30', 'bound_x1000'])
def test_speculative_quantizer_equals_its_model_on_adversarial_coefficients(ctx, scale):
    rng = np.random.default_rng(5)
    coefs, eps4, side, alloc, want_q, want_doubt, want_open, exact_flag, fields = [], [], [], [], [], [], [], [], []
    for name, pcm in material():
        _, eps_all, _ = M.run(pcm)
        for f, (ref, n, wl, sfi, _) in enumerate(reference_units(pcm)):
            if f == 0:
                continue
            kind = (f + len(coefs)) % 3                        # 0: speculative unit; 1: with an open scale factor; 2: exact coefficients (bounds of zero)
            eps = (eps_all[f] * scale).astype(np.float32)
            slots = P.to_slots(ref)
            F = adversarial(slots, eps, sfi, wl, n, 0.95, rng) if kind != 2 else slots
            if kind == 2:
                eps = np.zeros(3, dtype=np.float32)
            q, doubtful, _ = P.quantize(F, eps, sfi, wl, n)
            coefs.append(F)                                    # all long: slot order == coefficient order
            eps4.append(np.concatenate([eps, np.array([1 if kind == 1 else 0], dtype=np.uint32).view(np.float32)]))
            s = np.zeros(64, dtype=np.uint8)
            s[:52] = sfi
            side.append(s)
            alloc.append(alloc_record(n, wl))
            want_q.append(q)
            want_doubt.append(doubtful)
            want_open.append(kind == 1)
            exact_flag.append(kind == 2)
            fields.append((n, wl, sfi))
    units, (redo, realloc, reana) = run_tap(ctx, np.array(coefs), np.array(eps4), np.array(side), np.array(alloc))
    n_units = len(coefs)
    assert any(want_doubt) and not all(want_doubt)
    for u in range(n_units):
        fld = O.unpack_unit(units[u])
        n, wl, sfi = fields[u]
        assert fld.nbfu == n and list(fld.wl[:n]) == list(wl[:n]) and list(fld.sfi[:n]) == list(sfi[:n]), u
        flagged = want_doubt[u] or want_open[u]
        assert (u in redo) == flagged, (u, want_doubt[u], want_open[u])
        assert (u in realloc) == want_open[u], u
        assert (u in reana) == (flagged and not exact_flag[u]), u
        if not flagged:                                        # the bytes that are handed on without the exact kernels
            got = np.array(fld.q[:P.FIRST[n]])
            assert np.array_equal(got, want_q[u][:P.FIRST[n]]), (u, np.nonzero(got != want_q[u][:P.FIRST[n]])[0][:4])


# ---- k_pack<false, true>: the slots gathered per band mode ----------------------------------------------------------------

def from_slots(slots, modes):
    """the inverse of P.to_slots: BFU-major slots -> coefficient order (low128 | mid128 | high256) for the block modes"""
    out = np.empty(512, dtype=np.float32)
    for b in range(52):
        st = (P.START_LONG if modes[P.BAND_OF_BFU[b]] == 0 else P.START_SHORT)[b]
        out[st:st + P.SPECS[b]] = slots[P.FIRST[b]:P.FIRST[b + 1]]
    return out


_records = {}


def attacked_units(modes, scale):
    """per unit of the five materials under `modes`: what the kernel is given (coefficients in coefficient order, bounds with
    the flag word, side record with the mode byte at 52, allocation record) and what the model makes of it.  The three kinds
    of unit alternate: speculative, with an open scale factor, exact (bounds of zero)."""
    if (modes, scale) in _records:
        return _records[(modes, scale)]
    rng = np.random.default_rng(5)
    recs = []
    for name, pcm in material():
        eps_all = model_bounds(name, pcm, modes)
        for f, (ref, n, wl, sfi, _) in enumerate(reference_units(pcm, modes)):
            if f == 0:
                continue
            kind = (f + len(recs)) % 3
            eps = (eps_all[f] * scale).astype(np.float32)
            slots = P.to_slots(ref, modes)
            F = adversarial(slots, eps, sfi, wl, n, 0.95, rng) if kind != 2 else slots
            if kind == 2:
                eps = np.zeros(3, dtype=np.float32)
            q, doubtful, _ = P.quantize(F, eps, sfi, wl, n)
            coefs = from_slots(F, modes)
            assert np.array_equal(P.to_slots(coefs, modes).view(np.uint32), F.view(np.uint32))
            s = np.zeros(64, dtype=np.uint8)
            s[:52] = sfi
            s[52] = modes[0] | modes[1] << 2 | modes[2] << 4
            recs.append(dict(coefs=coefs, eps4=np.concatenate([eps, np.array([1 if kind == 1 else 0], dtype=np.uint32).view(np.float32)]),
                             side=s, alloc=alloc_record(n, wl), q=q, doubt=doubtful, open=kind == 1, exact=kind == 2,
                             fields=(n, wl, sfi), modes=modes))
    _records[(modes, scale)] = recs
    return recs


def check_against_model(recs, units, lists):
    """today's assertions per unit, and the first two bytes against the serialization formula; -> units flagged"""
    redo, realloc, reana = lists
    flagged_units = 0
    for u, r in enumerate(recs):
        fld = O.unpack_unit(units[u])
        n, wl, sfi = r['fields']
        m = r['modes']
        header = (2 - m[0]) << 14 | (2 - m[1]) << 12 | (3 - m[2]) << 10 | AMOUNTS.index(n) << 5        # serialization.js:46-53
        first_wl = (int(wl[0]) << 4 | int(wl[1])) if n > 1 else 0
        assert (int(units[u, 0]) << 8 | int(units[u, 1])) == header, (u, m, hex(header))
        assert int(units[u, 2]) == first_wl, u
        assert fld.nbfu == n and list(fld.wl[:n]) == list(wl[:n]) and list(fld.sfi[:n]) == list(sfi[:n]), u
        flagged = r['doubt'] or r['open']
        flagged_units += flagged
        assert (u in redo) == flagged, (u, m, r['doubt'], r['open'])
        assert (u in realloc) == r['open'], (u, m)
        assert (u in reana) == (flagged and not r['exact']), (u, m)
        if not flagged:                                        # the bytes that are handed on without the exact kernels
            got = np.array(fld.q[:P.FIRST[n]])
            assert np.array_equal(got, r['q'][:P.FIRST[n]]), (u, m, np.nonzero(got != r['q'][:P.FIRST[n]])[0][:4])
    return flagged_units


def tap(ctx, recs, all_long=False):
    return run_tap(ctx, *(np.array([r[k] for r in recs]) for k in ('coefs', 'eps4', 'side', 'alloc')), all_long=all_long)


@pytest.mark.parametrize('scale', [1.0, 30.0, 1000.0], ids=['bound', 'bound_x30', 'bound_x1000'])
@pytest.mark.parametrize('modes', MODE_SETS, ids=mode_id)
def test_mixed_mode_quantizer_equals_its_model_on_adversarial_coefficients(ctx, modes, scale):
    """k_pack<false, true>, one mode set per launch"""
    recs = attacked_units(modes, scale)
    units, lists = tap(ctx, recs)
    assert any(r['doubt'] for r in recs) and not all(r['doubt'] for r in recs)
    flagged = check_against_model(recs, units, lists)
    print('tap', mode_id(modes), 'x%g:' % scale, 'units', len(recs), 'flagged', flagged, 'accepted', len(recs) - flagged)
    if modes == (0, 0, 0):                                     # the same units through the all-long instantiation
        units_long, lists_long = tap(ctx, recs, all_long=True)
        assert np.array_equal(units_long, units) and lists_long == lists


def test_mixed_mode_quantizer_with_all_mode_bytes_in_one_launch(ctx):
    """units of the six mode bytes in shuffled order in one launch of k_pack<false, true>: every unit is gathered by its own
    byte (a wave fetches the byte of the unit after next one unit ahead), and more than two redo batches are listed"""
    recs = [r for modes in MODE_SETS for r in attacked_units(modes, 30.0)]
    order = np.random.default_rng(17).permutation(len(recs))
    recs = [recs[k] for k in order]
    assert len({r['side'][52] for r in recs[:64]}) == 6
    units, lists = tap(ctx, recs)
    flagged = check_against_model(recs, units, lists)
    print('tap, six mode bytes shuffled:', 'units', len(recs), 'flagged', flagged, 'accepted', len(recs) - flagged)
    assert flagged > 64 and len(recs) - flagged > 64


def test_mixed_mode_quantizer_with_many_units_per_wave(ctx):
    """The launches above give every wave one unit (the grid grows with the units up to the resident workgroups).  Here the
    shuffled launch is repeated 744 times over in one call, 1 049 040 units: a compute unit holds at most 32 waves and the
    grid is at most twice the resident workgroups, 16 384 waves on 256 compute units, so every wave packs 64 units or more, lists more than one batch of 32 from inside its loop, and
    addresses each unit after its first by a mode byte it fetched one unit ahead.  Every repetition must give the bytes and
    the list memberships of the first, which is compared with the model as above."""
    import torch
    recs = [r for modes in MODE_SETS for r in attacked_units(modes, 30.0)]
    order = np.random.default_rng(17).permutation(len(recs))
    recs = [recs[k] for k in order]
    n, T = len(recs), 744
    N = n * T
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert N >= 64 * (2 * 32 * cus), cus                             # 64 units per wave on a device of up to 256 compute units
    d = [torch.from_numpy(np.array([r[k] for r in recs])).cuda() for k in ('coefs', 'eps4', 'side', 'alloc')]
    d = [a.repeat(T, 1).contiguous() for a in d]
    out = torch.zeros(N * 212, dtype=torch.uint8, device='cuda')
    lists = torch.zeros(8 + 3 * N, dtype=torch.int32, device='cuda')
    torch.cuda.synchronize()
    ctx.pack_spec_tap_device(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), N, out.data_ptr(), lists.data_ptr(),
                             all_long=False)
    ctx.synchronize()
    out = out.view(T, n, 212)
    assert bool((out == out[0]).all())
    counts = lists[:3].cpu().numpy()
    member0 = []
    for k in range(3):
        listed = lists[8 + k * N:8 + k * N + int(counts[k])].long()
        assert int(listed.min()) >= 0 and int(listed.max()) < N
        hits = torch.bincount(listed, minlength=N)
        assert int(hits.max()) == 1                                 # no unit listed twice
        member = hits.view(T, n).bool()
        assert bool((member == member[0]).all()), k
        member0.append(set(np.nonzero(member[0].cpu().numpy())[0].tolist()))
    flagged = check_against_model(recs, out[0].cpu().numpy(), member0)
    assert int(counts[0]) == flagged * T
    print('tap, many units per wave:', 'units', N, 'flagged', flagged * T)


@pytest.mark.parametrize('name,pcm', list(signals()), ids=[s[0] for s in signals()])
def test_scale_factor_guard_equals_its_model(ctx, name, pcm):
    from test_gpu_spec import spec_stages
    co, eps, side = spec_stages(ctx, [pcm])
    for f in range(co.shape[0]):
        slots = P.to_slots(co[f, 0])
        if not np.isfinite(eps[f, 0, :3]).all():
            assert eps[f, 0, 3].view(np.uint32) & 1                # bounds that are not finite: flagged
            continue
        sfi, unstable = P.sf_guard(slots, eps[f, 0, :3])
        assert np.array_equal(side[f, 0, :52], sfi), (f, np.nonzero(side[f, 0, :52] != sfi)[0][:4])
        assert bool(eps[f, 0, 3].view(np.uint32) & 1) == unstable, f


@pytest.mark.parametrize('modes', [(2, 2, 3), (1, 2, 1)], ids=mode_id)
@pytest.mark.parametrize('name,pcm', list(signals()), ids=[s[0] for s in signals()])
def test_scale_factor_guard_equals_its_model_in_short_blocks(ctx, name, pcm, modes):
    """k_analysis_spec<true> (every triple without a zero): its indices and flag are the model's on its own coefficients and
    bounds, the slots gathered through BFU_START_SHORT"""
    from test_gpu_spec import spec_stages
    co, eps, side = spec_stages(ctx, [pcm], modes)
    opened = 0
    for f in range(co.shape[0]):
        assert side[f, 0, 52] == (modes[0] | modes[1] << 2 | modes[2] << 4), f
        slots = P.to_slots(co[f, 0], (2, 2, 3))
        if not np.isfinite(eps[f, 0, :3]).all():
            assert eps[f, 0, 3].view(np.uint32) & 1                # bounds that are not finite: flagged
            continue
        sfi, unstable = P.sf_guard(slots, eps[f, 0, :3])
        assert np.array_equal(side[f, 0, :52], sfi), (f, np.nonzero(side[f, 0, :52] != sfi)[0][:4])
        assert bool(eps[f, 0, 3].view(np.uint32) & 1) == unstable, f
        opened += unstable
    print('scale-factor guard', name, mode_id(modes), 'frames', co.shape[0], 'open units', opened)
