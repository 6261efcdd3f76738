"""GPU: what a change of k_analysis_spec's LDS layout (c1_k_spec.hip) can break and the large-batch
tests would hide -- a sample or a coefficient routed to a wrong slot at a run seam, in the warm-up frame, in the last
partial run, in the band-2 tail lanes 46..63, in the delay lines that are the work buffers' own tails.

The signal: every sample distinct and exactly representable (a multiplicative hash of its index, 20 bits), different per
channel, so any sample that reaches a wrong slot changes coefficients.  One stream of 133 frames per channel serves every
case; its references -- the CPU model of the kernel (tests/model/spec_model.c) and the oracle's sound units -- are computed
once.  A case is (frames, channels, halo): with a halo the body starts at frame 2 of the stream (one frame of history
gives these feed-forward filters what the whole stream gives them), without one at frame 0.

 * coefficients == the model bit for bit, scale-factor indices and guard flag == the pack model's on the kernel's own bound,
   the bound == the model's inside a run, through c1_spec_stages_device, long and short blocks;
 * units == the oracle's with speculation modes 1 and 2;
 * 65 frames: speculation_stats == the count of a reference pass on the CPU -- the model's coefficients through the pack
   model's scale-factor guard, the reference's allocation and the pack model's quantizer guard under the kernel's bounds:
   the flagged set did not move;
 * the same in fresh child processes that force 4-frame and 64-frame runs (C1_RUN_FRAMES is read once per process; batches
   this small get 4-frame runs by default, 64 is the run of the large batches: seams at 64 and 128, last runs of 1 and 3)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as O
import pack_model_lib as P
import spec_model_lib as M

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAME_COUNTS = (1, 2, 4, 5, 65, 129, 131)
MODES = ((0, 0, 0), (2, 2, 3))
START = 2                                   # first body frame of the cases with a halo
TOTAL = START + max(FRAME_COUNTS)
MULT = (2654435761, 2246822519)


def hashed(mult, n):
    k = np.arange(n, dtype=np.uint64)
    x = (((k * np.uint64(mult)) >> np.uint64(8)) & np.uint64(0xfffff)).astype(np.float64) / 1048576.0 - 0.5
    y = x.astype(np.float32)
    assert np.array_equal(y.astype(np.float64), x) and len(np.unique(y)) == n       # exact, all distinct
    return y


_ref = {}


def reference():
    """the stream, the model's coefficients and bounds per channel and block modes, the oracle's units (mono, stereo)"""
    if not _ref:
        chans = [hashed(m, TOTAL * 512) for m in MULT]
        _ref['pcm'] = chans
        for modes in MODES:
            short = modes != (0, 0, 0)
            _ref['model', modes] = [M.run(c, short)[:2] for c in chans]
            # the body that starts at frame 0 is a prefix of the stream; the oracle from frame 0 serves both kinds of case
            _ref['units', modes, 2] = O.encode_stream(chans, fixed_modes=modes)[0]
            _ref['units', modes, 1] = O.encode_stream(chans[:1], fixed_modes=modes)[0]
    return _ref


def case_slices(frames, halo):
    """-> (first sample of what is handed to the device, first body frame in the stream)"""
    first = START if halo else 0
    return (first - halo) * 512, first


def spec_stages(ctx, chans, frames, halo, modes):
    import torch
    import carta1_amd as c1
    dev = [torch.from_numpy(np.ascontiguousarray(c)).cuda() for c in chans]
    n = frames * len(chans)
    coefs = torch.zeros(n * 512, dtype=torch.float32, device='cuda')
    eps = torch.zeros(n * 4, dtype=torch.float32, device='cuda')
    side = torch.zeros(n * 64, dtype=torch.uint8, device='cuda')
    torch.cuda.synchronize()
    ctx.spec_stages_device([d.data_ptr() + halo * 2048 for d in dev], frames, coefs.data_ptr(), eps.data_ptr(), side.data_ptr(),
                           c1.EncoderOptions({'fixedBlockModes': list(modes)}), halo_frames=halo)
    ctx.synchronize()
    return (coefs.cpu().numpy().reshape(frames, len(chans), 512), eps.cpu().numpy().reshape(frames, len(chans), 4),
            side.cpu().numpy().reshape(frames, len(chans), 64))


def run_length(frames, channels):
    """the run c1k_pick_run (carta1_amd/csrc/c1_internal.h) gives a batch; it only decides which frames open a run, where
    the bound is compared with the model's loosely (test_gpu_spec.py does the same).  Change it with that function."""
    forced = int(os.environ.get('C1_RUN_FRAMES', '0'))
    if forced > 0:
        return max(4, forced)
    units = frames * channels
    return 64 if units >= 64 * 2048 else max(4, -(-units // 2048))


def flagged_on_cpu(mco, eps, modes):
    """the reference pass: is this unit redone?  Scale-factor guard open, or a mantissa in doubt under the reference's allocation"""
    slots = P.to_slots(mco, modes)
    sfi, unstable = P.sf_guard(slots, eps)
    if unstable:
        return True
    nbfu, wl, sfi_ref = P.allocate(mco, modes)
    assert np.array_equal(sfi_ref[:nbfu], sfi[:nbfu])                    # a closed guard: the reference's indices
    return P.quantize(slots, eps, sfi, wl, nbfu)[1]


def check_case(ctx, frames, nch, halo, stats=False):
    import carta1_amd as c1
    R = reference()
    s0, first = case_slices(frames, halo)
    chans = [c[s0:(first + frames) * 512] for c in R['pcm'][:nch]]
    run = run_length(frames, nch)
    for modes in MODES:
        co, eps, side = spec_stages(ctx, chans, frames, halo, modes)
        want_redone = 0
        for c in range(nch):
            mco, meps = R['model', modes][c]
            mco, meps = mco[first:first + frames], meps[first:first + frames]
            assert np.array_equal(co[:, c].view(np.uint32), mco.view(np.uint32)), (frames, nch, halo, modes, c, np.argwhere(co[:, c] != mco)[:4])
            inside = np.arange(frames) % run != 0                            # (test_gpu_spec.py: the first frame of a run)
            assert np.isfinite(eps[:, c, :3]).all()
            assert np.isclose(eps[:, c, :3], meps, rtol=2e-6, atol=0)[inside].all(), (frames, nch, halo, modes, c)
            assert np.allclose(eps[:, c, :3], meps, rtol=0.2, atol=0)
            assert (side[:, c, 52] == (modes[0] | modes[1] << 2 | modes[2] << 4)).all()
            for f in range(frames):
                sfi, unstable = P.sf_guard(P.to_slots(co[f, c], modes), eps[f, c, :3])
                assert np.array_equal(side[f, c, :52], sfi), (frames, nch, halo, modes, c, f)
                assert bool(eps[f, c, 3].view(np.uint32) & 1) == unstable, (frames, nch, halo, modes, c, f)
                if stats:
                    want_redone += bool(flagged_on_cpu(mco[f], eps[f, c, :3], modes))
        want = R['units', modes, nch][first * nch:(first + frames) * nch]
        opts = c1.EncoderOptions({'fixedBlockModes': list(modes)})
        for spec in (1, 2):
            ctx.set_speculation(spec)
            ctx.speculation_stats(reset=True)
            d0 = ctx.speculation_deferred()
            got = ctx.encode(chans, opts, halo_frames=halo)
            u, r = ctx.speculation_stats()
            d = ctx.speculation_deferred() - d0
            ctx.set_speculation(1)
            assert np.array_equal(got, want), (frames, nch, halo, modes, spec, np.nonzero((got != want).any(axis=1))[0][:8])
            through = frames * nch if spec == 2 or frames * nch >= 64 else 0     # default mode: calls below 64 units use the exact kernels only
            assert u + d == through and (spec == 1 or d == 0), (u, d, spec)
            if stats and d == 0:
                assert r == want_redone, (frames, nch, modes, spec, r, want_redone)
        if stats:
            assert 0 < want_redone < frames * nch                            # the pass flags some units and not all


@pytest.fixture(scope='module')
def ctx():
    import carta1_amd as c1
    c = c1.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize('halo', [0, 1, 2])
@pytest.mark.parametrize('nch', [1, 2], ids=['mono', 'stereo'])
@pytest.mark.parametrize('frames', FRAME_COUNTS)
def test_runs_seams_and_halos(ctx, frames, nch, halo):
    check_case(ctx, frames, nch, halo, stats=(frames == 65 and halo == 0))


def test_always_speculating_never_defers_and_flags_what_the_cpu_pass_flags(ctx):
    """mode 2 of the 65-frame stereo case once more, on its own: every unit goes through the speculative pass"""
    import carta1_amd as c1
    R = reference()
    chans = [c[:65 * 512] for c in R['pcm']]
    ctx.set_speculation(2)
    ctx.speculation_stats(reset=True)
    d0 = ctx.speculation_deferred()
    ctx.encode(chans, c1.EncoderOptions({'fixedBlockModes': [0, 0, 0]}))
    u, r = ctx.speculation_stats()
    d = ctx.speculation_deferred() - d0
    ctx.set_speculation(1)
    assert (u, d) == (130, 0) and 0 < r < u


CHILD = '''
import sys
import test_gpu_spec_layout as t
import carta1_amd as c1
ctx = c1.Context(0)
for frames, nch, halo in ((5, 2, 1), (65, 2, 0), (65, 1, 1), (129, 2, 2), (131, 1, 0), (131, 2, 1)):
    t.check_case(ctx, frames, nch, halo, stats=(frames == 65 and halo == 0))
ctx.close()
print('child ok')
'''


@pytest.mark.parametrize('run', [4, 64])
def test_forced_run_lengths_in_a_fresh_process(run):
    env = dict(os.environ, C1_RUN_FRAMES=str(run), PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, 'tests')]))
    p = subprocess.run([sys.executable, '-s', '-c', CHILD], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and 'child ok' in p.stdout, (p.stdout[-2000:], p.stderr[-4000:])
