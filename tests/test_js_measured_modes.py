"""GPU: the JavaScript host's encodeMeasuredModes and encodeAeaPcm(channels, { measuredAllocation: true, measuredModeCandidates })
(tests/js_measured_modes.mjs) against the Python host's Context.encode_measured_modes on the same PCM, candidates and offsets --
24 mono and 24 stereo frames, with and without the suggested offsets -- which tests/test_gpu_measured_modes.py pins to the CPU
model; the new TypeErrors; the twenty reference names still exported.  Skipped when node is not installed."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
node = shutil.which('node')
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(node is None, reason='node is not installed')]
FRAMES = 24


def test_js_encode_measured_modes(tmp_path):
    import carta1_amd as c1
    from carta1_amd import build
    import best_modes_lib as BMO
    build.build_library()
    if build.build_addon() is None:
        pytest.fail('the N-API addon did not build')
    body = [c[:FRAMES * 512] for c in BMO.material('pink')]
    ctx = c1.Context(0)
    try:
        for tag, chans in (('_1', body[:1]), ('_2', body)):
            for suffix, offsets in (('', None), ('_s', c1.SCALE_FACTOR_OFFSETS)):
                units, choice, modes, taken, shifts, dist, energy = ctx.encode_measured_modes(
                    chans, BMO.CANDIDATES, scale_factor_offsets=offsets, return_distortion=True, return_shifts=True)
                under = ctx.encode_measured(chans, modes=modes.reshape(-1, len(chans)), scale_factor_offsets=offsets)
                assert np.array_equal(under[0], units) and np.array_equal(under[1], taken)
                name = lambda what, ext: str(tmp_path / ('%s%s%s.%s' % (what, tag, suffix, ext)))
                units.tofile(name('units', 'u8'))
                choice.tofile(name('choice', 'u8'))
                modes.tofile(name('modes', 'u8'))
                taken.tofile(name('taken', 'u8'))
                shifts.tofile(name('shifts', 'i8'))
                dist.tofile(name('dist', 'f64'))
                energy.tofile(name('energy', 'f64'))
            for c, x in enumerate(chans):
                np.ascontiguousarray(x).tofile(str(tmp_path / ('ch%d%s.f32' % (c, tag))))
    finally:
        ctx.close()
    np.array(BMO.CANDIDATES, dtype=np.uint8).tofile(str(tmp_path / 'cand.u8'))
    p = subprocess.run([node, os.path.join(ROOT, 'tests', 'js_measured_modes.mjs'), str(tmp_path)], cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, universal_newlines=True, timeout=600)
    assert p.returncode == 0 and 'ALL OK' in p.stdout, p.stdout
