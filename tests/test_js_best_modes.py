"""GPU: the JavaScript host's encodeBestModes and encodeAeaPcm(channels, { blockModeCandidates }) (tests/js_best_modes.mjs)
against the Python host's Context.encode_best_modes on the same PCM and candidates, which tests/test_gpu_best_modes.py pins to
the CPU model; and the errors for blockModeCandidates given together with blockModes or allocationBiasCandidates.  Skipped when
node is not installed."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
node = shutil.which('node')
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(node is None, reason='node is not installed')]


def test_js_encode_best_modes(tmp_path):
    import carta1_amd as c1
    from carta1_amd import build
    import best_modes_lib as BMO
    build.build_library()
    if build.build_addon() is None:
        pytest.fail('the N-API addon did not build')
    body = BMO.material('pink')
    ctx = c1.Context(0)
    try:
        units, choice, modes, dist, energy = ctx.encode_best_modes(body, BMO.CANDIDATES, return_distortion=True)
        assert BMO.check_outputs('pink', units, choice, modes, dist, energy) is None
        ctx.encode_modes(body, np.full((len(body[0]) // 512, 2), 10, dtype=np.uint8)).tofile(str(tmp_path / 'units_const10.u8'))
    finally:
        ctx.close()
    units.tofile(str(tmp_path / 'units.u8'))
    choice.tofile(str(tmp_path / 'choice.u8'))
    modes.tofile(str(tmp_path / 'modes.u8'))
    dist.tofile(str(tmp_path / 'dist.f64'))
    energy.tofile(str(tmp_path / 'energy.f64'))
    for c, x in enumerate(body):
        np.ascontiguousarray(x).tofile(str(tmp_path / ('ch%d.f32' % c)))
    np.array(BMO.CANDIDATES, dtype=np.uint8).tofile(str(tmp_path / 'cand.u8'))
    p = subprocess.run([node, os.path.join(ROOT, 'tests', 'js_best_modes.mjs'), str(tmp_path)], cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, universal_newlines=True, timeout=600)
    assert p.returncode == 0 and 'ALL OK' in p.stdout, p.stdout
