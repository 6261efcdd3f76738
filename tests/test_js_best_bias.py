"""GPU: the JavaScript host's encodeBestBias and encodeAeaPcm(channels, { allocationBiasCandidates }) (tests/js_best_bias.mjs)
against the Python host's Context.encode_best_bias on the same PCM, candidates and modes, which tests/test_gpu_best_bias.py pins
to the CPU model; and the error for allocationBiases given together with allocationBiasCandidates.  Skipped when node is not
installed."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
node = shutil.which('node')
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(node is None, reason='node is not installed')]


def test_js_encode_best_bias(tmp_path):
    import carta1_amd as c1
    from carta1_amd import build
    import best_bias_lib as BB
    build.build_library()
    if build.build_addon() is None:
        pytest.fail('the N-API addon did not build')
    _, body = BB.material()
    modes = BB.given_modes()
    ctx = c1.Context(0)
    try:
        for tag, m in (('m', modes), ('d', None)):
            units, choice, dist, energy = ctx.encode_best_bias(body, BB.BIASES, modes=m, return_distortion=True)
            assert BB.check_outputs('modes' if m is not None else 'detect', units, choice, dist, energy) is None
            units.tofile(str(tmp_path / ('units_%s.u8' % tag)))
            choice.tofile(str(tmp_path / ('choice_%s.u8' % tag)))
            dist.tofile(str(tmp_path / ('dist_%s.f64' % tag)))
            energy.tofile(str(tmp_path / ('energy_%s.f64' % tag)))
    finally:
        ctx.close()
    for c, x in enumerate(body):
        np.ascontiguousarray(x).tofile(str(tmp_path / ('ch%d.f32' % c)))
    np.array(BB.BIASES, dtype=np.float64).tofile(str(tmp_path / 'cand.f64'))
    modes.tofile(str(tmp_path / 'modes.u8'))
    p = subprocess.run([node, os.path.join(ROOT, 'tests', 'js_best_bias.mjs'), str(tmp_path)], cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, universal_newlines=True, timeout=600)
    assert p.returncode == 0 and 'ALL OK' in p.stdout, p.stdout
