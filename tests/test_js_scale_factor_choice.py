"""GPU: the JavaScript host's encodeMeasured(channels, options, modes, scaleFactorOffsets) and encodeAeaPcm(channels,
{ measuredAllocation: true, scaleFactorOffsets }) (tests/js_scale_factor_choice.mjs) against the Python host's
Context.encode_measured(scale_factor_offsets=...) on the same PCM, under detection and under given modes, which
tests/test_gpu_scale_factor_choice.py pins to the CPU model: units, taken, shifts and both errors bit for bit; the project's own
decode() of the units is finite; and the TypeErrors for offsets that break the rules or come without measuredAllocation.
Skipped when node is not installed."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
node = shutil.which('node')
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(node is None, reason='node is not installed')]


def test_js_encode_measured_with_scale_factor_offsets(tmp_path):
    import carta1_amd as c1
    from carta1_amd import build
    import best_bias_lib as BB
    import scale_factor_choice_lib as SF
    build.build_library()
    if build.build_addon() is None:
        pytest.fail('the N-API addon did not build')
    body = BB.material()[1]
    modes = BB.given_modes()
    ctx = c1.Context(0)
    try:
        for tag, m in (('', None), ('_m', modes)):
            units, taken, shifts, dist, energy = ctx.encode_measured(body, modes=m, return_distortion=True,
                                                                     scale_factor_offsets=c1.SCALE_FACTOR_OFFSETS, return_shifts=True)
            if m is None:
                assert SF.check_outputs(SF.case('detect'), units, taken, shifts, dist, energy) is None
            units.tofile(str(tmp_path / ('units%s.u8' % tag)))
            taken.tofile(str(tmp_path / ('taken%s.u8' % tag)))
            shifts.tofile(str(tmp_path / ('shifts%s.i8' % tag)))
            dist.tofile(str(tmp_path / ('dist%s.f64' % tag)))
            energy.tofile(str(tmp_path / ('energy%s.f64' % tag)))
    finally:
        ctx.close()
    for c, x in enumerate(body):
        np.ascontiguousarray(x).tofile(str(tmp_path / ('ch%d.f32' % c)))
    np.ascontiguousarray(modes).tofile(str(tmp_path / 'modes.u8'))
    p = subprocess.run([node, os.path.join(ROOT, 'tests', 'js_scale_factor_choice.mjs'), str(tmp_path)], cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, universal_newlines=True, timeout=600)
    assert p.returncode == 0 and 'ALL OK' in p.stdout, p.stdout
