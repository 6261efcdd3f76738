"""GPU: the JavaScript host's measureUnits(channels, units, { masking, haloFrames }) (tests/js_measure_units.mjs) against the
Python host's Context.measure_units on the same PCM and units, which tests/test_gpu_measure_units.py pins to the CPU model: noise,
signal, totals and weights bit for bit over 24 mono and 24 stereo frames, flat and with masking: true; the halo; the TypeErrors,
raised before any native call; the twenty reference names still exported.  Skipped when node is not installed."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
node = shutil.which('node')
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(node is None, reason='node is not installed')]
FRAMES = 24


def test_js_measure_units(tmp_path):
    import carta1_amd as c1
    from carta1_amd import build
    import best_bias_lib as BB
    build.build_library()
    if build.build_addon() is None:
        pytest.fail('the N-API addon did not build')
    body = [c[:FRAMES * 512] for c in BB.material()[1]]
    modes = BB.given_modes()[:FRAMES]
    ctx = c1.Context(0)
    try:
        for tag, chans, m in (('_1', body[:1], modes[:, :1]), ('_2', body, modes)):
            units = ctx.encode_measured(chans, modes=m, scale_factor_offsets=c1.SCALE_FACTOR_OFFSETS, masking=True)[0]
            units.tofile(str(tmp_path / ('units%s.u8' % tag)))
            for c, x in enumerate(chans):
                np.ascontiguousarray(x).tofile(str(tmp_path / ('ch%d%s.f32' % (c, tag))))
            for suffix, masking in (('', None), ('_p', True)):
                res = ctx.measure_units(chans, units, masking=masking, return_weights=masking is not None)
                for name, a in zip(('noise', 'signal', 'totals', 'weights'), res):
                    assert a.any()
                    a.tofile(str(tmp_path / ('%s%s%s.f64' % (name, tag, suffix))))
    finally:
        ctx.close()
    p = subprocess.run([node, os.path.join(ROOT, 'tests', 'js_measure_units.mjs'), str(tmp_path)], cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, universal_newlines=True, timeout=600)
    assert p.returncode == 0 and 'ALL OK' in p.stdout, p.stdout
