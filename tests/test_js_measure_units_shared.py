"""GPU: the JavaScript host's measureUnits(channels, units, { masking, haloFrames, thresholdFrom }) (tests/
js_measure_units_shared.mjs) against the Python host's Context.measure_units(threshold_from=...) on the same PCM and units, which
tests/test_gpu_measure_units_shared.py pins: noise, signal, totals and weights bit for bit over 24 mono and 24 stereo frames of
the masked search's units under thresholdFrom 'long'; 'own' and an absent thresholdFrom give the bytes of the call that was there
before; the TypeErrors, raised before any native call; the twenty reference names still exported.  Skipped when node is not
installed."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
node = shutil.which('node')
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(node is None, reason='node is not installed')]
FRAMES = 24


def test_js_measure_units_shared(tmp_path):
    import carta1_amd as c1
    from carta1_amd import build
    import best_bias_lib as BB
    build.build_library()
    if build.build_addon() is None:
        pytest.fail('the N-API addon did not build')
    body = [c[:FRAMES * 512] for c in BB.material()[1]]
    ctx = c1.Context(0)
    try:
        for tag, chans in (('_1', body[:1]), ('_2', body)):
            units, choice, modes = ctx.encode_measured_modes(chans, [0, 58, 10], scale_factor_offsets=c1.SCALE_FACTOR_OFFSETS, masking=True)[:3]
            assert len(set(modes.tolist())) > 1
            units.tofile(str(tmp_path / ('units%s.u8' % tag)))
            for c, x in enumerate(chans):
                np.ascontiguousarray(x).tofile(str(tmp_path / ('ch%d%s.f32' % (c, tag))))
            for suffix, threshold in (('_own', 'own'), ('_long', 'long')):
                res = ctx.measure_units(chans, units, masking=True, return_weights=True, threshold_from=threshold)
                for name, a in zip(('noise', 'signal', 'totals', 'weights'), res):
                    assert a.any()
                    a.tofile(str(tmp_path / ('%s%s%s.f64' % (name, tag, suffix))))
    finally:
        ctx.close()
    p = subprocess.run([node, os.path.join(ROOT, 'tests', 'js_measure_units_shared.mjs'), str(tmp_path)], cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, universal_newlines=True, timeout=600)
    assert p.returncode == 0 and 'ALL OK' in p.stdout, p.stdout
