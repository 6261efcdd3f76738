"""GPU: the JavaScript host's encodeMeasured(channels, options, modes, scaleFactorOffsets, masking) and encodeAeaPcm(channels,
{ measuredAllocation: true, masking }) (tests/js_masked.mjs) against the Python host's Context.encode_measured(masking=...) on the
same PCM, which tests/test_gpu_masked_alloc.py pins to the CPU model: units, taken, shifts, both errors and weights bit for bit
under the packaged tables (detection and given modes) and under floor = SPECS_PER_BFU; MASKING_DEFAULT equals the JSON as the
Python host read it; the project's own decode() of the units is finite; and the TypeErrors for tables that break the rules or come
without measuredAllocation.  Skipped when node is not installed."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
node = shutil.which('node')
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(node is None, reason='node is not installed')]


def test_js_encode_measured_with_masking(tmp_path):
    import carta1_amd as c1
    from carta1_amd import build
    import best_bias_lib as BB
    import masked_alloc_lib as MK
    build.build_library()
    if build.build_addon() is None:
        pytest.fail('the N-API addon did not build')
    body = BB.material()[1]
    modes = BB.given_modes()
    ctx = c1.Context(0)
    try:
        for tag, m, offsets, masking in (('', None, c1.SCALE_FACTOR_OFFSETS, True), ('_m', modes, c1.SCALE_FACTOR_OFFSETS, True),
                                         ('_s', modes, None, MK.explicit('specs'))):
            units, taken, shifts, dist, energy, weights = ctx.encode_measured(
                body, modes=m, return_distortion=True, scale_factor_offsets=offsets or (0,), return_shifts=True, masking=masking,
                return_weights=True)
            if offsets is None:                                              # masking alone means the offset 0
                u2, t2 = ctx.encode_measured(body, modes=m, masking=masking)
                assert np.array_equal(u2, units) and np.array_equal(t2, taken)
            for name, a in (('units%s.u8', units), ('taken%s.u8', taken), ('shifts%s.i8', shifts), ('dist%s.f64', dist),
                            ('energy%s.f64', energy), ('weights%s.f64', weights)):
                a.tofile(str(tmp_path / (name % tag)))
    finally:
        ctx.close()
    for c, x in enumerate(body):
        np.ascontiguousarray(x).tofile(str(tmp_path / ('ch%d.f32' % c)))
    np.ascontiguousarray(modes).tofile(str(tmp_path / 'modes.u8'))
    np.ascontiguousarray(c1.MASKING_DEFAULT[0]).tofile(str(tmp_path / 'floor.f64'))
    np.ascontiguousarray(c1.MASKING_DEFAULT[1]).tofile(str(tmp_path / 'spread.f64'))
    p = subprocess.run([node, os.path.join(ROOT, 'tests', 'js_masked.mjs'), str(tmp_path)], cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, universal_newlines=True, timeout=600)
    assert p.returncode == 0 and 'ALL OK' in p.stdout, p.stdout
