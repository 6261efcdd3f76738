"""GPU: the JavaScript host's encodeAeaPcm(channels, { allocationBiases }) (tests/js_bias_palette.mjs) against the reference's
bytes for its own bias schedule (tests/golden/option_changes.json, bias_fixed000) and, combined with blockModes, against the
Python host's Context.encode_biases on the same PCM, which tests/test_gpu_bias_palette.py pins to the oracle.  Skipped when node
is not installed."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
node = shutil.which('node')
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(node is None, reason='node is not installed')]


def test_js_encode_with_allocation_biases(tmp_path):
    import carta1_amd as c1
    from carta1_amd import build
    import bias_palette_lib as BP
    import block_modes_lib as BM
    import option_changes_lib as OC
    build.build_library()
    if build.build_addon() is None:
        pytest.fail('the N-API addon did not build')
    fix = OC.fixture()
    s = fix['schedules']['bias_fixed000']
    frames = fix['frames']
    chans = OC.signal(fix['signals']['pinkT34'], frames)
    sched = np.array([v['allocationBias'] for v in OC.options_at(s['initial'], s['changes'], frames)], dtype=np.float64)
    index = BP.random_index(20261018, frames, 2, 8)
    biases = np.array(BP.PACKAGED_BIASES, dtype=np.float64)[index]
    modes = BM.random_modes(20261019, frames, 2)
    ctx = c1.Context(0)
    try:
        units = ctx.encode_biases(chans, biases, modes=modes)
    finally:
        ctx.close()
    assert np.array_equal(units, BP.oracle_encode_schedule(chans, list(BP.PACKAGED_BIASES), index, modes)[0])
    for c, x in enumerate(chans):
        x.tofile(str(tmp_path / ('ch%d.f32' % c)))
    sched.tofile(str(tmp_path / 'sched.f64'))
    biases.reshape(-1).tofile(str(tmp_path / 'biases.f64'))
    modes.tofile(str(tmp_path / 'modes.u8'))
    units.tofile(str(tmp_path / 'units.u8'))
    (tmp_path / 'sha.txt').write_text(s['results']['pinkT34']['sha256'] + '\n')
    p = subprocess.run([node, os.path.join(ROOT, 'tests', 'js_bias_palette.mjs'), str(tmp_path)], cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, universal_newlines=True, timeout=600)
    assert p.returncode == 0 and 'ALL OK' in p.stdout, p.stdout
