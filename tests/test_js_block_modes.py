"""GPU: the JavaScript host's encodeAeaPcm(channels, { blockModes }) and encodeBatchModes (tests/js_block_modes.mjs) against
the Python host's Context.encode_modes on the same PCM and per-frame, per-channel modes, which tests/test_gpu_block_modes.py
pins to the oracle.  Skipped when node is not installed."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
node = shutil.which('node')
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(node is None, reason='node is not installed')]


def test_js_encode_with_block_modes(tmp_path):
    import carta1_amd as c1
    from carta1_amd import build
    import block_modes_lib as BM
    import oracle_lib as O
    build.build_library()
    if build.build_addon() is None:
        pytest.fail('the N-API addon did not build')
    frames = 130
    chans = [O.gen_pinkT(3, frames * 512), O.gen_white(2, frames * 512)]
    modes = BM.random_modes(20261018, frames, 2)
    ctx = c1.Context(0)
    try:
        units = ctx.encode_modes(chans, modes)
    finally:
        ctx.close()
    assert np.array_equal(units, BM.oracle_encode_modes(chans, modes)[0])
    for c, x in enumerate(chans):
        x.tofile(str(tmp_path / ('ch%d.f32' % c)))
    modes.tofile(str(tmp_path / 'modes.u8'))
    units.tofile(str(tmp_path / 'units.u8'))
    p = subprocess.run([node, os.path.join(ROOT, 'tests', 'js_block_modes.mjs'), str(tmp_path)], cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, universal_newlines=True, timeout=600)
    assert p.returncode == 0 and 'ALL OK' in p.stdout, p.stdout
