"""GPU: the JavaScript encoder stages (blockSelectorStage, quantizationStage from carta1_amd/js/pipeline/encoder.js) over the
frames of tests/golden/encoder_stages.json against the reference's own outputs, pipe() of the four stages against encode(),
and the reference's messages for a missing bufferPool / options (tests/js_encoder_stages.mjs).  Skipped when node is not
installed."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
node = shutil.which('node')
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(node is None, reason='node is not installed')]


def test_js_encoder_stages_against_reference():
    from carta1_amd import build
    build.build_library()
    if build.build_addon() is None:
        pytest.fail('the N-API addon did not build')
    p = subprocess.run([node, os.path.join(ROOT, 'tests', 'js_encoder_stages.mjs')], cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, universal_newlines=True, timeout=600)
    assert p.returncode == 0 and 'ALL OK' in p.stdout, p.stdout
