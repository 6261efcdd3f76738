"""GPU: the JavaScript encode() closure and AudioProcessor.encodeStream (batchFrames 1 and 16) with their EncoderOptions
changed between frames, against the reference's encode() closures under the same changes (tests/js_option_changes.mjs,
tests/golden/option_changes.json).  Skipped when node is not installed."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
node = shutil.which('node')
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(node is None, reason='node is not installed')]


def test_js_encode_follows_option_changes():
    from carta1_amd import build
    build.build_library()
    if build.build_addon() is None:
        pytest.fail('the N-API addon did not build')
    p = subprocess.run([node, os.path.join(ROOT, 'tests', 'js_option_changes.mjs')], cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, universal_newlines=True, timeout=600)
    assert p.returncode == 0 and 'ALL OK' in p.stdout, p.stdout
