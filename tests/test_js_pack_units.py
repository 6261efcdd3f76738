"""GPU: serializeFrames (carta1_amd/js/io/serialization.js) against the reference's own serializeFrame
(tests/golden/pack_units.json), pipe() of the four JavaScript encoder stages followed by serializeFrames against the committed
KAT units, and its RangeErrors (tests/js_pack_units.mjs).  Skipped when node is not installed."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
node = shutil.which('node')
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(node is None, reason='node is not installed')]


def test_js_serialize_frames_against_reference():
    from carta1_amd import build
    build.build_library()
    if build.build_addon() is None:
        pytest.fail('the N-API addon did not build')
    p = subprocess.run([node, os.path.join(ROOT, 'tests', 'js_pack_units.mjs')], cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, universal_newlines=True, timeout=600)
    assert p.returncode == 0 and 'ALL OK' in p.stdout, p.stdout
