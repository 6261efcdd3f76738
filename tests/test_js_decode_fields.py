"""GPU: the JavaScript decode() closure over frameData objects (carta1_amd/js/pipeline/decoder.js, through the addon's
decStreamPushFields) against the reference's decode() PCM of every case of tests/golden/decoder_stages.json, units and objects
mixed in one closure, and its argument errors (tests/js_decode_fields.mjs).  Skipped when node is not installed."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
node = shutil.which('node')
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(node is None, reason='node is not installed')]


def test_js_decode_closure_on_frame_fields():
    from carta1_amd import build
    build.build_library()
    if build.build_addon() is None:
        pytest.fail('the N-API addon did not build')
    p = subprocess.run([node, os.path.join(ROOT, 'tests', 'js_decode_fields.mjs')], cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, universal_newlines=True, timeout=600)
    assert p.returncode == 0 and 'ALL OK' in p.stdout, p.stdout
