"""GPU: the JavaScript quantize / dequantize wrappers (carta1_amd/js/coding/quantization.js) over every (sfi, bitsPerSample)
record of tests/golden/export_domain.json, against the reference's own outputs, and the arguments they refuse with a
RangeError (tests/js_export_domain.mjs).  Skipped when node is not installed."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
node = shutil.which('node')
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(node is None, reason='node is not installed')]


def test_js_quantize_and_dequantize_over_the_domain():
    from carta1_amd import build
    build.build_library()
    if build.build_addon() is None:
        pytest.fail('the N-API addon did not build')
    p = subprocess.run([node, os.path.join(ROOT, 'tests', 'js_export_domain.mjs')], cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, universal_newlines=True, timeout=600)
    assert p.returncode == 0 and 'ALL OK' in p.stdout, p.stdout
