"""GPU: performFFT / detectTransient (carta1_amd/js/analysis/transient.js) and findScaleFactor / allocateBits
(carta1_amd/js/coding/bitallocation.js) against the reference's own functions (tests/golden/decision.json), with the reference's
return types and lengths and the documented RangeErrors (tests/js_decision.mjs).  Skipped when node is not installed."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
node = shutil.which('node')
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(node is None, reason='node is not installed')]


def test_js_decision_functions_against_reference():
    from carta1_amd import build
    build.build_library()
    if build.build_addon() is None:
        pytest.fail('the N-API addon did not build')
    p = subprocess.run([node, os.path.join(ROOT, 'tests', 'js_decision.mjs')], cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, universal_newlines=True, timeout=600)
    assert p.returncode == 0 and 'ALL OK' in p.stdout, p.stdout
