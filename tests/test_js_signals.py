"""Many items in one native call from JavaScript (carta1_amd/js/io/processor.js: encodeAeaPcmMany / decodeAeaPcmMany, the addon's
encodeSignals / decodeSignals) and AudioProcessor.createWavBlob / assemblePcmFrames, through carta1_amd/js/selftest_signals.mjs:
layout, argument shapes, errors and the WAV helpers on the host; on the GPU the many-item functions against the per-item ones
byte for byte, and createWavBlob against decodeAeaToWav16.  Skipped when node is not installed."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JS = os.path.join(ROOT, 'carta1_amd', 'js')

node = shutil.which('node')
pytestmark = pytest.mark.skipif(node is None, reason='node is not installed')


def _run(args):
    from carta1_amd import build
    build.build_library()
    if build.build_addon() is None:
        pytest.fail('the N-API addon did not build')
    p = subprocess.run([node, 'selftest_signals.mjs'] + args, cwd=JS, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       universal_newlines=True, timeout=600)
    return p.returncode, p.stdout


def test_js_signals_host_side():
    rc, out = _run([])
    assert rc == 0 and 'ALL OK' in out, out


@pytest.mark.gpu
def test_js_signals_against_the_per_item_calls_on_gpu():
    rc, out = _run(['--gpu'])
    assert rc == 0 and 'ALL OK' in out, out
