"""The JavaScript BufferPool's state in the reference's layout (carta1_amd/js/core/buffers.js, selftest_state.mjs): getter
shapes, a set kept until the stream exists and bad shapes on the host; on the GPU, encode() and decode() continued from the
reference's dumped pools (tests/golden/stream_state.json), from forked pools and from foreign ones.  Skipped when node is
not installed."""
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
    p = subprocess.run([node, 'selftest_state.mjs'] + args, cwd=JS, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       universal_newlines=True, timeout=600)
    return p.returncode, p.stdout


def test_js_pool_state_host_side():
    rc, out = _run([])
    assert rc == 0 and 'ALL OK' in out, out


@pytest.mark.gpu
def test_js_pool_state_against_reference_on_gpu():
    rc, out = _run(['--gpu'])
    assert rc == 0 and 'ALL OK' in out, out
