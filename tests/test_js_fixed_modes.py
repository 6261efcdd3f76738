"""GPU: the JavaScript encode() closures and encodeAeaPcm under four fixedBlockModes triples outside the canonical header
values, and decode() / decodeAeaPcm back, against the reference (tests/js_fixed_modes.mjs, tests/golden/fixed_modes.json).
The inputs are rebuilt here and handed over as raw Float32 files.  Skipped when node is not installed."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
node = shutil.which('node')
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(node is None, reason='node is not installed')]
TRIPLES = [(1, 1, 1), (1, 0, 2), (2, 2, 1), (0, 1, 0)]


def test_js_encode_and_decode_under_non_canonical_fixed_modes(tmp_path):
    import fixed_modes_lib as F
    import option_domain_lib as L
    from carta1_amd import build
    build.build_library()
    if build.build_addon() is None:
        pytest.fail('the N-API addon did not build')
    for c in F.fixture()['cases']:
        if F.modes_of(c) in TRIPLES:
            for ch, x in enumerate(L.inputs(c)):
                x.tofile(str(tmp_path / ('case%d_c%d.f32' % (c['id'], ch))))
    p = subprocess.run([node, os.path.join(ROOT, 'tests', 'js_fixed_modes.mjs'), str(tmp_path)], cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, universal_newlines=True, timeout=600)
    assert p.returncode == 0 and 'ALL OK' in p.stdout, p.stdout
