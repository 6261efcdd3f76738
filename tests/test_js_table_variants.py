"""The JavaScript host under another engine's Math (tests/js_table_variants.mjs): with Math.sin / cos / pow wrapped as the
reference was for tests/golden/table_variants.json, buildNativeTables() -- what native.js hands c1_set_tables() -- equals
the tables the reference built; on the GPU, encode() / decode() then reproduce the reference's units and decoded frames.
Skipped when node is not installed."""
import os
import shutil
import subprocess

import pytest

import table_variants_lib as TV

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
node = shutil.which('node')
pytestmark = pytest.mark.skipif(node is None, reason='node is not installed')


def run(*args):
    p = subprocess.run([node, os.path.join(ROOT, 'tests', 'js_table_variants.mjs')] + list(args), cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=600)
    assert p.returncode == 0 and 'ALL OK' in p.stdout, p.stdout


@pytest.mark.parametrize('name', TV.names())
def test_js_host_builds_the_variant_tables(name):
    run(name)


@pytest.mark.gpu
@pytest.mark.parametrize('name', TV.names())
def test_js_host_encodes_and_decodes_under_the_variant(name):
    from carta1_amd import build
    build.build_library()
    if build.build_addon() is None:
        pytest.fail('the N-API addon did not build')
    run(name, 'gpu')
