"""CPU: decoding from frame fields -- c1_decode_fields_device, c1_decode_fields_batch and c1_dec_stream_push_fields -- is
declared, exported and bound, with its Python and N-API names; and the route it replaces in the JavaScript decode() closure
(serializeFrame, then decoding the unit) does not reproduce the reference's decode() on the hand-built fields of
tests/golden/decoder_stages.json, as the CPU oracle and the NumPy serializeFrame model show."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import decoder_stages_golden as DG
import oracle_lib as O
import pack_units_model as PM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('c1_decode_fields_device', 'c1_decode_fields_batch', 'c1_dec_stream_push_fields')


def test_symbols_declared_exported_and_bound():
    from carta1_amd import build, capi
    build.build_library()
    lib = capi.load()
    header = open(os.path.join(ROOT, 'include', 'carta1_hip.h')).read()
    for name in NAMES:
        assert re.search(r'^int %s\(' % name, header, re.M), name
        assert hasattr(lib, name), name
        assert name in capi.SIGNATURES, name
    assert '"decode_fields"' in header                      # the c1_ctx_kernel_ms name
    assert re.search(r'^#define C1_ABI_VERSION 3$', header, re.M)


def test_python_methods_exist():
    import carta1_amd as c1
    assert callable(getattr(c1.Context, 'decode_fields', None))
    assert callable(getattr(c1.Context, 'decode_fields_device', None))
    assert callable(getattr(c1.DecoderStream, 'push_fields', None))


@pytest.mark.skipif(shutil.which('node') is None, reason='node is not installed')
def test_addon_exports():
    from carta1_amd import build
    build.build_library()
    if build.build_addon() is None:
        pytest.skip('no node headers: the N-API addon is not built')
    p = subprocess.run([shutil.which('node'), '-e',
                        "const a = require('./carta1_amd/js/addon/carta1_napi.node');"
                        "console.log(typeof a.decodeFieldsBatch, typeof a.decStreamPushFields)"],
                       cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=120)
    assert p.stdout.split() == ['function', 'function'], p.stdout


def test_serialize_round_trip_does_not_decode_as_the_reference():
    # the hand-built case holds fields serializeFrame cannot carry (nBfu outside BFU_AMOUNTS, mode 1, wide mantissas):
    # decoding them through a unit, as the closure used to, gives other PCM than the reference's decode() of the fields
    case = DG.cases()['fields']
    units = PM.pack(DG.fields_of(case))
    pcm, _ = O.decode_stream(units, 1)
    got = np.asarray(pcm[0], dtype=np.float32).reshape(-1, 512)
    want = case['pcm']
    assert got.shape == want.shape
    differs = (got.view(np.uint32) != want.view(np.uint32)).any(axis=1)
    assert differs.any()
