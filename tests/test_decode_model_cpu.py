"""No GPU: the decode model's symbols (c1_ctx_set_decode_model / c1_ctx_get_decode_model) in the header, the library and the
Python binding; their NULL-context errors; the Python precision keyword's ValueErrors and the JavaScript option's TypeErrors,
all raised before any library call."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ('c1_ctx_set_decode_model', 'c1_ctx_get_decode_model')
node = shutil.which('node')


def header():
    with open(os.path.join(ROOT, 'include', 'carta1_hip.h')) as f:
        return f.read()


def test_symbols_are_declared_exported_and_bound():
    from carta1_amd import capi
    h = header()
    lib = capi.load()
    for name in SYMBOLS:
        assert re.search(r'^int %s\(c1_ctx \*ctx, int \*?model\);' % name, h, re.M), name
        assert name in capi.SIGNATURES and getattr(lib, name) is not None, name
    for name, value in (('C1_DECODE_EXACT', 0), ('C1_DECODE_BINARY32_BULK', 1), ('C1_DECODE_BINARY32', 2)):
        assert re.search(r'^#define %s %d$' % (name, value), h, re.M), name
    assert re.search(r'^#define C1_ABI_VERSION 3$', h, re.M) and lib.c1_abi_version() == 3, 'the ABI version stays'
    import carta1_amd as c1
    assert (c1.DECODE_EXACT, c1.DECODE_BINARY32_BULK, c1.DECODE_BINARY32) == (0, 1, 2)
    assert callable(c1.Context.set_decode_model) and isinstance(c1.Context.decode_model, property)


def test_null_context_is_an_error():
    from carta1_amd import capi
    lib = capi.load()
    m = C.c_int(7)
    assert lib.c1_ctx_set_decode_model(None, 2) == 1                 # C1_ERR_ARG
    assert b'NULL' in lib.c1_last_error()
    assert lib.c1_ctx_get_decode_model(None, C.byref(m)) == 1 and m.value == 7
    assert lib.c1_ctx_set_decode_precision(None, 1) == 1


class NoLibrary:
    """stands in for a context: any use of it is a failure"""

    def __getattr__(self, name):
        raise AssertionError('the context was used (%s) before the precision was checked' % name)


@pytest.mark.parametrize('bad', ['float', 'BINARY32', 'binary64', '', 2, True, b'exact'])
def test_python_precision_errors_come_before_any_library_call(bad, monkeypatch):
    import carta1_amd as c1
    from carta1_amd import capi, codec

    def no_load():
        raise AssertionError('the library was loaded before the precision was checked')
    monkeypatch.setattr(capi, 'load', no_load)
    units = np.zeros((2, 212), dtype=np.uint8)
    image = c1.aea_header('t', 2, 1) + units.tobytes()
    for ctx in (None, NoLibrary()):
        with pytest.raises(ValueError, match='precision'):
            c1.decode_units(units, 1, ctx=ctx, precision=bad)
        with pytest.raises(ValueError, match='precision'):
            c1.decode_aea_pcm(image, ctx=ctx, precision=bad)
        with pytest.raises(ValueError, match='precision'):
            c1.decode_aea_pcm_many([image], ctx=ctx, precision=bad)
    assert codec.check_precision(None) is None and codec.check_precision('exact') == 0 and codec.check_precision('binary32') == 2


@pytest.mark.skipif(node is None, reason='node is not installed')
def test_js_precision_errors_need_no_device():
    p = subprocess.run([node, os.path.join(ROOT, 'tests', 'js_decode_model.mjs'), 'errors'], cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, universal_newlines=True, timeout=120,
                       env=dict(os.environ, HIP_VISIBLE_DEVICES='-1', ROCR_VISIBLE_DEVICES='-1'))
    assert p.returncode == 0 and 'ALL OK' in p.stdout, p.stdout
