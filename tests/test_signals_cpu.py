"""CPU-only: the library exports the c1_*_signals* entry points, capi binds them with the header's argument types, and the pure
host part of the many-item functions (splitting items into signals, offsets, padding, interleaving units into L, R order and
back, reading an AEA image) round-trips.  No device is touched."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('c1_encode_signals_device', 'c1_decode_signals_device', 'c1_encode_signals', 'c1_decode_signals')


@pytest.fixture(scope='module')
def lib():
    from carta1_amd import build, capi
    build.build_library()
    return capi.load()


def header_params(name):
    header = open(os.path.join(ROOT, 'include', 'carta1_hip.h')).read()
    m = re.search(r'^int %s\s*\(([^;]*)\);' % name, header, re.M | re.S)
    assert m, name + ' is not declared in the header'
    return [re.sub(r'/\*.*?\*/', '', p, flags=re.S).strip() for p in m.group(1).split(',')]


def ctype_of(param):
    """the ctypes type a header parameter is bound with in capi.SIGNATURES"""
    from carta1_amd import capi
    if re.match(r'const c1_encode_options \*', param):
        return C.POINTER(capi.EncodeOptions)
    if re.match(r'const int64_t \*', param):
        return C.POINTER(C.c_int64)
    if '*' in param:
        return C.c_void_p
    assert re.match(r'int64_t \w+$', param), param
    return C.c_int64


@pytest.mark.parametrize('name', NAMES)
def test_signals_entry_points_are_exported_and_bound_as_declared(lib, name):
    from carta1_amd import capi
    fn = getattr(lib, name)
    params = header_params(name)
    res, args = capi.SIGNATURES[name]
    assert res is C.c_int and fn.restype is C.c_int
    assert [ctype_of(p) for p in params] == list(args) == list(fn.argtypes), params
    names = [re.search(r'(\w+)$', p).group(1) for p in params]
    if 'encode' in name:
        assert names == ['ctx', 'n', 'frame_offsets', 'pcm', 'in', 'opts', 'units', 'out']
    else:
        assert names == ['ctx', 'n', 'frame_offsets', 'units', 'in', 'pcm', 'out']
    assert lib.c1_abi_version() == 3


def test_signals_calls_without_a_context_fail_loudly(lib):
    from carta1_amd import capi
    off = (C.c_int64 * 1)(0)
    for name in NAMES:
        args = [None, 0, off] + [None] * (len(capi.SIGNATURES[name][1]) - 3)
        assert getattr(lib, name)(*args) == 1                      # C1_ERR_ARG: the context is NULL
        assert b'context' in lib.c1_last_error()


def test_pad_and_layout():
    from carta1_amd import codec as K
    rng = np.random.RandomState(1)
    raw = [rng.uniform(-1, 1, n).astype(np.float32) for n in (0, 1, 511, 512, 513, 1024, 700)]
    sigs = [K.pad_signal(x) for x in raw]
    for x, p in zip(raw, sigs):
        assert p.dtype == np.float32 and p.size == (x.size + 511) // 512 * 512
        assert np.array_equal(p[:x.size], x) and not p[x.size:].any()
    assert np.shares_memory(K.pad_signal(raw[3]), raw[3])                          # whole frames are passed through
    assert K.pad_signal(np.arange(3, dtype=np.float64)).dtype == np.float32
    pcm, off = K.signals_layout(sigs)
    assert off.dtype == np.int64 and list(off) == [0, 0, 1, 2, 3, 5, 7, 9]
    assert pcm.dtype == np.float32 and pcm.flags['C_CONTIGUOUS'] and pcm.size == 9 * 512
    for i, p in enumerate(sigs):
        assert np.array_equal(pcm[off[i] * 512:off[i + 1] * 512], p)
    pcm, off = K.signals_layout([])
    assert pcm.size == 0 and list(off) == [0]
    with pytest.raises(ValueError):
        K.signals_layout([np.zeros(100, dtype=np.float32)])
    rows = (np.arange(9 * 212) % 251).astype(np.uint8).reshape(9, 212)
    parts = K.split_rows(rows, np.array([0, 0, 1, 2, 3, 5, 7, 9]))
    assert [p.shape[0] for p in parts] == [0, 1, 1, 1, 2, 2, 2] and np.array_equal(np.concatenate(parts), rows)


def test_items_round_trip_through_signals_and_interleaved_units():
    from carta1_amd import codec as K
    rng = np.random.RandomState(2)

    def f32(n):
        return rng.uniform(-1, 1, n).astype(np.float32)
    items = [[f32(700)], [f32(1), f32(1)], [f32(1300), f32(900)], [f32(0)], [f32(40000), f32(40000)], [f32(0), f32(0)]]
    signals, counts = K.items_to_signals(items)
    assert counts == [1, 2, 2, 1, 2, 2] and len(signals) == 10
    frames = [2, 1, 1, 3, 3, 0, 79, 79, 0, 0]
    assert [s.size for s in signals] == [n * 512 for n in frames]
    flat = [c for item in items for c in item]
    for x, s in zip(flat, signals):
        assert s.dtype == np.float32 and np.array_equal(s[:x.size], x) and not s[x.size:].any()
    # units that name their signal and frame: interleaved L, R per item, and back
    units = [np.zeros((n, 212), dtype=np.uint8) for n in frames]
    for i, u in enumerate(units):
        u[:, 0] = i
        u[:, 1] = np.arange(u.shape[0]) % 256
    per_item = K.interleave_item_units(units, counts)
    assert [u.shape[0] for u in per_item] == [2, 2, 6, 0, 158, 0]
    stereo = per_item[2]
    assert list(stereo[:, 0]) == [3, 4, 3, 4, 3, 4] and list(stereo[:, 1]) == [0, 0, 1, 1, 2, 2]
    back = K.deinterleave_item_units(per_item, counts)
    assert len(back) == len(units) and all(np.array_equal(a, b) for a, b in zip(back, units))
    with pytest.raises(ValueError):
        K.deinterleave_item_units([np.zeros((3, 212), dtype=np.uint8)], [2])
    with pytest.raises(TypeError):
        K.items_to_signals([[np.zeros(4, dtype=np.float64)]])
    with pytest.raises(TypeError):
        K.items_to_signals([[]])


def test_aea_image_units_reads_a_file_as_the_reference_does():
    from carta1_amd import codec as K
    body = (np.arange(5 * 212) % 253).astype(np.uint8)
    mono = K.aea_header('m', 5, 1) + body.tobytes() + b'\x01\x02\x03'        # a trailing partial unit is dropped
    u, nch = K.aea_image_units(mono)
    assert nch == 1 and u.shape == (5, 212) and np.array_equal(u.reshape(-1), body)
    stereo = K.aea_header('s', 5, 2) + body.tobytes()                          # a lone trailing left unit gets the dummy partner
    u, nch = K.aea_image_units(bytearray(stereo))
    assert nch == 2 and u.shape == (6, 212) and np.array_equal(u[:5].reshape(-1), body)
    assert u[5, 0] == 0xAC and not u[5, 1:].any()
    u, nch = K.aea_image_units(np.frombuffer(K.aea_header('', 0, 2), dtype=np.uint8))
    assert nch == 2 and u.shape == (0, 212)
    with pytest.raises(TypeError):
        K.aea_image_units('text')
    with pytest.raises(ValueError):
        K.aea_image_units(K.aea_header('x', 0, 3))
