"""GPU: the JavaScript decode option { precision: 'exact' | 'binary32' } (carta1_amd/js/native.js, pipeline/decoder.js,
io/processor.js) against this host's results under decode model 2 on 24 mono and 24 stereo frames, bit for bit; its RMS against
the exact decode; the exact results without the option; a pool switched after 12 frames against a DecoderStream whose context
is switched at the same frame (tests/js_decode_model.mjs).  Skipped when node is not installed."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
node = shutil.which('node')
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(node is None, reason='node is not installed')]
FRAMES, SWITCH = 24, 12


def expected():
    import carta1_amd as c1
    units = np.fromfile(os.path.join(ROOT, 'tests', 'golden', 'kat64_pinkT_detect_thr0.3.units.bin'), dtype=np.uint8).reshape(-1, 2, 212)
    stereo = np.ascontiguousarray(units[:FRAMES].reshape(-1, 212))
    mono = np.ascontiguousarray(units[:FRAMES, 0])
    ctx = c1.Context(0)
    try:
        exact = ctx.decode(mono, 1) + ctx.decode(stereo, 2)
        wav = ctx.decode_wav16(mono, 1)
        ctx.set_decode_model(c1.DECODE_BINARY32)
        b32 = ctx.decode(mono, 1) + ctx.decode(stereo, 2)
        wav32 = ctx.decode_wav16(mono, 1)
        ctx.set_decode_model(c1.DECODE_EXACT)
        s = c1.DecoderStream(ctx, 1)
        parts = [s.push(mono[f:f + 1])[0] for f in range(SWITCH)]
        ctx.set_decode_model(c1.DECODE_BINARY32)
        parts += [s.push(mono[f:f + 1])[0] for f in range(SWITCH, FRAMES)]
        s.close()
    finally:
        ctx.close()
    for a, b in zip(b32, exact):
        assert np.sqrt(np.mean((a.astype(np.float64) - b) ** 2)) <= 1e-5 and not np.array_equal(a, b)
    arrays = b32 + exact + [np.concatenate(parts), np.asarray(wav32).reshape(-1).astype(np.float32), np.asarray(wav).reshape(-1).astype(np.float32)]
    assert all(a.size == FRAMES * 512 for a in arrays)
    return np.concatenate(arrays).astype(np.float32)


def test_js_decode_precision_option(tmp_path):
    from carta1_amd import build
    build.build_library()
    if build.build_addon() is None:
        pytest.fail('the N-API addon did not build')
    path = tmp_path / 'expected.f32'
    expected().tofile(str(path))
    p = subprocess.run([node, os.path.join(ROOT, 'tests', 'js_decode_model.mjs')], cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, universal_newlines=True, timeout=600,
                       env=dict(os.environ, C1_DECODE_MODEL_EXPECTED=str(path)))
    print(p.stdout)
    assert p.returncode == 0 and 'ALL OK' in p.stdout, p.stdout
