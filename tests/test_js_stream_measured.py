"""GPU: the JavaScript host's encode(options, bufferPool, { measuredAllocation: true, scaleFactorOffsets, masking }) frame closure
(tests/js_stream_measured.mjs) against the Python host's EncoderStream.push_measured on the same PCM, which
tests/test_gpu_stream_measured.py pins to the whole-buffer calls and the CPU model: 24 mono frames of pink noise with transients,
frame by frame; the serialised fields are the Python stream's units bit for bit with the tables, with the offsets alone and with
neither; without the third argument, or with measuredAllocation falsy, the closure is today's; the object is read per call; the
TypeErrors.  Skipped when node is not installed."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
node = shutil.which('node')
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(node is None, reason='node is not installed')]
FRAMES = 24


def test_js_frame_closure_with_measured_allocation(tmp_path):
    import carta1_amd as c1
    from carta1_amd import build
    import best_bias_lib as BB
    build.build_library()
    if build.build_addon() is None:
        pytest.fail('the N-API addon did not build')
    pcm = np.ascontiguousarray(BB.material()[1][0][:FRAMES * 512])
    frame = lambda f: [pcm[f * 512:(f + 1) * 512]]
    masked = dict(scale_factor_offsets=c1.SCALE_FACTOR_OFFSETS, masking=True)
    ctx = c1.Context(0)
    try:
        for tag, kw in (('masked', masked), ('sf', dict(scale_factor_offsets=c1.SCALE_FACTOR_OFFSETS)), ('measured', {}), ('plain', None),
                        ('mixed', masked)):
            s = c1.EncoderStream(ctx, 1)
            try:
                units = [s.push(frame(f)) if kw is None or (tag == 'mixed' and f % 2 == 0) else s.push_measured(frame(f), **kw)[0]
                         for f in range(FRAMES)]
            finally:
                s.close()
            np.concatenate(units).tofile(str(tmp_path / ('units_%s.u8' % tag)))
    finally:
        ctx.close()
    pcm.tofile(str(tmp_path / 'ch0.f32'))
    p = subprocess.run([node, os.path.join(ROOT, 'tests', 'js_stream_measured.mjs'), str(tmp_path)], cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, universal_newlines=True, timeout=600)
    assert p.returncode == 0 and 'ALL OK' in p.stdout, p.stdout
