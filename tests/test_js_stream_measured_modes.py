"""GPU: the JavaScript host's encode(options, bufferPool, { measuredAllocation: true, measuredModeCandidates, scaleFactorOffsets })
frame closure (tests/js_stream_measured_modes.mjs) against the Python host's EncoderStream.push_measured_modes on the same PCM,
which tests/test_gpu_stream_measured_modes.py pins to the whole-buffer call and the CPU model: 24 mono frames of pink noise with
transients, frame by frame; the serialised fields are the Python stream's units bit for bit with and without the offsets, and the
fields' blockModes are the unit's, also under fixedBlockModes; the object is read per call; the TypeErrors.  Skipped when node is
not installed."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
node = shutil.which('node')
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(node is None, reason='node is not installed')]
FRAMES = 24


def test_js_frame_closure_with_measured_mode_candidates(tmp_path):
    import carta1_amd as c1
    from carta1_amd import build
    import best_bias_lib as BB
    import measured_modes_lib as MM
    build.build_library()
    if build.build_addon() is None:
        pytest.fail('the N-API addon did not build')
    pcm = np.ascontiguousarray(BB.material()[1][0][:FRAMES * 512])
    frame = lambda f: [pcm[f * 512:(f + 1) * 512]]
    ctx = c1.Context(0)
    try:
        for tag, offsets, mixed in (('sf', c1.SCALE_FACTOR_OFFSETS, False), ('plain', None, False), ('mixed', c1.SCALE_FACTOR_OFFSETS, True)):
            s = c1.EncoderStream(ctx, 1)
            try:
                out = [(s.push(frame(f)), None) if mixed and f % 2 == 0 else
                       s.push_measured_modes(frame(f), MM.CANDIDATES, scale_factor_offsets=offsets)[0:3:2] for f in range(FRAMES)]
            finally:
                s.close()
            np.concatenate([u for u, _ in out]).tofile(str(tmp_path / ('units_%s.u8' % tag)))
            if not mixed:
                modes = np.concatenate([m for _, m in out])
                assert len(set(modes.tolist())) > 1                            # the candidates decide something
                modes.tofile(str(tmp_path / ('modes_%s.u8' % tag)))
    finally:
        ctx.close()
    pcm.tofile(str(tmp_path / 'ch0.f32'))
    p = subprocess.run([node, os.path.join(ROOT, 'tests', 'js_stream_measured_modes.mjs'), str(tmp_path)], cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, universal_newlines=True, timeout=600)
    assert p.returncode == 0 and 'ALL OK' in p.stdout, p.stdout
