"""GPU: the JavaScript host's encodeMeasuredModesMasked, encodeAeaPcm(channels, { measuredAllocation: true, measuredModeCandidates,
modeSearchMasking }) and the encode(options, bufferPool, measured) frame closure with modeSearchMasking
(tests/js_measured_modes_masked.mjs) against the Python host's Context.encode_measured_modes(masking=...) and
EncoderStream.push_measured_modes(masking=...) on the same PCM, candidates, offsets and tables -- 24 mono and 24 stereo frames --
which tests/test_gpu_measured_modes_masked.py and tests/test_gpu_stream_measured_modes_masked.py pin; the new TypeErrors, and
{ measuredModeCandidates, masking } still the TypeError it was.  Skipped when node is not installed."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
node = shutil.which('node')
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(node is None, reason='node is not installed')]
FRAMES = 24


def test_js_encode_measured_modes_masked(tmp_path):
    import carta1_amd as c1
    from carta1_amd import build
    import best_modes_lib as BMO
    import masked_alloc_lib as MK
    build.build_library()
    if build.build_addon() is None:
        pytest.fail('the N-API addon did not build')
    body = [c[:FRAMES * 512] for c in BMO.material('pink')]
    explicit = MK.explicit('self')
    ctx = c1.Context(0)
    try:
        for tag, chans in (('_1', body[:1]), ('_2', body)):
            for suffix, offsets, masking in (('', None, True), ('_s', c1.SCALE_FACTOR_OFFSETS, True), ('_x', c1.SCALE_FACTOR_OFFSETS, explicit)):
                out = ctx.encode_measured_modes(chans, BMO.CANDIDATES, scale_factor_offsets=offsets, return_distortion=True, return_shifts=True,
                                                masking=masking, return_weights=True)
                plain = ctx.encode_measured_modes(chans, BMO.CANDIDATES, scale_factor_offsets=offsets)
                assert not np.array_equal(out[1], plain[1])                    # the weights change the choice
                name = lambda what, ext: str(tmp_path / ('%s%s%s.%s' % (what, tag, suffix, ext)))
                for what, ext, a in zip(('units', 'choice', 'modes', 'taken', 'shifts', 'dist', 'energy', 'weights'),
                                        ('u8', 'u8', 'u8', 'u8', 'i8', 'f64', 'f64', 'f64'), out):
                    a.tofile(name(what, ext))
            for c, x in enumerate(chans):
                np.ascontiguousarray(x).tofile(str(tmp_path / ('ch%d%s.f32' % (c, tag))))
            # the frame closure's twin: one stream, a frame per push
            s = c1.EncoderStream(ctx, len(chans))
            try:
                rows = [s.push_measured_modes([c[f * 512:(f + 1) * 512] for c in chans], BMO.CANDIDATES, scale_factor_offsets=c1.SCALE_FACTOR_OFFSETS,
                                              masking=True) for f in range(FRAMES)]
            finally:
                s.close()
            np.concatenate([r[0] for r in rows]).tofile(str(tmp_path / ('stream_units%s.u8' % tag)))
            np.concatenate([r[2] for r in rows]).tofile(str(tmp_path / ('stream_modes%s.u8' % tag)))
    finally:
        ctx.close()
    np.array(BMO.CANDIDATES, dtype=np.uint8).tofile(str(tmp_path / 'cand.u8'))
    np.ascontiguousarray(explicit[0], dtype=np.float64).tofile(str(tmp_path / 'floor_x.f64'))
    np.ascontiguousarray(explicit[1], dtype=np.float64).tofile(str(tmp_path / 'spread_x.f64'))
    p = subprocess.run([node, os.path.join(ROOT, 'tests', 'js_measured_modes_masked.mjs'), str(tmp_path)], cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, universal_newlines=True, timeout=600)
    assert p.returncode == 0 and 'ALL OK' in p.stdout, p.stdout
