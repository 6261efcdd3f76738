"""GPU: many items with the measured block-mode search in one call, from both hosts.  The Python host's
encode_aea_pcm_many(items, measured_allocation=True, measured_mode_candidates=...) against Context.encode_measured_modes for every
item alone, byte for byte; then the JavaScript host's encodeSignalsMeasuredModes over the same items, every channel one signal
(tests/js_signals_measured_modes.mjs), against encodeAeaPcm(item, { measuredAllocation: true, measuredModeCandidates, ... }) and
against the Python host's images, with its errors.  The items are tests/signals_lib.py's: mono of 700 samples, stereo of 1 sample, stereo of unequal channels, mono of
0 samples, stereo of 40 000 samples.  The JavaScript part is skipped when node is not installed."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import signals_lib as SL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
node = shutil.which('node')
pytestmark = pytest.mark.gpu
CANDIDATES = [0, 10, 58]


def kinds():
    import carta1_amd as c1
    assert tuple(c1.SCALE_FACTOR_OFFSETS) == (0, -1, 1, -2, -3)
    return (('sf', dict(scale_factor_offsets=c1.SCALE_FACTOR_OFFSETS)), ('plain', {}))


def per_item(ctx, channels, kw, title='encoded by carta1'):
    """the image of one item by Context.encode_measured_modes alone"""
    import carta1_amd as c1
    frames = (max(len(c) for c in channels) + 511) // 512
    padded = []
    for c in channels:
        p = np.zeros(frames * 512, dtype=np.float32)
        p[:len(c)] = c
        padded.append(p)
    units = ctx.encode_measured_modes(padded, CANDIDATES, **kw)[0] if frames else np.zeros((0, 212), dtype=np.uint8)
    return c1.aea_header(title, units.shape[0], len(channels)) + units.tobytes()


def test_python_many_items_equal_the_per_item_calls():
    import carta1_amd as c1
    items = SL.aea_items()
    ctx = c1.Context(0)
    try:
        plain = c1.encode_aea_pcm_many(items, ctx=ctx)
        assert plain == [c1.encode_aea_pcm(it, ctx=ctx) for it in items]                 # the default arguments: today's bytes
        for tag, kw in kinds():
            many = c1.encode_aea_pcm_many(items, ctx=ctx, measured_allocation=True, measured_mode_candidates=CANDIDATES, **kw)
            assert len(many) == len(items)
            for k, it in enumerate(items):
                assert many[k] == per_item(ctx, it, kw), (tag, 'item', k)
            assert many != c1.encode_aea_pcm_many(items, ctx=ctx, measured_allocation=True, **kw), tag   # the search chose something
            assert many == c1.encode_aea_pcm_many(items, ctx=ctx, measured_allocation=True, measured_mode_candidates=[(0, 0, 0), (2, 2, 0), (2, 2, 3)], **kw)
        titled = c1.encode_aea_pcm_many(items, {'title': ['item %d' % k for k in range(len(items))], 'allocationBias': 2}, ctx=ctx,
                                        measured_allocation=True, measured_mode_candidates=CANDIDATES)
        for k, it in enumerate(items):
            assert titled[k] == per_item(ctx, it, {'options': c1.EncoderOptions({'allocationBias': 2})}, 'item %d' % k), ('titled', k)
        with pytest.raises(ValueError, match='measured_mode_candidates needs measured_allocation'):
            c1.encode_aea_pcm_many(items, ctx=ctx, measured_mode_candidates=CANDIDATES)
        with pytest.raises(ValueError, match='measured_mode_candidates and masking'):
            c1.encode_aea_pcm_many(items, ctx=ctx, measured_allocation=True, measured_mode_candidates=CANDIDATES, masking=True)
    finally:
        ctx.close()


@pytest.mark.skipif(node is None, reason='node is not installed')
def test_js_many_items_equal_the_per_item_calls(tmp_path):
    import carta1_amd as c1
    from carta1_amd import build
    build.build_library()
    if build.build_addon() is None:
        pytest.fail('the N-API addon did not build')
    items = SL.aea_items()
    for k, it in enumerate(items):
        for c, x in enumerate(it):
            np.ascontiguousarray(x, dtype=np.float32).tofile(str(tmp_path / ('item%d_%d.f32' % (k, c))))
    (tmp_path / 'counts.json').write_text(json.dumps([len(it) for it in items]))
    ctx = c1.Context(0)
    try:
        for tag, kw in kinds():
            images = c1.encode_aea_pcm_many(items, ctx=ctx, measured_allocation=True, measured_mode_candidates=CANDIDATES, **kw)
            for k, image in enumerate(images):
                (tmp_path / ('image_%s_%d.aea' % (tag, k))).write_bytes(image)
    finally:
        ctx.close()
    p = subprocess.run([node, os.path.join(ROOT, 'tests', 'js_signals_measured_modes.mjs'), str(tmp_path)], cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, universal_newlines=True, timeout=600)
    assert p.returncode == 0 and 'ALL OK' in p.stdout, p.stdout
