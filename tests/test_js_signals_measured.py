"""GPU: many items with the measured allocation in one call, from both hosts.  The Python host's
encode_aea_pcm_many(items, measured_allocation=True, ...) against Context.encode_measured for every item alone, byte for byte;
then the JavaScript host's encodeAeaPcmMany(items, { measuredAllocation: true, ... }) (tests/js_signals_measured.mjs) against
encodeAeaPcm(item, sameOptions) and against the Python host's images, with its TypeErrors.  The items are
tests/signals_lib.py's: mono of 700 samples, stereo of 1 sample, stereo of unequal channels, mono of 0 samples, stereo of 40 000
samples.  The JavaScript part is skipped when node is not installed."""
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


def kinds():
    import carta1_amd as c1
    return (('measured', {}), ('sf', dict(scale_factor_offsets=c1.SCALE_FACTOR_OFFSETS)),
            ('masked', dict(scale_factor_offsets=c1.SCALE_FACTOR_OFFSETS, masking=True)), ('masking_alone', dict(masking=True)))


def per_item(ctx, channels, kw, title='encoded by carta1'):
    """the image of one item by Context.encode_measured alone"""
    import carta1_amd as c1
    frames = (max(len(c) for c in channels) + 511) // 512
    padded = []
    for c in channels:
        p = np.zeros(frames * 512, dtype=np.float32)
        p[:len(c)] = c
        padded.append(p)
    units = ctx.encode_measured(padded, **kw)[0] if frames else np.zeros((0, 212), dtype=np.uint8)
    return c1.aea_header(title, units.shape[0], len(channels)) + units.tobytes()


def test_python_many_items_equal_the_per_item_calls():
    import carta1_amd as c1
    items = SL.aea_items()
    ctx = c1.Context(0)
    try:
        plain = c1.encode_aea_pcm_many(items, ctx=ctx)
        assert plain == [c1.encode_aea_pcm(it, ctx=ctx) for it in items]                 # the default arguments: today's bytes
        for tag, kw in kinds():
            many = c1.encode_aea_pcm_many(items, ctx=ctx, measured_allocation=True, **kw)
            assert len(many) == len(items)
            for k, it in enumerate(items):
                assert many[k] == per_item(ctx, it, kw), (tag, 'item', k)
            assert many != plain, tag
        titled = c1.encode_aea_pcm_many(items, {'title': ['item %d' % k for k in range(len(items))], 'allocationBias': 2}, ctx=ctx,
                                        measured_allocation=True)
        for k, it in enumerate(items):
            frames = (max(len(c) for c in it) + 511) // 512
            want = per_item(ctx, it, {'options': c1.EncoderOptions({'allocationBias': 2})}, 'item %d' % k) if frames else \
                c1.aea_header('item %d' % k, 0, len(it))
            assert titled[k] == want, ('titled', k)
        with pytest.raises(ValueError, match='need measured_allocation'):
            c1.encode_aea_pcm_many(items, ctx=ctx, scale_factor_offsets=(0, 1))
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
        for tag, kw in kinds()[:3]:
            for k, image in enumerate(c1.encode_aea_pcm_many(items, ctx=ctx, measured_allocation=True, **kw)):
                (tmp_path / ('image_%s_%d.aea' % (tag, k))).write_bytes(image)
    finally:
        ctx.close()
    p = subprocess.run([node, os.path.join(ROOT, 'tests', 'js_signals_measured.mjs'), str(tmp_path)], cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, universal_newlines=True, timeout=600)
    assert p.returncode == 0 and 'ALL OK' in p.stdout, p.stdout
