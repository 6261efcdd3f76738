"""Reader of tests/golden/encoder_stages.json (made by tests/golden/gen/gen_encoder_stages.mjs from the reference's own
qmfAnalysisStage, blockSelectorStage, mdctStage and quantizationStage): one dict of numpy arrays per case, with the bands and
coefficients other cases share filled in and the mantissas widened to int32."""
import json
import os
import struct

import numpy as np

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
FIELDS = ('nbfu', 'block_modes', 'sfi', 'wl', 'quantized')


def cases():
    index = json.load(open(os.path.join(G, 'encoder_stages.json')))
    out = {}
    for case in index['cases']:
        raw = open(os.path.join(G, case['file']), 'rb').read()
        at, arrays = 0, {}
        for a in case['arrays']:
            dt = np.dtype(a['dtype']).newbyteorder('<')
            n = int(np.prod(a['shape']))
            arrays[a['name']] = np.frombuffer(raw, dtype=dt, count=n, offset=at).reshape(a['shape']).astype(a['dtype'])
            at += n * dt.itemsize
        assert at == len(raw), case['file']
        if 'quantized' in arrays:
            arrays['quantized'] = arrays['quantized'].astype(np.int32)
        if 'biased' in case:
            arrays['biased'] = np.array([struct.unpack('>d', bytes.fromhex(h))[0] for h in case['biased']])
        arrays['meta'] = case
        out[case['name']] = arrays
    for case in out.values():
        meta = case['meta']
        for key, ref in (('bands', 'bands_from'), ('coefficients', 'coefs_from')):
            if key not in case and ref in meta:
                case[key] = out[meta[ref]][key]
    return out


def fields_of(case):
    return {k: np.ascontiguousarray(case[k]) for k in FIELDS}
