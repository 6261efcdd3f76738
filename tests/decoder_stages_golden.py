"""Reader of tests/golden/decoder_stages.json (made by tests/golden/gen/gen_decoder_stages.mjs from the reference's own
deserializeFrame, dequantizationStage, imdctStage and qmfSynthesisStage): one dict of numpy arrays per case."""
import json
import os

import numpy as np

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
FIELDS = ('nbfu', 'block_modes', 'sfi', 'wl', 'quantized')


def cases():
    index = json.load(open(os.path.join(G, 'decoder_stages.json')))
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
        arrays['meta'] = case
        if 'source' in case and case['source'].endswith('.units.bin'):
            units = np.fromfile(os.path.join(G, case['source']), dtype=np.uint8).reshape(-1, case['channels'], 212)
            f0 = case['first_frame']
            arrays['units'] = np.ascontiguousarray(units[f0:f0 + case['frames'], case['channel']])
        out[case['name']] = arrays
    return out


def fields_of(case, start=0, stop=None):
    return {k: np.ascontiguousarray(case[k][start:stop]) for k in FIELDS}
