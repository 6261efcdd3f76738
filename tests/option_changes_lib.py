"""Option schedules on one encoder stream (tests/golden/option_changes.json, gen_option_changes.mjs): the fixture, its signals,
and the CPU oracle run segment by segment with its states carried (the model the GPU tests compare against)."""
import hashlib
import json
import os

import numpy as np

import oracle_lib as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'option_changes.json')
_GEN = {'white': O.gen_white, 'pinkT': O.gen_pinkT}


def fixture():
    with open(GOLDEN) as f:
        return json.load(f)


def signal(spec, frames):
    """the fixture's channels: [[generator, seed], ...] -> float32 arrays of frames * 512 samples"""
    return [_GEN[g](seed, frames * 512) for g, seed in spec]


def options_at(initial, changes, frames):
    """the option values of every frame: the reference's defaults, then `initial`, then each change before its frame"""
    cur = {'transientThresholdLow': 1.0, 'allocationBias': 1.0, 'fixedBlockModes': None}
    cur.update(initial)
    by_frame = {}
    for f, change in changes:
        by_frame.setdefault(f, []).append(change)
    out = []
    for f in range(frames):
        for change in by_frame.get(f, []):
            cur = dict(cur, **change)
        out.append(dict(cur))
    return out


def segments(per_frame):
    """runs of equal options: [(first frame, end frame, values), ...]"""
    runs = []
    for f, v in enumerate(per_frame):
        if runs and runs[-1][2] == v:
            runs[-1] = (runs[-1][0], f + 1, v)
        else:
            runs.append((f, f + 1, v))
    return runs


def oracle_args(v):
    modes = v['fixedBlockModes']
    return dict(fixed_modes=tuple(modes) if modes is not None else None, bias=v['allocationBias'],
                threshold=v['transientThresholdLow'])


def oracle_encode(chans, per_frame):
    """the CPU oracle over the schedule: one encode_stream call per run of equal options, states carried"""
    states = None
    parts = []
    for a, b, v in segments(per_frame):
        units, states = O.encode_stream([c[a * 512:b * 512] for c in chans], states=states, **oracle_args(v))
        parts.append(units)
    return np.concatenate(parts)


def unit_modes(units):
    """the block modes of every unit from its header (serializeFrame: 2 - low, 2 - mid, 3 - high in the top bits)"""
    b = np.asarray(units, dtype=np.uint8).reshape(-1, 212)[:, 0].astype(np.int32)
    return ''.join('%d%d%d' % (2 - ((x >> 6) & 3), 2 - ((x >> 4) & 3), 3 - ((x >> 2) & 3)) for x in b)


def sha(units):
    return hashlib.sha256(np.ascontiguousarray(units, dtype=np.uint8).tobytes()).hexdigest()


def check_against(result, units, nch):
    """compare units [frames * nch, 212] with one fixture result; returns a message or None"""
    if unit_modes(units) != result['modes']:
        return 'block modes differ'
    for f, hexed in result['switch_units'].items():
        f = int(f)
        got = np.ascontiguousarray(units[f * nch:(f + 2) * nch]).tobytes().hex()
        if got != hexed:
            return 'units at the switch before frame %d differ' % f
    if sha(units) != result['sha256']:
        return 'SHA-256 of all units differs'
    return None
