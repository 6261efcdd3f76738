"""The fixed-modes fixture (tests/golden/fixed_modes.json, written by tests/golden/gen/gen_fixed_modes.mjs from the
reference encoder under every fixedBlockModes triple the library accepts: low and mid band 0..2, high band 0..3) and the
partition of those 36 triples.

A band is coded in short blocks when its mode is non-zero and long when it is zero (quantization.js:117 and the MDCT test
blockMode === 0); the value of a non-zero mode reaches the sound unit only through the header, which carries 2 - m0,
2 - m1, 3 - m2 in the top six bits of byte 0 (serialization.js:48-50).  So the triples fall into the 8 classes of
(m0 != 0, m1 != 0, m2 != 0): within a class the units differ in those six bits alone and decode to the same PCM.

The inputs are option_domain_lib's `patch` material, rebuilt bit for bit (test_fixed_modes_cpu.py checks the hashes)."""
import json
import os

import numpy as np

import option_domain_lib as L

G = L.G
TRIPLES = [(a, b, c) for a in range(3) for b in range(3) for c in range(4)]
CANONICAL_TESTED = [(0, 0, 0), (2, 2, 3), (0, 2, 0), (2, 0, 3), (2, 2, 0), (0, 2, 3)]   # what the suite ran before this fixture
_fixture = None


def fixture():
    """the JSON, with each case's 2-byte unit digests (fixed_modes_digests.bin) attached as `digests`"""
    global _fixture
    if _fixture is None:
        fx = json.load(open(os.path.join(G, 'fixed_modes.json')))
        dig = np.fromfile(os.path.join(G, 'fixed_modes_digests.bin'), dtype=np.uint8).reshape(-1, 2)
        at = 0
        for c in fx['cases']:
            n = c['frames'] * c['channels']
            c['digests'] = dig[at:at + n]
            at += n
        assert at == dig.shape[0]
        _fixture = fx
    return _fixture


def modes_of(case):
    return tuple(case['options']['fixedBlockModes'])


def stereo_cases():
    """the 36 cases of 40 stereo frames, in TRIPLES order"""
    return [c for c in fixture()['cases'] if c['channels'] == 2]


def short_cases():
    """the mono cases of 3 frames"""
    return [c for c in fixture()['cases'] if c['channels'] == 1]


def class_of(modes):
    return tuple(int(m != 0) for m in modes)


def canonical(modes):
    """the triple of the class that the canonical header values 0 | 2, 0 | 2, 0 | 3 name"""
    k = class_of(modes)
    return (2 * k[0], 2 * k[1], 3 * k[2])


def classes():
    """{class: its triples}, 8 classes, 36 triples in all"""
    out = {}
    for t in TRIPLES:
        out.setdefault(class_of(t), []).append(t)
    return out


ALL_SHORT = classes()[(1, 1, 1)]                       # the 12 triples the host sends to the speculative all-short analysis


def mode_bits(modes):
    """the top six bits of a unit's byte 0 (serialization.js:48-50), in place"""
    return ((2 - modes[0]) << 6 | (2 - modes[1]) << 4 | (3 - modes[2]) << 2) & 0xFC


def mode_byte(modes):
    """m0 | m1 << 2 | m2 << 4, as pack_block_modes() and the kernels' side records carry it"""
    return modes[0] | modes[1] << 2 | modes[2] << 4


def without_mode_bits(units):
    u = np.array(units, dtype=np.uint8).reshape(-1, 212)
    u[:, 0] &= 0x03
    return u


def assert_same_but_mode_bits(units_a, modes_a, units_b, modes_b, what=''):
    """units of two triples of one class: the six mode bits are each triple's own, everything else is equal"""
    a = np.asarray(units_a, dtype=np.uint8).reshape(-1, 212)
    b = np.asarray(units_b, dtype=np.uint8).reshape(-1, 212)
    assert a.shape == b.shape and a.shape[0] > 0, (what, a.shape, b.shape)
    assert ((a[:, 0] & 0xFC) == mode_bits(modes_a)).all(), (what, modes_a, 'mode bits', np.unique(a[:, 0] & 0xFC))
    assert ((b[:, 0] & 0xFC) == mode_bits(modes_b)).all(), (what, modes_b, 'mode bits', np.unique(b[:, 0] & 0xFC))
    diff = np.nonzero((without_mode_bits(a) != without_mode_bits(b)).any(axis=1))[0]
    assert diff.size == 0, (what, modes_a, modes_b, 'first unit that differs outside the mode bits', int(diff[0]))
