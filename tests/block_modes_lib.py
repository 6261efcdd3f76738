"""Block modes supplied per frame by the caller (c1_encode_modes_*, c1_enc_stream_push_modes): mode bytes, the CPU oracle
run over per-frame and per-channel modes with its states carried, and the plan that drives one encoder stream through an
option schedule of tests/golden/option_changes.json with modes pushes where fixedBlockModes is set (the model the GPU tests
compare against, checked against the fixture on the CPU in tests/test_block_modes_cpu.py)."""
import numpy as np

import option_changes_lib as OC
import stream_state_lib as SL

DOMAIN_TRIPLES = [(a, b, c) for a in (0, 2) for b in (0, 2) for c in (0, 3)]
DOMAIN_BYTES = [a | b << 2 | c << 4 for a, b, c in DOMAIN_TRIPLES]
MAGS = slice(SL.ENC_FIELDS['transient_mags'][0], sum(SL.ENC_FIELDS['transient_mags']))   # transient_mags within a state row


def byte_of(triple):
    return int(triple[0]) | int(triple[1]) << 2 | int(triple[2]) << 4


def triple_of(b):
    return (b & 3, (b >> 2) & 3, (b >> 4) & 3)


def modes_of_units(units):
    """the mode byte of every unit, from its header (OC.unit_modes)"""
    s = OC.unit_modes(units)
    return np.array([byte_of((int(s[i]), int(s[i + 1]), int(s[i + 2]))) for i in range(0, len(s), 3)], dtype=np.uint8)


def oracle_encode_modes(chans, modes, bias=1.0, states=None):
    """the reference with fixedBlockModes = the frame's modes set before every frame, channel by channel: chans = list of
    float32 arrays, modes = uint8 [frames, nch] (or flat).  One oracle call per run of equal modes of a channel, states carried.
    Returns (units [frames * nch, 212], states (nch, 483))."""
    nch = len(chans)
    frames = len(chans[0]) // 512
    m = np.asarray(modes, dtype=np.uint8).reshape(frames, nch)
    st = np.zeros((nch, SL.ENC_FLOATS), dtype=np.float32) if states is None else np.array(states, dtype=np.float32)
    units = np.zeros((frames * nch, 212), dtype=np.uint8)
    for c in range(nch):
        a = 0
        while a < frames:
            b = a + 1
            while b < frames and m[b, c] == m[a, c]:
                b += 1
            u, s = SL.oracle_encode([chans[c][a * 512:b * 512]], {'fixedBlockModes': triple_of(int(m[a, c])), 'allocationBias': bias},
                                    st[c:c + 1])
            units[a * nch + c:b * nch:nch] = u
            st[c] = s[0]
            a = b
    return units, st


# ---- an option schedule as the steps of one stream created under detection ----
def detection_options(v):
    return {'allocationBias': v['allocationBias'], 'transientThresholdLow': v['transientThresholdLow'], 'fixedBlockModes': None}


def plan(per_frame, nch, split=None):
    """[('options', values) | ('plain', a, b) | ('modes', a, b, bytes [b - a, nch])]: options steps only where bias or
    threshold change (never a fixedBlockModes), a modes push for every run of frames with fixedBlockModes set, a plain push
    for every run under detection.  split: no push longer than that many frames."""
    steps = []
    cur = None
    n = len(per_frame)
    a = 0
    while a < n:
        v = per_frame[a]
        key = (v['allocationBias'], v['transientThresholdLow'])
        fixed = v['fixedBlockModes'] is not None
        b = a + 1
        while b < n and (per_frame[b]['allocationBias'], per_frame[b]['transientThresholdLow']) == key and \
                (per_frame[b]['fixedBlockModes'] is not None) == fixed:
            b += 1
        if key != cur:
            steps.append(('options', detection_options(v)))
            cur = key
        k = split or (b - a)
        for x in range(a, b, k):
            y = min(b, x + k)
            if fixed:
                row = np.array([byte_of(per_frame[f]['fixedBlockModes']) for f in range(x, y)], dtype=np.uint8)
                steps.append(('modes', x, y, np.repeat(row[:, None], nch, axis=1)))
            else:
                steps.append(('plain', x, y))
        a = b
    return steps


def run_plan_on_oracle(chans, steps):
    """-> (units, states (nch, 483) after the last step)"""
    nch = len(chans)
    st = np.zeros((nch, SL.ENC_FLOATS), dtype=np.float32)
    out = []
    cur = None
    for step in steps:
        if step[0] == 'options':
            cur = step[1]
            continue
        a, b = step[1], step[2]
        part = [c[a * 512:b * 512] for c in chans]
        if step[0] == 'plain':
            u, st = SL.oracle_encode(part, cur, st)
        else:
            u, st = oracle_encode_modes(part, step[3], cur['allocationBias'], st)
        out.append(u)
    return np.concatenate(out), st


def run_plan_on_stream(stream, options_of, chans, steps):
    """the same steps on a carta1_amd.EncoderStream; options_of(values) -> EncoderOptions"""
    out = []
    for step in steps:
        if step[0] == 'options':
            stream.set_options(options_of(step[1]))
            continue
        a, b = step[1], step[2]
        part = [c[a * 512:b * 512] for c in chans]
        out.append(stream.push(part) if step[0] == 'plain' else stream.push(part, modes=step[3]))
    return np.concatenate(out)


def random_modes(seed, frames, nch):
    """per-frame, per-channel modes over the whole domain; runs of 1 to 9 frames, each channel with its own schedule"""
    rng = np.random.RandomState(seed)
    m = np.zeros((frames, nch), dtype=np.uint8)
    for c in range(nch):
        f = 0
        while f < frames:
            k = int(rng.randint(1, 10))
            m[f:f + k, c] = DOMAIN_BYTES[int(rng.randint(0, 8))]
            f += k
    return m


def alternating_modes(frames, nch):
    """000, 223, 000, ... every frame, on every channel"""
    return np.repeat(np.where(np.arange(frames) % 2 == 0, byte_of((0, 0, 0)), byte_of((2, 2, 3))).astype(np.uint8)[:, None], nch, axis=1)
