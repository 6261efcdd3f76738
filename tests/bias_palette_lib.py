"""The allocation bias supplied per frame and channel from a palette (c1_encode_biases_*, c1_enc_stream_push_biases): the CPU
oracle run over a per-unit (bias, mode) schedule with its states carried, generators for index schedules, and the plan that
drives one encoder stream through an option schedule of tests/golden/option_changes.json with the bias given only through
the pushes (the model the GPU tests compare against, checked against the fixture on the CPU in
tests/test_bias_palette_cpu.py)."""
import numpy as np

import block_modes_lib as BM
import oracle_lib as O
import stream_state_lib as SL

PACKAGED_BIASES = (0, 0.25, 0.5, 1, 1.5, 2, 3.3, 5)      # carta1_amd/biased_tables.json: V8's pow for these


def entry_table(entry):
    """a palette entry is an allocation bias (a number) or an explicit biased scale-factor table (64 doubles)"""
    if np.ndim(entry) == 0:
        return O.biased_table(float(entry))
    t = np.asarray(entry, dtype=np.float64)
    assert t.shape == (64,)
    return t


def oracle_encode_schedule(chans, palette, index, modes=None, base=None, states=None):
    """the reference with allocationBias (and, modes given, fixedBlockModes) set before every frame, channel by channel.
    chans: list of float32 arrays; palette: list of entries (entry_table); index: [frames, nch] (or flat) palette indices;
    modes: None or uint8 mode bytes [frames, nch]; base: the other option values ({'transientThresholdLow', 'fixedBlockModes'})
    when modes is None.  One oracle call per run of equal (entry, mode) of a channel, states carried.
    Returns (units [frames * nch, 212], states (nch, 483))."""
    nch = len(chans)
    frames = len(chans[0]) // 512
    idx = np.asarray(index).reshape(frames, nch)
    m = None if modes is None else np.asarray(modes, dtype=np.uint8).reshape(frames, nch)
    base = base or {}
    tables = [entry_table(e) for e in palette]
    st = np.zeros((nch, SL.ENC_FLOATS), dtype=np.float32) if states is None else np.array(states, dtype=np.float32)
    units = np.zeros((frames * nch, 212), dtype=np.uint8)
    for c in range(nch):
        a = 0
        while a < frames:
            b = a + 1
            while b < frames and idx[b, c] == idx[a, c] and (m is None or m[b, c] == m[a, c]):
                b += 1
            fixed = BM.triple_of(int(m[a, c])) if m is not None else base.get('fixedBlockModes')
            u, s = O.encode_stream([chans[c][a * 512:b * 512]], fixed_modes=tuple(fixed) if fixed is not None else None,
                                   threshold=base.get('transientThresholdLow', 1.0), states=SL.enc_states_to_oracle(st[c:c + 1]),
                                   biased=tables[int(idx[a, c])])
            units[a * nch + c:b * nch:nch] = u
            st[c] = SL.enc_states_from_oracle(s)[0]
            a = b
    return units, st


def palette_of(biases):
    """per-unit bias values -> (sorted distinct values, index of every value), as carta1_amd.codec.bias_palette orders them"""
    b = np.asarray(biases, dtype=np.float64)
    values, index = np.unique(b.reshape(-1), return_inverse=True)
    return [float(v) for v in values], index.reshape(b.shape).astype(np.uint8)


def differing_units(units_a, units_b):
    return int((np.asarray(units_a) != np.asarray(units_b)).any(axis=1).sum())


# ---- index schedules ----
def random_index(seed, frames, nch, n):
    """runs of 1 to 9 frames, each channel on its own schedule, entries drawn from 0 .. n - 1"""
    rng = np.random.RandomState(seed)
    idx = np.zeros((frames, nch), dtype=np.uint8)
    for c in range(nch):
        f = 0
        while f < frames:
            k = int(rng.randint(1, 10))
            idx[f:f + k, c] = int(rng.randint(0, n))
            f += k
    return idx


def pattern_index(kind, units, n):
    """'cycle': u % n; 'last': everything in the last entry; 'single': one unit (the middle one) in entry 0, the rest in the last"""
    if kind == 'cycle':
        return (np.arange(units) % n).astype(np.uint8)
    idx = np.full(units, n - 1, dtype=np.uint8)
    if kind == 'single':
        idx[units // 2] = 0
    return idx


def compose(index, per_entry_units):
    """the expected units of a call: unit u from the constant-bias encode of entry index[u] (units are independent given the PCM)"""
    idx = np.asarray(index).reshape(-1)
    out = np.zeros_like(per_entry_units[0])
    for k, u in enumerate(per_entry_units):
        out[idx == k] = u[idx == k]
    return out


# ---- an option schedule as the steps of one stream whose bias comes through the pushes alone ----
def plan(per_frame, nch, split=None):
    """[('options', {'transientThresholdLow': t}) | ('push', a, b, biases [b - a], mode bytes [b - a, nch] or None)]: an options
    step only where the threshold changes (always detection, never a bias), one push per run of frames that share the threshold
    and are all under fixedBlockModes or all under detection.  split: no push longer than that many frames."""
    steps = []
    cur = None
    n = len(per_frame)
    a = 0
    while a < n:
        v = per_frame[a]
        thr, fixed = v['transientThresholdLow'], v['fixedBlockModes'] is not None
        b = a + 1
        while b < n and per_frame[b]['transientThresholdLow'] == thr and (per_frame[b]['fixedBlockModes'] is not None) == fixed:
            b += 1
        if thr != cur:
            steps.append(('options', {'transientThresholdLow': thr, 'fixedBlockModes': None}))
            cur = thr
        k = split or (b - a)
        for x in range(a, b, k):
            y = min(b, x + k)
            biases = np.array([per_frame[f]['allocationBias'] for f in range(x, y)], dtype=np.float64)
            modes = None
            if fixed:
                row = np.array([BM.byte_of(per_frame[f]['fixedBlockModes']) for f in range(x, y)], dtype=np.uint8)
                modes = np.repeat(row[:, None], nch, axis=1)
            steps.append(('push', x, y, biases, modes))
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
        _, a, b, biases, modes = step
        values, index = palette_of(np.repeat(biases[:, None], nch, axis=1))
        u, st = oracle_encode_schedule([c[a * 512:b * 512] for c in chans], values, index, modes, cur, st)
        out.append(u)
    return np.concatenate(out), st


def run_plan_on_stream(stream, options_of, chans, steps):
    """the same steps on a carta1_amd.EncoderStream; options_of(values) -> EncoderOptions"""
    out = []
    for step in steps:
        if step[0] == 'options':
            stream.set_options(options_of(step[1]))
            continue
        _, a, b, biases, modes = step
        out.append(stream.push([c[a * 512:b * 512] for c in chans], modes=modes, biases=biases))
    return np.concatenate(out)
