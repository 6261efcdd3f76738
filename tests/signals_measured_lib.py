"""The measured allocation for n signals of any lengths in one call (c1_encode_signals_measured*): what the CPU and the GPU
tests share.  The shapes are tests/signals_lib.py's.  The oracle is the composition the header defines the call by: per signal
one mono EncoderStream on the same context, restored to the signal's pool when pools are given, one push_measured with every
output asked for, then get_state.  Computed once per key and never modified."""
import numpy as np

import carta1_amd as c1
import signals_lib as SL
import stream_measured_lib as SM
import stream_state_lib as SS

LENGTHS = SL.LENGTHS
OPTION_SETS = SL.OPTION_SETS
OFFSETS = SM.OFFSETS
OUTPUTS = SM.OUTPUTS
# the four definitions: (scale_factor_offsets, masking)
DEFINITIONS = {'plain': (None, None), 'offsets': (OFFSETS, None), 'masked_offsets': (OFFSETS, True), 'masked': (None, True)}
# the eight bytes of blockSelectorStage's domain
DOMAIN = (0x00, 0x02, 0x08, 0x0a, 0x30, 0x32, 0x38, 0x3a)

signals, enc_pools, offsets = SL.signals, SL.enc_pools, SL.offsets

_cache = {}


def opts(oname):
    return c1.EncoderOptions(dict(OPTION_SETS[oname]))


def mode_rows(lengths=LENGTHS):
    """one array of mode bytes per signal, cycling through the eight domain bytes by frame index of the concatenation: frames 0
    and 1 of neighbouring signals differ"""
    rows, at = [], 0
    for n in lengths:
        rows.append(np.array([DOMAIN[(at + k) % 8] for k in range(n)], dtype=np.uint8))
        at += n
    return rows


def ask(definition):
    """the keyword arguments that ask for everything a definition can report"""
    offs, masking = DEFINITIONS[definition]
    return dict(scale_factor_offsets=offs, masking=masking, return_distortion=True, return_shifts=offs is not None,
                return_weights=masking is not None)


def named(result, definition):
    """a full result of encode_signals_measured / push_measured under ask(definition) -> dict by output name (+ 'states')"""
    offs, masking = DEFINITIONS[definition]
    names = ['units', 'taken'] + (['shifts'] if offs is not None else []) + ['distortion', 'energy'] + (['weights'] if masking is not None else [])
    return dict(zip(names + ['states'], result))


def compose(ctx, sigs, oname, definition, pools=None, modes=None):
    """the oracle by composition -> dict of per-signal lists by output name, and 'states' (n, 483)"""
    kw = ask(definition)
    names = list(named(tuple(range(8)), definition))
    names.remove('states')
    out = {k: [] for k in names}
    states = np.zeros((len(sigs), SS.ENC_FLOATS), dtype=np.float32)
    for i, x in enumerate(sigs):
        s = c1.EncoderStream(ctx, 1, opts(oname))
        try:
            if pools is not None:
                s.set_state(np.ascontiguousarray(pools[i:i + 1]).copy())
            got = s.push_measured([np.ascontiguousarray(x)], modes=None if modes is None else modes[i], **kw)
            for k, v in zip(names, got):
                out[k].append(v)
            states[i] = np.asarray(s.get_state()).reshape(-1, SS.ENC_FLOATS)[0]
        finally:
            s.close()
    out['states'] = states
    return out


def want(ctx, key, oname, definition, pools, material='pink', with_modes=False):
    """compose() of the shared shapes, once per (key, ...): key names the context the oracle ran on"""
    k = (key, oname, definition, bool(pools), material, with_modes)
    if k not in _cache:
        w = compose(ctx, signals(material), oname, definition, enc_pools() if pools else None, mode_rows() if with_modes else None)
        for v in w.values():
            for a in (v if isinstance(v, list) else [v]):
                a.setflags(write=False)
        _cache[k] = w
    return _cache[k]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def first_bad(got, wanted):
    """two dicts as compose() returns them: None, or (output, signal, frame) of the first difference, bitwise"""
    for k in wanted:
        if k == 'states':
            continue
        if k not in got or len(got[k]) != len(wanted[k]):
            return (k, 'missing or of another length')
        for i, (g, w) in enumerate(zip(got[k], wanted[k])):
            g, w = np.asarray(g), np.asarray(w)
            if g.shape != w.shape or g.dtype != w.dtype:
                return (k, 'signal', i, 'shape', g.shape, w.shape, g.dtype, w.dtype)
            if len(g) == 0:
                continue
            bad = np.flatnonzero((bits(g).reshape(len(g), -1) != bits(w).reshape(len(w), -1)).any(axis=1))
            if len(bad):
                return (k, 'signal', i, 'frame', int(bad[0]))
    if 'states' in wanted and got.get('states') is not None:
        bad = np.flatnonzero((SS.bits(got['states']) != SS.bits(wanted['states'])).any(axis=1))
        if len(bad):
            return ('states', 'signal', int(bad[0]))
    return None
