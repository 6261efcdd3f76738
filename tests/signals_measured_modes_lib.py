"""The measured block-mode search for n signals of any lengths in one call (c1_encode_signals_measured_modes*): what its GPU tests
share.  The shapes are tests/signals_lib.py's (0, 1, 2, 3, 1, 0, 7, 66, 2, 130, 1 frames: both start rows, the first bulk frame,
short neighbours back to back, more than one 64-frame run).  The oracle is the composition the header defines the call by: per
signal one mono EncoderStream on the same context, restored to the signal's pool when pools are given, one push_measured_modes
with every output asked for, then get_state.  Computed once per key and never modified."""
import numpy as np

import carta1_amd as c1
import signals_lib as SL
import stream_state_lib as SS

LENGTHS = SL.LENGTHS
OPTION_SETS = SL.OPTION_SETS
ONAMES = ('detect', 'long', 'short_bias2')
OFFSETS = (0, -1, 1, -2, -3)
DOMAIN = (0x00, 0x02, 0x08, 0x0a, 0x30, 0x32, 0x38, 0x3a)
# (candidates, scale-factor offsets): three candidates with the five offsets; all eight with offsets NULL
CONFIGS = {'three-offsets': ((0, 10, 58), OFFSETS), 'eight-plain': (DOMAIN, None)}
OUTPUTS = ('units', 'choice', 'modes', 'taken', 'shifts', 'distortion', 'energy')

signals, enc_pools, offsets = SL.signals, SL.enc_pools, SL.offsets

_cache = {}


def opts(oname):
    return c1.EncoderOptions(dict(OPTION_SETS[oname]))


def compose(ctx, sigs, oname, cand, offs, pools=None):
    """the oracle by composition -> dict of per-signal lists by output name, and 'states' (n, 483)"""
    out = {k: [] for k in OUTPUTS}
    states = np.zeros((len(sigs), SS.ENC_FLOATS), dtype=np.float32)
    for i, x in enumerate(sigs):
        s = c1.EncoderStream(ctx, 1, opts(oname))
        try:
            if pools is not None:
                s.set_state(np.ascontiguousarray(pools[i:i + 1]).copy())
            got = s.push_measured_modes([np.ascontiguousarray(x)], list(cand), scale_factor_offsets=offs, return_distortion=True,
                                        return_shifts=True)
            for k, v in zip(OUTPUTS, got):
                out[k].append(v)
            states[i] = np.asarray(s.get_state()).reshape(-1, SS.ENC_FLOATS)[0]
        finally:
            s.close()
    out['states'] = states
    return out


def want(ctx, key, oname, config, pools, material='pink'):
    """compose() of the shared shapes, once per (key, ...): key names the context the oracle ran on"""
    k = (key, oname, config, bool(pools), material)
    if k not in _cache:
        cand, offs = CONFIGS[config]
        w = compose(ctx, signals(material), oname, cand, offs, enc_pools() if pools else None)
        for v in w.values():
            for a in (v if isinstance(v, list) else [v]):
                a.setflags(write=False)
        _cache[k] = w
    return _cache[k]


def run(ctx, oname, cand, offs, pools, material='pink', sigs=None, states=None):
    """Context.encode_signals_measured_modes with every output and the pools after -> dict"""
    sigs = signals(material) if sigs is None else sigs
    st = states if states is not None else (enc_pools() if pools else None)
    res = ctx.encode_signals_measured_modes(sigs, list(cand), options=opts(oname), states=st, return_states=True,
                                            scale_factor_offsets=offs, return_distortion=True, return_shifts=True)
    return dict(zip(OUTPUTS + ('states',), res))


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
