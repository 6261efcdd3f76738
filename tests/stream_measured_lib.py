"""The measured allocation on live streams (c1_enc_stream_push_measured): what the CPU and the GPU tests share.  The per-unit
function is c1_encode_measured_masked_*'s, so the model is tests/masked_alloc_lib.py's, unchanged, over the units the reference
leaves for the same stream: the shared cases of that library for streams that never change options, and the oracle run segment
by segment (tests/option_changes_lib.py) for the stream that does."""
import numpy as np

import best_modes_lib as BMO
import masked_alloc_lib as MK
import option_changes_lib as OC
import scale_factor_choice_lib as SF

OFFSETS = SF.OFFSETS
OUTPUTS = ('units', 'taken', 'shifts', 'distortion', 'energy', 'weights')
# the stream that changes options: pink material, fixedBlockModes [2, 2, 0] for frames 0 .. SWITCH - 1, detection from frame
# SWITCH on.  The first push after the switch is one frame: it is encoded by the stage kernels against the detection history a
# fresh pool holds (zeros), the frames after it take the usual path
SWITCH = 40
CHANGE_FRAMES = 56
CHANGE_INITIAL = {'fixedBlockModes': [2, 2, 0]}
CHANGE_SCHEDULE = [(SWITCH, {'fixedBlockModes': None})]

_change = {}


def option_change_material():
    return [c[:CHANGE_FRAMES * 512] for c in BMO.material('pink')]


def option_change_case():
    """the model of the option-change stream under the packaged tables and OFFSETS, over the oracle's units; computed once per
    process, shared, never written"""
    if 'model' not in _change:
        chans = option_change_material()
        per_frame = OC.options_at(CHANGE_INITIAL, CHANGE_SCHEDULE, CHANGE_FRAMES)
        ref = OC.oracle_encode(chans, per_frame)
        _change['model'] = MK.model_of(MK.tables_of(chans, ref, OFFSETS), *MK.packaged())
    return _change['model']


def as_dict(result):
    """EncoderStream.push_measured's / Context.encode_measured's full result -> dict by output name"""
    return dict(zip(OUTPUTS, result))


def concat(parts):
    return {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}


def same(a, b):
    """bitwise equality of two output dicts (doubles compared as bit patterns)"""
    return a.keys() == b.keys() and all(a[k].shape == b[k].shape and np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) for k in a)


def rows(out, a, b, nch):
    return {k: v[a * nch:b * nch] for k, v in out.items()}
