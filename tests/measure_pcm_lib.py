"""The error of the decoded PCM of given sound units against their PCM (c1_measure_pcm_*): the CPU model, built from the oracle
alone.

y is oracle_lib.decode_stream of the units from a zero DecState (the halo unit, when there is one, is decoded first and its
frame dropped: the state it leaves is the continued one); x is the input DELAY samples earlier, zero before the history given.
The squares are summed per 32 samples with i ascending (cumsum) and the sixteen segments of a unit in order (cumsum):
include/carta1_hip.h's definition, line by line."""
import numpy as np

import masked_alloc_lib as MK
import oracle_lib as O

DELAY = 266
SEGMENTS = 16


def decoded(units, nch, halo_units=0):
    """y: float32 [nch][512 * frames] of units uint8 [(halo_units + frames) * nch, 212]"""
    units = np.ascontiguousarray(units, dtype=np.uint8).reshape(-1, 212)
    outs, _ = O.decode_stream(units, nch)
    return [o[512 * halo_units:] for o in outs]


def delayed(chan, halo_frames, delay=DELAY):
    """x: float32 [512 * frames] of one channel's PCM with halo_frames frames of history first"""
    chan = np.asarray(chan, dtype=np.float32)
    n = len(chan) - 512 * halo_frames
    src = 512 * halo_frames - delay + np.arange(n)
    return np.where(src >= 0, chan[np.clip(src, 0, None)], np.float32(0.0)).astype(np.float32)


def sums(y, x):
    """y, x: [nch][512 * frames] float32 -> dict 'noise', 'signal' float64 [U, 16], 'totals' float64 [U, 2], u = frame * nch + channel"""
    nch, frames = len(y), len(y[0]) // 512
    noise, signal = np.zeros((frames * nch, SEGMENTS)), np.zeros((frames * nch, SEGMENTS))
    with np.errstate(invalid='ignore', over='ignore'):
        for c in range(nch):
            xd = np.asarray(x[c], dtype=np.float32).astype(np.float64).reshape(frames, SEGMENTS, 32)
            e = np.asarray(y[c], dtype=np.float32).astype(np.float64).reshape(frames, SEGMENTS, 32) - xd
            noise[c::nch] = np.cumsum(e * e, axis=2)[:, :, -1]
            signal[c::nch] = np.cumsum(xd * xd, axis=2)[:, :, -1]
        totals = np.stack([np.cumsum(noise, axis=1)[:, -1], np.cumsum(signal, axis=1)[:, -1]], axis=1)
    return {'noise': noise, 'signal': signal, 'totals': totals}


def model(chans, units, halo_frames=0, halo_units=0, delay=DELAY):
    """chans: [nch] float32, halo_frames frames of real history then the frames; units uint8 [(halo_units + frames) * nch, 212]"""
    nch = len(chans)
    return sums(decoded(units, nch, halo_units), [delayed(c, halo_frames, delay) for c in chans])


def snr_db(totals, nch, skip=2, stop=None):
    """10 log10(sum signal / sum noise) over frames skip .. stop - 1"""
    t = np.asarray(totals).reshape(-1, nch, 2)[skip:stop]
    return 10.0 * np.log10(t[..., 1].sum() / t[..., 0].sum())


def bitwise(a, b):
    return MK.bitwise(a, b)
