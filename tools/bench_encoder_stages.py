"""tools/bench_encoder_stages.py (GPU) -- rate of the encoder's stage entry points composed (c1_qmf_analysis_batch ->
c1_select_block_modes -> c1_mdct_batch -> c1_quantize_frames, host pointers, synchronous) on 1 M mono frames, beside
c1_encode_batch (host pointers) on the same PCM: pink noise with bursts, transient detection on."""
import ctypes, os, sys, time
import numpy as np
R = os.getcwd(); sys.path[:0] = [R, os.path.join(R, 'tests')]
import carta1_amd as c1
from carta1_amd import capi
import oracle_lib as O

frames = int(sys.argv[1]) if len(sys.argv) > 1 else 1 << 20
reps = 3
pcm = np.resize(O.gen_pinkT(3, 4096 * 512), frames * 512).astype(np.float32)
ctx = c1.Context(0)
lib, h = capi.load(), ctx._h
opts = c1.EncoderOptions().to_c()
C_opts = ctypes.byref(opts)
bands, coefs, windowed = (np.ones((frames, 512), np.float32) for _ in range(3))
modes = np.ones((frames, 3), np.int32)
nb, sf, wl, q = np.ones(frames, np.int32), np.ones((frames, 52), np.int32), np.ones((frames, 52), np.int32), np.ones((frames, 512), np.int32)
units = np.zeros((frames, 212), np.uint8)
P = lambda a: a.ctypes.data


def stages():
    t = [time.perf_counter()]
    capi.check(lib.c1_qmf_analysis_batch(h, P(pcm), frames, 0, P(bands))); t.append(time.perf_counter())
    capi.check(lib.c1_select_block_modes(h, P(bands), frames, 0, 1.0, P(modes))); t.append(time.perf_counter())
    capi.check(lib.c1_mdct_batch(h, P(bands), frames, 0, P(modes), P(coefs), P(windowed))); t.append(time.perf_counter())
    capi.check(lib.c1_quantize_frames(h, P(coefs), frames, P(modes), C_opts, P(nb), P(sf), P(wl), P(q))); t.append(time.perf_counter())
    return np.diff(t)



def batch():
    t = time.perf_counter(); ctx.encode([pcm], c1.EncoderOptions(), out=units); return time.perf_counter() - t


per = [stages() for _ in range(reps + 1)][1:]
st = np.min(np.array(per), axis=0)
batch()
tb = min(batch() for _ in range(reps))
ref = ctx.unpack_units(units)
for k, a in (('nbfu', nb), ('block_modes', modes), ('sfi', sf), ('wl', wl), ('quantized', q)):
    assert np.array_equal(a, ref[k]), 'stage chain differs from c1_encode_batch: ' + k
rate = lambda s: frames / s / 1e6
print('frames %d mono (best of %d)' % (frames, reps))
for name, s in zip(('c1_qmf_analysis_batch', 'c1_select_block_modes', 'c1_mdct_batch', 'c1_quantize_frames'), st):
    print('  %-24s %8.1f ms' % (name, s * 1e3))
print('stage chain (host)       %8.1f ms  %6.2f M frames/s' % (st.sum() * 1e3, rate(st.sum())))
print('c1_encode_batch (host)   %8.1f ms  %6.2f M frames/s' % (tb * 1e3, rate(tb)))
ctx.close()
