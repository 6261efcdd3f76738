"""tools/bench_decoder_stages.py (GPU) -- rate of the decoder's stage entry points composed (c1_unpack_units -> c1_dequantize_frames
-> c1_imdct_batch -> c1_qmf_synthesis_batch, host pointers, synchronous) on 1 M mono frames, beside c1_decode_batch (host
pointers) and c1_decode_device (device pointers) on the same units.  The units are channel 0 of the eleven KAT files, tiled."""
import glob, os, sys, time
import numpy as np, torch
R = os.getcwd(); sys.path[:0] = [R, os.path.join(R, 'tests')]
import carta1_amd as c1
from carta1_amd import capi

frames = int(sys.argv[1]) if len(sys.argv) > 1 else 1 << 20
reps = 3
kat = np.concatenate([np.fromfile(p, dtype=np.uint8).reshape(-1, 2, 212)[:, 0] for p in sorted(glob.glob('tests/golden/kat64_*.units.bin'))])
units = np.ascontiguousarray(np.resize(kat, (frames, 212)))
ctx = c1.Context(0)
lib, h = capi.load(), ctx._h
nb, md = np.ones(frames, np.int32), np.ones((frames, 3), np.int32)
sf, wl, q = np.ones((frames, 52), np.int32), np.ones((frames, 52), np.int32), np.ones((frames, 512), np.int32)
co, bd, pcm, ref = (np.ones((frames, 512), np.float32) for _ in range(4))
P = lambda a: a.ctypes.data


def stages():
    t = [time.perf_counter()]
    capi.check(lib.c1_unpack_units(h, P(units), frames, P(nb), P(md), P(sf), P(wl), P(q))); t.append(time.perf_counter())
    capi.check(lib.c1_dequantize_frames(h, frames, P(nb), P(md), P(sf), P(wl), P(q), P(co))); t.append(time.perf_counter())
    capi.check(lib.c1_imdct_batch(h, P(co), frames, 0, P(md), P(bd))); t.append(time.perf_counter())
    capi.check(lib.c1_qmf_synthesis_batch(h, P(bd), frames, 0, P(pcm))); t.append(time.perf_counter())
    return np.diff(t)


def best(fn):
    fn()
    return min(fn() for _ in range(reps))


def batch():
    t = time.perf_counter(); ctx.decode(units, 1, out=[ref.reshape(-1)]); return time.perf_counter() - t


du = torch.from_numpy(units.reshape(-1)).cuda()
dp = torch.empty(frames * 512, dtype=torch.float32, device='cuda')


def device():
    ctx.synchronize(); t = time.perf_counter()
    ctx.decode_device(du.data_ptr(), 1, frames, [dp.data_ptr()]); ctx.synchronize()
    return time.perf_counter() - t


per = [stages() for _ in range(reps + 1)][1:]
st = np.min(np.array(per), axis=0)
tb, td = best(batch), best(device)
assert np.array_equal(pcm.view(np.uint32), ref.view(np.uint32)), 'stage chain differs from c1_decode_batch'
assert np.array_equal(dp.cpu().numpy().view(np.uint32), ref.reshape(-1).view(np.uint32))
rate = lambda s: frames / s / 1e6
print('frames %d mono (best of %d)' % (frames, reps))
for name, s in zip(('c1_unpack_units', 'c1_dequantize_frames', 'c1_imdct_batch', 'c1_qmf_synthesis_batch'), st):
    print('  %-24s %8.1f ms' % (name, s * 1e3))
print('stage chain (host)       %8.1f ms  %6.2f M frames/s' % (st.sum() * 1e3, rate(st.sum())))
print('c1_decode_batch (host)   %8.1f ms  %6.2f M frames/s' % (tb * 1e3, rate(tb)))
print('c1_decode_device         %8.1f ms  %6.2f M frames/s' % (td * 1e3, rate(td)))
ctx.close()
