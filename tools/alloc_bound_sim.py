#!/usr/bin/env python3
"""tools/alloc_bound_sim.py -- CPU study behind k_alloc_bound (carta1_amd/csrc/c1_k_allocate.hip): how many greedy heaps per
sound unit allocateBits (bitallocation.js:74-142) really needs when candidates are excluded by a Lagrangian lower bound
on their total distortion, and how far that bound sits below the totals the heaps produce.  Uses the C oracle for the
transforms and a Python restatement of distributeBitsRDO / calculateTotalDistortion; asserts bound <= total on every
candidate it looks at.  Typical output: tonal material 7-8 heaps per unit -> 2, gap 1-4 %."""
import os, sys, math, ctypes as C, numpy as np
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests'))
import oracle_lib as O
L = O.lib()
SPECS = [8,8,8,8,4,4,4,4,8,8,8,8,6,6,6,6,6,6,6,6,6,6,6,6,7,7,7,7,9,9,9,9,10,10,10,10,12,12,12,12,12,12,12,12,20,20,20,20,20,20,20,20]
START = np.concatenate([[0], np.cumsum(SPECS)])[:52]
AMOUNTS = [20,28,32,36,40,44,48,52]
WLB = [0,2,3,4,5,6,7,8,9,10,11,12,13,14,15,16]
DB = [WLB[i+1]-WLB[i] for i in range(15)]
IP2 = [2.0**-b for b in range(17)]
DDF = [2.0 - IP2[2]] + [IP2[WLB[i]] - IP2[WLB[i+1]] for i in range(1,15)]
SF = np.array([O.h2d(h) for h in O.golden_tables()['scale_factors']]) if 'scale_factors' in O.golden_tables() else None
f32 = np.float32

def sift(hi, hp, i, n):
    iv, pv = hi[i], hp[i]
    while True:
        l = 2*i+1; r = l+1; m = i; mp = pv
        if l < n and hp[l] > mp: m = l; mp = hp[l]
        if r < n and hp[r] > mp: m = r
        if m == i: break
        hi[i] = hi[m]; hp[i] = hp[m]; i = m
    hi[i] = iv; hp[i] = pv

def distribute(n, rem, bsf, sfi):
    wl = [0]*n; hi = []; hp = []
    for b in range(n):
        if sfi[b] == 0: continue
        hi.append(b); hp.append(f32(bsf[sfi[b]]*DDF[0]/DB[0]))
    hs = len(hi)
    if hs == 0: return wl
    for i in range((hs>>1)-1, -1, -1): sift(hi, hp, i, hs)
    while rem > 0 and hs > 0:
        b = hi[0]; cur = wl[b]; cost = DB[cur]*SPECS[b]
        if cost > rem or cost <= 0:
            hi[0] = hi[hs-1]; hp[0] = hp[hs-1]; hs -= 1
            if hs > 0: sift(hi, hp, 0, hs)
            continue
        rem -= cost; nxt = cur+1; wl[b] = nxt
        if nxt < 15 and DB[nxt] > 0:
            hp[0] = f32(bsf[sfi[b]]*DDF[nxt]/DB[nxt]); sift(hi, hp, 0, hs)
        else:
            hi[0] = hi[hs-1]; hp[0] = hp[hs-1]; hs -= 1
            if hs > 0: sift(hi, hp, 0, hs)
    return wl

def total(n, wl, sfi, bsf, z):
    t = 0.0
    for i in range(n):
        bits = WLB[wl[i]]
        if bits == 0: t += float(z[i]); continue
        if sfi[i] == 0: continue
        t += bsf[sfi[i]]*IP2[bits]*SPECS[i]
    for i in range(n, 52): t += float(z[i])
    return t

def lower_bound(n, B, lam, sfi, bsf, z):
    s = 0.0
    for b in range(n):
        if sfi[b] == 0: continue
        best = float(z[b])
        for w in range(1, 16):
            v = bsf[sfi[b]]*IP2[WLB[w]]*SPECS[b] + lam*SPECS[b]*WLB[w]
            if v < best: best = v
        s += best
    for b in range(n, 52): s += float(z[b])
    return s - lam*B

def analyse(pcm, bias=1.0):
    st = O.EncState(); L.c1o_enc_state_init(C.byref(st))
    bsf = np.zeros(64); L.c1o_default_biased_sf(C.c_double(bias), bsf.ctypes.data_as(C.POINTER(C.c_double)))
    frames = len(pcm)//512
    out = []
    modes = (C.c_int*3)(0,0,0)
    for f in range(frames):
        x = np.ascontiguousarray(pcm[512*f:512*f+512], dtype=np.float32)
        bands = np.zeros(512, np.float32); coefs = np.zeros(512, np.float32)
        L.c1o_qmf_analysis_frame(C.byref(st), O._fp(x), O._fp(bands))
        L.c1o_mdct_frame(C.byref(st), O._fp(bands), modes, O._fp(coefs))
        sfi = [L.c1o_find_scale_factor(O._fp(coefs[START[b]:START[b]+SPECS[b]].copy()), SPECS[b]) for b in range(52)]
        out.append(sfi)
    return out, bsf

ITERS=8
def study(name, pcm, bias=1.0, skip=2, maxu=150):
    units, bsf = analyse(pcm, bias)
    evals_now = evals_new = 0; nun = 0; worst_gap = 0
    hist = [0]*8
    for sfi in units[skip:skip+maxu]:
        nun += 1
        z = [f32(bsf[sfi[b]]*2.0*SPECS[b]) if sfi[b] > 0 else f32(0) for b in range(52)]
        tot = []
        for n in AMOUNTS:
            wl = distribute(n, 1696-40-10*n, bsf, sfi); tot.append(total(n, wl, sfi, bsf, z))
        win = min(range(8), key=lambda c: (tot[c], c)); hist[win] += 1
        # current scheme: survivors by zero-bit bound vs total_52
        surv = [c for c in range(7) if not (sum(float(z[b]) for b in range(AMOUNTS[c], 52)) > tot[7])]
        evals_now += 1 + len(surv)
        if not surv: evals_new += 1; continue
        # lambda from the 52 run: marginal priority at the end ~ estimate by bisection so that the relaxed budget is met
        def lam_for(n, B):
            lo, hi = 1e-30, 1e3
            for _ in range(80):
                mid = math.sqrt(lo*hi)
                used = 0
                for b in range(n):
                    if sfi[b] == 0: continue
                    best = float(z[b]); bw = 0
                    for w in range(1, 16):
                        v = bsf[sfi[b]]*IP2[WLB[w]]*SPECS[b] + mid*SPECS[b]*WLB[w]
                        if v < best: best = v; bw = w
                    used += SPECS[b]*WLB[bw]
                if used > B: lo = mid
                else: hi = mid
            return hi
        lbs = {}
        la = [math.log2(bsf[sfi[b]]) if sfi[b] > 0 else None for b in range(52)]
        def bits_of(y): return 0 if y <= 0.19 else (2 if y < 3 else min(int(math.floor(y)), 16))
        for c in surv:
            n = AMOUNTS[c]; B = 1696-40-10*n
            act = [b for b in range(n) if sfi[b] > 0]
            lo = min(la[b] for b in act) - 17.0 if act else 0.0
            hi = max(la[b] for b in act) if act else 1.0
            for it in range(ITERS):
                x = 0.5*(lo+hi)
                used = sum(SPECS[b]*bits_of(la[b]-x) for b in act)
                if used > B: lo = x
                else: hi = x
            lam = 2.0**hi
            lbs[c] = lower_bound(n, B, lam, sfi, bsf, z)
            worst_gap = max(worst_gap, (tot[c]-lbs[c])/tot[c] if tot[c] > 0 else 0)
            assert lbs[c] <= tot[c]*(1+1e-12), (lbs[c], tot[c])
        best = tot[7]; e = 1
        alive = [c for c in surv if not lbs[c] > best]
        if alive:
            c0 = min(alive, key=lambda c: lbs[c]); e += 1; best = min(best, tot[c0])
            rest = [c for c in alive if c != c0 and not lbs[c] > best]
            e += len(rest)
        evals_new += e
    print('%-10s units %d  heaps/unit now %.2f  with bound %.2f  worst relative gap %.3f  winners %s' % (name, nun, evals_now/nun, evals_new/nun, worst_gap, hist))

rng = np.random.default_rng(1)
N = 512*160
t = np.arange(N)/44100.0
white = (rng.random(N).astype(np.float32)*2-1)*0.5
ton = sum(a*np.sin(2*np.pi*f*t+p) for a, f, p in [(0.3,220,0),(0.2,440,1),(0.1,660,2),(0.05,1320,.5),(0.02,3300,.1),(0.01,7040,.3)]).astype(np.float32)
ton2 = sum((0.4/(k+1))*np.sin(2*np.pi*(110*(k+1))*t+k) for k in range(40)).astype(np.float32)
quiet = white*1e-3
pink = np.cumsum(white).astype(np.float32); pink = (pink/np.abs(pink).max()*0.5).astype(np.float32)
music = (ton2*0.5 + white*0.01).astype(np.float32)
for ITERS in [6, 8, 10, 12]:
  print('ITERS', ITERS)
  for nm, s in [('white', white), ('tonal6', ton), ('harm40', ton2), ('quiet', quiet), ('brown', pink), ('music', music)]:
      study(nm, s)
