#!/usr/bin/env python3
"""tools/lds_model_spec.py [--parent] [-v] -- LDS-array cycles of one frame of k_analysis_spec<false> (long blocks,
emitting path), one wave, from the real lane addresses of every LDS instruction of its frame loop.

The instruction list is the one `hipcc -S` shows for carta1_amd/csrc/c1_k_spec.hip (the compiler pairs some 4- and
8-byte accesses into ds_read2 / ds_write2, which are costed as their two halves); the addresses restate the kernel's
index arithmetic.  --parent: the kernel before the layout change of DESIGN.md 6b round 5 (delay-line arrays, work
buffers at index + 0, in0 | in1 side by side), whose counters are on file: profiles/r04_pmc_summary.txt,
SQ_LDS_IDX_ACTIVE 524.6 and SQ_LDS_BANK_CONFLICT 95.5 per unit.

This is a hand-kept transcription of ONE compiler output: which accesses the compiler pairs, the order of the
instructions and both layouts are restated here and checked against nothing.  After any change of the kernel or of the
compiler, re-derive the list from a fresh listing (ds_ lines of the frame loop) before trusting a number it prints.

Cost rule (MI355X LDS table): an instruction is served in fixed lane groups, one array cycle per group, plus one cycle
for every further distinct dword on the busiest bank of the group.  32 banks for ds_read_b32 and every store, 64 for
ds_read_b64 / b128; the halves of ds_read2_b64 go 4 x 16 lanes over 32 banks.  Two totals are printed: `all groups`
charges a group whether or not one of its lanes is active (what the counters turn out to do), `active`
only groups with an active lane.  conflict = cycles beyond one per charged group."""
import collections
import sys

from lds_model import cycles, groups as std_groups, WIDTH as STD_WIDTH, BANKS as STD_BANKS

PARENT = '--parent' in sys.argv
VERBOSE = '-v' in sys.argv

KINDS = dict((k, (std_groups(k), STD_WIDTH[k], STD_BANKS[k])) for k in STD_WIDTH)
KINDS['r64h'] = ([list(range(16 * i, 16 * i + 16)) for i in range(4)], 2, 32)    # one half of ds_read2_b64


def cost(kind, fn):
    """-> (cycles with only active groups charged, cycles with every group charged, conflict cycles)"""
    grp, width, banks = KINDS[kind]
    active = total = 0
    for g in grp:
        per_bank = collections.defaultdict(set)
        for lane in g:
            a = fn(lane)
            if a is None:
                continue
            assert a % (4 * min(width, 4)) == 0 or kind in ('r32', 'w32'), (kind, lane, a)
            for d in range(width):
                per_bank[(a // 4 + d) % banks].add(a // 4 + d)
        worst = max((len(v) for v in per_bank.values()), default=0)
        active += worst
        total += max(worst, 1)
    if kind in STD_WIDTH:
        assert active == cycles(kind, fn)
    return active, total, total - len(grp)


def bitrev(k, bits):
    return int(format(k, '0%db' % bits)[::-1], 2)


def zslot(pos):
    return pos + 4 * (pos >> 4)


def w1_phys(v):
    return 12 * (v >> 3) + (v & 7)


# ---- the wave's LDS (float indices into SpecLds::mem unless said otherwise; byte addresses = 4 x, wave 0) -----------
K_R2, K_IN2 = 840, 1
if PARENT:
    MEM_FLOATS = K_R2 + 576
    D1 = MEM_FLOATS
    D2 = D1 + 48
    PRE2 = D2 + 48
    SFI = PRE2 + 76                      # 64 bytes
    GEO = SFI + 16                       # [3][64] words
    WAVE_BYTES = 4 * (GEO + 192)
else:
    K_W2 = K_R2 + 320
    MEM_FLOATS = K_W2 + 304
    PRE2 = MEM_FLOATS
    SFI = PRE2 + 76
    WAVE_BYTES = 4 * (SFI + 16)
    GEO = WAVE_BYTES                     # float index of the workgroup's one geo[64] x 16 bytes, behind the four waves
TAB = 4 * WAVE_BYTES + (0 if PARENT else 1024)      # bytes; win32 | pre32_64 | pre32_256 | pre32_512 | r4b | r4c | r2d
T_PRE256, T_PRE512 = TAB + 128 + 128, TAB + 128 + 128 + 512
T_R4B = T_PRE512 + 1024
T_R4C = T_R4B + 96
T_R2D = T_R4C + 384
TAIL_W = T_R2D + 512
OUT_W = TAIL_W + 28 * 16                 # new kernel: tail_w has an entry of ones in front; out_w[64][2] behind it
assert (TAIL_W + 27 * 16 if PARENT else OUT_W + 512) <= 32000      # 25 LDS blocks of 1 280 bytes: 5 workgroups per CU

START_LONG = [0]
for n in [8] * 4 + [4] * 4 + [8] * 4 + [6] * 12 + [7] * 4 + [9] * 4 + [10] * 4 + [12] * 8 + [20] * 8:
    START_LONG.append(START_LONG[-1] + n)


def in01(b, i):
    return K_R2 + 64 * (i >> 5) + 32 * b + ((i & 31) ^ b)


def base(lane):
    """spec_base() of c1_k_spec.hip"""
    band = 0 if lane < 16 else (1 if lane < 32 else 2)
    g = lane - (0, 16, 32)[band]
    n4 = 128 if band == 2 else 64
    q = n4 // 4
    r = bitrev(g, 5 if band == 2 else 4)
    if PARENT:
        ib = (K_R2, K_R2 + 256, K_IN2)[band]
        inp = lambda i: ib + i
    else:
        inp = (lambda i: K_IN2 + i) if band == 2 else (lambda i: in01(band, i))
    B = dict(band=band, g=g, r=r, q2=2 * q, use_lo=r < 8, use_hi=r >= q - 8)
    step = B['q2'] if PARENT else 64     # floats between the operands of points q apart
    a0, c0 = inp(3 * n4 - 1 - 2 * r), inp(n4 + 2 * r)
    if not PARENT and band != 2:
        assert all(inp(3 * n4 - 1 - 2 * r - 32 * k) == a0 - 64 * k and inp(n4 + 2 * r + 32 * k) == c0 + 64 * k for k in range(4))
    B['a'] = [a0, a0 - 2 * step, a0 - step, a0 - 3 * step]
    B['c'] = [c0, c0 + 2 * step, c0 + step, c0 + 3 * step]
    B['ib'] = inp(3 * n4 + 2 * r) if B['use_lo'] else inp(2 * r + 2 * q)
    B['id'] = inp(n4 - 1 - 2 * r) if B['use_lo'] else inp(14 * q - 1 - 2 * r)
    tab = T_PRE512 if band == 2 else T_PRE256
    B['pt0'] = tab + 8 * r
    pb = (0, 64, 128)[band]
    B['za'], B['zb'] = zslot(pb + 4 * g), zslot(pb + 16 * (g >> 2) + (g & 3))
    B['zc'], B['zd'] = zslot(pb + 64 * (g >> 4) + (g & 15)), zslot(128 + (g & 31))
    cb, n2 = (0, 128, 256)[band], 2 * n4
    B['e0'], B['e1'] = cb + 2 * g, cb + n2 - 1 - 2 * g
    B['po0'] = tab + 8 * g
    B['d'] = [0, 64, 32, 96] if band == 2 else [0, 16, 32, 48]
    return B


BASE = [base(l) for l in range(64)]
rows = []                                # (phase, name, kind, active, all, conflict)


def I(phase, name, kind, fn):
    a, t, c = cost(kind, fn)
    rows.append((phase, name, kind, a, t, c))


def pair(phase, name, kind, f0, f1):     # ds_read2 / ds_write2: two accesses
    if kind == 'r64h' and not PARENT:    # the new kernel keeps 8-byte reads single (lds_f2): ds_read_b64
        kind = 'r64'
    I(phase, name + ' (1st half)', kind, f0)
    I(phase, name + ' (2nd half)', kind, f1)


F = lambda idx: 4 * idx                  # float index -> byte address
only = lambda pred, fn: (lambda l: fn(l) if pred(l) else None)

# ---------------- staging of the PCM, stage-1 delay line ----------------
if PARENT:
    I('stage', 'pcm a', 'w128', lambda l: F(w1_phys(44 + 4 * l)))
    I('stage', 'pcm b', 'w128', lambda l: F(w1_phys(300 + 4 * l)))
    I('stage', 'pcm tail (lane 63)', 'w64', only(lambda l: l == 63, lambda l: F(w1_phys(556))))
    I('stage', 'd1 read', 'r32', only(lambda l: l < 46, lambda l: F(D1 + l)))
    I('stage', 'd1 -> work', 'w32', only(lambda l: l < 46, lambda l: F(w1_phys(l))))
else:
    I('stage', 'delay tail read', 'r32', only(lambda l: l < 48, lambda l: F(768 + w1_phys(l))))
    I('stage', 'pcm a', 'w128', lambda l: F(w1_phys(48 + 4 * l)))
    I('stage', 'pcm b', 'w128', lambda l: F(w1_phys(304 + 4 * l)))
    I('stage', 'delay -> head', 'w32', only(lambda l: l < 48, lambda l: F(w1_phys(l))))
# ---------------- first QMF stage ----------------
for k in range(14):
    kind = 'r64' if (PARENT and k == 13) else 'r128'
    I('qmf1', 'window %d' % k, kind, lambda l, k=k: F(12 * l + 12 * (k >> 1) + 4 * (k & 1)))
if PARENT:
    I('qmf1', 'work tail read', 'r32', only(lambda l: l < 46, lambda l: F(w1_phys(512 + l))))
    I('qmf1', 'd2 read', 'r32', only(lambda l: l < 46, lambda l: F(D2 + l)))
    pair('qmf1', 'd1 save | d2 -> work2', 'w32', only(lambda l: l < 46, lambda l: F(D1 + l)), only(lambda l: l < 46, lambda l: F(K_R2 + l)))
    pair('qmf1', 'low-band outputs', 'w64', lambda l: F(K_R2 + 46 + 4 * l), lambda l: F(K_R2 + 48 + 4 * l))
    I('qmf1', 'pre2 -> in2, pass 1', 'r32', lambda l: F(PRE2 + 1 + l))
    I('qmf1', 'pre2 -> in2, pass 1', 'w32', lambda l: F(K_IN2 + 112 + l))
    I('qmf1', 'pre2 -> in2, pass 2', 'r32', only(lambda l: l < 7, lambda l: F(PRE2 + 65 + l)))
    I('qmf1', 'pre2 -> in2, pass 2', 'w32', only(lambda l: l < 7, lambda l: F(K_IN2 + 176 + l)))
else:
    I('qmf1', 'work2 tail read', 'r32', only(lambda l: l < 48, lambda l: F(K_W2 + 256 + l)))
    I('qmf1', 'work2 tail -> head', 'w32', only(lambda l: l < 48, lambda l: F(K_W2 + l)))
    I('qmf1', 'low-band outputs', 'w128', lambda l: F(K_W2 + 48 + 4 * l))
    I('qmf1', 'pre2 -> in2', 'r64', only(lambda l: l < 36, lambda l: F(PRE2 + 2 * l)))
    I('qmf1', 'pre2 -> in2', 'w64', only(lambda l: l < 36, lambda l: F(K_IN2 + 111 + 2 * l)))
if PARENT:
    I('qmf1', 'tail weights (next)', 'r128', only(lambda l: l >= 46, lambda l: TAIL_W + 16 * (9 + l - 46)))
    I('qmf1', 'pre2 write', 'w128', only(lambda l: l >= 46, lambda l: F(PRE2 + 4 * (l - 46))))
    I('qmf1', 'tail weights (this)', 'r128', only(lambda l: 46 <= l <= 54, lambda l: TAIL_W + 16 * (l - 46)))
    I('qmf1', 'in2 tail write', 'w128', only(lambda l: 46 <= l <= 54, lambda l: F(K_IN2 + 183 + 4 * l)))
    I('qmf1', 'in2 write', 'w128', only(lambda l: l <= 45, lambda l: F(K_IN2 + 183 + 4 * l)))
else:
    I('qmf1', 'weights (this frame), all lanes', 'r128', lambda l: TAIL_W + 16 * min(max(l - 45, 0), 10))
    I('qmf1', 'in2 write, lanes ..54', 'w128', only(lambda l: l <= 54, lambda l: F(K_IN2 + 183 + 4 * l)))
    I('qmf1', 'tail weights (next)', 'r128', only(lambda l: l >= 46, lambda l: TAIL_W + 16 * (10 + l - 46)))
    I('qmf1', 'pre2 write', 'w128', only(lambda l: l >= 46, lambda l: F(PRE2 + 4 * (l - 46))))
# ---------------- second QMF stage ----------------
W2 = K_R2 if PARENT else K_W2
for k in range(13):
    kind = 'r64' if (PARENT and k == 12) else 'r128'
    I('qmf2', 'window %d' % k, kind, lambda l, k=k: F(W2 + 4 * l + 4 * k))
if PARENT:
    I('qmf2', 'work2 tail read', 'r32', only(lambda l: l < 46, lambda l: F(K_R2 + 256 + l)))
    I('qmf2', 'd2 save', 'w32', only(lambda l: l < 46, lambda l: F(D2 + l)))
I('qmf2', 'window (W[k], W[k+1])', 'r64', only(lambda l: l >= 48, lambda l: TAB + 8 * (l - 48)))
if PARENT:
    I('qmf2', 'window (W[30-k], W[31-k])', 'r64', only(lambda l: l >= 48, lambda l: TAB + 4 * (30 - 2 * (l - 48))))
else:
    I('qmf2', 'out_w, all lanes', 'r64', lambda l: OUT_W + 8 * l)
if PARENT:
    at0 = lambda l: K_R2 + 80 + 2 * l
    at1 = lambda l: K_R2 + 336 + 2 * l
    ov0 = lambda l: K_R2 + 48 + 2 * (l - 48)
    ov1 = lambda l: K_R2 + 304 + 2 * (l - 48)
else:
    at0 = lambda l: in01(0, 80 + 2 * l)
    at1 = lambda l: in01(1, 80 + 2 * l + 1)
    ov0 = lambda l: in01(0, 2 * l - 48)
    ov1 = lambda l: in01(1, 2 * l - 48 + 1)
    assert all(at1(l) == at0(l) + 32 and at0(l) == K_R2 + 2 * (l + 40 + ((l + 40) & ~15)) for l in range(64))
    assert all(ov1(l) == ov0(l) + 32 and ov0(l) == K_R2 + 2 * (l - 24 + ((l - 24) & ~15)) for l in range(48, 64))
hi48 = lambda l: l >= 48
if PARENT:
    pair('qmf2', 'overlap | band 0 out (lanes 48..)', 'w64', only(hi48, lambda l: F(ov0(l))), only(hi48, lambda l: F(at0(l))))
    pair('qmf2', 'overlap | band 1 out (lanes 48..)', 'w64', only(hi48, lambda l: F(ov1(l))), only(hi48, lambda l: F(at1(l))))
    pair('qmf2', 'band 0 | band 1 out (lanes ..47)', 'w64', only(lambda l: l < 48, lambda l: F(at0(l))), only(lambda l: l < 48, lambda l: F(at1(l))))
else:
    pair('qmf2', 'band 0 | band 1 out, all lanes', 'w64', lambda l: F(at0(l)), lambda l: F(at1(l)))
    pair('qmf2', 'overlaps (lanes 48..)', 'w64', only(hi48, lambda l: F(ov0(l))), only(hi48, lambda l: F(ov1(l))))
# ---------------- long-block MDCT ----------------
for j, m in enumerate((0, 2, 1, 3)):     # t0, t1 (2 qb), t2 (qb), t3 (3 qb)
    I('mdct', 'pre-twiddle pair %d' % j, 'r64', lambda l, m=m: BASE[l]['pt0'] + m * 4 * BASE[l]['q2'])
for j in range(4):
    I('mdct', 'a%d' % j, 'r32', lambda l, j=j: F(BASE[l]['a'][j]))
    I('mdct', 'c%d' % j, 'r32', lambda l, j=j: F(BASE[l]['c'][j]))
I('mdct', 'b', 'r32', lambda l: F(BASE[l]['ib']))
I('mdct', 'd', 'r32', lambda l: F(BASE[l]['id']))
Z = lambda slot: 8 * slot
I('mdct', 'z write 0', 'w128', lambda l: Z(BASE[l]['za']))
I('mdct', 'z write 1', 'w128', lambda l: Z(BASE[l]['za']) + 16)
I('mdct', 'twiddle B a', 'r64', lambda l: T_R4B + 24 * (BASE[l]['g'] & 3))
pair('mdct', 'twiddles B b, c', 'r64h', lambda l: T_R4B + 24 * (BASE[l]['g'] & 3) + 8, lambda l: T_R4B + 24 * (BASE[l]['g'] & 3) + 16)
for h, (o0, o1) in enumerate(((0, 4), (8, 12))):
    pair('mdct', 'round B read %d' % h, 'r64h', lambda l, o=o0: Z(BASE[l]['zb'] + o), lambda l, o=o1: Z(BASE[l]['zb'] + o))
for h, (o0, o1) in enumerate(((0, 4), (8, 12))):
    pair('mdct', 'round B write %d' % h, 'w64', lambda l, o=o0: Z(BASE[l]['zb'] + o), lambda l, o=o1: Z(BASE[l]['zb'] + o))
pair('mdct', 'twiddles C a, b', 'r64h', lambda l: T_R4C + 24 * (BASE[l]['g'] & 15), lambda l: T_R4C + 24 * (BASE[l]['g'] & 15) + 8)
I('mdct', 'twiddle C c', 'r64', lambda l: T_R4C + 24 * (BASE[l]['g'] & 15) + 16)
pair('mdct', 'twiddles D', 'r64h', lambda l: T_R2D + 8 * (BASE[l]['g'] & 31), lambda l: T_R2D + 8 * (BASE[l]['g'] & 31) + 256)
for h, (o0, o1) in enumerate(((0, 20), (40, 60))):
    pair('mdct', 'round C read %d' % h, 'r64h', lambda l, o=o0: Z(BASE[l]['zc'] + o), lambda l, o=o1: Z(BASE[l]['zc'] + o))
b2 = lambda l: l >= 32
for h, (o0, o1) in enumerate(((0, 20), (40, 60))):
    pair('mdct', 'round C write %d (band 2)' % h, 'w64', only(b2, lambda l, o=o0: Z(BASE[l]['zc'] + o)), only(b2, lambda l, o=o1: Z(BASE[l]['zc'] + o)))
if PARENT:
    I('mdct', 'geo word 1', 'r32', lambda l: F(GEO + 64 + l))
    I('mdct', 'geo word 2', 'r32', lambda l: F(GEO + 128 + l))
else:
    I('mdct', 'geo', 'r128', lambda l: F(GEO + 4 * l))
pair('mdct', 'post-twiddle pairs 0, 2', 'r64h', lambda l: BASE[l]['po0'], lambda l: BASE[l]['po0'] + 256)
I('mdct', 'post-twiddle pair 1', 'r64', lambda l: BASE[l]['po0'] + 8 * BASE[l]['d'][1])
I('mdct', 'post-twiddle pair 3', 'r64', lambda l: BASE[l]['po0'] + 8 * BASE[l]['d'][3])
for h, (o0, o1) in enumerate(((80, 120), (0, 40))):
    pair('mdct', 'round D read %d (band 2)' % h, 'r64h', only(b2, lambda l, o=o0: Z(BASE[l]['zd'] + o)), only(b2, lambda l, o=o1: Z(BASE[l]['zd'] + o)))
for j in range(4):
    sgn = lambda l: 1 if BASE[l]['band'] == 0 else -1
    first = lambda l: BASE[l]['e0'] if BASE[l]['band'] == 0 else BASE[l]['e1']
    second = lambda l: BASE[l]['e1'] if BASE[l]['band'] == 0 else BASE[l]['e0']
    I('mdct', 'coefficient %d, -o.x' % j, 'w32', lambda l, j=j: F(K_R2 + first(l) + sgn(l) * 2 * BASE[l]['d'][j]))
    I('mdct', 'coefficient %d, o.y' % j, 'w32', lambda l, j=j: F(K_R2 + second(l) - sgn(l) * 2 * BASE[l]['d'][j]))
# ---------------- coefficients out, scale factors ----------------
I('out', 'coefficients 0..255', 'r128', lambda l: F(K_R2 + 4 * l))
I('out', 'coefficients 256..511', 'r128', lambda l: F(K_R2 + 256 + 4 * l))
if PARENT:
    I('out', 'geo word 0', 'r32', lambda l: F(GEO + l))


def sf_src(l):
    wide = l >= 44
    b = 44 + ((l - 44) >> 1) if wide else l
    b = b if l < 60 else 0
    return (START_LONG[b] + (10 * (l & 1) if wide and l < 60 else 0)) & ~3


for k in range(3):
    I('out', 'scale-factor scan %d' % k, 'r128', lambda l, k=k: F(K_R2 + sf_src(l) + 4 * k))
I('out', 'sfi store', 'w32', only(lambda l: l < 60 and (l < 44 or not l & 1), lambda l: F(SFI) + ((44 + ((l - 44) >> 1) if l >= 44 else l) & ~3)))
I('out', 'sfi -> side', 'r32', only(lambda l: l < 16, lambda l: F(SFI + l)))

# ---- consistency of the new layout: every operand the pre-twiddle reads is where the QMF stage put that sample -------
if not PARENT:
    where = {}
    for l in range(64):
        for j, smp in enumerate((80 + 2 * l, 81 + 2 * l)):
            where[(0, smp)] = at0(l) + j
            where[(1, smp)] = at1(l) + (1 - j)
        if l >= 48:
            for j, smp in enumerate((2 * l - 48, 2 * l - 47)):
                where[(0, smp)] = ov0(l) + j
                where[(1, smp)] = ov1(l) + (1 - j)
    assert len(set(where.values())) == len(where) == 2 * 160 and all(K_R2 <= v < K_R2 + 512 for v in where.values())
    for l in range(32):
        B = BASE[l]
        n4, q, r, b = 64, 16, B['r'], B['band']
        ks = (0, 2, 1, 3)                # point position j holds k = r + q * bitrev2(j)
        for j in range(4):
            assert B['a'][j] == where[(b, 3 * n4 - 1 - 2 * (r + q * ks[j]))], (l, j)
            assert B['c'][j] == where[(b, n4 + 2 * (r + q * ks[j]))], (l, j)
        if B['use_lo']:
            assert B['ib'] == where[(b, 3 * n4 + 2 * r)] and B['id'] == where[(b, n4 - 1 - 2 * r)]
        else:
            assert B['ib'] == where[(b, 2 * r + 2 * q)] and B['id'] == where[(b, 14 * q - 1 - 2 * r)]

# ---- report ----
tot = collections.OrderedDict()
for phase, name, kind, a, t, c in rows:
    if VERBOSE:
        print('%-6s %-44s %-5s active %3d  all groups %3d  conflict %3d' % (phase, name, kind, a, t, c))
    p = tot.setdefault(phase, [0, 0, 0, 0])
    p[0] += 1; p[1] += a; p[2] += t; p[3] += c
print('%s kernel, one wave, one emitted long-block frame' % ('parent' if PARENT else 'new'))
print('%-8s %6s %8s %11s %9s' % ('phase', 'instr', 'active', 'all groups', 'conflict'))
for p, v in tot.items():
    print('%-8s %6d %8d %11d %9d' % (p, v[0], v[1], v[2], v[3]))
s = [sum(v[i] for v in tot.values()) for i in range(4)]
print('%-8s %6d %8d %11d %9d' % ('total', s[0], s[1], s[2], s[3]))
if PARENT:
    print('measured per unit (profiles/r04_pmc_summary.txt): SQ_LDS_IDX_ACTIVE 524.6, SQ_LDS_BANK_CONFLICT 95.5')
