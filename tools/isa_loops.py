#!/usr/bin/env python3
"""tools/isa_loops.py FILE.s KERNEL_SUBSTRING [MIN_VALU [hist]] -- static census of every backward-branch span (label to
the branch back to it) of a kernel in a hipcc -S listing, where tools/isa_count.py looks at the outermost loop only: the
inner loops of the allocation kernels (the spending loop of heap_phase).  A loop with several back
edges shows up once per edge; blocks the compiler placed out of line (behind __builtin_expect) are outside the span."""
import collections
import re
import sys

lines = open(sys.argv[1]).read().split('\n')
key = sys.argv[2]
minv = int(sys.argv[3]) if len(sys.argv) > 3 else 30
start = next(i for i, l in enumerate(lines) if re.match(r'^_Z\S*:', l) and key in l)
end = next(i for i in range(start, len(lines)) if 's_endpgm' in lines[i])
body = lines[start:end]
labels = {}
for i, l in enumerate(body):
    m = re.match(r'^(\.LBB\d+_\d+):', l)
    if m:
        labels[m.group(1)] = i
for i, l in enumerate(body):
    m = re.search(r's_cbranch_\w+\s+(\.LBB\d+_\d+)', l) or re.search(r's_branch\s+(\.LBB\d+_\d+)', l)
    if not (m and m.group(1) in labels and labels[m.group(1)] < i):
        continue
    lo, hi = labels[m.group(1)], i
    cnt = collections.Counter()
    for x in body[lo:hi + 1]:
        t = x.strip().split()
        if not t or t[0].startswith(('.', ';')) or t[0].endswith(':'):
            continue
        cnt[t[0]] += 1

    def tot(*prefixes):
        return sum(v for k, v in cnt.items() if k.startswith(prefixes))
    valu = tot('v_')
    if valu < minv:
        continue
    salu = sum(v for k, v in cnt.items() if k.startswith('s_') and not k.startswith(('s_waitcnt', 's_nop', 's_cbranch', 's_branch', 's_barrier')))
    print('listing lines %d..%d  VALU %d  LDS %d  SALU %d  VMEM %d | v_cndmask %d  v_cmp %d  v_lshl_or %d  v_max %d  v_mov %d' % (
        start + lo + 1, start + hi + 1, valu, tot('ds_'), salu, tot('global_', 'buffer_', 'scratch_'),
        tot('v_cndmask'), tot('v_cmp'), tot('v_lshl_or'), tot('v_max'), tot('v_mov')))
    if len(sys.argv) > 4:
        for k, v in cnt.most_common(40):
            print('   %4d %s' % (v, k))
