// c1_k_allocate.hip -- allocateBits (bitallocation.js:74-142): the greedy RDO heaps, one lane per heap
#include "c1_device.h"

namespace {

// =====================================================================================================
// bit allocation : allocateBits (bitallocation.js:74-142) as three small kernels
// =====================================================================================================
// The reference runs the greedy heap (distributeBitsRDO, :203-281) for all 8 candidate BFU counts and
// keeps the one with the smallest total distortion (:116-129).  Each candidate is independent, so:
//   k_alloc_first   one lane per sound unit: the 52-BFU candidate.  It then bounds every other candidate
//                   from below without running it: a candidate that codes n BFUs pays at least the
//                   zero-bit distortion of BFUs n..51, summed in the reference's own order (floating-point
//                   addition is monotone, every term is >= 0, so the bound holds for the rounded sums too).
//                   A candidate whose bound already exceeds the 52-BFU total can never win the strict `<`
//                   comparison and is skipped; the others are appended to a work list.
//   k_alloc_bound   one lane per unit that still has candidates alive: a second, much sharper lower bound for each of
//                   them (Lagrangian relaxation of the greedy's knapsack, below), drops what that already excludes
//                   and sends the most promising candidate of the unit to the first round of heaps.
//   k_alloc_rest    one lane per work-list entry (unit, candidate): the same heap run.  First round: one entry per
//                   unit; the lane then sends the unit's other candidates whose bound does not exceed the best total
//                   known now (52 BFUs or this one) to the second round; the others can never win.
//   k_alloc_select  one lane per unit: smallest total, smallest count on ties (:116-129), or the
//                   fallback when no total is finite (:132-139).
// On white noise 97 % of the units stop after k_alloc_first; stationary tonal material keeps all eight candidates
// alive under the first bound (its upper BFUs are nearly silent, so dropping them costs nothing) and ran 8 heaps per
// unit; with the second bound it runs 2.
//
// Heap entry (one 32-bit word, bit 31 clear):  rank(10) | size(5) | sfi(6) | wl(4) | bfu(6).
// `rank` orders the Float32 priorities biasedSF[sfi]*DISTORTION_DELTA_FACTORS[wl]/WORD_LENGTH_DELTA_BITS[wl]
// (bitallocation.js:226-231,267-269) exactly: equal priorities have equal rank, so the strict `>` of
// siftDown (:325-331) -- and with it the tie order -- is reproduced.  With kLow = the 21 payload bits,
// rank(a) > rank(b)  <=>  a > (b | kLow): one integer compare, no field extraction.  Rank 0 never occurs
// in a live entry, so unused slots (kSentinel: rank 0) and parked entries (below) act as sentinels: no bounds checks in the sift.
//
// Heaps live in LDS as heap[row][lane] (64 dwords per row: conflict-free, the two children of a node one
// ds_read2st64 apart).  An entry that leaves the heap is parked, rank cleared, in the slot the shrinking
// heap frees, so when the loop ends slots [0, initial size) hold every BFU with its final word length.
// Slots 0..2 (the root and its children) live in registers from the construction to the word-length gather and have
// no row: row r holds slot r + 3, and the last row is the sentinel behind slot 51.  The children of the slot in row q
// are rows 2q + 4 and 2q + 5, its grandchildren rows 4q + 12 .. 4q + 15.
// 50 rows are 12 800 bytes, and a CU hands out its LDS in 128 blocks of 1 280 bytes: 10 blocks per single-wave
// workgroup, 12 workgroups per CU.  (With a row per slot, 53 rows = 13 568 bytes took 11 blocks: 11 waves per CU,
// not the 12 this comment claimed before.)
constexpr int kHeapRows = 52 - 3 + 1;
constexpr int kHeapLdsBytes = kHeapRows * 64 * 4;
static_assert((kHeapLdsBytes + 1279) / 1280 * 12 <= 128, "heaps: 12 single-wave workgroups per CU = at most 10 LDS blocks of 1 280 bytes each");
constexpr uint32_t kLow = 0x1FFFFFu;
constexpr uint32_t kSentinel = 52u;           // rank 0, word length 0, "BFU 52": the gather behind the heap run sends it to the spare slot
constexpr int kCandBytes = kCandidateBytes;  // per unit: 8 totals (double) + 8 x 32-byte results + 8 lower bounds
constexpr double kAlive = -1.0;              // total of a candidate that may still win and has not been evaluated (real totals are >= 0)

__device__ __forceinline__ uint32_t heap_entry(uint32_t rank, int size, int s, int wl, int b) {
  return (rank << 21) | ((uint32_t)size << 16) | ((uint32_t)s << 10) | ((uint32_t)wl << 6) | (uint32_t)b;
}

// siftDown (bitallocation.js:314-341) for every lane of the wave at once, from a slot `i` >= 3 (one that has a row).
// `el`,`er` are the already loaded children of `i`; lanes finish at different depths, the loop runs while any lane still moves.
__device__ __forceinline__ void heap_sift_down(uint32_t *hp, int i, uint32_t v, uint32_t el, uint32_t er, bool active) {
  const uint32_t vmax = v | kLow;
  for (;;) {
    const uint32_t m = max(el | kLow, vmax);
    const bool take_r = er > m;                    // pr > max(pl, pv)
    const bool take_l = !take_r && el > vmax;      // pl > pv
    const bool moved = active && (take_r || take_l);
    if (active) hp[(i - 3) * 64] = moved ? (take_r ? er : el) : v;   // a lane that stops here drops v into place
    active = moved;
    if (__builtin_amdgcn_ballot_w64(active) == 0) break;
    i = moved ? 2 * i + 1 + (take_r ? 1 : 0) : i;
    // children 2i+1, 2i+2; a node without children reads (slot 51, sentinel) and its left value is masked
    const int l = 2 * i + 1;
    const uint32_t *src = hp + (min(l, 51) - 3) * 64;
    el = l < 52 ? src[0] : 0u;
    er = src[64];
  }
}

// the same from slot `k` = 1 or 2, which lives in a register and holds `v`: returns what the slot holds afterwards.
// Its children are slots 3,4 or 5,6 = rows 2k - 2, 2k - 1.
__device__ __forceinline__ uint32_t heap_sift_below_root(uint32_t *hp, int k, uint32_t v, bool active) {
  const uint32_t *src = hp + (2 * k - 2) * 64;
  const uint32_t el = src[0], er = src[64];
  const uint32_t vmax = v | kLow;
  const bool take_r = er > max(el | kLow, vmax);
  const bool take_l = !take_r && el > vmax;
  const bool moved = active && (take_r || take_l);
  if (__builtin_amdgcn_ballot_w64(moved) != 0) {
    const int i = 2 * k + 1 + (take_r ? 1 : 0);                       // 3..6: its children are slots 7..14
    heap_sift_down(hp, i, v, hp[(2 * i + 1 - 3) * 64], hp[(2 * i + 2 - 3) * 64], moved);
  }
  return moved ? (take_r ? er : el) : v;
}

// kSpecs as compile-time constants: in the 52-way unrolled loops below a size is then part of an immediate, where the
// table in constant memory cost a scalar register per BFU (168 of them spilled to vector lanes in k_alloc_first)
constexpr int kSpecsHost[52] = {8, 8, 8, 8, 4, 4, 4, 4, 8, 8, 8, 8, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6, 7, 7, 7, 7, 9, 9, 9, 9, 10, 10, 10, 10,
                                12, 12, 12, 12, 12, 12, 12, 12, 20, 20, 20, 20, 20, 20, 20, 20};
constexpr int dist_class(int size) {   // index of a BFU size in kDistSizes (C1DevEncOpts::dist)
  for (int c = 0; c < 8; c++) if (kDistSizes[c] == size) return c;
  return -1;
}
constexpr bool sizes_come_in_fours() {
  for (int b = 0; b < 52; b++) if (kSpecsHost[b] != kSpecsHost[b & ~3]) return false;
  return true;
}
static_assert(sizes_come_in_fours(), "the four BFUs whose indices share a dword share a size");
static_assert(dist_class(4) == 0 && dist_class(20) == 7 && dist_class(kSpecsHost[24]) == 2, "every BFU size has its row of the distortion tables");

// The 52 scale-factor indices are taken apart three times (guess, initial heap, totals).  Left alone, the compiler forms
// the 52 "s != 0" lane masks once and keeps them for later: 104 scalar registers, which it then spills to vector lanes.
// Passing the packed indices through an empty asm between the phases makes each phase form what it needs itself.
__device__ __forceinline__ void reopen(uint32_t (&sf)[13]) {
#pragma unroll
  for (int i = 0; i < 13; i++) asm volatile("" : "+v"(sf[i]));
}

// The heap phase of one candidate: initial heap, heapify, spending loop.  AFFINE (wave-uniform, C1DevEncOpts::rank_affine)
// chooses between two instances so that neither carries the other's code: ranks by the integer form, where a
// successful step is ONE addition to the root's entry (rank_step0 / rank_step, verified on the host for every
// (sfi, wl)), or ranks looked up in the table of the Float32 priorities.
// The three top slots of the heap live in registers (r0 = root, r1/r2 = its children) and are handed back in them:
// most steps end at the root (equal priorities do not move, :325-331), so they touch no memory.
template <bool AFFINE>
__device__ __forceinline__ void heap_phase(uint32_t *hp, int n, const uint32_t (&sf)[13], const C1DevEncOpts *O, bool live,
                                           uint32_t &r0, uint32_t &r1, uint32_t &r2) {
  const __attribute__((address_space(4))) uint16_t *rank_t = (const __attribute__((address_space(4))) uint16_t *)O->rank;
  // (an LDS copy of this table is slower: 512 more bytes per wave cost a wave per CU, measured 1.50 -> 1.63 ms)
  // entry of (s, wl = 0) in the integer form: ((A s + C + off) << 21) | (s << 10) = (((A << 11) | 1) s + ((C + off) << 11)) << 10,
  // a 24-bit multiply-add and a shift that ORs the BFU's constant bits in
  const uint32_t mul0 = ((uint32_t)O->rank_a << 11) | 1u, add0 = (uint32_t)(O->rank_c + O->rank_off) << 11;
  const uint32_t step0 = O->rank_step0, step = O->rank_step;
  int remaining = 212 * 8 - 40 - 10 * n;                   // bitallocation.js:97-100
  // distributeBitsRDO (:203-281): initial heap = BFUs below n with a non-zero scale factor
  // branch-free: every BFU writes its entry at the cursor, only live ones advance it (the next one overwrites the
  // slot otherwise; what the last dead one leaves behind is cleared with the sentinels)
  // (in blocks of 13 BFUs that the scheduler cannot interleave: see totals_tabled)
  // The cursor is lane-varying, so slots 0..2 cannot go to registers as they are written: while BFUs 0..49 are placed
  // they borrow the last three rows (47..49), which slots 50, 51 and the sentinel need only afterwards.  `cur` is the
  // heap size + 47; the row of the cursor is cur mod 50, one subtraction and one unsigned minimum.
  uint32_t cur = 47;
#pragma unroll
  for (int b0 = 0; b0 < 52; b0 += 13) if (own_block()) {
#pragma unroll
  for (int b = b0; b < b0 + 13 && b < 50; b++) {
    if (b < n) {
      const int s = (sf[b >> 2] >> ((b & 3) * 8)) & 63;
      const uint32_t fixed = ((uint32_t)kSpecsHost[b] << 16) | (uint32_t)b;
      uint32_t *at = hp + min(cur, cur - (uint32_t)kHeapRows) * 64;
      if constexpr (AFFINE) *at = ((__umul24(mul0, (uint32_t)s) + add0) << 10) | fixed;
      else *at = ((uint32_t)rank_t[s * 16] << 21) | ((uint32_t)s << 10) | fixed;
      cur += (s != 0 && live) ? 1 : 0;
    }
  }
  }
  int hs = (int)cur - 47;
  r0 = hp[47 * 64]; r1 = hp[48 * 64]; r2 = hp[49 * 64];
  // BFUs 50 and 51: the cursor is at most 51, that is row 48
#pragma unroll
  for (int b = 50; b < 52; b++) {
    if (b < n) {
      const int s = (sf[b >> 2] >> ((b & 3) * 8)) & 63;
      const uint32_t fixed = ((uint32_t)kSpecsHost[b] << 16) | (uint32_t)b;
      uint32_t e;
      if constexpr (AFFINE) e = ((__umul24(mul0, (uint32_t)s) + add0) << 10) | fixed;
      else e = ((uint32_t)rank_t[s * 16] << 21) | ((uint32_t)s << 10) | fixed;
      r0 = hs == 0 ? e : r0; r1 = hs == 1 ? e : r1; r2 = hs == 2 ? e : r2;
      if (hs >= 3) hp[(hs - 3) * 64] = e;
      hs += (s != 0 && live) ? 1 : 0;
    }
  }
  // rank 0 behind the heap: below every live entry
  r0 = hs > 0 ? r0 : kSentinel; r1 = hs > 1 ? r1 : kSentinel; r2 = hs > 2 ? r2 : kSentinel;
  for (int k = max(hs, 3) - 3; k < kHeapRows; k++) hp[k * 64] = kSentinel;
  // heapify (:238-241), per-lane trip counts: the slots that have a row, then slots 2, 1 and the root
  const int half = hs >> 1;
  for (int i = half - 1; i >= 3; i--) {
    const int l = 2 * i + 1;
    heap_sift_down(hp, i, hp[(i - 3) * 64], hp[(l - 3) * 64], hp[(l - 2) * 64], true);
  }
  if (__builtin_amdgcn_ballot_w64(half >= 2) != 0) {
    r2 = heap_sift_below_root(hp, 2, r2, half >= 3);
    r1 = heap_sift_below_root(hp, 1, r1, half >= 2);
  }
  if (__builtin_amdgcn_ballot_w64(half >= 1) != 0) {
    const uint32_t v = r0, vmax = v | kLow;
    const bool take_r = r2 > max(r1 | kLow, vmax);
    const bool take_l = !take_r && r1 > vmax;
    const bool moved = half >= 1 && (take_r || take_l);
    r0 = moved ? (take_r ? r2 : r1) : v;
    const uint32_t below = heap_sift_below_root(hp, take_r ? 2 : 1, v, moved);
    r1 = (moved && !take_r) ? below : r1; r2 = (moved && take_r) ? below : r2;
  }
  // greedy spending loop (:244-278): the root either takes its next priority or leaves the heap (does not
  // fit :251-258, or reached the last word length :271-277); then one sift.
  // The smallest BFU has 4 coefficients, so with fewer than 4 bits left no entry can take its next step: the
  // remaining iterations of the reference only pop entries that do not fit and change nothing (:251-258).
  // A lane whose heap is empty gives its bits up, so "4 bits left" alone says whether a lane still runs.
  remaining = hs > 0 ? remaining : 0;
  while (__builtin_amdgcn_ballot_w64(remaining >= 4) != 0) {
    const bool run = remaining >= 4;
    const uint32_t top = r0;
    const bool wl0 = (top & (15u << 6)) == 0;
    const int size = (top >> 16) & 31;
    const int cost = size << (wl0 ? 1 : 0);                // WORD_LENGTH_DELTA_BITS = [2,1,1,...]
    const bool fits = cost <= remaining;
    uint32_t v, upd;                                       // the root after its step; the same BFU as it leaves (rank 0)
    bool last_wl;                                          // the step reaches the last word length
    if constexpr (AFFINE) {
      v = top + (wl0 ? step0 : step);
      upd = (fits ? v : top) & kLow;
      last_wl = (v & (15u << 6)) == (15u << 6);
    } else {
      const int wl = (top >> 6) & 15, s = (top >> 10) & 63;
      const int nxt = wl + (fits ? 1 : 0);
      upd = (top & ~((0x3FFu << 21) | (15u << 6))) | ((uint32_t)nxt << 6);
      v = upd | ((uint32_t)rank_t[s * 16 + (nxt & 15)] << 21);
      last_wl = nxt >= 15;
    }
    remaining -= fits ? cost : 0;                          // (a lane that no longer runs has less than any cost left, or a sentinel of size 0 on top)
    const bool leaves = run && (!fits || last_wl);
    if (__builtin_expect(__builtin_amdgcn_ballot_w64(leaves) != 0, 0)) {
      // Out of line, behind its vote: the last element replaces the root; the leaver is parked, rank 0, in the slot that
      // frees.  A heap of one parks its root where it is (nothing below it has a rank, so the sift leaves it there) and
      // the lane stops.
      const int li = hs - 1;
      const uint32_t deep = hp[(max(li, 3) - 3) * 64];
      if (leaves) {
        v = li == 0 ? upd : (li == 1 ? r1 : (li == 2 ? r2 : deep));
        hs = li;
        if (li > 2) hp[(li - 3) * 64] = upd;
        r1 = li == 1 ? upd : r1; r2 = li == 2 ? upd : r2;
        remaining = li == 0 ? 0 : remaining;
      }
    }
    // The sift moves a hole, not the entry: at every level the winning child (one compare, one select) moves up if it
    // beats v (one compare) and the hole follows it; v itself is written once, where the descent stops.
    const uint32_t vmax = v | kLow;
    // level 0: root against r1, r2
    const bool t0 = r2 > (r1 | kLow);                      // pr > pl
    const uint32_t w0 = t0 ? r2 : r1;
    const bool mv0 = run && w0 > vmax;                     // max(pl, pr) > pv
    if (run) r0 = mv0 ? w0 : v;
    // level 1: the chosen child's children are slots 3,4 or 5,6 = rows 0,1 or 2,3.  (No "does any lane still move?" test
    // in front of levels 1 and 2: among 64 heaps one nearly always does, and the test costs more than the level it would skip.)
    const uint32_t *s1 = hp + (t0 ? 2 : 0) * 64;
    const uint32_t el = s1[0], er = s1[64];
    // both pairs of grandchildren (slots 7..10 or 11..14 = rows 4..7 or 8..11) are requested with the children: one LDS
    // round trip decides two levels -- the loop is a chain of dependent round trips, not of instructions
    const uint32_t *s2 = hp + (t0 ? 8 : 4) * 64;
    const uint32_t g0 = s2[0], g1 = s2[64], g2 = s2[128], g3 = s2[192];
    const bool t1 = er > (el | kLow);
    const uint32_t w1 = t1 ? er : el;
    const bool mv1 = mv0 && w1 > vmax;
    const uint32_t val = mv1 ? w1 : v;
    r1 = (mv0 && !t0) ? val : r1; r2 = (mv0 && t0) ? val : r2;
    // levels 2..5 unrolled (a heap of 52 has six): the hole in rows 0..3 against its children (the grandchildren above),
    // then ONE more round trip for the children (rows 12..27) and grandchildren (rows 28..) of the row in 4..11 it moves
    // to.  Two round trips per step where the loop of heap_sift_down made up to five (one per level and one more to find
    // that the last level has no children); a lane that stops early just stops writing.
    const uint32_t cl = t1 ? g2 : g0, cr = t1 ? g3 : g1;
    const bool t2 = cr > (cl | kLow);
    const uint32_t w2 = t2 ? cr : cl;
    const bool mv2 = mv1 && w2 > vmax;
    const int q2 = (t0 ? 2 : 0) + (t1 ? 1 : 0);
    uint32_t *hole = hp + q2 * 64;
    if (mv2) *hole = w2;
    if (__builtin_amdgcn_ballot_w64(mv2) != 0) {
      const int q3 = 2 * q2 + 4 + (t2 ? 1 : 0);                   // rows 4..11 (slots 7..14)
      const uint32_t *s3 = hp + (2 * q3 + 4) * 64;                // children: rows 12..27 (slots 15..30)
      const uint32_t d0 = s3[0], d1 = s3[64];
      // grandchildren: the four rows from 4 q3 + 12, one base and immediate offsets.  Only rows 9..11 have grandchildren
      // past slot 51; of those only slot 51 (a real one) and the sentinel row behind it (whose rank 0 never wins) matter, as
      // the children of slot 25 (row 22).  Such a lane reads rows 46..49 and takes the upper pair; a slot from 26 on (row 23)
      // has no children, which its number says.
      const bool far = q3 >= 9;
      const uint32_t *s4 = hp + min(4 * q3 + 12, kHeapRows - 4) * 64;
      const uint32_t h0 = s4[0], h1 = s4[64], h2 = s4[128], h3 = s4[192];
      const bool t3 = d1 > (d0 | kLow);
      const uint32_t w3 = t3 ? d1 : d0;
      const bool mv3 = mv2 && w3 > vmax;
      uint32_t *p3 = hp + q3 * 64;
      hole = mv2 ? p3 : hole;
      if (mv3) *p3 = w3;
      const int q4 = 2 * q3 + 4 + (t3 ? 1 : 0);                   // rows 12..27
      const bool upper = t3 || far;
      const uint32_t e0 = upper ? h2 : h0, e1 = upper ? h3 : h1;
      const bool t4 = e1 > (e0 | kLow);
      const uint32_t w4 = t4 ? e1 : e0;
      const bool mv4 = mv3 && q4 < 23 && w4 > vmax;
      uint32_t *p4 = hp + q4 * 64;
      hole = mv3 ? p4 : hole;
      if (mv4) *p4 = w4;
      hole = mv4 ? hp + (2 * q4 + 4 + (t4 ? 1 : 0)) * 64 : hole;   // rows 28..48 (slots 31..51): no children
    }
    if (mv1) *hole = v;                                    // (a hole in slots 0..2 took v as it was decided, above)
  }
}

// calculateTotalDistortion (:157-190), sequential double sum, index ascending, from the host's tables of its terms
// (C1DevEncOpts::dist, verified there): one 16-byte lane-varying read and an exponent subtraction per BFU where the
// reference's order of operations costs two conversions and three binary64 products.  BOUND: moreover the first lower
// bounds of the seven smaller candidates (k_alloc_first), which are sums of the zero-bit terms this loop loads anyway.
// The reads go where `biased` goes (constant address space): unconditional, so the compiler requests them in batches
// (tools/isa_waits.py).  A silent BFU (s = 0) has word length 0 and a zero-bit term of 0.
template <bool BOUND>
__device__ __forceinline__ void totals_tabled(int n, const uint32_t (&sf)[13], const C1DevEncOpts *O, uint64_t res0, uint64_t res1,
                                              uint64_t res2, uint64_t res3, double &total, double (&lbs)[7]) {
  typedef double d2 __attribute__((ext_vector_type(2)));
  const __attribute__((address_space(4))) d2 *dist = (const __attribute__((address_space(4))) d2 *)O->dist;
  total = 0.0;
#pragma unroll
  for (int c = 0; c < 7; c++) lbs[c] = 0.0;
  // (in blocks of 13 BFUs the scheduler cannot interleave: across all 52 it forms every "wl == 0" lane mask first and
  // runs out of scalar registers to hold them)
#pragma unroll
  for (int b0 = 0; b0 < 52; b0 += 13) if (own_block()) {
#pragma unroll
  for (int b = b0; b < b0 + 13; b++) {
    const int s = (sf[b >> 2] >> ((b & 3) * 8)) & 63;
    const uint64_t word = b < 16 ? res0 : (b < 32 ? res1 : (b < 48 ? res2 : res3));
    const int wl = (int)((word >> ((b & 15) * 4)) & 15);
    const d2 zc = dist[dist_class(kSpecsHost[b]) * 64 + s];
    // biased * size * INV_POWER_OF_TWO[wl + 1]
    const double coded = __hiloint2double(__double2hiint(zc.y) - ((wl + 1) << 20), __double2loint(zc.y));
    total += (b >= n || wl == 0) ? zc.x : coded;
    if constexpr (BOUND) {
      if (b >= 20) lbs[0] += zc.x;
      if (b >= 28) lbs[1] += zc.x;
      if (b >= 32) lbs[2] += zc.x;
      if (b >= 36) lbs[3] += zc.x;
      if (b >= 40) lbs[4] += zc.x;
      if (b >= 44) lbs[5] += zc.x;
      if (b >= 48) lbs[6] += zc.x;
    }
  }
  }
}

// the same in the reference's own order of operations: for a biased table whose terms the host could not tabulate
template <bool BOUND>
__device__ __forceinline__ void totals_direct(int n, const uint32_t (&sf)[13], const C1DevEncOpts *O, uint64_t res0, uint64_t res1,
                                              uint64_t res2, uint64_t res3, double &total, double (&lbs)[7]) {
  const __attribute__((address_space(4))) double *biased = (const __attribute__((address_space(4))) double *)O->biased;
  total = 0.0;
#pragma unroll
  for (int c = 0; c < 7; c++) lbs[c] = 0.0;
#pragma unroll
  for (int b0 = 0; b0 < 52; b0 += 13) if (own_block()) {
#pragma unroll
  for (int b = b0; b < b0 + 13; b++) {
    const int s = (sf[b >> 2] >> ((b & 3) * 8)) & 63;
    const uint64_t word = b < 16 ? res0 : (b < 32 ? res1 : (b < 48 ? res2 : res3));
    const int wl = (int)((word >> ((b & 15) * 4)) & 15);
    const int size = kSpecsHost[b];
    // the table value is loaded whatever s is (index 0 is a valid entry) and masked afterwards: a lane-varying table read is
    // a cache round trip, and under a condition each of the 52 is waited for where it is issued, one after the other
    const double bs = biased[s];
    // zeroBitDistortions[b] = Float32(biasedSF * 2 * size), 0 when sfi == 0 (:76,87-89)
    const double z = s != 0 ? (double)f32(bs * 2.0 * (double)size) : 0.0;
    const double ip2 = __hiloint2double((1023 - wl_bits(wl)) << 20, 0);     // INV_POWER_OF_TWO[bits] = 2^-bits
    const double coded = s != 0 ? bs * ip2 * (double)size : 0.0;            // (a silent BFU adds nothing: the total is never -0)
    total += (b >= n || wl == 0) ? z : coded;
    if constexpr (BOUND) {
      if (b >= 20) lbs[0] += z;
      if (b >= 28) lbs[1] += z;
      if (b >= 32) lbs[2] += z;
      if (b >= 36) lbs[3] += z;
      if (b >= 40) lbs[4] += z;
      if (b >= 44) lbs[5] += z;
      if (b >= 48) lbs[6] += z;
    }
  }
  }
}

// One greedy heap per lane: candidate with `n` BFUs.  sf = the unit's 52 scale-factor indices (13 dwords).
// Returns the 52 final word-length indices (4 bits each) and the candidate's total distortion; with BOUND also the
// zero-bit distortion of BFUs 20.., 28.., 32.., .. 48.. upwards, each summed from its first BFU.
template <bool BOUND>
__device__ __forceinline__ void run_candidate(uint32_t *hp, int n, uint32_t (&sf)[13], const C1DevEncOpts *O,
                                              bool live, uint64_t &res0, uint64_t &res1, uint64_t &res2,
                                              uint64_t &res3, double &total, double (&lbs)[7]) {
  uint32_t top[3];
  if (O->rank_affine != 0) heap_phase<true>(hp, n, sf, O, live, top[0], top[1], top[2]);
  else heap_phase<false>(hp, n, sf, O, live, top[0], top[1], top[2]);
  // Every BFU that ever entered the heap now sits in one of the first slots (as many as the heap started with: three registers,
  // then the rows) with its final word length; the slots behind hold the sentinel, which names BFU 52.  The word lengths are put
  // in BFU order through the lane's own column of the heap: the upper half of every entry is done with (rank, size), so
  // BFU b's word length goes to byte 2 + (b & 1) of row b >> 1 (a byte store: the low half, which names an unread
  // entry's BFU and word length, stays as it is; the sentinel's byte is in row 26 and is never read), then the 52 bytes are
  // read back in order and packed with constant shifts.  6 vector instructions per BFU; selecting one of four 64-bit
  // words by a lane-varying index cost 25 (1 300 of the 8 300 a wave of k_alloc_first issued).
  {
    uint8_t *hb = reinterpret_cast<uint8_t *>(hp);
    auto put = [hb](uint32_t e) { hb[((e & 62u) << 7) + (e & 1u) + 2] = (uint8_t)((e >> 6) & 15u); };
#pragma unroll
    for (int k = 0; k < 26; k++) *reinterpret_cast<uint16_t *>(hb + k * 256 + 2) = 0;
#pragma unroll
    for (int j = 0; j < 3; j++) put(top[j]);
#pragma unroll
    for (int k0 = 0; k0 < kHeapRows - 1; k0 += 8) {
      uint32_t e[8];
#pragma unroll
      for (int j = 0; j < 8; j++) if (k0 + j < kHeapRows - 1) e[j] = hp[(k0 + j) * 64];
#pragma unroll
      for (int j = 0; j < 8; j++) if (k0 + j < kHeapRows - 1) put(e[j]);
    }
    uint32_t d[8];
#pragma unroll
    for (int i = 0; i < 8; i++) {
      d[i] = 0;
#pragma unroll
      for (int j = 0; j < 8; j++) if (8 * i + j < 52) d[i] |= (uint32_t)hb[((8 * i + j) >> 1) * 256 + 2 + (j & 1)] << (4 * j);
    }
    res0 = (uint64_t)d[0] | ((uint64_t)d[1] << 32); res1 = (uint64_t)d[2] | ((uint64_t)d[3] << 32);
    res2 = (uint64_t)d[4] | ((uint64_t)d[5] << 32); res3 = (uint64_t)d[6] | ((uint64_t)d[7] << 32);
  }
  reopen(sf);
  if (O->dist_tables != 0) totals_tabled<BOUND>(n, sf, O, res0, res1, res2, res3, total, lbs);
  else totals_direct<BOUND>(n, sf, O, res0, res1, res2, res3, total, lbs);
}

__device__ __forceinline__ void load_sfi(const uint8_t *side, int64_t unit, uint32_t (&sf)[13]) {
  const uint4 *src = reinterpret_cast<const uint4 *>(side + unit * kSideBytes);
  const uint4 a = src[0], b = src[1], c = src[2];
  const uint32_t d = reinterpret_cast<const uint32_t *>(src)[12];
  sf[0] = a.x; sf[1] = a.y; sf[2] = a.z; sf[3] = a.w; sf[4] = b.x; sf[5] = b.y; sf[6] = b.z; sf[7] = b.w;
  sf[8] = c.x; sf[9] = c.y; sf[10] = c.z; sf[11] = c.w; sf[12] = d;
}

__device__ __forceinline__ void store_candidate(uint8_t *cand, int64_t unit, int c, double total, uint64_t r0,
                                                uint64_t r1, uint64_t r2, uint64_t r3) {
  uint8_t *base = cand + unit * kCandBytes;
  reinterpret_cast<double *>(base)[c] = total;
  uint64_t *dst = reinterpret_cast<uint64_t *>(base + 64 + c * 32);
  dst[0] = r0; dst[1] = r1; dst[2] = r2; dst[3] = r3;
}

__device__ __forceinline__ bool getenv_no_tonal(const C1DevEncOpts *O) { return O->alloc_no_tonal != 0; }   // C1_ALLOC_NO_TONAL=1 (experiments)

__global__ __launch_bounds__(C1_WAVE, 3) void k_alloc_first(C1EncodeLaunch L) {
  __shared__ uint32_t heap[kHeapRows * 64];
  const C1DevEncOpts *O = L.opts;
  const __attribute__((address_space(4))) double *biased = (const __attribute__((address_space(4))) double *)O->biased;
  const int lane = threadIdx.x;
  // list mode (exact redo after the speculative pass): positions index L.unit_list
  const bool listed = L.unit_list != nullptr;
  const int64_t units_total = listed ? (int64_t)*L.unit_count : L.frames * L.channels;
  for (int64_t pos0 = (int64_t)blockIdx.x * 64; pos0 < units_total; pos0 += (int64_t)gridDim.x * 64) {
  const int64_t pos = pos0 + lane;
  const bool live = pos < units_total;
  const int64_t unit = listed ? (int64_t)L.unit_list[live ? pos : 0] : pos;
  uint32_t sf[13];
  load_sfi(L.side, live ? unit : 0, sf);
  // Which candidate to run first?  Where the upper BFUs carry next to nothing (tones, low-passed material) dropping
  // them is free, a smaller candidate wins, and the 52-BFU heap would be run for nothing: such units go to
  // k_alloc_bound with all eight candidates open.  The test is a guess (it only chooses the order of work, every
  // path ends in the same exact comparison): the continuous relaxation of the 52-BFU problem spends its 1 136 bits at
  // log2 lambda = (sum size_b log2 biasedSF_b - 1136) / N over the N coefficients of non-silent BFUs and then has a
  // total of about N lambda / ln 2 (measured: the 52-BFU total is 0.7-1.0 of that estimate).  Units whose 52-BFU
  // candidate wins have a zero-bit distortion t6 of the top four BFUs above 0.44 of the estimate (5 % quantile over
  // white, pink and mixed material), units where a smaller candidate wins mostly below 0.4 (tools/alloc_tonal_stats.py).
  bool tonal = false;
  {
    // N and sum size_b s_b as integers, four BFUs (one dword of indices, one size) at a time: both stay far below 2^24, so
    // the binary32 sums they stand for are exact
    uint32_t n_int = 0, s_int = 0;
#pragma unroll
    for (int g = 0; g < 13; g++) {
      const uint32_t x = sf[g] & 0x3F3F3F3Fu;
      const uint32_t nz = ((x + 0x3F3F3F3Fu) >> 6) & 0x01010101u;              // 1 in every byte whose index is not 0
      n_int = __umul24(__builtin_amdgcn_sad_u8(nz, 0u, 0u), (uint32_t)kSpecsHost[4 * g]) + n_int;
      s_int = __umul24(__builtin_amdgcn_sad_u8(x, 0u, 0u), (uint32_t)kSpecsHost[4 * g]) + s_int;
    }
    const float n_coef = (float)n_int, s_la = (float)s_int;
    // sum size la = la_slope * sum size s + la_off * N
    const float la_sum = __builtin_fmaf(O->la_slope, s_la, O->la_off * n_coef);
    const float t_est = 1.442695f * n_coef * __builtin_amdgcn_exp2f((la_sum - 1136.0f) / n_coef);
    float t6f = 0.0f;                                       // zero-bit distortion of the top four BFUs (a guess needs no more than binary32)
#pragma unroll
    for (int b = 48; b < 52; b++) {
      const int s = (sf[b >> 2] >> ((b & 3) * 8)) & 63;
      const float bs = (float)biased[s];
      t6f += s != 0 ? bs * (2.0f * (float)kSpecsHost[b]) : 0.0f;
    }
    const bool mine = n_coef > 0.0f && t6f < 0.35f * t_est && !getenv_no_tonal(O);
    // one decision per wave (the majority's): a heap loop runs as long as any lane of the wave needs it, so skipping
    // it pays only when every lane does
    tonal = 2 * __popcll(__builtin_amdgcn_ballot_w64(live && mine)) > __popcll(__builtin_amdgcn_ballot_w64(live));
  }
  uint64_t r0, r1, r2, r3;
  double total;
  // with it, the lower bounds of the other seven candidates: zero-bit distortion of the BFUs they do not code, each
  // summed from its first uncoded BFU upwards (seven running sums in the pass that forms the total)
  double lbs[7];
  reopen(sf);
  run_candidate<true>(heap + lane, 52, sf, O, live && !tonal, r0, r1, r2, r3, total, lbs);
  uint32_t survivors = 0;
  {
    const double t0 = lbs[0], t1 = lbs[1], t2 = lbs[2], t3 = lbs[3], t4 = lbs[4], t5 = lbs[5], t6 = lbs[6];
    // skip only when the bound is strictly above a finite 52-BFU total; NaN / Inf totals prune nothing
    const bool finite = total < __builtin_huge_val();
    survivors = (!(finite && t0 > total) ? 1u : 0u) | (!(finite && t1 > total) ? 2u : 0u) |
                (!(finite && t2 > total) ? 4u : 0u) | (!(finite && t3 > total) ? 8u : 0u) |
                (!(finite && t4 > total) ? 16u : 0u) | (!(finite && t5 > total) ? 32u : 0u) |
                (!(finite && t6 > total) ? 64u : 0u);
  }
  if (tonal) survivors = 0xffu;                               // nothing evaluated, everything open (bit 7 = the 52-BFU candidate)
  const bool finite52 = total < __builtin_huge_val();
  if (live && survivors == 0) {
    // nothing else can win: the 52-BFU candidate is the allocation (or the fallback when its total is not finite,
    // bitallocation.js:132-139); no candidate record, no selection pass for this unit
    uint64_t *dst = reinterpret_cast<uint64_t *>(L.alloc + unit * kAllocBytes);
    if (finite52) { dst[0] = r0; dst[1] = r1; dst[2] = r2; dst[3] = r3 | (7ull << 60); }
    else { dst[0] = 0; dst[1] = 0; dst[2] = 0; dst[3] = 1ull << 59; }
  } else if (live) {
    // totals of the other candidates: +inf = cannot win, kAlive = still possible and not evaluated yet
    uint8_t *base = L.cand + unit * kCandBytes;
    double *tot = reinterpret_cast<double *>(base);
#pragma unroll
    for (int c = 0; c < 7; c++) tot[c] = ((survivors >> c) & 1u) ? kAlive : __builtin_huge_val();
    if (tonal) tot[7] = kAlive;
    else store_candidate(L.cand, unit, 7, finite52 ? total : __builtin_huge_val(), r0, r1, r2, r3);
  }
  // append the unit to the selection list: one atomic per wave
  const uint64_t sel_mask = __builtin_amdgcn_ballot_w64(live && survivors != 0);
  uint32_t sel_base = 0;
  if (lane == 0 && sel_mask != 0) sel_base = atomicAdd(L.work_count + 1, (uint32_t)__popcll(sel_mask));
  sel_base = (uint32_t)__builtin_amdgcn_readfirstlane((int)sel_base);
  if (live && survivors != 0) L.sel_list[sel_base + (uint32_t)__popcll(sel_mask & ((1ull << lane) - 1ull))] = (uint32_t)unit;
  }
}

// =====================================================================================================
// The second bound.  For a candidate that codes n BFUs with B = 1656 - 10 n bits, ANY word lengths wl_b that fit the
// budget (sum size_b bits(wl_b) <= B) -- in particular the ones the greedy heap ends with -- satisfy, for every
// multiplier lambda >= 0,
//     sum_{b<n} D_b(wl_b)  >=  sum_{b<n} [D_b(wl_b) + lambda size_b bits(wl_b)] - lambda B
//                          >=  sum_{b<n} min_wl [D_b(wl) + lambda size_b bits(wl)] - lambda B,
// with D_b(0) = zeroBitDistortions[b] and D_b(wl) = biasedSF * 2^-bits * size the very terms calculateTotalDistortion adds
// (bitallocation.js:157-190).  Adding the zero-bit terms of the BFUs the candidate does not code gives a lower bound
// on its total for every lambda; it is sharpest near the multiplier at which the relaxed problem spends exactly B bits,
// found by bisection on log2 lambda (the relaxed spend is a decreasing step function of it).  The inner minimum is
// explicit: D + lambda size bits is convex in bits >= 2 (each further bit gains biasedSF 2^-(bits+1) per coefficient),
// so its minimum over 2..16 bits sits at clamp(floor(log2(biasedSF / lambda)), 2, 16); the zero-bit term competes
// separately because it is stored as a Float32.  Measured against the totals the heaps produce the bound is within
// 2-4 % (tools/alloc_bound_sim.py).
// Rounding: the reference's total is a sequential sum of at most 52 non-negative doubles, so it is at least
// (1 - 51 * 2^-53) times the exact sum; our P = sum of minima and M = lambda B carry a few roundings each.  The bound
// handed on is (P - M) - 2^-44 (P + M): three orders of magnitude more slack than all of that, and still 1e-13 of the
// totals it is compared with.  A candidate is dropped only when this bound is strictly above a total that was really
// computed, i.e. when it cannot even tie (:116-129 keeps the earlier candidate on ties).
// =====================================================================================================
typedef _Float16 h2 __attribute__((ext_vector_type(2)));
__global__ __launch_bounds__(256) void k_alloc_bound(C1EncodeLaunch L) {
  __shared__ double biased_s[64];
  const C1DevEncOpts *O = L.opts;
  // index 0 = silent BFU: with a zero here every term of such a BFU below is zero by itself
  if (threadIdx.x < 64) biased_s[threadIdx.x] = threadIdx.x == 0 ? 0.0 : ((const __attribute__((address_space(4))) double *)O->biased)[threadIdx.x];
  __syncthreads();
  const float la_slope = O->la_slope, la_off = O->la_off;
  const int lane = threadIdx.x & 63;
  const uint32_t count = L.work_count[1];
  for (uint32_t pos0 = blockIdx.x * 256u; pos0 < count; pos0 += gridDim.x * 256u) {
    const uint32_t pos = pos0 + threadIdx.x;
    const bool live = pos < count;
    const int64_t unit = live ? (int64_t)L.sel_list[pos] : (int64_t)L.sel_list[0];
    uint32_t sf[13];
    load_sfi(L.side, unit, sf);
    uint8_t *base = L.cand + unit * kCandBytes;
    double *tot = reinterpret_cast<double *>(base);
    double *lb = reinterpret_cast<double *>(base + kCandLbOffset);
    const double t52 = tot[7];
    const double best = t52 == kAlive ? __builtin_huge_val() : t52;     // the 52-BFU candidate may be open too (k_alloc_first)
    // bracket of log2 lambda for the first candidate: from "every BFU at 16 bits" to "nothing coded"
    int smin = 64, smax = 0;
#pragma unroll
    for (int b = 0; b < 52; b++) {
      const int s = (sf[b >> 2] >> ((b & 3) * 8)) & 63;
      if (s != 0) { smin = s < smin ? s : smin; smax = s > smax ? s : smax; }
    }
    // The multiplier search needs no precision (every lambda gives a valid bound; a poor one only prunes less), so it
    // runs on packed halves: two BFUs per instruction, the spend accumulated by v_dot2_f32_f16.  The relaxed word
    // length floor(y) is replaced by its mean y - 1/2 (clamped to 2..16 bits, nothing below the point where two bits
    // stop paying); silent BFUs sit far below everything.
    h2 sp[26];
#pragma unroll
    for (int k = 0; k < 26; k++) {
      const int s0 = (sf[(2 * k) >> 2] >> (((2 * k) & 3) * 8)) & 63, s1 = (sf[(2 * k + 1) >> 2] >> (((2 * k + 1) & 3) * 8)) & 63;
      sp[k] = h2{s0 != 0 ? (_Float16)s0 : (_Float16)-1000.0f, s1 != 0 ? (_Float16)s1 : (_Float16)-1000.0f};
    }
    const h2 slope2 = h2{(_Float16)la_slope, (_Float16)la_slope};
    float x_prev = 0.0f;
    bool have_prev = false;
    int c_star = -1;
    double lb_star = __builtin_huge_val();
    for (int c = 0; c < 8; c++) {
      const bool mine = live && tot[c] == kAlive;
      if (__builtin_amdgcn_ballot_w64(mine) == 0) continue;
      const int n = bfu_amount(c);
      const int B = 212 * 8 - 40 - 10 * n;
      float lo = have_prev ? x_prev - 0.05f : __builtin_fmaf(la_slope, (float)smin, la_off) - 17.0f;
      float hi = have_prev ? x_prev + 3.15f : __builtin_fmaf(la_slope, (float)smax, la_off);
      const int iters = __builtin_amdgcn_ballot_w64(mine && !have_prev) != 0 ? 8 : 5;
      for (int it = 0; it < iters; it++) {
        const float x = 0.5f * (lo + hi);
        const _Float16 by = (_Float16)(la_off - x - 0.5f);
        const h2 base2 = h2{by, by};
        float used = 0.0f;
#pragma unroll
        for (int k = 0; k < 26; k++) {
          if (2 * k < n) {
            const h2 y = __builtin_elementwise_fma(sp[k], slope2, base2);                     // log2(biasedSF / lambda) - 1/2
            const h2 bits = __builtin_elementwise_min(__builtin_elementwise_max(y, h2{(_Float16)2.0f, (_Float16)2.0f}), h2{(_Float16)16.0f, (_Float16)16.0f});
            const h2 ramp = __builtin_elementwise_fma(y, h2{(_Float16)64.0f, (_Float16)64.0f}, h2{(_Float16)20.0f, (_Float16)20.0f});   // 0 below y = -0.31, 1 above -0.30
            const h2 on = __builtin_elementwise_min(__builtin_elementwise_max(ramp, h2{(_Float16)0.0f, (_Float16)0.0f}), h2{(_Float16)1.0f, (_Float16)1.0f});
            used = __builtin_amdgcn_fdot2(bits * on, h2{(_Float16)(float)kSpecsHost[2 * k], (_Float16)(float)kSpecsHost[2 * k + 1]}, used, false);
          }
        }
        if (used > (float)B) lo = x; else hi = x;
      }
      const float x = hi;
      const double lambda = (double)__builtin_amdgcn_exp2f(x);
      const double inv_lambda = 1.0 / lambda;
      double P = 0.0;
#pragma unroll
      for (int b = 0; b < 52; b++) {
        const int s = (sf[b >> 2] >> ((b & 3) * 8)) & 63;
        const double a = biased_s[s], size = (double)kSpecs[b];
        const double z = (double)f32(a * 2.0 * size);                 // zeroBitDistortions[b] (:87-89)
        double g = z;
        if (b < n) {
          const double q = a * inv_lambda;
          int e = ((__double2hiint(q) >> 20) & 0x7ff) - 1023;         // floor(log2 q) for normal q
          e = e < 2 ? 2 : (e > 16 ? 16 : e);
          const double ip2 = __hiloint2double((1023 - e) << 20, 0);
          const double h = a * ip2 * size + lambda * size * (double)e;   // (:183-187) + the price of e bits
          g = h < z ? h : z;
        }
        P += g;
      }
      const double M = lambda * (double)B;
      const double bound = (P - M) - 5.684341886080802e-14 * (P + M);
      if (mine) {
        if (bound > best) tot[c] = __builtin_huge_val();               // cannot win, cannot tie
        else {
          lb[c] = bound;
          if (bound < lb_star || c_star < 0) { lb_star = bound; c_star = c; }
        }
        x_prev = x; have_prev = true;
      }
    }
    // first round of heaps: the candidate with the smallest bound
    const bool has = live && c_star >= 0;
    const uint64_t m = __builtin_amdgcn_ballot_w64(has);
    uint32_t at = 0;
    if (lane == 0 && m != 0) at = atomicAdd(L.work_count, (uint32_t)__popcll(m));
    at = (uint32_t)__builtin_amdgcn_readfirstlane((int)at);
    if (has) L.work_list[at + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = ((uint32_t)unit << 3) | (uint32_t)c_star;
  }
}

// FIRST_ROUND: every entry is the most promising candidate of its unit (one entry per unit).  With its total known,
// the unit's other live candidates are settled on the spot: a bound above the best total known now (52 BFUs or this
// one) can never win, the rest is appended to the second round's list.
template <bool FIRST_ROUND>
__global__ __launch_bounds__(C1_WAVE, 3) void k_alloc_rest(C1EncodeLaunch L, const uint32_t *__restrict__ list, const uint32_t *__restrict__ list_count,
                                                           uint32_t *__restrict__ list2) {
  __shared__ uint32_t heap[kHeapRows * 64];
  const C1DevEncOpts *O = L.opts;
  const int lane = threadIdx.x;
  const uint32_t count = *list_count;
  for (uint32_t base = blockIdx.x * 64u; base < count; base += gridDim.x * 64u) {
    const uint32_t idx = base + lane;
    const bool live = idx < count;
    const uint32_t item = live ? list[idx] : 0u;
    const int64_t unit = item >> 3;
    const int c = item & 7;
    uint32_t sf[13];
    load_sfi(L.side, unit, sf);
    uint64_t r0, r1, r2, r3;
    double total;
    double unused[7];
    run_candidate<false>(heap + lane, bfu_amount(c), sf, O, live, r0, r1, r2, r3, total, unused);
    total = total < __builtin_huge_val() ? total : __builtin_huge_val();
    if (live) store_candidate(L.cand, unit, c, total, r0, r1, r2, r3);
    if constexpr (FIRST_ROUND) {
      uint8_t *cbase = L.cand + unit * kCandBytes;
      double *tot = reinterpret_cast<double *>(cbase);
      const double *lb = reinterpret_cast<const double *>(cbase + kCandLbOffset);
      uint32_t keep = 0;
      if (live) {
        const double t52 = tot[7];
        const double best = (c == 7 || t52 == kAlive || total < t52) ? total : t52;
#pragma unroll
        for (int k = 0; k < 8; k++) {
          if (k != c && tot[k] == kAlive) {
            if (lb[k] > best) tot[k] = __builtin_huge_val();
            else keep |= 1u << k;
          }
        }
      }
      const int mine = __popc(keep);
      const int scan = wave_inclusive_scan(mine);
      const int wave_total = __builtin_amdgcn_readlane(scan, 63);
      uint32_t at = 0;
      if (lane == 0 && wave_total > 0) at = atomicAdd(L.work_count + 2, (uint32_t)wave_total);
      at = (uint32_t)__builtin_amdgcn_readfirstlane((int)at) + (uint32_t)(scan - mine);
      for (int k = 0; k < 8; k++)
        if ((keep >> k) & 1u) list2[at++] = ((uint32_t)unit << 3) | (uint32_t)k;
    }
  }
}

// the units on the selection list (those with more than one candidate alive): smallest total, smallest count on ties
__global__ __launch_bounds__(256) void k_alloc_select(C1EncodeLaunch L) {
  const int64_t count = (int64_t)L.work_count[1];
  for (int64_t pos = (int64_t)blockIdx.x * 256 + threadIdx.x; pos < count; pos += (int64_t)gridDim.x * 256) {
  const int64_t unit = (int64_t)L.sel_list[pos];
  const uint8_t *base = L.cand + unit * kCandBytes;
  const double *tot = reinterpret_cast<const double *>(base);
  double best = __builtin_huge_val();
  int best_c = 8;
#pragma unroll
  for (int c = 0; c < 8; c++) {            // ascending count, strict `<`: the smallest count wins ties (:116-129)
    const double t = tot[c];
    if (t < best) { best = t; best_c = c; }
  }
  uint64_t *dst = reinterpret_cast<uint64_t *>(L.alloc + unit * kAllocBytes);
  if (best_c < 8) {
    const uint64_t *src = reinterpret_cast<const uint64_t *>(base + 64 + best_c * 32);
    dst[0] = src[0]; dst[1] = src[1]; dst[2] = src[2];
    dst[3] = src[3] | ((uint64_t)best_c << 60);
  } else {
    dst[0] = 0; dst[1] = 0; dst[2] = 0;
    dst[3] = 1ull << 59;                   // fallback (:132-139): 20 BFUs, all indices zero
  }
  }
}

// ---- test tap: every candidate's total next to its lower bound (c1_alloc_bounds_device) -------------------------------
__global__ __launch_bounds__(256) void k_alloc_tap_init(C1EncodeLaunch L, int64_t units) {
  const int64_t unit = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (unit == 0) { L.work_count[0] = 0; L.work_count[1] = (uint32_t)units; L.work_count[2] = (uint32_t)(units * 8); }
  if (unit >= units) return;
  double *tot = reinterpret_cast<double *>(L.cand + unit * kCandBytes);
  for (int c = 0; c < 7; c++) tot[c] = kAlive;            // everything alive, nothing known: the bound kernel drops nothing
  tot[7] = __builtin_huge_val();
  L.sel_list[unit] = (uint32_t)unit;
  for (int c = 0; c < 8; c++) L.work_list[units + unit * 8 + c] = ((uint32_t)unit << 3) | (uint32_t)c;
}
__global__ __launch_bounds__(256) void k_alloc_tap_gather(C1EncodeLaunch L, int64_t units, double *out) {
  const int64_t unit = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (unit >= units) return;
  const double *tot = reinterpret_cast<const double *>(L.cand + unit * kCandBytes);
  const double *lb = reinterpret_cast<const double *>(L.cand + unit * kCandBytes + kCandLbOffset);
  for (int c = 0; c < 8; c++) { out[unit * 16 + c] = tot[c]; out[unit * 16 + 8 + c] = c < 7 ? lb[c] : 0.0; }   // (slot 15 is overwritten below)
  // slot 15: what the production path (c1k_launch_allocate, run before the tap) chose: amount index, or -1 for the fallback
  const uint32_t a7 = reinterpret_cast<const uint32_t *>(L.alloc + unit * kAllocBytes)[7];
  out[unit * 16 + 15] = ((a7 >> 27) & 1u) ? -1.0 : (double)((a7 >> 28) & 7u);
}

}  // namespace

// out: units x 16 doubles: totals of the eight candidates (calculateTotalDistortion after distributeBitsRDO), then the
// seven lower bounds k_alloc_bound gives them, then the candidate the production path chose.  Needs a work list of
// 9 entries per unit.
void c1k_launch_alloc_tap(const C1EncodeLaunch &L, double *out, hipStream_t stream) {
  const int64_t units = L.frames * L.channels;
  c1k_launch_allocate(L, stream);                           // the pruned path, for slot 15
  const dim3 grid((unsigned)((units + 255) / 256)), block(256);
  hipLaunchKernelGGL(k_alloc_tap_init, grid, block, 0, stream, L, units);
  hipLaunchKernelGGL(k_alloc_bound, dim3((unsigned)std::min<int64_t>((units + 255) / 256, 2048)), block, 0, stream, L);
  hipLaunchKernelGGL((k_alloc_rest<false>), dim3((unsigned)std::min<int64_t>((units * 8 + 63) / 64, 256 * 10)), dim3(C1_WAVE), 0, stream, L,
                     (const uint32_t *)(L.work_list + units), (const uint32_t *)(L.work_count + 2), (uint32_t *)nullptr);
  hipLaunchKernelGGL(k_alloc_tap_gather, grid, block, 0, stream, L, units, out);
}

namespace {
}  // namespace

void c1k_launch_allocate(const C1EncodeLaunch &L, hipStream_t stream) {
  const int64_t units = L.frames * L.channels;
  const bool listed = L.unit_list != nullptr;            // the list's length is only known on the device: bounded grids stride over it
  (void)hipMemsetAsync(L.work_count, 0, 3 * sizeof(uint32_t), stream);
  const int64_t first_blocks = listed ? std::min<int64_t>((units + 63) / 64, 256 * 12) : (units + 63) / 64;
  hipLaunchKernelGGL(k_alloc_first, dim3((unsigned)first_blocks), dim3(C1_WAVE), 0, stream, L);
  // every kernel below strides over a list whose length only the device knows
  const int64_t unit_blocks = std::min<int64_t>((units + 255) / 256, 2048);
  uint32_t *list2 = L.work_list + units;                   // first round: at most one entry per unit
  hipLaunchKernelGGL(k_alloc_bound, dim3((unsigned)unit_blocks), dim3(256), 0, stream, L);
  const int64_t rest1_blocks = std::min<int64_t>((units + 63) / 64, 256 * 10);
  hipLaunchKernelGGL((k_alloc_rest<true>), dim3((unsigned)rest1_blocks), dim3(C1_WAVE), 0, stream, L, (const uint32_t *)L.work_list, (const uint32_t *)L.work_count, list2);
  const int64_t rest2_blocks = std::min<int64_t>((units * 6 + 63) / 64, 256 * 10);
  hipLaunchKernelGGL((k_alloc_rest<false>), dim3((unsigned)rest2_blocks), dim3(C1_WAVE), 0, stream, L, (const uint32_t *)list2, (const uint32_t *)(L.work_count + 2), (uint32_t *)nullptr);
  const int64_t select_blocks = std::min<int64_t>((units + 255) / 256, 1024);      // strides over the selection list
  hipLaunchKernelGGL(k_alloc_select, dim3((unsigned)select_blocks), dim3(256), 0, stream, L);
}
