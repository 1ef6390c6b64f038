// sz4_slot_plan.h -- the plan of one SLOT of a sized compress queue (sz4_cq_create_sized), as host and device
// compute it.  A slot is the fixed place of caller item i: its staged bytes start at the running sum of the
// capacities' strides, and its share of every plan table (Segment, DpSeg, walk entry, Token slot, sort
// element, rank) is reserved for the LARGEST need of any size n <= cap.  The functions below turn (slot, n)
// into the slot's Block and its table entries: the arithmetic of Plan::add_segments / Plan::finish_plan
// (sz4_plan.cpp) for a one-block plan of n bytes at the slot's start, with the slot's static offsets.  The
// host builds the capacity plan with them (Plan::build_slots), k_cq_plan (sz4_batch.hip) rewrites the
// entries for the sizes of an enqueue, and tests/cpp/slot_plan_check.cpp compares them with build_ragged.
//
// Entries a smaller n does not need are INERT, and every kernel that takes an entry returns on one:
//   Segment   s0 == s1                         (a live segment has at least one target)
//   DpSeg     k >= its block's dpCount         (block and k of an entry never change)
//   walk      index >= its block's walkCount   (walk entries never change at all)
//   Block     start == end                     (the slot is empty at this enqueue)
// No other builder of Plan produces such an entry.
// SZ4_DP_SIZE (sz4_plan.cpp) does not apply here: the device cannot read the environment.
#pragma once
#include "sz4_internal.h"

#ifdef __HIP__
#define SZ4_SLOT_HD __host__ __device__
#else
#define SZ4_SLOT_HD
#endif

namespace sz4 {

struct Slot {
  uint64_t start;      // first staged byte (a multiple of kBatchAlign)
  uint64_t tokOff;     // first Token slot (token_capacity(cap) of them: the token walk's match records)
  uint64_t elemOff;    // first sort element
  uint64_t rankOff;    // first rank entry
  uint32_t cap;        // the largest size an enqueue may give the item
  uint32_t elem;       // the item's element width
  uint32_t segFirst, segCount;    // reserved entries of each table
  uint32_t dpFirst, dpCount;
  uint32_t walkFirst, walkCount;
};

// ---- counts for a block of n bytes ------------------------------------------------------------------------
SZ4_SLOT_HD inline uint32_t slot_seg_count(uint64_t n)
{
  // targets [0, n - 11) in segments of 65536 (kSegTargets)
  return n < (uint64_t)kTailNoMatch ? 0u : (uint32_t)((n - kTailNoMatch + 1 + 65535) / 65536);
}
SZ4_SLOT_HD inline uint32_t slot_dp_size(uint64_t n) { return n <= 65536 ? 4096u : 8192u; }  // dp_segment_size
SZ4_SLOT_HD inline uint32_t slot_dp_count(uint64_t n)
{
  // positions [0, n - 6] of a block longer than 12 bytes
  if (n <= (uint64_t)kTailNoMatch) return 0u;
  const uint64_t seg = slot_dp_size(n);
  return (uint32_t)((n - kTailLiterals + seg - 1) / seg);
}
SZ4_SLOT_HD inline uint32_t slot_walk_count(uint64_t n) { return (uint32_t)((n + kWalkSeg - 1) / kWalkSeg); }

// ---- what a slot of capacity cap reserves: the largest count any n <= cap needs -----------------------------
// Segments, walk sub-segments, Token slots and sort elements grow with n.  Parse segments do not: their
// size doubles above 65536 bytes, so a 65536-byte block has 16 of them and a 65537-byte block 8.
SZ4_SLOT_HD inline uint32_t slot_dp_reserve(uint64_t cap)
{
  const uint32_t c = slot_dp_count(cap);
  return cap > 65536 && c < 16u ? 16u : c;
}
// sort elements (window positions) and rank entries (targets) of the first j segments of a block that has
// more than j of them: all j are full, the first with a window of its own 65536 targets, the others with
// kWindow positions more
SZ4_SLOT_HD inline uint64_t slot_elems_before(uint32_t j) { return j ? 65536ull + (uint64_t)(j - 1) * (65536ull + kWindow) : 0ull; }
SZ4_SLOT_HD inline uint64_t slot_ranks_before(uint32_t j) { return (uint64_t)j * 65536ull; }
SZ4_SLOT_HD inline uint64_t slot_elem_reserve(uint64_t cap)
{
  const uint32_t c = slot_seg_count(cap);
  if (!c) return 0;
  const uint64_t s0 = (uint64_t)(c - 1) * 65536ull, t1 = cap - kTailNoMatch + 1;  // the last segment, block-relative
  return slot_elems_before(c - 1) + (t1 - (s0 >= kWindow ? s0 - kWindow : 0));
}
SZ4_SLOT_HD inline uint64_t slot_rank_reserve(uint64_t cap) { return cap < (uint64_t)kTailNoMatch ? 0 : cap - kTailNoMatch + 1; }

// ---- the entries of slot `bi` (the slot's index is its block's) for n bytes ---------------------------------
SZ4_SLOT_HD inline Block slot_block(const Slot& s, uint64_t n)
{
  Block B{};
  B.start = s.start;
  B.end = s.start + n;
  B.low = s.start;
  B.cut = kNone;
  B.tokOff = s.tokOff;
  B.prev = kNoBlock;
  B.flags = 0;
  B.dpFirst = s.dpFirst;
  B.dpCount = slot_dp_count(n);
  B.walkFirst = s.walkFirst;
  B.walkCount = slot_walk_count(n);
  B.dpSize = B.dpCount ? slot_dp_size(n) : 0u;
  B.pad = 0;
  return B;
}
// segment j < s.segCount
SZ4_SLOT_HD inline Segment slot_segment(const Slot& s, uint32_t bi, uint32_t j, uint64_t n)
{
  Segment S{};
  S.block = bi;
  S.elemOff = s.elemOff + slot_elems_before(j);
  S.rankOff = s.rankOff + slot_ranks_before(j);
  S.w0 = S.s0 = S.s1 = s.start;  // inert
  if (j < slot_seg_count(n)) {
    const uint64_t t1 = s.start + n - kTailNoMatch + 1;
    const uint64_t s0 = s.start + (uint64_t)j * 65536ull, e = s0 + 65536ull;
    const uint64_t back = s0 >= kWindow ? s0 - kWindow : 0;
    S.s0 = s0;
    S.s1 = e < t1 ? e : t1;
    S.w0 = back > s.start ? back : s.start;
  }
  return S;
}
// parse segment k < s.dpCount (k = 0 holds the block's last parsed position)
SZ4_SLOT_HD inline DpSeg slot_dp(uint32_t bi, uint32_t k, uint64_t n)
{
  DpSeg G{bi, k, 0u, 0u};  // inert when k >= slot_dp_count(n)
  if (k < slot_dp_count(n)) {
    const uint64_t seg = slot_dp_size(n), hi = n - 1 - kTailLiterals - (uint64_t)k * seg;
    G.hi = (uint32_t)hi;
    G.lo = (uint32_t)(hi + 1 >= seg ? hi + 1 - seg : 0);
  }
  return G;
}

}  // namespace sz4
