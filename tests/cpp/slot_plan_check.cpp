// slot_plan_check.cpp -- the slot plan of a sized compress queue (smallz4_amd/csrc/sz4_slot_plan.h,
// Plan::build_slots) checked on the CPU against the planner itself: for a slot of capacity cap and every size
// n <= cap of a list that sweeps the plan's edges, the entries the shared header derives for (slot, n) are
// Plan::build_ragged({n})'s entries moved to the slot's offsets, every other reserved entry is inert, and
// nothing a size needs exceeds what the capacity reserved.  Stand-alone: links sz4_plan.cpp only, makes no
// HIP call, runs without a GPU (tests/test_slot_plan_host.py builds it with the address and
// undefined-behaviour sanitizers).  Exit status 1 and one line per failed check on a mismatch.
#include <stdio.h>

#include <vector>

#include "../../smallz4_amd/csrc/sz4_plan.h"

using namespace sz4;

static int g_failed = 0;
static uint64_t g_cap = 0, g_n = 0;
#define CHECK(cond)                                                                                     \
  do {                                                                                                  \
    if (!(cond)) {                                                                                      \
      if (g_failed++ < 50)                                                                              \
        printf("FAILED %s:%d [cap %llu n %llu] %s\n", __FILE__, __LINE__, (unsigned long long)g_cap,    \
               (unsigned long long)g_n, #cond);                                                         \
    }                                                                                                   \
  } while (0)

static const uint64_t kPadBytes = 64;  // the driver stages 64 bytes after the last block
static const uint32_t kCaps[] = {0, 1, 11, 12, 13, 4096, 4102, 65536, 65537, 65541, 65548, 70000, 131083, 4u << 20};

static std::vector<uint64_t> sizes_for(uint64_t cap)
{
  const uint64_t list[] = {0,     1,     11,    12,    13,    4095,  4096,  4097,  4101, 4102,
                           65535, 65536, 65537, 65541, 65542, 65547, 65548, cap - 1, cap};
  std::vector<uint64_t> v;
  for (uint64_t n : list) {
    if (n > cap || (cap == 0 && n != 0)) continue;  // (cap - 1 wraps for cap 0)
    bool seen = false;
    for (uint64_t x : v) seen |= x == n;
    if (!seen) v.push_back(n);
  }
  return v;
}

static bool same_block(const Block& a, const Block& b)
{
  return a.start == b.start && a.end == b.end && a.low == b.low && a.cut == b.cut && a.tokOff == b.tokOff &&
         a.prev == b.prev && a.flags == b.flags && a.dpFirst == b.dpFirst && a.dpCount == b.dpCount &&
         a.walkFirst == b.walkFirst && a.walkCount == b.walkCount && a.dpSize == b.dpSize;
}

// slot `bi` of the plan SP at size n against the planner's one-block plan of n bytes
static void check_pair(const Plan& SP, uint32_t bi, uint64_t n)
{
  const Slot& s = SP.slots[bi];
  g_cap = s.cap, g_n = n;
  const Block B = slot_block(s, n);
  Plan R;
  if (n) R.build_ragged({n});
  const uint32_t nseg = n ? (uint32_t)R.segs.size() : 0, ndp = n ? (uint32_t)R.dp.size() : 0,
                 nwalk = n ? (uint32_t)R.walk.size() : 0;
  // nothing the size needs exceeds the reservation
  CHECK(nseg <= s.segCount && ndp <= s.dpCount && nwalk <= s.walkCount);
  CHECK(n <= s.cap);
  if (n) {
    CHECK(R.tokTotal <= token_capacity(s.cap));
    CHECK(R.elemTotal <= slot_elem_reserve(s.cap) && R.rankTotal <= slot_rank_reserve(s.cap));
    CHECK(R.maxDpCount <= SP.maxDpCount);
    Block E = R.blocks[0];
    E.start += s.start, E.end += s.start, E.low += s.start;
    E.tokOff = s.tokOff, E.dpFirst = s.dpFirst, E.walkFirst = s.walkFirst;
    CHECK(same_block(B, E));
    CHECK(B.start != B.end);
  } else {
    CHECK(B.start == B.end && B.start == s.start && B.dpCount == 0 && B.walkCount == 0);  // inert
    CHECK(B.tokOff == s.tokOff && B.dpFirst == s.dpFirst && B.walkFirst == s.walkFirst);
  }
  CHECK(B.dpCount == ndp && B.walkCount == nwalk);
  for (uint32_t j = 0; j < s.segCount; j++) {
    const Segment S = slot_segment(s, bi, j, n);
    CHECK(S.block == bi);
    CHECK(S.elemOff == SP.segs[s.segFirst + j].elemOff && S.rankOff == SP.segs[s.segFirst + j].rankOff);  // never move
    if (j < nseg) {
      const Segment& E = R.segs[j];
      CHECK(S.w0 == E.w0 + s.start && S.s0 == E.s0 + s.start && S.s1 == E.s1 + s.start);
      CHECK(S.elemOff == E.elemOff + s.elemOff && S.rankOff == E.rankOff + s.rankOff);
      CHECK(S.s0 < S.s1);
      // the segment's scratch stays inside the slot's reservation
      CHECK(S.elemOff + (S.s1 - S.w0) <= s.elemOff + slot_elem_reserve(s.cap));
      CHECK(S.rankOff + (S.s1 - S.s0) <= s.rankOff + slot_rank_reserve(s.cap));
    } else {
      CHECK(S.s0 == S.s1);  // inert
    }
  }
  for (uint32_t k = 0; k < s.dpCount; k++) {
    const DpSeg G = slot_dp(bi, k, n);
    CHECK(G.block == bi && G.k == k);
    if (k < ndp) {
      const DpSeg& E = R.dp[k];
      CHECK(G.lo == E.lo && G.hi == E.hi && E.k == k);
    } else {
      CHECK(G.k >= B.dpCount);  // inert
    }
  }
  for (uint32_t j = 0; j < s.walkCount; j++) {
    const uint2 w = SP.walk[s.walkFirst + j];  // walk entries never change
    CHECK(w.x == bi && w.y == j);
    if (j < nwalk) CHECK(R.walk[j].y == j);
    else CHECK(w.y >= B.walkCount);  // inert
  }
}

int main()
{
  // 1. all the capacities as the slots of one queue
  Plan SP;
  std::vector<uint32_t> caps(kCaps, kCaps + sizeof(kCaps) / sizeof(kCaps[0]));
  const uint64_t staged = SP.build_slots(caps);
  CHECK(SP.slots.size() == caps.size() && SP.blocks.size() == caps.size());
  uint64_t at = 0, tok = 0, elem = 0, rank = 0;
  uint32_t seg = 0, dp = 0, walk = 0, maxDp = 1;
  for (uint32_t i = 0; i < caps.size(); i++) {
    const Slot& s = SP.slots[i];
    g_cap = caps[i], g_n = 0;
    CHECK(s.cap == caps[i] && s.start == at && s.start % kBatchAlign == 0);
    CHECK(s.tokOff == tok && s.elemOff == elem && s.rankOff == rank);
    CHECK(s.segFirst == seg && s.dpFirst == dp && s.walkFirst == walk);
    at += batch_stride(caps[i]);
    tok += token_capacity(caps[i]);
    elem += slot_elem_reserve(caps[i]);
    rank += slot_rank_reserve(caps[i]);
    seg += s.segCount, dp += s.dpCount, walk += s.walkCount;
    maxDp = s.dpCount > maxDp ? s.dpCount : maxDp;
    // the plan as built holds the entries of size == cap
    CHECK(same_block(SP.blocks[i], slot_block(s, caps[i])));
    for (uint64_t n : sizes_for(caps[i])) check_pair(SP, i, n);
  }
  g_cap = g_n = 0;
  CHECK(staged == at && SP.tokTotal == tok && SP.elemTotal == elem && SP.rankTotal == rank);
  CHECK(SP.segs.size() == seg && SP.dp.size() == dp && SP.walk.size() == walk && SP.maxDpCount == maxDp);
  CHECK(!SP.ldsWindow);

  // 2. the trap: parse segments do not grow with the size.  A 70000-byte slot reserves 16
  {
    Plan P;
    P.build_slots({70000});
    const Slot& s = P.slots[0];
    g_cap = 70000;
    CHECK(slot_dp_count(70000) == 9 && s.dpCount == 16 && P.dp.size() == 16 && P.maxDpCount == 16);
    CHECK(slot_block(s, 65536).dpCount == 16 && slot_block(s, 65536).dpSize == 4096);
    CHECK(slot_block(s, 65537).dpCount == 8 && slot_block(s, 65537).dpSize == 8192);
    CHECK(s.segCount == 2 && slot_seg_count(65547) == 1 && slot_seg_count(65548) == 2);
    // entries 9 .. 15 of the plan as built (size == cap) are inert
    for (uint32_t k = 0; k < 16; k++) CHECK((P.dp[k].k >= P.blocks[0].dpCount) == (k >= 9));
    CHECK(!P.ldsWindow);
    Plan Q;
    Q.build_slots({65541, 65536, 0});
    CHECK(Q.ldsWindow && Q.maxDpCount == 16);
    // around the finders' LDS (65552 bytes for the block and 8 more, in whole words): as the planner decides
    for (uint32_t cap = 65540; cap <= 65548; cap++) {
      Plan R;
      R.build_ragged({cap});
      Q.build_slots({65536, cap, 12});
      g_cap = cap;
      CHECK(Q.ldsWindow == R.ldsWindow);
      CHECK(Q.ldsWindow == (cap <= 65544));
    }
  }

  // 3. the scratch laid out for a capacity holds every smaller plan
  for (uint32_t cap : caps) {
    if (!cap) continue;
    Plan P;
    const uint64_t st = P.build_slots({cap}) + kPadBytes;
    const uint64_t W = P.work_layout(st);
    for (uint64_t n : sizes_for(cap)) {
      if (!n) continue;
      g_cap = cap, g_n = n;
      Plan R;
      const uint64_t rs = R.build_ragged({n}) + kPadBytes;
      CHECK(R.work_layout(rs) <= W && rs <= st);
      CHECK(R.ldsWindow || !P.ldsWindow);  // a queue that runs the LDS finders never holds a size that does not fit
      CHECK(R.segs.size() <= P.segs.size() && R.dp.size() <= P.dp.size() && R.walk.size() <= P.walk.size());
      CHECK(R.elemTotal <= P.elemTotal && R.rankTotal <= P.rankTotal && R.tokTotal <= P.tokTotal);
      if (n == cap) CHECK(R.elemTotal == P.elemTotal && R.rankTotal == P.rankTotal && R.tokTotal == P.tokTotal);
    }
  }

  if (g_failed) {
    printf("slot_plan_check: %d checks failed\n", g_failed);
    return 1;
  }
  printf("slot_plan_check ok\n");
  return 0;
}
