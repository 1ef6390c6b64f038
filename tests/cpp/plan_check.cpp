// plan_check.cpp -- the block planner (smallz4_amd/csrc/sz4_plan.cpp) checked on the CPU against values
// written out by hand from the definitions: smallz4.h's block-end constants (no match starts in a block's
// last 12 bytes, its last 5 are literals), the 65535-byte window, and DESIGN section 4 (segments of 65536
// targets, parse segments of 4096 / 8192 positions, walk sub-segments of 4096, the shared work region).
// Stand-alone: links sz4_plan.cpp only, makes no HIP call, runs without a GPU (tests/test_plan_host.py
// builds it with the address and undefined-behaviour sanitizers).
//
//   plan_check          run the checks; exit status 1 and one line per failed check on a mismatch
//   plan_check --dump   print the plans of the same shapes (profiles/r08/plans_*.txt)
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../smallz4_amd/csrc/sz4_plan.h"

using namespace sz4;

static int g_failed = 0;
static const char* g_plan = "";
#define CHECK(cond)                                                            \
  do {                                                                         \
    if (!(cond)) {                                                             \
      g_failed++;                                                              \
      printf("FAILED %s:%d [%s] %s\n", __FILE__, __LINE__, g_plan, #cond);     \
    }                                                                          \
  } while (0)

static const uint64_t L = 3 * 65536 + 17;
static const uint64_t kPadBytes = 64;  // the driver stages 64 bytes after the last block

// ---- what holds for every plan ---------------------------------------------------------------------
struct Span {
  uint64_t lo, hi;
};
static bool disjoint_inside(const std::vector<Span>& v, uint64_t size)
{
  for (size_t i = 0; i < v.size(); i++) {
    if (v[i].hi > size || v[i].lo > v[i].hi) return false;
    for (size_t j = i + 1; j < v.size(); j++)
      if (v[i].lo < v[j].hi && v[j].lo < v[i].hi) return false;
  }
  return true;
}

static void check_common(Plan& P, uint64_t staged)
{
  const uint64_t nb = P.blocks.size();
  uint64_t si = 0, elem = 0, rank = 0, tok = 0, walk = 0, dp = 0;
  uint32_t maxDp = 1;
  bool lds = true;
  for (uint64_t b = 0; b < nb; b++) {
    const Block& B = P.blocks[b];
    const uint64_t n = B.end - B.start;
    CHECK(B.end > B.start);
    // segments tile the targets [start, end - 11) in order, at most 65536 each
    uint64_t at = B.start;
    const uint64_t t1 = n >= 12 ? B.end - 11 : B.start;
    while (at < t1) {
      CHECK(si < P.segs.size());
      if (si >= P.segs.size()) return;
      const Segment& S = P.segs[si++];
      CHECK(S.block == b);
      CHECK(S.s0 == at);
      CHECK(S.s1 > S.s0 && S.s1 - S.s0 <= 65536 && S.s1 <= t1);
      CHECK(S.s1 == t1 || S.s1 - S.s0 == 65536);
      const uint64_t back = S.s0 >= 65535 ? S.s0 - 65535 : 0;
      CHECK(S.w0 == (back > B.low ? back : B.low));
      CHECK(S.elemOff == elem && S.rankOff == rank);
      elem += S.s1 - S.w0;
      rank += S.s1 - S.s0;
      if ((B.end - S.w0 + 11) / 4 * 4 > 65536 + 16) lds = false;
      at = S.s1;
    }
    // parse segments tile [0, n - 6] from the top down
    CHECK(B.dpFirst == dp);
    if (n <= 12) {
      CHECK(B.dpCount == 0);
    } else {
      CHECK(B.dpSize == (n <= 65536 ? 4096u : 8192u));
      CHECK(B.dpCount == (n - 5 + B.dpSize - 1) / B.dpSize);
      uint64_t hi = n - 6;
      for (uint32_t k = 0; k < B.dpCount && dp + k < P.dp.size(); k++) {
        const DpSeg& D = P.dp[dp + k];
        CHECK(D.block == b && D.k == k);
        CHECK(D.hi == hi);
        CHECK(D.lo <= D.hi && D.hi - D.lo < B.dpSize);
        CHECK(k + 1 == B.dpCount ? D.lo == 0 : D.hi - D.lo + 1 == B.dpSize);
        hi = (uint64_t)D.lo - 1;
      }
      if (B.dpCount > maxDp) maxDp = B.dpCount;
    }
    dp += B.dpCount;
    // walk sub-segments
    CHECK(B.walkFirst == walk);
    CHECK(B.walkCount == (n + 4095) / 4096);
    for (uint32_t k = 0; k < B.walkCount && walk + k < P.walk.size(); k++)
      CHECK(P.walk[walk + k].x == b && P.walk[walk + k].y == k);
    walk += B.walkCount;
    CHECK(B.tokOff == tok);
    tok += n / 2 + 4;
  }
  CHECK(si == P.segs.size());
  CHECK(dp == P.dp.size());
  CHECK(walk == P.walk.size());
  CHECK(P.elemTotal == elem && P.rankTotal == rank && P.tokTotal == tok);
  CHECK(P.maxDpCount == maxDp);
  CHECK(P.ldsWindow == lds);

  // the shared region: 256-aligned offsets, every stage's arrays inside it and apart from each other
  // (array sizes as PipeArgs in sz4_internal.h states them)
  const uint64_t size = P.work_layout(staged);
  const Plan::WorkOffsets& o = P.off;
  for (uint64_t x : {o.elemB, o.rmqUp, o.rmqDown, o.side, o.lazy, o.tok, o.walk}) CHECK(x % 256 == 0);
  const Span sel{0, staged * 4};
  const uint64_t rmq = (staged + nb + 8) * 4;
  CHECK(disjoint_inside({{0, elem * 8}, {o.elemB, o.elemB + elem * 8}}, size));
  CHECK(disjoint_inside({sel, {o.rmqUp, o.rmqUp + rmq}, {o.rmqDown, o.rmqDown + rmq}, {o.side, o.side + dp * 1280 * 8}}, size));
  CHECK(disjoint_inside({sel, {o.lazy, o.lazy + walk * 2800 * 4}}, size));
  CHECK(disjoint_inside({sel, {o.tok, o.tok + tok * 16}, {o.walk, o.walk + walk * 2 * 1026 * 4}}, size));
}

// ---- the plans ---------------------------------------------------------------------------------------
static void uniform_64k(Plan& P)
{
  g_plan = "uniform 64 KiB";
  P.build_uniform(L, 65536);
  CHECK(P.blocks.size() == 4 && P.segs.size() == 4);
  if (P.blocks.size() != 4 || P.segs.size() != 4) return;
  uint64_t tok = 0;
  for (uint32_t b = 0; b < 4; b++) {
    const Block& B = P.blocks[b];
    const Segment& S = P.segs[b];
    const uint64_t start = 65536ull * b, end = b < 3 ? start + 65536 : L;
    CHECK(B.start == start && B.end == end && B.low == start && B.cut == ~0ull && B.prev == 0xFFFFFFFFu && B.flags == 0);
    CHECK(S.block == b && S.s0 == start && S.s1 == end - 11 && S.w0 == start);
    CHECK(B.dpCount == (b < 3 ? 16u : 1u) && B.walkCount == (b < 3 ? 16u : 1u));
    CHECK(B.tokOff == tok);
    tok += (end - start) / 2 + 4;
  }
  CHECK(P.segs[3].s1 - P.segs[3].s0 == 6);
  // a full block: ceil((65536 - 5) / 4096) = 16 parse segments from 65530 down to 0
  CHECK(P.dp.size() == 49 && P.walk.size() == 49);
  CHECK(P.dp[0].hi == 65530 && P.dp[0].lo == 65530 - 4095 && P.dp[15].lo == 0 && P.dp[15].hi == 65530 - 15 * 4096);
  CHECK(P.dp[48].block == 3 && P.dp[48].lo == 0 && P.dp[48].hi == 11);
  CHECK(P.tokTotal == 3 * 32772 + 12);
  CHECK(P.elemTotal == 3 * 65525 + 6 && P.rankTotal == 3 * 65525 + 6);
  CHECK(P.ldsWindow);
  CHECK(P.maxDpCount == 16);
  check_common(P, L + kPadBytes);
}

static void uniform_11(Plan& P)
{
  g_plan = "uniform 11 B";
  // L = 17875 x 11: every block, the last one included, is shorter than 12 bytes
  P.build_uniform(L, 11);
  CHECK(P.blocks.size() == 17875);
  CHECK(P.segs.empty() && P.dp.empty() && P.walk.size() == 17875);
  for (size_t b = 0; b < P.blocks.size(); b++) {
    const Block& B = P.blocks[b];
    CHECK(B.end - B.start == 11 && B.dpCount == 0 && B.dpFirst == 0 && B.walkCount == 1 && B.walkFirst == b);
    CHECK(B.tokOff == 9 * b);
  }
  CHECK(!P.blocks.empty() && P.blocks.back().end == L);
  CHECK(P.elemTotal == 0 && P.rankTotal == 0 && P.maxDpCount == 1);
  check_common(P, L + kPadBytes);
}

static void one_large_block(Plan& P)
{
  g_plan = "one block of 128 KiB + 100";
  const uint64_t n = 2 * 65536 + 100;
  P.build_uniform(n, (uint32_t)n);
  CHECK(P.blocks.size() == 1 && P.segs.size() == 3);
  if (P.blocks.size() != 1 || P.segs.size() != 3) return;
  CHECK(P.segs[0].s0 == 0 && P.segs[0].s1 == 65536 && P.segs[0].w0 == 0);
  CHECK(P.segs[1].s0 == 65536 && P.segs[1].s1 == 131072 && P.segs[1].w0 == 65536 - 65535);
  CHECK(P.segs[2].s0 == 131072 && P.segs[2].s1 == n - 11 && P.segs[2].w0 == 131072 - 65535);
  // the lookback is counted once per segment that shares it
  CHECK(P.elemTotal == 65536 + (65536 + 65535) + (n - 11 - 131072 + 65535));
  CHECK(P.rankTotal == n - 11);
  CHECK(P.blocks[0].dpSize == 8192 && P.blocks[0].dpCount == 17 && P.blocks[0].walkCount == 33);
  CHECK(!P.ldsWindow);
  check_common(P, n + kPadBytes);
}

static void stream_plans(Plan& P)
{
  const uint64_t pre = 65536 + 777, n = (4ull << 20) + 5, start = pre, mid = pre + (4ull << 20);
  g_plan = "stream chunk, continued";
  P.build_stream(pre, n, false, 0, false);
  CHECK(P.blocks.size() == 2);
  if (P.blocks.size() != 2) return;
  CHECK(P.blocks[0].start == start && P.blocks[0].end == mid && P.blocks[1].start == mid && P.blocks[1].end == pre + n);
  CHECK(P.blocks[0].prev == 2);  // the ghost slot: the previous chunk's last block
  CHECK(P.blocks[0].low == start - 65535 && P.blocks[0].cut == start - 12 && P.blocks[0].flags == 0);
  CHECK(P.blocks[1].prev == 0 && P.blocks[1].low == mid - 65535 && P.blocks[1].cut == mid - 12);
  CHECK(P.segs.size() == 64 && P.segs[0].w0 == start - 65535 && P.segs[63].s1 == mid - 11);
  CHECK(P.blocks[1].dpCount == 0 && P.blocks[1].walkCount == 1);
  CHECK(P.blocks[0].dpSize == 8192 && P.blocks[0].dpCount == 512 && !P.ldsWindow);
  check_common(P, pre + n + kPadBytes);

  g_plan = "stream chunk, first";
  // the stream's first block sees nothing before it; the next one still sees its 64 KiB (smallz4.h:572-585)
  P.build_stream(pre, n, true, 0, false);
  CHECK(P.blocks.size() == 2);
  if (P.blocks.size() != 2) return;
  CHECK(P.blocks[0].low == start && P.blocks[0].cut == ~0ull && P.blocks[0].prev == 0xFFFFFFFFu && P.blocks[0].flags == 0);
  CHECK(P.blocks[1].prev == 0 && P.blocks[1].low == mid - 65535 && P.blocks[1].cut == mid - 12);
  CHECK(P.segs[0].w0 == start);
  check_common(P, pre + n + kPadBytes);

  g_plan = "stream chunk, legacy";
  // legacy blocks hold 8 MiB and are independent
  P.build_stream(pre, n, false, 1, false);
  CHECK(P.blocks.size() == 1);
  if (P.blocks.size() != 1) return;
  CHECK(P.blocks[0].start == start && P.blocks[0].end == pre + n);
  CHECK(P.blocks[0].low == start && P.blocks[0].cut == ~0ull && P.blocks[0].prev == 0xFFFFFFFFu);
  CHECK(P.blocks[0].flags == kBlkLegacy && kBlkLegacy == 1);
  CHECK(P.segs.size() == 64 && P.segs[0].w0 == start && P.segs[1].w0 == P.segs[1].s0 - 65535);
  check_common(P, pre + n + kPadBytes);
}

static void ragged_plans(Plan& P)
{
  g_plan = "ragged, five items";
  const std::vector<uint64_t> sizes = {1, 200, 5000, 70000, 66000};
  const uint64_t starts[5] = {0, 64, 320, 320 + 5056, 320 + 5056 + 70016};
  const uint64_t end = P.build_ragged(sizes);
  CHECK(end == starts[4] + 66048);
  CHECK(P.blocks.size() == 5);
  if (P.blocks.size() != 5) return;
  uint64_t top = 0;
  for (uint32_t b = 0; b < 5; b++) {
    const Block& B = P.blocks[b];
    CHECK(B.start == starts[b] && B.start % 64 == 0 && B.end == B.start + sizes[b]);
    CHECK(b == 0 || B.start > P.blocks[b - 1].start);
    CHECK(B.low == B.start && B.cut == ~0ull && B.prev == 0xFFFFFFFFu && B.flags == 0);
    if (B.end > top) top = B.end;
  }
  CHECK(P.blocks[4].end == top);
  CHECK(P.blocks[0].dpCount == 0 && P.blocks[0].walkCount == 1);  // 1 byte: nothing to search or parse
  CHECK(P.segs.size() == 6);  // 1 B: none, 200 B: 1, 5000 B: 1, 70000 B: 2, 66000 B: 2 (65989 targets)
  CHECK(!P.ldsWindow);  // the 70000-byte item's window does not fit 64 KiB + 16
  check_common(P, end + kPadBytes);

  g_plan = "ragged, small items";
  const uint64_t end3 = P.build_ragged({1, 200, 5000});
  CHECK(end3 == 320 + 5056 && P.blocks.size() == 3);
  CHECK(P.ldsWindow);
  check_common(P, end3 + kPadBytes);
}

// one entry, one key: an equal key keeps the plan (same version), any other key builds it again
static void cache_key(Plan& P)
{
  g_plan = "cache key";
  auto rebuilt = [&](uint64_t& v) {
    const bool r = P.version != v;
    v = P.version;
    return r;
  };
  uint64_t v = P.version;
  P.build_uniform(L, 65536);
  CHECK(rebuilt(v));
  P.build_uniform(L, 65536);
  CHECK(!rebuilt(v));
  P.build_uniform(L + 1, 65536);
  CHECK(rebuilt(v));
  P.build_uniform(L + 1, 32768);
  CHECK(rebuilt(v));
  P.build_uniform(L, 65536);
  CHECK(rebuilt(v) && P.blocks.size() == 4);
  // a ragged build never hits, not even itself, and the uniform key it displaced builds again
  P.build_ragged({65536, 65536, 65536, 17});
  CHECK(rebuilt(v));
  P.build_ragged({65536, 65536, 65536, 17});
  CHECK(rebuilt(v));
  const PlanKey rk{PlanKey::kRagged};
  CHECK(!(rk == rk) && !(PlanKey{} == PlanKey{}));
  P.build_uniform(L, 65536);
  CHECK(rebuilt(v) && P.blocks.size() == 4 && P.blocks[1].start == 65536);
  // stream: every parameter on its own
  P.build_stream(0, L, true, 0, false);
  CHECK(rebuilt(v));
  P.build_stream(0, L, true, 0, false);
  CHECK(!rebuilt(v));
  P.build_stream(65535, L, true, 0, false);
  CHECK(rebuilt(v));
  P.build_stream(65535, L + 1, true, 0, false);
  CHECK(rebuilt(v));
  P.build_stream(65535, L + 1, false, 0, false);
  CHECK(rebuilt(v));
  P.build_stream(65535, L + 1, false, 1, false);
  CHECK(rebuilt(v));
  P.build_stream(65535, L + 1, false, 1, true);
  CHECK(rebuilt(v));
  P.build_stream(65535, L + 1, false, 1, true);
  CHECK(!rebuilt(v));
  // a uniform plan of L bytes in 64 KiB blocks and a stream chunk of n = L do not hit each other
  P.build_uniform(L, 65536);
  CHECK(rebuilt(v) && P.blocks.size() == 4);
  P.build_stream(0, L, true, 0, false);
  CHECK(rebuilt(v) && P.blocks.size() == 1);
  P.build_stream(L, 65536, false, 0, false);
  CHECK(rebuilt(v));
  P.build_uniform(L, 65536);
  CHECK(rebuilt(v) && P.blocks.size() == 4);
  P.build_uniform(L, 65536);
  CHECK(!rebuilt(v));
}

// ---- --dump --------------------------------------------------------------------------------------------
// every array in full up to 600 entries; a longer one as its first and last 8 entries and a hash of all
static uint64_t fnv(const void* p, size_t n)
{
  uint64_t h = 1469598103934665603ull;
  for (size_t i = 0; i < n; i++) h = (h ^ static_cast<const uint8_t*>(p)[i]) * 1099511628211ull;
  return h;
}
template <class T, class F>
static void dump_array(const char* what, const std::vector<T>& v, F line)
{
  printf("%s %zu fnv %016llx\n", what, v.size(), (unsigned long long)fnv(v.data(), v.size() * sizeof(T)));
  for (size_t i = 0; i < v.size(); i++)
    if (v.size() <= 600 || i < 8 || i + 8 >= v.size()) {
      printf("  %s[%zu] ", what, i);
      line(v[i]);
    }
}
#define U(x) (unsigned long long)(x)
static void dump(const char* name, Plan& P, uint64_t staged)
{
  const uint64_t size = P.work_layout(staged);
  printf("== %s (staged %llu)\n", name, U(staged));
  dump_array("block", P.blocks, [](const Block& B) {
    printf("[%llu,%llu) low %llu cut %llu tokOff %llu prev %u flags %u dp %u+%u walk %u+%u dpSize %u\n", U(B.start), U(B.end),
           U(B.low), U(B.cut), U(B.tokOff), B.prev, B.flags, B.dpFirst, B.dpCount, B.walkFirst, B.walkCount, B.dpSize);
  });
  dump_array("seg", P.segs, [](const Segment& S) {
    printf("w0 %llu s0 %llu s1 %llu elemOff %llu rankOff %llu block %u\n", U(S.w0), U(S.s0), U(S.s1), U(S.elemOff), U(S.rankOff),
           S.block);
  });
  dump_array("dp", P.dp, [](const DpSeg& D) { printf("block %u k %u [%u,%u]\n", D.block, D.k, D.lo, D.hi); });
  dump_array("walk", P.walk, [](const uint2& W) { printf("block %u k %u\n", W.x, W.y); });
  printf("totals elem %llu rank %llu tok %llu ldsWindow %d maxDpCount %u\n", U(P.elemTotal), U(P.rankTotal), U(P.tokTotal),
         (int)P.ldsWindow, P.maxDpCount);
  printf("work elemB %llu rmqUp %llu rmqDown %llu side %llu lazy %llu tok %llu walk %llu size %llu\n", U(P.off.elemB),
         U(P.off.rmqUp), U(P.off.rmqDown), U(P.off.side), U(P.off.lazy), U(P.off.tok), U(P.off.walk), U(size));
}

static int dump_all()
{
  Plan P;
  const uint64_t big = 2 * 65536 + 100, pre = 65536 + 777, n = (4ull << 20) + 5;
  P.build_uniform(L, 65536);
  dump("uniform L 65536", P, L + kPadBytes);
  P.build_uniform(L, 11);
  dump("uniform L 11", P, L + kPadBytes);
  P.build_uniform(big, (uint32_t)big);
  dump("uniform one block", P, big + kPadBytes);
  P.build_stream(pre, n, false, 0, false);
  dump("stream continued", P, pre + n + kPadBytes);
  P.build_stream(pre, n, true, 0, false);
  dump("stream first", P, pre + n + kPadBytes);
  P.build_stream(pre, n, false, 1, false);
  dump("stream legacy", P, pre + n + kPadBytes);
  uint64_t end = P.build_ragged({1, 200, 5000, 70000, 66000});
  dump("ragged five", P, end + kPadBytes);
  end = P.build_ragged({1, 200, 5000});
  dump("ragged small", P, end + kPadBytes);
  return 0;
}

int main(int argc, char** argv)
{
  if (argc > 1 && strcmp(argv[1], "--dump") == 0) return dump_all();
  // one Plan through every shape, as a context keeps one
  Plan P;
  uniform_64k(P);
  uniform_11(P);
  one_large_block(P);
  stream_plans(P);
  ragged_plans(P);
  cache_key(P);
  if (g_failed) {
    printf("plan_check: %d checks failed\n", g_failed);
    return 1;
  }
  printf("plan_check ok\n");
  return 0;
}
