// sz4_plan.cpp -- builds the block / segment / parse-segment / walk plan of a pipeline run (sz4_plan.h).
#include "sz4_plan.h"

#include <stdlib.h>

#include <algorithm>

namespace sz4 {

Block independent_block(uint64_t start, uint64_t end, uint32_t flags)
{
  Block B{};
  B.start = start;
  B.end = end;
  B.low = start;
  B.cut = kNone;
  B.prev = kNoBlock;
  B.flags = flags;
  return B;
}

// the plan is rebuilt: empty, and without a key until finish_plan has completed it
bool Plan::begin(const PlanKey& k)
{
  if (k == key) return false;
  key = PlanKey{};
  blocks.clear();
  slots.clear();
  return true;
}

// Targets of block B are positions [start, end - 11) (smallz4.h:629); the window of a segment
// reaches back 64 KiB - 1 but never below the block's lowest visible byte.
void Plan::add_segments(uint32_t bi)
{
  const Block& B = blocks[bi];
  if (B.end - B.start < (uint64_t)kTailNoMatch) return;
  const uint64_t t1 = B.end - kTailNoMatch + 1;
  for (uint64_t s0 = B.start; s0 < t1; s0 += kSegTargets) {
    Segment S{};
    S.s0 = s0;
    S.s1 = std::min(s0 + kSegTargets, t1);
    S.w0 = std::max(B.low, s0 >= kWindow ? s0 - kWindow : 0);
    S.block = bi;
    S.elemOff = elemTotal;
    S.rankOff = rankTotal;
    elemTotal += S.s1 - S.w0;
    rankTotal += S.s1 - S.s0;
    segs.push_back(S);
  }
}

void Plan::finish_plan(const PlanKey& k)
{
  version++;
  tokTotal = 0;
  for (Block& B : blocks) {
    B.tokOff = tokTotal;
    tokTotal += token_capacity(B.end - B.start);
  }
  segs.clear();
  elemTotal = rankTotal = 0;
  for (uint32_t b = 0; b < blocks.size(); b++) add_segments(b);
  // token-walk sub-segments: kWalkSeg positions each
  walk.clear();
  for (uint32_t b = 0; b < blocks.size(); b++) {
    Block& B = blocks[b];
    const uint64_t n = B.end - B.start;
    B.walkFirst = (uint32_t)walk.size();
    B.walkCount = (uint32_t)((n + kWalkSeg - 1) / kWalkSeg);
    for (uint32_t i = 0; i < B.walkCount; i++) walk.push_back(make_uint2(b, i));
  }
  // parse segments: positions [0, n - 6] of every block longer than 12 bytes, top segment first
  dp.clear();
  maxDpCount = 1;
  for (uint32_t b = 0; b < blocks.size(); b++) {
    Block& B = blocks[b];
    const uint64_t n = B.end - B.start;
    B.dpFirst = (uint32_t)dp.size();
    B.dpCount = 0;
    if (n <= (uint64_t)kTailNoMatch) continue;
    const uint64_t top = n - 1 - kTailLiterals;
    uint64_t seg = dp_segment_size(n);
    if (n > 65536) {
      // tuning knob for blocks above 64 KiB: a multiple of 256 (the parse's range-minimum blocks)
      if (const char* e = getenv("SZ4_DP_SIZE")) {
        const uint64_t v = strtoull(e, nullptr, 10);
        if (v >= 1024 && v % 256 == 0 && (n + v - 1) / v <= kMaxDpSegs) seg = v;
      }
    }
    B.dpSize = (uint32_t)seg;
    for (uint64_t hi = top, i = 0;; hi -= seg, i++) {
      const uint64_t lo = hi + 1 >= seg ? hi + 1 - seg : 0;
      dp.push_back(DpSeg{b, (uint32_t)i, (uint32_t)lo, (uint32_t)hi});
      B.dpCount++;
      if (lo == 0) break;
    }
    maxDpCount = std::max(maxDpCount, B.dpCount);
  }
  // the finders' LDS-window kernels take the launch when every block's window fits their LDS
  ldsWindow = true;
  for (const Segment& S : segs) {
    const Block& B = blocks[S.block];
    if ((B.end - S.w0 + 8 + 3) / 4 * 4 > find_lds_bytes()) ldsWindow = false;
  }
  key = k;
}

uint64_t Plan::work_layout(uint64_t stagedBytes)
{
  auto al = [](uint64_t b) { return (b + 255) & ~255ull; };
  const uint64_t nb = blocks.size();
  const uint64_t elem = al(elemTotal * sizeof(uint2) + 64);
  off.elemB = elem;
  const uint64_t findEnd = 2 * elem;
  const uint64_t selBytes = al(stagedBytes * 4 + 64), rmq = al((stagedBytes + nb + 8) * 4);
  off.rmqUp = selBytes;
  off.rmqDown = selBytes + rmq;
  off.side = selBytes + 2 * rmq;
  const uint64_t parseEnd = off.side + al(dp.size() * dp_side_positions() * sizeof(uint2) + 64);
  off.lazy = selBytes;
  const uint64_t lazyEnd = off.lazy + al(walk.size() * lazy_slots_per_walk() * 4ull + 64);
  off.tok = selBytes;
  // the Token area, 16 bytes per entry, holds the token walk's 8-byte match records (walk_slot_first); the
  // walk area behind it keeps its place and size and is unused
  off.walk = off.tok + al(tokTotal * 16 + 64);
  const uint64_t emitEnd = off.walk + al(walk.size() * 2 * kWalkCap * 4 + 64);
  return std::max(std::max(findEnd, parseEnd), std::max(lazyEnd, emitEnd));
}

void Plan::build_uniform(uint64_t len, uint32_t blockSize)
{
  const PlanKey k{PlanKey::kUniform, len, blockSize};
  if (!begin(k)) return;
  for (uint64_t st = 0; st < len; st += blockSize)
    blocks.push_back(independent_block(st, std::min<uint64_t>(st + blockSize, len)));
  finish_plan(k);
}

void Plan::build_stream(uint64_t pre, uint64_t n, bool first, int legacy, bool dictMode)
{
  const PlanKey k{PlanKey::kStream, 0, 0, pre, n, first, legacy, dictMode};
  if (!begin(k)) return;
  const uint64_t bs = legacy ? kBlockMaxLegacy : kBlockMaxDict;
  for (uint64_t st = 0; st < n; st += bs) {
    Block B = independent_block(pre + st, pre + std::min(st + bs, n), legacy ? kBlkLegacy : 0);
    if (!legacy && !(st == 0 && first)) {
      B.low = B.start - kWindow;
      B.cut = B.start - kTailNoMatch;  // re-inserted by the lookback of the next block
      B.prev = st == 0 ? kNoBlock - 1 : (uint32_t)blocks.size() - 1;  // first: the ghost slot, below
    }
    blocks.push_back(B);
  }
  const uint32_t nb = (uint32_t)blocks.size();
  if (nb && blocks[0].prev == kNoBlock - 1) blocks[0].prev = nb;
  finish_plan(k);
}

uint64_t Plan::build_ragged(const std::vector<uint64_t>& sizes)
{
  const PlanKey k{PlanKey::kRagged};
  begin(k);
  uint64_t at = 0;
  for (uint64_t n : sizes) {
    blocks.push_back(independent_block(at, at + n));
    at += batch_stride(n);
  }
  finish_plan(k);
  return at;
}

uint64_t Plan::build_slots(const std::vector<uint32_t>& caps)
{
  const PlanKey k{PlanKey::kRagged};
  begin(k);
  version++;
  segs.clear();
  dp.clear();
  walk.clear();
  elemTotal = rankTotal = tokTotal = 0;
  maxDpCount = 1;
  ldsWindow = true;
  uint64_t at = 0;
  for (uint32_t cap : caps) {
    const uint32_t bi = (uint32_t)blocks.size();
    Slot s{};
    s.start = at;
    s.tokOff = tokTotal;
    s.elemOff = elemTotal;
    s.rankOff = rankTotal;
    s.cap = cap;
    s.elem = 1;
    s.segFirst = (uint32_t)segs.size();
    s.segCount = slot_seg_count(cap);
    s.dpFirst = (uint32_t)dp.size();
    s.dpCount = slot_dp_reserve(cap);
    s.walkFirst = (uint32_t)walk.size();
    s.walkCount = slot_walk_count(cap);
    slots.push_back(s);
    blocks.push_back(slot_block(s, cap));
    for (uint32_t j = 0; j < s.segCount; j++) segs.push_back(slot_segment(s, bi, j, cap));
    for (uint32_t j = 0; j < s.dpCount; j++) dp.push_back(slot_dp(bi, j, cap));
    for (uint32_t j = 0; j < s.walkCount; j++) walk.push_back(make_uint2(bi, j));
    tokTotal += token_capacity(cap);
    elemTotal += slot_elem_reserve(cap);
    rankTotal += slot_rank_reserve(cap);
    maxDpCount = std::max(maxDpCount, s.dpCount);
    // the widest window of any size is the capacity's: block end - w0 grows with the size
    for (uint32_t j = 0; j < s.segCount; j++)
      if ((blocks[bi].end - segs[s.segFirst + j].w0 + 8 + 3) / 4 * 4 > find_lds_bytes()) ldsWindow = false;
    at += batch_stride(cap);
  }
  key = k;
  return at;
}

}  // namespace sz4
