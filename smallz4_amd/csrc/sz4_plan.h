// sz4_plan.h -- the block plan of one pipeline run and its cache key.  Pure host arithmetic over the
// descriptors of sz4_internal.h: no HIP call, so it builds and runs without the kernels or a GPU
// (tests/cpp/plan_check.cpp).
//
// A plan is a function of its key alone.  The context keeps ONE plan; a builder is a no-op when the plan
// was built for an equal key, and builds it again otherwise, whatever kind of call built it before.
#pragma once
#include <vector>

#include "sz4_internal.h"
#include "sz4_slot_plan.h"

namespace sz4 {

constexpr uint64_t kSegTargets = 65536;  // target positions per segment

inline uint64_t token_capacity(uint64_t n) { return n / 2 + 4; }

// an independent block over the staged bytes [start, end): it sees nothing before its first byte
Block independent_block(uint64_t start, uint64_t end, uint32_t flags = 0);

// ragged plans: every item starts at the next multiple of kBatchAlign
inline uint64_t batch_stride(uint64_t size) { return (size + kBatchAlign - 1) / kBatchAlign * kBatchAlign; }

// The shape a plan was built for.  uniform: `len` bytes in independent blocks of `blockSize`.  stream: one
// chunk of a reference stream, `n` new bytes after `pre` carried ones.  Ragged plans (an item list) are
// never reused: their key compares unequal to every key, itself included, and so does the empty key.
struct PlanKey {
  enum Kind : uint32_t { kEmpty, kUniform, kStream, kRagged };
  Kind kind = kEmpty;
  uint64_t len = 0, blockSize = 0;  // uniform
  uint64_t pre = 0, n = 0;          // stream ...
  bool first = false;
  int legacy = 0;
  bool dictMode = false;
  bool operator==(const PlanKey& o) const
  {
    return kind == o.kind && (kind == kUniform || kind == kStream) && len == o.len && blockSize == o.blockSize &&
           pre == o.pre && n == o.n && first == o.first && dictMode == o.dictMode && legacy == o.legacy;
  }
};

struct Plan {
  std::vector<Block> blocks;
  std::vector<Segment> segs;  // the match search's segments
  std::vector<DpSeg> dp;      // the parse's segments
  std::vector<uint2> walk;    // the token walk's sub-segments (block, index in the block)
  std::vector<Slot> slots;    // build_slots alone: the slot of every block (empty for every other plan)
  uint64_t elemTotal = 0, rankTotal = 0, tokTotal = 0;
  bool ldsWindow = false;     // every segment's window fits the finders' LDS
  uint32_t maxDpCount = 1;    // the largest dpCount of the blocks (at least 1)
  uint64_t version = 0;       // counts the builds: the device copy of another version is stale
  PlanKey key;                // what the vectors above were built for

  // One region for the arrays whose lifetimes do not overlap (offsets in bytes; elemA and sel start at 0):
  //   match search   sort elements A | B  (dead once the search has finished)
  //   after it       parse choices (sel) | greedy/lazy replay slots, or the parse's range minima UP | DOWN and
  //                  k_dp_fix's saved speculative values, or the frame tokens | token-walk slots
  // sel stays live from k_prep (its tail) through the parse to the token walk; the rest are per stage.
  struct WorkOffsets {
    uint64_t elemB = 0, rmqUp = 0, rmqDown = 0, side = 0, lazy = 0, tok = 0, walk = 0;
  } off;
  // lays the region out for this plan over `stagedBytes` of input; returns its size in bytes
  uint64_t work_layout(uint64_t stagedBytes);

  // The three builders.  Each is a no-op when the plan already has the key it would build.
  void build_uniform(uint64_t len, uint32_t blockSize);
  // smallz4.h:572-585: 4 MiB blocks seeing the previous 64 KiB, or 8 MiB independent legacy blocks; the first
  // block of a chunk that continues a stream has prev == blocks.size(), the ghost slot
  void build_stream(uint64_t pre, uint64_t n, bool first, int legacy, bool dictMode);
  // one independent block per item (sizes > 0), at ascending multiples of kBatchAlign; returns the end of the
  // last item's stride (the bytes the gather stages, before the pad)
  uint64_t build_ragged(const std::vector<uint64_t>& sizes);
  // a sized compress queue's plan (sz4_slot_plan.h): one slot per capacity (0 allowed), empty ones included, at
  // the running sum of the capacities' strides.  Every table holds what the slot reserves -- the largest count
  // any size <= cap needs -- with the entries of size == cap, the rest inert; the totals, maxDpCount and
  // ldsWindow follow from the reserved counts and the capacities, so the scratch laid out for this plan holds
  // every plan of smaller sizes.  Slot::elem is left 1.  Returns the end of the last slot's stride
  uint64_t build_slots(const std::vector<uint32_t>& caps);

 private:
  bool begin(const PlanKey& k);
  void add_segments(uint32_t bi);
  void finish_plan(const PlanKey& k);
};

}  // namespace sz4
