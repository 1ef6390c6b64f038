// sz4_batch.hip -- device pieces of the ragged batch API (sz4_compress_batch_device) for gfx950:
//   k_batch_gather  stages many separately allocated buffers into the context's padded staging buffer
//   k_batch_move    moves compressed blocks to their caller-order place when one piece ran as two
//                   pipeline runs (items whose window fits the finders' LDS, and items whose does not)
// Both are plain copies, bound by memory: 16-byte accesses on the aligned side, work cut by bytes.
#include <hip/hip_runtime.h>

#include "sz4_internal.h"

namespace sz4 {
namespace {

constexpr uint32_t kGatherThreads = 256;
constexpr uint32_t kGatherTile = 1024;  // 16-byte staging words per workgroup step (16 KiB, 4 per thread)
constexpr uint32_t kGatherGrid = 2048;  // workgroups at most (256 CUs x 8); the rest is a grid-stride loop

// index of the last item in [lo, hi) whose start is <= pos (items[lo].start <= pos)
__device__ __forceinline__ uint32_t item_at(const BatchItem* __restrict__ items, uint32_t lo, uint32_t hi, uint64_t pos)
{
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (items[mid].start <= pos) lo = mid;
    else hi = mid;
  }
  return lo;
}

// Every thread writes whole 16-byte words of the staging buffer; a word belongs to the last item that starts
// at or below it (starts are multiples of kBatchAlign, so no word holds bytes of two items).  The work is
// cut by staged bytes, not by item: a tile of kGatherTile words first narrows the item range to the items
// that start inside it (a wave-uniform search), then every word searches that range only -- one step
// where items are large, log2(items per 16 KiB) where they are tiny.
// The source has any alignment: a word is built from the one or two ALIGNED 16-byte source words that hold
// its bytes.  The first holds the word's first byte, which lies inside the item; the second is read only
// when it starts below the item's end -- nothing outside the aligned words that overlap [src, src + size)
// is touched (a caller's buffer may end at the end of its allocation).  Bytes past the item's end, the gap
// up to the next item and the pad after the last item are written as 0.
__global__ __launch_bounds__(kGatherThreads) void k_batch_gather(const BatchItem* __restrict__ items, uint32_t n,
                                                                 uint8_t* __restrict__ staged, uint64_t words)
{
  const uint64_t tiles = (words + kGatherTile - 1) / kGatherTile;
  for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const uint64_t w0 = tile * kGatherTile;
    const uint64_t w1 = w0 + kGatherTile < words ? w0 + kGatherTile : words;
    const uint32_t first = item_at(items, 0, n, 16 * w0);
    const uint32_t last = item_at(items, first, n, 16 * (w1 - 1));
    for (uint64_t w = w0 + threadIdx.x; w < w1; w += kGatherThreads) {
      const BatchItem it = items[item_at(items, first, last + 1, 16 * w)];
      const uint64_t o = 16 * w - it.start;  // item-relative offset of the word
      uint64_t r0 = 0, r1 = 0;
      if (o < it.size) {
        const uint64_t p = it.src + o;
        const uint32_t a = (uint32_t)(p & 15u);
        const uint4* q = reinterpret_cast<const uint4*>(p - a);
        const uint4 lo = q[0];
        uint4 hi = make_uint4(0u, 0u, 0u, 0u);
        if (a && p - a + 16 < it.src + it.size) hi = q[1];
        const uint64_t x0 = lo.x | ((uint64_t)lo.y << 32), x1 = lo.z | ((uint64_t)lo.w << 32);
        const uint64_t x2 = hi.x | ((uint64_t)hi.y << 32), x3 = hi.z | ((uint64_t)hi.w << 32);
        // bytes [a, a + 16) of the 32 bytes x0..x3
        const bool up = a >= 8;
        const uint64_t s0 = up ? x1 : x0, s1 = up ? x2 : x1, s2 = up ? x3 : x2;
        const uint32_t sh = (a & 7u) * 8u;
        r0 = sh ? (s0 >> sh) | (s1 << (64u - sh)) : s0;
        r1 = sh ? (s1 >> sh) | (s2 << (64u - sh)) : s1;
        const uint64_t left = it.size - o;  // bytes of the item from this word on
        if (left < 16) {
          if (left <= 8) {
            r1 = 0;
            if (left < 8) r0 &= (1ull << (8 * left)) - 1;
          } else {
            r1 &= (1ull << (8 * (left - 8))) - 1;
          }
        }
      }
      *reinterpret_cast<uint4*>(staged + 16 * w) =
          make_uint4((uint32_t)r0, (uint32_t)(r0 >> 32), (uint32_t)r1, (uint32_t)(r1 >> 32));
    }
  }
}

struct __attribute__((packed)) Unaligned16 {
  uint32_t x, y, z, w;
};

// One workgroup per entry (at most kBatchMoveMax bytes): bytes up to the destination's first 16-byte
// boundary, 16-byte stores from there (the source side is read unaligned, inside [src, src + len) only),
// then the last bytes.
__global__ __launch_bounds__(256) void k_batch_move(const BatchMove* __restrict__ moves, const uint8_t* __restrict__ from,
                                                    uint8_t* __restrict__ to)
{
  const BatchMove m = moves[blockIdx.x];
  const uint8_t* src = from + m.src;
  uint8_t* dst = to + m.dst;
  uint64_t head = (16 - (reinterpret_cast<uintptr_t>(dst) & 15u)) & 15u;
  if (head > m.len) head = m.len;
  const uint64_t body = (m.len - head) / 16;
  for (uint64_t k = threadIdx.x; k < head; k += 256) dst[k] = src[k];
  for (uint64_t k = threadIdx.x; k < body; k += 256) {
    const Unaligned16 v = *reinterpret_cast<const Unaligned16*>(src + head + 16 * k);
    *reinterpret_cast<uint4*>(dst + head + 16 * k) = make_uint4(v.x, v.y, v.z, v.w);
  }
  for (uint64_t k = head + 16 * body + threadIdx.x; k < m.len; k += 256) dst[k] = src[k];
}

}  // namespace

void launch_batch_gather(const BatchItem* items, uint32_t n, uint8_t* staged, uint64_t stagedBytes, hipStream_t s)
{
  const uint64_t words = stagedBytes / 16;
  if (!n || !words) return;
  const uint64_t tiles = (words + kGatherTile - 1) / kGatherTile;
  hipLaunchKernelGGL(k_batch_gather, dim3((uint32_t)(tiles < kGatherGrid ? tiles : kGatherGrid)), dim3(kGatherThreads), 0, s,
                     items, n, staged, words);
}

void launch_batch_move(const BatchMove* moves, uint32_t n, const uint8_t* from, uint8_t* to, hipStream_t s)
{
  if (n) hipLaunchKernelGGL(k_batch_move, dim3(n), dim3(256), 0, s, moves, from, to);
}

}  // namespace sz4
