// sz4_batch.hip -- device pieces of the ragged batch API (sz4_compress_batch_device) for gfx950:
//   k_batch_gather  stages many separately allocated buffers into the context's padded staging buffer
//   k_batch_gather_planes  the same with the byte-plane split of typed items folded in
//                   (sz4_compress_batch_typed_device: byte k of every element of an item stored together)
//   k_batch_move    moves compressed blocks to their caller-order place when one piece ran as two
//                   pipeline runs (items whose window fits the finders' LDS, and items whose does not)
//   k_batch_merge   the inverse of the split, after the batch decoder (sz4_unlz4_batch_typed_device)
//   k_batch_gather_bits, k_batch_merge_bits  the same two for a table that holds an item of SZ4_FILTER_BITS
//                   (sz4_compress_batch_filtered_device, sz4_unlz4_batch_filtered_device): that item is shuffled
//                   into its bit planes and back, 8 x 8 bit transposes in registers and a transpose across lanes
// All are copies, bound by memory: 16-byte accesses on the aligned side, work cut by bytes.
//   k_cq_items, k_cq_finish  the compress queue's ends (sz4_cq_enqueue): the caller's device pointer table
//                   into the gather's item table, and the run's offsets and sizes out to the caller's tables
//   k_cq_plan       a sized queue's first kernel (sz4_cq_enqueue_sized): k_cq_items' job, and every slot's plan
//                   entries rewritten for the sizes in the caller's device table (sz4_slot_plan.h)
#include <hip/hip_runtime.h>

#include "sz4_internal.h"
#include "sz4_slot_plan.h"

namespace sz4 {
namespace {

constexpr uint32_t kGatherThreads = 256;
constexpr uint32_t kGatherTile = 1024;  // 16-byte staging words per workgroup step (16 KiB, 4 per thread)
constexpr uint32_t kGatherGrid = 2048;  // workgroups at most (256 CUs x 8); the rest is a grid-stride loop

// index of the last item in [lo, hi) whose start is <= pos (items[lo].start <= pos)
template <typename Item>
__device__ __forceinline__ uint32_t item_at(const Item* __restrict__ items, uint32_t lo, uint32_t hi, uint64_t pos)
{
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (items[mid].start <= pos) lo = mid;
    else hi = mid;
  }
  return lo;
}

// bytes [o, o + 16) of the item at `src` (o < size; bytes from the item's end on read 0), from the one or two
// aligned 16-byte source words that hold them
__device__ __forceinline__ void gather_word(uint64_t src, uint64_t size, uint64_t o, uint64_t& r0, uint64_t& r1)
{
  const uint64_t p = src + o;
  const uint32_t a = (uint32_t)(p & 15u);
  const uint4* q = reinterpret_cast<const uint4*>(p - a);
  const uint4 lo = q[0];
  uint4 hi = make_uint4(0u, 0u, 0u, 0u);
  if (a && p - a + 16 < src + size) hi = q[1];
  const uint64_t x0 = lo.x | ((uint64_t)lo.y << 32), x1 = lo.z | ((uint64_t)lo.w << 32);
  const uint64_t x2 = hi.x | ((uint64_t)hi.y << 32), x3 = hi.z | ((uint64_t)hi.w << 32);
  // bytes [a, a + 16) of the 32 bytes x0..x3
  const bool up = a >= 8;
  const uint64_t s0 = up ? x1 : x0, s1 = up ? x2 : x1, s2 = up ? x3 : x2;
  const uint32_t sh = (a & 7u) * 8u;
  r0 = sh ? (s0 >> sh) | (s1 << (64u - sh)) : s0;
  r1 = sh ? (s1 >> sh) | (s2 << (64u - sh)) : s1;
  const uint64_t left = size - o;  // bytes of the item from this word on
  if (left < 16) {
    if (left <= 8) {
      r1 = 0;
      if (left < 8) r0 &= (1ull << (8 * left)) - 1;
    } else {
      r1 &= (1ull << (8 * (left - 8))) - 1;
    }
  }
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
      if (o < it.size) gather_word(it.src, it.size, o, r0, r1);
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

// ---- typed items: the byte-plane split and its inverse -----------------------------------------------
// An item of `size` bytes and element width E (2, 4 or 8) has m = size / E whole elements: byte k of element
// e is split byte k * m + e, and the size % E tail bytes follow the planes unchanged.
struct __attribute__((packed)) Unaligned8 {
  uint32_t x, y;
};
struct __attribute__((packed)) Unaligned4 {
  uint32_t x;
};
struct __attribute__((packed)) Unaligned2 {
  uint16_t x;
};

// v_perm_b32: result byte i is byte sel[i] of the 8 bytes {hi, lo} (0..3 = lo, 4..7 = hi, 0x0c = zero)
__device__ __forceinline__ uint32_t perm(uint32_t hi, uint32_t lo, uint32_t sel) { return __builtin_amdgcn_perm(hi, lo, sel); }

// byte k (0..3) of each of four words
__device__ __forceinline__ uint32_t pick4(uint32_t d0, uint32_t d1, uint32_t d2, uint32_t d3, uint32_t k)
{
  const uint32_t sel = 0x0c0c0400u + k * 0x0101u;
  return perm(perm(d3, d2, sel), perm(d1, d0, sel), 0x05040100u);
}

// 16 bytes of plane k: byte k of the 16 consecutive elements at p (16 * E source bytes, all inside the item,
// so the loads may be unaligned and still touch nothing outside it)
template <int E>
__device__ __forceinline__ uint4 plane_word(const uint8_t* __restrict__ p, uint32_t k)
{
  uint32_t d[4 * E], r[4];
#pragma unroll
  for (int i = 0; i < E; i++) {
    const Unaligned16 v = *reinterpret_cast<const Unaligned16*>(p + 16 * i);
    d[4 * i] = v.x, d[4 * i + 1] = v.y, d[4 * i + 2] = v.z, d[4 * i + 3] = v.w;
  }
#pragma unroll
  for (int j = 0; j < 4; j++) {
    if (E == 2) {
      r[j] = perm(d[2 * j + 1], d[2 * j], 0x06040200u + k * 0x01010101u);
    } else if (E == 4) {
      r[j] = pick4(d[4 * j], d[4 * j + 1], d[4 * j + 2], d[4 * j + 3], k);
    } else {
      const bool h = k >= 4;  // the element's upper word
      r[j] = pick4(h ? d[8 * j + 1] : d[8 * j], h ? d[8 * j + 3] : d[8 * j + 2], h ? d[8 * j + 5] : d[8 * j + 4],
                   h ? d[8 * j + 7] : d[8 * j + 6], k & 3u);
    }
  }
  return make_uint4(r[0], r[1], r[2], r[3]);
}

// split bytes [o, o + 16) of an item byte by byte (a word that straddles two planes, the tail or the item's
// end; bytes from the end on read 0): one division for the first byte, then the position is stepped
__device__ __forceinline__ uint4 plane_bytes(const uint8_t* __restrict__ src, uint32_t size, uint32_t E, uint32_t m, uint32_t o)
{
  const uint32_t planes = m * E;
  uint32_t k = 0, e = 0;
  if (o < planes) {
    k = o / m;
    e = o - k * m;
  }
  uint64_t r[2] = {0, 0};
#pragma unroll
  for (uint32_t i = 0; i < 16; i++) {
    const uint32_t pos = o + i;
    if (pos < size) {
      uint32_t at = pos;  // the tail lies where it lay
      if (pos < planes) {
        at = e * E + k;
        if (++e == m) e = 0, k++;
      }
      r[i / 8] |= (uint64_t)src[at] << (8 * (i % 8));
    }
  }
  return make_uint4((uint32_t)r[0], (uint32_t)(r[0] >> 32), (uint32_t)r[1], (uint32_t)(r[1] >> 32));
}

// The staged word of a byte-split item that the thread of item-relative offset `off` takes (`off` becomes that
// word's offset; zeros from the item's end on).
// Which word a thread takes is permuted inside the item: with wp = m / 16 whole words per plane, slot
// j * E + k takes word k * wp + j (a bijection of the first E * wp words, the rest keep their place).  E
// neighbouring lanes then build words of E different planes from the SAME 16 * E source bytes, so a
// wave's load touches 64 / E spans and not 64, and every source line is fetched once per wave and
// not by E waves far apart in the grid; the lanes of one plane still store 16 * 64 / E consecutive bytes.
__device__ __forceinline__ uint4 split_word(const BatchTyped& it, uint64_t& off)
{
  const uint32_t E = it.elem, lg = __ffs(E) - 1, m = it.size >> lg;
  if (E > 1) {
    const uint64_t slot = off / 16, wp = m / 16;
    if (slot < wp * E) off = 16 * ((slot & (E - 1)) * wp + (slot >> lg));
  }
  uint4 v = make_uint4(0u, 0u, 0u, 0u);
  if (off < it.size) {
    const uint32_t o = (uint32_t)off;
    if (E == 1) {
      uint64_t r0, r1;
      gather_word(it.src, it.size, o, r0, r1);
      v = make_uint4((uint32_t)r0, (uint32_t)(r0 >> 32), (uint32_t)r1, (uint32_t)(r1 >> 32));
    } else {
      const uint8_t* src = reinterpret_cast<const uint8_t*>(it.src);
      uint32_t k = 0, e = m;  // e + 16 <= m: the word lies inside plane k, from element e on
      if (o + 16 <= m * E) {
        k = o / m;
        e = o - k * m;
      }
      if (e + 16 <= m) {
        const uint8_t* p = src + (uint64_t)e * E;
        v = E == 2 ? plane_word<2>(p, k) : E == 4 ? plane_word<4>(p, k) : plane_word<8>(p, k);
      } else {
        v = plane_bytes(src, it.size, E, m, o);
      }
    }
  }
  return v;
}

// k_batch_gather with the split folded in: the same contract (every 16-byte word of the staging buffer is
// written, zeros outside the items, work cut by staged bytes, any source alignment, no read outside the
// aligned 16-byte source words that overlap an item).  One thread per staged word.  A word that lies inside one
// plane takes its 16 bytes from the 16 * E source bytes of 16 consecutive elements (E 16-byte loads, bytes
// picked with v_perm_b32); the words that straddle planes go byte by byte; an item of width 1 is staged as
// k_batch_gather stages it.
__global__ __launch_bounds__(kGatherThreads) void k_batch_gather_planes(const BatchTyped* __restrict__ items, uint32_t n,
                                                                        uint8_t* __restrict__ staged, uint64_t words)
{
  const uint64_t tiles = (words + kGatherTile - 1) / kGatherTile;
  for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const uint64_t w0 = tile * kGatherTile;
    const uint64_t w1 = w0 + kGatherTile < words ? w0 + kGatherTile : words;
    const uint32_t first = item_at(items, 0, n, 16 * w0);
    const uint32_t last = item_at(items, first, n, 16 * (w1 - 1));
    for (uint64_t w = w0 + threadIdx.x; w < w1; w += kGatherThreads) {
      const BatchTyped it = items[item_at(items, first, last + 1, 16 * w)];
      uint64_t off = 16 * w - it.start;  // item-relative offset of the word
      const uint4 v = split_word(it, off);
      *reinterpret_cast<uint4*>(staged + it.start + off) = v;
    }
  }
}

// the bytes of output positions [lo, hi) (at most 16, in the aligned word that starts at `base`, which may lie
// below 0) one by one, from item idx on: the items follow each other without gaps, none is empty
__device__ __forceinline__ uint4 merge_bytes(const BatchTyped* __restrict__ items, uint32_t idx, const uint8_t* __restrict__ from,
                                             int64_t base, uint64_t lo, uint64_t hi)
{
  BatchTyped it = items[idx];
  uint64_t r0 = 0, r1 = 0;
  for (uint64_t pos = lo; pos < hi; pos++) {
    while (pos >= it.start + it.size) it = items[++idx];
    const uint32_t b = (uint32_t)(pos - it.start), E = it.elem, lg = __ffs(E) - 1, m = it.size >> lg;
    const uint32_t at = b < (m << lg) ? (b & (E - 1)) * m + (b >> lg) : b;
    const uint32_t i = (uint32_t)((int64_t)pos - base);
    const uint64_t x = (uint64_t)from[it.src + at] << (8 * (i % 8));
    if (i < 8) r0 |= x;
    else r1 |= x;
  }
  return make_uint4((uint32_t)r0, (uint32_t)(r0 >> 32), (uint32_t)r1, (uint32_t)(r1 >> 32));
}

// the bytes of output positions [lo, hi) of a byte-split item's merge: item idx (= it) holds position lo
__device__ __forceinline__ uint4 merge_word(const BatchTyped* __restrict__ items, uint32_t idx, const BatchTyped& it,
                                            const uint8_t* __restrict__ from, int64_t base, uint64_t lo, uint64_t hi)
{
  const uint32_t b = (uint32_t)(lo - it.start), E = it.elem, lg = __ffs(E) - 1, m = it.size >> lg;
  const uint8_t* p = from + it.src;
  uint4 v;
  if (hi - lo == 16 && b + 16 <= it.size && E == 1) {
    const Unaligned16 x = *reinterpret_cast<const Unaligned16*>(p + b);
    v = make_uint4(x.x, x.y, x.z, x.w);
  } else if (hi - lo == 16 && b + 16 <= (m << lg) && !(b & (E - 1))) {
    const uint8_t* q = p + (b >> lg);
    if (E == 2) {
      const Unaligned8 x = *reinterpret_cast<const Unaligned8*>(q), y = *reinterpret_cast<const Unaligned8*>(q + m);
      v = make_uint4(perm(y.x, x.x, 0x05010400u), perm(y.x, x.x, 0x07030602u), perm(y.y, x.y, 0x05010400u),
                     perm(y.y, x.y, 0x07030602u));
    } else if (E == 4) {
      uint32_t x[4];
#pragma unroll
      for (uint32_t k = 0; k < 4; k++) x[k] = reinterpret_cast<const Unaligned4*>(q + (uint64_t)k * m)->x;
      const uint32_t l0 = perm(x[1], x[0], 0x05010400u), l1 = perm(x[3], x[2], 0x05010400u);
      const uint32_t h0 = perm(x[1], x[0], 0x07030602u), h1 = perm(x[3], x[2], 0x07030602u);
      v = make_uint4(perm(l1, l0, 0x05040100u), perm(l1, l0, 0x07060302u), perm(h1, h0, 0x05040100u),
                     perm(h1, h0, 0x07060302u));
    } else {
      uint32_t t[4];
#pragma unroll
      for (uint32_t k = 0; k < 4; k++)
        t[k] = perm(reinterpret_cast<const Unaligned2*>(q + (uint64_t)(2 * k + 1) * m)->x,
                    reinterpret_cast<const Unaligned2*>(q + (uint64_t)(2 * k) * m)->x, 0x05010400u);
      v = make_uint4(perm(t[1], t[0], 0x05040100u), perm(t[3], t[2], 0x05040100u), perm(t[1], t[0], 0x07060302u),
                     perm(t[3], t[2], 0x07060302u));
    }
  } else {
    v = merge_bytes(items, idx, from, base, lo, hi);
  }
  return v;
}

// stores the bytes of positions [lo, hi) of the aligned word at `base`: whole, or byte by byte at the buffer's ends
__device__ __forceinline__ void merge_store(uint8_t* __restrict__ to, uint4 v, int64_t base, uint64_t lo, uint64_t hi)
{
  if (hi - lo == 16) {
    *reinterpret_cast<uint4*>(to + lo) = v;
  } else {
    const uint64_t x0 = v.x | ((uint64_t)v.y << 32), x1 = v.z | ((uint64_t)v.w << 32);
    for (uint64_t pos = lo; pos < hi; pos++) {
      const uint32_t i = (uint32_t)((int64_t)pos - base);
      to[pos] = (uint8_t)((i < 8 ? x0 : x1) >> (8 * (i % 8)));
    }
  }
}

// The inverse of the split, from the batch decoder's scratch (item i's split bytes at from + src) to the
// caller's buffer (the item at to + start; `to` has any alignment, the items lie back to back).  One thread
// per ALIGNED 16-byte word of the destination, work cut by bytes as in the gather.  A word inside one item
// whose position in the item is a multiple of E (every word of an item that starts at a multiple of its
// element width) takes 16 / E bytes from each plane -- unaligned loads inside the item's scratch extent --
// and interleaves them with v_perm_b32; width 1 is one unaligned 16-byte load.  Every other word (another
// phase, the tail, two items in one word) goes byte by byte, and the first and last words of the destination
// store only the bytes inside [to, to + total).
__global__ __launch_bounds__(kGatherThreads) void k_batch_merge(const BatchTyped* __restrict__ items, uint32_t n,
                                                                const uint8_t* __restrict__ from, uint8_t* __restrict__ to,
                                                                uint64_t total, uint64_t words)
{
  const int64_t a0 = (int64_t)(reinterpret_cast<uintptr_t>(to) & 15u);
  const uint64_t tiles = (words + kGatherTile - 1) / kGatherTile;
  for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const uint64_t w0 = tile * kGatherTile;
    const uint64_t w1 = w0 + kGatherTile < words ? w0 + kGatherTile : words;
    const uint32_t first = item_at(items, 0, n, w0 ? 16 * w0 - a0 : 0);
    const uint32_t last = item_at(items, first, n, total - 1 < 16 * w1 - a0 - 1 ? total - 1 : 16 * w1 - a0 - 1);
    for (uint64_t w = w0 + threadIdx.x; w < w1; w += kGatherThreads) {
      const int64_t base = (int64_t)(16 * w) - a0;
      const uint64_t lo = base < 0 ? 0 : (uint64_t)base;
      const uint64_t hi = (uint64_t)(base + 16) < total ? (uint64_t)(base + 16) : total;
      const uint32_t idx = item_at(items, first, last + 1, lo);
      const BatchTyped it = items[idx];
      merge_store(to, merge_word(items, idx, it, from, base, lo, hi), base, lo, hi);
    }
  }
}

// ---- typed items: the bit-plane shuffle (SZ4_FILTER_BITS) and its inverse ------------------------------------
// An item of `size` bytes and width E has m = size / E whole elements, of which g = m - m % 8 are shuffled into
// 8 * E bit rows of G = g / 8 bytes: bit (e & 7) of shuffled byte (8 * k + b) * G + (e >> 3) is bit b of byte k of
// element e.  The m % 8 left-over elements and the size % E tail bytes follow the rows unchanged.
// BatchTyped::elem holds the width in its low byte and the filter above it.
constexpr uint32_t kFilterShift = 8;
__device__ __forceinline__ uint32_t item_width(const BatchTyped& it) { return it.elem & 0xFFu; }
__device__ __forceinline__ bool item_bits(const BatchTyped& it) { return (it.elem >> kFilterShift) != 0; }

// the transpose of an 8 x 8 bit matrix: bit c of byte r becomes bit r of byte c (three masked swap rounds)
__device__ __forceinline__ uint64_t transpose8(uint64_t x)
{
  uint64_t t = (x ^ (x >> 7)) & 0x00AA00AA00AA00AAull;
  x ^= t ^ (t << 7);
  t = (x ^ (x >> 14)) & 0x0000CCCC0000CCCCull;
  x ^= t ^ (t << 14);
  t = (x ^ (x >> 28)) & 0x00000000F0F0F0F0ull;
  x ^= t ^ (t << 28);
  return x;
}

// one round of a transpose across lanes: the lanes whose `up` is clear keep (a0, a1) and give (b0, b1) to the
// lane `mask` above them, from which they take its (a0, a1) into (b0, b1); the upper lanes the other way round.
// Both lanes of a pair are in the same branch (the callers' fast paths hold for whole groups of lanes).
__device__ __forceinline__ void lane_swap(uint32_t& a0, uint32_t& a1, uint32_t& b0, uint32_t& b1, bool up, int mask)
{
  const uint32_t r0 = (uint32_t)__shfl_xor((int)(up ? a0 : b0), mask), r1 = (uint32_t)__shfl_xor((int)(up ? a1 : b1), mask);
  if (up) a0 = r0, a1 = r1;
  else b0 = r0, b1 = r1;
}

// (x0, x1): byte k of elements 0..7 and 8..15.  Returns d[q] = the two bytes of bit row 2q (low half) and of
// bit row 2q + 1 (high half) that these 16 elements make
__device__ __forceinline__ uint4 bit_rows16(uint64_t x0, uint64_t x1)
{
  const uint64_t t0 = transpose8(x0), t1 = transpose8(x1);
  const uint32_t l0 = (uint32_t)t0, h0 = (uint32_t)(t0 >> 32), l1 = (uint32_t)t1, h1 = (uint32_t)(t1 >> 32);
  return make_uint4(perm(l1, l0, 0x05010400u), perm(l1, l0, 0x07030602u), perm(h1, h0, 0x05010400u),
                    perm(h1, h0, 0x07030602u));
}

// bit b of each of the 8 bytes of x, byte t's into bit t
__device__ __forceinline__ uint32_t bits8(uint64_t x, uint32_t b)
{
  return (uint32_t)((((x >> b) & 0x0101010101010101ull) * 0x0102040810204080ull) >> 56);
}

// shuffled bytes [o, o + 16) of an item row byte by row byte (a word that straddles two rows, a row that does not
// start at a multiple of 16, the left-over elements, the tail or the item's end; bytes from the end on read 0):
// one division for the first byte, then the position is stepped.  At widths 1 and 2 two bytes of a row at a time
// where the row has them -- bit b of byte k of 16 elements, 16 * E source bytes; at widths 4 and 8 that moved
// more bytes through the L1 than eight byte loads cost, and ran slower -- and everything else bit by bit.
__device__ __forceinline__ uint4 bits_bytes(const uint8_t* __restrict__ src, uint32_t size, uint32_t E, uint32_t G, uint32_t o)
{
  const uint32_t body = 8 * G * E;
  uint32_t r = 0, c = 0;
  if (o < body) {
    r = o / G;
    c = o - r * G;
  }
  uint64_t out[2] = {0, 0};
#pragma unroll 1
  for (uint32_t i = 0; i < 16;) {
    const uint32_t pos = o + i;
    if (pos >= size) break;
    uint32_t v, step = 1;
    if (pos < body) {
      const uint32_t k = r >> 3, b = r & 7u;
      const uint8_t* p = src + (uint64_t)(8 * c) * E;  // element 8c
      if (E <= 2 && i < 15 && c + 1 < G) {             // the elements 8c .. 8c + 15 are inside the body
        uint4 x;
        if (E == 1) {
          const Unaligned16 y = *reinterpret_cast<const Unaligned16*>(p);
          x = make_uint4(y.x, y.y, y.z, y.w);
        } else {
          x = plane_word<2>(p, k);
        }
        v = bits8(x.x | ((uint64_t)x.y << 32), b) | bits8(x.z | ((uint64_t)x.w << 32), b) << 8;
        step = 2;
      } else {
        v = 0;
#pragma unroll
        for (uint32_t t = 0; t < 8; t++) v |= ((p[t * E + k] >> b) & 1u) << t;
      }
      c += step;
      if (c == G) c = 0, r++;
    } else {
      v = src[pos];  // the left-over elements and the tail lie where they lay
    }
    out[i / 8] |= (uint64_t)(v & 0xFFu) << (8 * (i % 8));
    if (step == 2) out[(i + 1) / 8] |= (uint64_t)(v >> 8) << (8 * ((i + 1) % 8));
    i += step;
  }
  return make_uint4((uint32_t)out[0], (uint32_t)(out[0] >> 32), (uint32_t)out[1], (uint32_t)(out[1] >> 32));
}

// The staged word of a bit-shuffled item that the thread of item-relative offset `off` takes, as split_word.
// With wr = G / 16 whole words per row when every row starts at a multiple of 16 (G % 16 == 0; otherwise 0),
// the words of the item's 8 * E * wr row words are dealt to octets of lanes: octet (j, k) takes word j of the rows
// 8k..8k + 7, lane i of it row 8k + i.  The octets of one j are neighbours, so E octets read the same 128 * E
// source bytes.  Lane i loads byte k of the elements 128j + 16i .. + 15 (plane_word), transposes them as two
// 8 x 8 bit blocks, and then holds two bytes for each of the eight rows; three lane_swap rounds (distances 4, 2,
// 1: a transpose of an 8 x 8 matrix of 16-bit values held one row per lane) leave lane i with the sixteen bytes
// of row 8k + i.  A staged item starts at a multiple of 64 bytes = 4 words, so the octets are lane-aligned only
// after `pre` = 0 or 4 slots: those and the last octet's other slots take that octet's words bit by bit.
__device__ __forceinline__ uint4 shuffle_word(const BatchTyped& it, uint64_t& off)
{
  const uint32_t E = item_width(it), lg = __ffs(E) - 1, m = it.size >> lg, G = m >> 3;
  const uint32_t wr = G & 15u ? 0 : G >> 4, fast = wr << lg;  // octets in all
  const uint32_t pre = (8 - ((uint32_t)(it.start >> 4) & 7u)) & 7u;
  const uint32_t whole = fast - (pre && fast ? 1 : 0);  // lane-aligned octets
  const uint64_t slot = off / 16;
  uint32_t u = ~0u;
  if (slot < 8ull * fast) {
    u = (uint32_t)slot >= pre ? (uint32_t)slot - pre : (uint32_t)slot + 8 * fast - pre;
    const uint32_t i = u & 7u, k = (u >> 3) & (E - 1), j = u >> (3 + lg);
    off = 16ull * ((8 * k + i) * wr + j);
  }
  const uint8_t* src = reinterpret_cast<const uint8_t*>(it.src);
  uint4 v = make_uint4(0u, 0u, 0u, 0u);
  if ((u >> 3) < whole) {
    const uint32_t i = u & 7u, k = (u >> 3) & (E - 1), j = u >> (3 + lg);
    const uint8_t* p = src + ((uint64_t)(128 * j + 16 * i) << lg);
    uint4 x;
    if (E == 1) {
      const Unaligned16 y = *reinterpret_cast<const Unaligned16*>(p);
      x = make_uint4(y.x, y.y, y.z, y.w);
    } else {
      x = E == 2 ? plane_word<2>(p, k) : E == 4 ? plane_word<4>(p, k) : plane_word<8>(p, k);
    }
    uint4 d = bit_rows16(x.x | ((uint64_t)x.y << 32), x.z | ((uint64_t)x.w << 32));
    lane_swap(d.x, d.y, d.z, d.w, (i & 4u) != 0, 4);
    lane_swap(d.x, d.z, d.y, d.w, (i & 2u) != 0, 2);
    // distance 1 swaps the 16-bit halves: the lower lane keeps the low halves
    {
      const bool up = (i & 1u) != 0;
      const uint32_t s0 = up ? perm(d.y, d.x, 0x05040100u) : perm(d.y, d.x, 0x07060302u);
      const uint32_t s1 = up ? perm(d.w, d.z, 0x05040100u) : perm(d.w, d.z, 0x07060302u);
      const uint32_t r0 = (uint32_t)__shfl_xor((int)s0, 1), r1 = (uint32_t)__shfl_xor((int)s1, 1);
      if (up) {
        d = make_uint4(perm(d.x, r0, 0x07060100u), perm(d.y, r0, 0x07060302u), perm(d.z, r1, 0x07060100u),
                       perm(d.w, r1, 0x07060302u));
      } else {
        d = make_uint4(perm(r0, d.x, 0x05040100u), perm(r0, d.y, 0x07060100u), perm(r1, d.z, 0x05040100u),
                       perm(r1, d.w, 0x07060100u));
      }
    }
    v = d;
  } else if (off < it.size) {
    v = bits_bytes(src, it.size, E, G, (uint32_t)off);
  }
  return v;
}

// k_batch_gather_planes for a run that has a bit-shuffled item: the same contract and the same tiling; an item
// with the byte filter is staged by split_word, exactly as k_batch_gather_planes stages it.
__global__ __launch_bounds__(kGatherThreads) void k_batch_gather_bits(const BatchTyped* __restrict__ items, uint32_t n,
                                                                      uint8_t* __restrict__ staged, uint64_t words)
{
  const uint64_t tiles = (words + kGatherTile - 1) / kGatherTile;
  for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const uint64_t w0 = tile * kGatherTile;
    const uint64_t w1 = w0 + kGatherTile < words ? w0 + kGatherTile : words;
    const uint32_t first = item_at(items, 0, n, 16 * w0);
    const uint32_t last = item_at(items, first, n, 16 * (w1 - 1));
    for (uint64_t w = w0 + threadIdx.x; w < w1; w += kGatherThreads) {
      BatchTyped it = items[item_at(items, first, last + 1, 16 * w)];
      uint64_t off = 16 * w - it.start;
      uint4 v;
      if (item_bits(it)) {
        v = shuffle_word(it, off);
      } else {
        it.elem = item_width(it);
        v = split_word(it, off);
      }
      *reinterpret_cast<uint4*>(staged + it.start + off) = v;
    }
  }
}

// the bytes of output positions [lo, hi) one by one, as merge_bytes, where items may be bit-shuffled
__device__ __forceinline__ uint4 unshuffle_bytes(const BatchTyped* __restrict__ items, uint32_t idx, const uint8_t* __restrict__ from,
                                                 int64_t base, uint64_t lo, uint64_t hi)
{
  BatchTyped it = items[idx];
  uint64_t r0 = 0, r1 = 0;
#pragma unroll 1
  for (uint64_t pos = lo; pos < hi; pos++) {
    while (pos >= it.start + it.size) it = items[++idx];
    const uint32_t b = (uint32_t)(pos - it.start), E = item_width(it), lg = __ffs(E) - 1, m = it.size >> lg;
    const uint8_t* p = from + it.src;
    uint32_t v;
    if (!item_bits(it)) {
      v = p[b < (m << lg) ? (b & (E - 1)) * m + (b >> lg) : b];
    } else if (b < ((m & ~7u) << lg)) {
      const uint32_t G = m >> 3, e = b >> lg, k = b & (E - 1);
      const uint8_t* q = p + (uint64_t)(8 * k) * G + (e >> 3);
      v = 0;
#pragma unroll
      for (uint32_t t = 0; t < 8; t++) v |= ((q[(uint64_t)t * G] >> (e & 7u)) & 1u) << t;
    } else {
      v = p[b];
    }
    const uint32_t i = (uint32_t)((int64_t)pos - base);
    const uint64_t x = (uint64_t)v << (8 * (i % 8));
    if (i < 8) r0 |= x;
    else r1 |= x;
  }
  return make_uint4((uint32_t)r0, (uint32_t)(r0 >> 32), (uint32_t)r1, (uint32_t)(r1 >> 32));
}

// The word at position lo = it.start + b of a bit-shuffled item's inverse.  The unit of the inverse is 8
// consecutive elements, 8 * E output bytes: one byte from each of the 8 * E rows, an 8 x 8 bit transpose per
// plane.  A unit is W = max(1, E / 2) output words, taken by W neighbouring lanes, so every lane loads 16 row
// bytes whatever the width:
//   E = 1  the word is two units: two bytes from each of the 8 rows
//   E = 2  the word is one unit: one byte from each of the 16 rows
//   E = 4, 8  lane q of the W loads the 16 rows of the planes 2q and 2q + 1, transposes them and then holds two
//          bytes of each of the unit's 8 elements; one (E = 4) or two (E = 8) lane_swap rounds -- a transpose of a
//          W x W matrix of 8 / W elements x 2 bytes -- leave it with all the bytes of its own 8 / W elements
// The fast path needs the unit to start at an aligned word that is the first of W lanes (b a multiple of 8 * E
// for the first word, of 8 for E = 1; word index a multiple of W); everything else goes bit by bit.
__device__ __forceinline__ uint4 unshuffle_word(const BatchTyped* __restrict__ items, uint32_t idx, const BatchTyped& it,
                                                const uint8_t* __restrict__ from, int64_t base, uint64_t lo, uint64_t hi,
                                                uint64_t w)
{
  const uint32_t b = (uint32_t)(lo - it.start), E = item_width(it), lg = __ffs(E) - 1, m = it.size >> lg, G = m >> 3;
  const uint32_t W = E > 2 ? E >> 1 : 1, q = (uint32_t)w & (W - 1), b0 = b - 16 * q;  // the unit's first word
  const uint32_t need = E == 1 ? 7u : 8 * E - 1;
  const bool fast = hi - lo == 16 && b >= 16 * q && !(b0 & need) && b0 + 16 * W <= 8 * G * E;
  if (!fast) return unshuffle_bytes(items, idx, from, base, lo, hi);
  const uint8_t* p = from + it.src;
  if (E == 1) {
    p += b >> 3;
    uint64_t x0 = 0, x1 = 0;
#pragma unroll
    for (uint32_t t = 0; t < 8; t++) {
      const uint32_t y = reinterpret_cast<const Unaligned2*>(p + (uint64_t)t * G)->x;
      x0 |= (uint64_t)(y & 0xFFu) << (8 * t);
      x1 |= (uint64_t)(y >> 8) << (8 * t);
    }
    x0 = transpose8(x0), x1 = transpose8(x1);
    return make_uint4((uint32_t)x0, (uint32_t)(x0 >> 32), (uint32_t)x1, (uint32_t)(x1 >> 32));
  }
  p += (uint64_t)(16 * q) * G + ((b0 >> lg) >> 3);
  uint64_t x0 = 0, x1 = 0;
#pragma unroll
  for (uint32_t t = 0; t < 8; t++) {
    x0 |= (uint64_t)p[(uint64_t)t * G] << (8 * t);
    x1 |= (uint64_t)p[(uint64_t)(8 + t) * G] << (8 * t);
  }
  // d[n]: the bytes 2q, 2q + 1 of the elements 2n (low half) and 2n + 1 (high half)
  uint4 d = bit_rows16(x0, x1);
  if (E == 2) return d;
  if (E == 4) {
    lane_swap(d.x, d.y, d.z, d.w, q != 0, 1);
    // lane 0: (x, y) its own bytes 0, 1 of elements 0..3 and (z, w) bytes 2, 3; lane 1 the same of elements 4..7
    return make_uint4(perm(d.z, d.x, 0x05040100u), perm(d.z, d.x, 0x07060302u), perm(d.w, d.y, 0x05040100u),
                      perm(d.w, d.y, 0x07060302u));
  }
  lane_swap(d.x, d.y, d.z, d.w, (q & 2u) != 0, 2);
  lane_swap(d.x, d.z, d.y, d.w, (q & 1u) != 0, 1);
  // d[n]: the bytes 2n, 2n + 1 of the elements 2q (low half) and 2q + 1 (high half)
  return make_uint4(perm(d.y, d.x, 0x05040100u), perm(d.w, d.z, 0x05040100u), perm(d.y, d.x, 0x07060302u),
                    perm(d.w, d.z, 0x07060302u));
}

// k_batch_merge for a call that has a bit-shuffled item: the same contract and the same tiling; a word that
// starts in an item with the byte filter is merged by merge_word where that item holds all of it.
__global__ __launch_bounds__(kGatherThreads) void k_batch_merge_bits(const BatchTyped* __restrict__ items, uint32_t n,
                                                                     const uint8_t* __restrict__ from, uint8_t* __restrict__ to,
                                                                     uint64_t total, uint64_t words)
{
  const int64_t a0 = (int64_t)(reinterpret_cast<uintptr_t>(to) & 15u);
  const uint64_t tiles = (words + kGatherTile - 1) / kGatherTile;
  for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const uint64_t w0 = tile * kGatherTile;
    const uint64_t w1 = w0 + kGatherTile < words ? w0 + kGatherTile : words;
    const uint32_t first = item_at(items, 0, n, w0 ? 16 * w0 - a0 : 0);
    const uint32_t last = item_at(items, first, n, total - 1 < 16 * w1 - a0 - 1 ? total - 1 : 16 * w1 - a0 - 1);
    for (uint64_t w = w0 + threadIdx.x; w < w1; w += kGatherThreads) {
      const int64_t base = (int64_t)(16 * w) - a0;
      const uint64_t lo = base < 0 ? 0 : (uint64_t)base;
      const uint64_t hi = (uint64_t)(base + 16) < total ? (uint64_t)(base + 16) : total;
      const uint32_t idx = item_at(items, first, last + 1, lo);
      BatchTyped it = items[idx];
      uint4 v;
      if (item_bits(it)) {
        v = unshuffle_word(items, idx, it, from, base, lo, hi, w);
      } else if (hi <= it.start + it.size) {
        it.elem = item_width(it);
        v = merge_word(items, idx, it, from, base, lo, hi);
      } else {
        v = unshuffle_bytes(items, idx, from, base, lo, hi);
      }
      merge_store(to, v, base, lo, hi);
    }
  }
}

// ---- compress queue: the two ends of an enqueue ------------------------------------------------------------
// One thread per caller item.  A non-empty item's source goes into its block's entry of the run's item table,
// with the size the gather is to copy: the block's, or 0 for a null source (the item is then staged as zeros
// and reported as kItemArg).  An empty item's source entry is not read.
// The kernel also clears what a synchronous run clears with memsets before its first kernel -- the status
// word, every block's longFlag, the ghost slot's interval count (a queue's first block has no predecessor)
// and, in a run without blocks, the body's size: a memset captured in a graph was seen to store other bytes
// than its value from the second replay on, so an enqueue issues kernels only.
template <typename Item>
__global__ __launch_bounds__(256) void k_cq_items(const uint64_t* __restrict__ src, const uint32_t* __restrict__ map,
                                                  uint32_t count, uint32_t nblocks, const Block* __restrict__ blocks,
                                                  Item* __restrict__ items, uint32_t* __restrict__ status,
                                                  int* __restrict__ pipeStatus, uint32_t* __restrict__ longFlag,
                                                  uint32_t* __restrict__ ivCount, uint64_t* __restrict__ offsets)
{
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i == 0) {
    *pipeStatus = 0;
    ivCount[nblocks] = 0;
    if (!nblocks) offsets[0] = 0;
  }
  if (i >= count) return;
  const uint32_t b = map[i];
  uint32_t st = kItemOk;
  if (!(b & kCqEmpty)) {
    const uint64_t p = src[i];
    if (!p) st = kItemArg;
    items[b].src = p;
    items[b].size = p ? (decltype(items[b].size))(blocks[b].end - blocks[b].start) : 0;
    longFlag[b] = 0;
  }
  status[i] = st;
}

// A sized queue's k_cq_items: one wavefront per slot (caller item i is block i).  With n = srcSizes[i]:
//   n > cap            the slot is empty at this enqueue (kItemCapacity); neither the source entry nor the
//                      source is read
//   n == 0             the slot is empty (kItemOk); the source entry is not read
//   null source        the gather's size is 0, so the slot's n staged bytes are zeros (kItemArg)
// Lane 0 writes the gather's item entry (source and size; start and width stay as uploaded), the slot's Block
// and the statuses; the lanes share the slot's Segment and DpSeg entries, which sz4_slot_plan.h derives from
// (slot, n) -- inert where n needs fewer than the capacity reserved.  Walk entries never change.  A 4 MiB slot
// has 64 + 512 entries.  It clears what k_cq_items clears.
template <typename Item>
__global__ __launch_bounds__(256) void k_cq_plan(const uint64_t* __restrict__ src, const uint32_t* __restrict__ srcSizes,
                                                 uint32_t count, const Slot* __restrict__ slots, Block* __restrict__ blocks,
                                                 Segment* __restrict__ segs, DpSeg* __restrict__ dp, Item* __restrict__ items,
                                                 uint32_t* __restrict__ status, int* __restrict__ pipeStatus,
                                                 uint32_t* __restrict__ longFlag, uint32_t* __restrict__ ivCount)
{
  const uint32_t lane = threadIdx.x & 63, i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    *pipeStatus = 0;
    ivCount[count] = 0;
  }
  if (i >= count) return;
  const Slot s = slots[i];
  const uint32_t want = srcSizes[i];
  uint32_t st = kItemOk, n = want;
  uint64_t p = 0;
  if (want > s.cap) {
    st = kItemCapacity;
    n = 0;
  } else if (want) {
    p = src[i];
    if (!p) st = kItemArg;
  }
  if (lane == 0) {
    items[i].src = p;
    items[i].size = p ? (decltype(items[i].size))n : 0;
    blocks[i] = slot_block(s, n);
    longFlag[i] = 0;
    status[i] = st;
  }
  for (uint32_t j = lane; j < s.segCount; j += 64) segs[s.segFirst + j] = slot_segment(s, i, j, n);
  for (uint32_t j = lane; j < s.dpCount; j += 64) dp[s.dpFirst + j] = slot_dp(i, j, n);
}

// zeroes `words` 16-byte words at p (the pass-2 marker bits, which the finders OR into)
__global__ __launch_bounds__(256) void k_cq_zero(uint4* __restrict__ p, uint64_t words)
{
  for (uint64_t w = (uint64_t)blockIdx.x * 256 + threadIdx.x; w < words; w += (uint64_t)gridDim.x * 256)
    p[w] = make_uint4(0u, 0u, 0u, 0u);
}

// A grid-stride loop over the caller's items: block b lies at out + offsets[b] and is blockBytes[b] long (top
// bit: stored); an empty item gets the address where the next block starts (offsets[nblocks] is the body's
// size) and size 0.  A run whose capacity invariant failed has no valid block: every item is kItemInternal
// with size 0 at `out`, and the total is 0.
__global__ __launch_bounds__(256) void k_cq_finish(const uint32_t* __restrict__ map, uint32_t count, uint32_t nblocks,
                                                   const uint32_t* __restrict__ blockBytes,
                                                   const uint64_t* __restrict__ offsets, const int* __restrict__ pipeStatus,
                                                   uint8_t* out, uint64_t* __restrict__ blockPtrs,
                                                   uint32_t* __restrict__ blockSizes, uint32_t* __restrict__ status,
                                                   uint64_t* __restrict__ total)
{
  const bool bad = (*pipeStatus & kStInvariant) != 0;
  for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < count; i += gridDim.x * 256) {
    const uint32_t m = map ? map[i] : i, b = m & ~kCqEmpty;
    blockPtrs[i] = reinterpret_cast<uint64_t>(out) + (bad ? 0 : offsets[b]);
    blockSizes[i] = bad || (m & kCqEmpty) ? 0u : blockBytes[b] & 0x7FFFFFFFu;
    if (bad) status[i] = kItemInternal;
  }
  if (total && blockIdx.x == 0 && threadIdx.x == 0) *total = bad ? 0 : offsets[nblocks];
}

}  // namespace

void launch_cq_items(const CqTables& T, const PipeArgs& P, void* items, bool typed, hipStream_t s)
{
  const dim3 grid((T.count + 255) / 256), block(256);
  if (typed)
    hipLaunchKernelGGL(k_cq_items<BatchTyped>, grid, block, 0, s, T.src, T.map, T.count, P.nblocks, P.blocks,
                       static_cast<BatchTyped*>(items), T.status, P.status, P.longFlag, P.ivCount, P.offsets);
  else
    hipLaunchKernelGGL(k_cq_items<BatchItem>, grid, block, 0, s, T.src, T.map, T.count, P.nblocks, P.blocks,
                       static_cast<BatchItem*>(items), T.status, P.status, P.longFlag, P.ivCount, P.offsets);
}

void launch_cq_plan(const CqTables& T, const uint32_t* srcSizes, const Slot* slots, const PipeArgs& P, void* items, bool typed,
                    hipStream_t s)
{
  // the plan tables are the queue's own (held) buffers: PipeArgs names them const for the pipeline's kernels
  Block* blocks = const_cast<Block*>(P.blocks);
  Segment* segs = const_cast<Segment*>(P.segs);
  DpSeg* dp = const_cast<DpSeg*>(P.dpSegs);
  const dim3 grid((T.count + 3) / 4), block(256);
  if (typed)
    hipLaunchKernelGGL(k_cq_plan<BatchTyped>, grid, block, 0, s, T.src, srcSizes, T.count, slots, blocks, segs, dp,
                       static_cast<BatchTyped*>(items), T.status, P.status, P.longFlag, P.ivCount);
  else
    hipLaunchKernelGGL(k_cq_plan<BatchItem>, grid, block, 0, s, T.src, srcSizes, T.count, slots, blocks, segs, dp,
                       static_cast<BatchItem*>(items), T.status, P.status, P.longFlag, P.ivCount);
}

void launch_cq_zero(void* p, uint64_t bytes, hipStream_t s)
{
  const uint64_t words = (bytes + 15) / 16, groups = (words + 255) / 256;
  if (words)
    hipLaunchKernelGGL(k_cq_zero, dim3((uint32_t)(groups < kGatherGrid ? groups : kGatherGrid)), dim3(256), 0, s,
                       static_cast<uint4*>(p), words);
}

void launch_cq_finish(const CqTables& T, const PipeArgs& P, hipStream_t s)
{
  const uint32_t groups = (T.count + 255) / 256;
  hipLaunchKernelGGL(k_cq_finish, dim3(groups < kGatherGrid ? groups : kGatherGrid), dim3(256), 0, s, T.map, T.count, P.nblocks,
                     P.blockBytes, P.offsets, P.status, T.out, T.blockPtrs, T.blockSizes, T.status, T.total);
}

void launch_batch_gather(const BatchItem* items, uint32_t n, uint8_t* staged, uint64_t stagedBytes, hipStream_t s)
{
  const uint64_t words = stagedBytes / 16;
  if (!n || !words) return;
  const uint64_t tiles = (words + kGatherTile - 1) / kGatherTile;
  hipLaunchKernelGGL(k_batch_gather, dim3((uint32_t)(tiles < kGatherGrid ? tiles : kGatherGrid)), dim3(kGatherThreads), 0, s,
                     items, n, staged, words);
}

void launch_batch_gather_planes(const BatchTyped* items, uint32_t n, uint8_t* staged, uint64_t stagedBytes, hipStream_t s)
{
  const uint64_t words = stagedBytes / 16;
  if (!n || !words) return;
  const uint64_t tiles = (words + kGatherTile - 1) / kGatherTile;
  hipLaunchKernelGGL(k_batch_gather_planes, dim3((uint32_t)(tiles < kGatherGrid ? tiles : kGatherGrid)), dim3(kGatherThreads), 0,
                     s, items, n, staged, words);
}

void launch_batch_gather_bits(const BatchTyped* items, uint32_t n, uint8_t* staged, uint64_t stagedBytes, hipStream_t s)
{
  static_assert(kFilterShift == kBatchFilterShift, "the host's encoding of BatchTyped::elem");
  const uint64_t words = stagedBytes / 16;
  if (!n || !words) return;
  const uint64_t tiles = (words + kGatherTile - 1) / kGatherTile;
  hipLaunchKernelGGL(k_batch_gather_bits, dim3((uint32_t)(tiles < kGatherGrid ? tiles : kGatherGrid)), dim3(kGatherThreads), 0,
                     s, items, n, staged, words);
}

void launch_batch_merge(const BatchTyped* items, uint32_t n, const uint8_t* from, uint8_t* to, uint64_t total, hipStream_t s)
{
  if (!n || !total) return;
  const uint64_t words = ((reinterpret_cast<uintptr_t>(to) & 15u) + total + 15) / 16;
  const uint64_t tiles = (words + kGatherTile - 1) / kGatherTile;
  hipLaunchKernelGGL(k_batch_merge, dim3((uint32_t)(tiles < kGatherGrid ? tiles : kGatherGrid)), dim3(kGatherThreads), 0, s,
                     items, n, from, to, total, words);
}

void launch_batch_merge_bits(const BatchTyped* items, uint32_t n, const uint8_t* from, uint8_t* to, uint64_t total, hipStream_t s)
{
  if (!n || !total) return;
  const uint64_t words = ((reinterpret_cast<uintptr_t>(to) & 15u) + total + 15) / 16;
  const uint64_t tiles = (words + kGatherTile - 1) / kGatherTile;
  hipLaunchKernelGGL(k_batch_merge_bits, dim3((uint32_t)(tiles < kGatherGrid ? tiles : kGatherGrid)), dim3(kGatherThreads), 0, s,
                     items, n, from, to, total, words);
}

void launch_batch_move(const BatchMove* moves, uint32_t n, const uint8_t* from, uint8_t* to, hipStream_t s)
{
  if (n) hipLaunchKernelGGL(k_batch_move, dim3(n), dim3(256), 0, s, moves, from, to);
}

}  // namespace sz4
