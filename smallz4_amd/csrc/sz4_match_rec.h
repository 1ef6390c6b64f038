// sz4_match_rec.h -- one match of the token walk as the emit kernels pass it on, and the encoded size of a
// sequence.  The walk (k_walk, k_walk_fix_*) records every match of the path as ONE 8-byte word: its
// block-relative position, its length and its distance.  A sub-segment's final matches are contiguous in its
// slots, so the sizes pass and the frame writer read them coalesced and derive each literal run from the end
// of the match before; nothing is gathered again from the per-position arrays.
//
//   bits  0 .. 23   position in the block   (< 2^23: an 8 MiB legacy block is the largest)
//   bits 24 .. 47   match length            (<= the block size)
//   bits 48 .. 63   distance                (1 .. 65535)
//
// Host and device compute the same values; as host code the header needs nothing of HIP
// (tests/cpp/match_rec_check.cpp).
#pragma once
#include <stdint.h>

#ifdef __HIP__
#define SZ4_REC_HD __host__ __device__
#else
#define SZ4_REC_HD
#endif

namespace sz4 {

constexpr uint32_t kRecPosBits = 24, kRecLenBits = 24, kRecDistBits = 16;
constexpr uint32_t kRecMask24 = (1u << 24) - 1u;

SZ4_REC_HD inline uint64_t mrec_pack(uint32_t pos, uint32_t len, uint32_t dist)
{
  return (uint64_t)(pos & kRecMask24) | ((uint64_t)(len & kRecMask24) << kRecPosBits) |
         ((uint64_t)(dist & 0xFFFFu) << (kRecPosBits + kRecLenBits));
}
SZ4_REC_HD inline uint32_t mrec_pos(uint64_t r) { return (uint32_t)r & kRecMask24; }
SZ4_REC_HD inline uint32_t mrec_len(uint64_t r) { return (uint32_t)(r >> kRecPosBits) & kRecMask24; }
SZ4_REC_HD inline uint32_t mrec_dist(uint64_t r) { return (uint32_t)(r >> (kRecPosBits + kRecLenBits)); }
SZ4_REC_HD inline uint32_t mrec_end(uint64_t r) { return mrec_pos(r) + mrec_len(r); }

// bytes of one sequence (smallz4.h:259-371): the token, the literal length's extra bytes, the literals, and --
// unless it is the block's closing literal run -- the distance and the match length's extra bytes
constexpr int kRecMinMatch = 4;  // MinMatch (kMinMatch of sz4_internal.h)
SZ4_REC_HD inline uint64_t token_bytes(uint64_t lits, uint32_t mlen, bool last)
{
  uint64_t b = 1 + lits + (lits >= 15 ? (lits - 15) / 255 + 1 : 0);
  if (!last) {
    const int64_t mcode = (int64_t)mlen - kRecMinMatch;
    b += 2 + (mcode >= 15 ? (uint64_t)(mcode - 15) / 255 + 1 : 0);
  }
  return b;
}

}  // namespace sz4
