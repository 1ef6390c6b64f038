// match_rec_check.cpp -- the token walk's 8-byte match record and the size of a sequence
// (smallz4_amd/csrc/sz4_match_rec.h) checked on the CPU: every field comes back from the packed word at the
// edges of its range, and token_bytes equals a naive LZ4 sequence encoder that counts the bytes it would
// write one by one.  Stand-alone: includes the header alone, makes no HIP call, runs without a GPU
// (tests/test_match_rec_host.py builds it with the address and undefined-behaviour sanitizers).  Exit status
// 1 and one line per failed check on a mismatch.
#include <stdio.h>

#include <vector>

#include "../../smallz4_amd/csrc/sz4_match_rec.h"

using namespace sz4;

static int g_failed = 0;
#define CHECK(cond, ...)                                             \
  do {                                                               \
    if (!(cond)) {                                                   \
      if (g_failed++ < 50) {                                         \
        printf("FAILED %s:%d %s  ", __FILE__, __LINE__, #cond);      \
        printf(__VA_ARGS__);                                         \
        printf("\n");                                                \
      }                                                              \
    }                                                                \
  } while (0)

// the bytes of one sequence as an encoder writes them (LZ4 block format: token, literal length bytes while the
// rest is >= 255 and one more, the literals, then -- unless this is the closing literal run -- two distance
// bytes and the match length bytes by the same rule, the length stored less MinMatch = 4)
static uint64_t naive_bytes(uint64_t lits, uint32_t mlen, bool last)
{
  uint64_t out = 0;  // bytes written so far
  const uint64_t mcode = last ? 0 : (uint64_t)mlen - 4;
  out++;  // the token: min(lits, 15) << 4 | min(mcode, 15)
  if (lits >= 15) {
    uint64_t v = lits - 15;
    while (v >= 255) {
      out++;  // 255
      v -= 255;
    }
    out++;  // v
  }
  for (uint64_t i = 0; i < lits; i++) out++;  // a literal
  if (!last) {
    out += 2;  // the distance, little endian
    if (mcode >= 15) {
      uint64_t v = mcode - 15;
      while (v >= 255) {
        out++;
        v -= 255;
      }
      out++;
    }
  }
  return out;
}

static void check_bytes(uint64_t lits, uint32_t mlen)
{
  CHECK(token_bytes(lits, mlen, false) == naive_bytes(lits, mlen, false), "lits %llu mlen %u", (unsigned long long)lits, mlen);
  CHECK(token_bytes(lits, mlen, true) == naive_bytes(lits, mlen, true), "lits %llu mlen %u last", (unsigned long long)lits, mlen);
  // the closing literal run carries no match, whatever length is passed
  CHECK(token_bytes(lits, 0, true) == naive_bytes(lits, 0, true), "lits %llu last, no match", (unsigned long long)lits);
}

int main()
{
  // pack / unpack round trip
  const uint32_t poss[] = {0, 1, (1u << 23) - 1};
  const uint32_t lens[] = {4, 18, 19, 20, 273, 274, 65535, 65536, (1u << 23) - 1};
  const uint32_t dists[] = {1, 65535};
  for (uint32_t pos : poss)
    for (uint32_t len : lens)
      for (uint32_t dist : dists) {
        const uint64_t r = mrec_pack(pos, len, dist);
        CHECK(mrec_pos(r) == pos && mrec_len(r) == len && mrec_dist(r) == dist, "pos %u len %u dist %u -> %016llx", pos, len,
              dist, (unsigned long long)r);
        CHECK(mrec_end(r) == pos + len, "pos %u len %u", pos, len);
      }
  CHECK(kRecPosBits + kRecLenBits + kRecDistBits == 64, "field widths");
  // records of one block order by position first only through mrec_pos: two records differ when any field does
  CHECK(mrec_pack(5, 4, 1) != mrec_pack(5, 4, 2) && mrec_pack(5, 4, 1) != mrec_pack(5, 5, 1) &&
            mrec_pack(5, 4, 1) != mrec_pack(6, 4, 1),
        "distinct");

  // token_bytes against the naive encoder
  for (uint64_t lits = 0; lits <= 600; lits++)
    for (uint32_t mlen = 4; mlen <= 600; mlen++) {
      CHECK(token_bytes(lits, mlen, false) == naive_bytes(lits, mlen, false), "lits %llu mlen %u", (unsigned long long)lits, mlen);
      CHECK(token_bytes(lits, mlen, true) == naive_bytes(lits, mlen, true), "lits %llu mlen %u last", (unsigned long long)lits,
            mlen);
    }
  // the edges of the length codes: 14, 15, 16 and 15 + 255 k - 1, + 0, + 1, for the literal count and for the
  // match code (match length less 4)
  std::vector<uint64_t> edges = {14, 15, 16};
  for (uint64_t k = 1; k <= 300; k++)
    for (int d = -1; d <= 1; d++) edges.push_back(15 + 255 * k + d);
  for (uint64_t e : edges) {
    for (uint32_t mlen : {4u, 18u, 19u, 20u, 273u, 274u}) check_bytes(e, mlen);
    for (uint64_t lits : {0ull, 14ull, 15ull, 16ull, 269ull, 270ull, 271ull}) check_bytes(lits, (uint32_t)e + 4);
  }
  // every pair of edges up to 15 + 255 * 4 + 1
  for (uint64_t a : edges)
    for (uint64_t b : edges)
      if (a <= 15 + 255 * 4 + 1 && b <= 15 + 255 * 4 + 1) check_bytes(a, (uint32_t)b + 4);

  if (g_failed) {
    printf("match_rec_check: %d checks failed\n", g_failed);
    return 1;
  }
  printf("match_rec_check ok\n");
  return 0;
}
