// typed_map_check -- the decode queue's position map (smallz4_amd/csrc/sz4_typed_map.h) on the CPU, as plain
// C++ under the sanitizers.  For every width E in 1, 2, 4, 8 and every item length n in 0..71 and 4093..4100
// it checks that x -> typed_map(x, n / E, E) is a permutation of [0, n), in the 32-bit form the kernels use
// and in the 64-bit one, and prints the map, one line "E n: a0 a1 ..." per case, for
// tests/test_decode_queue_model.py to hold against planes.merge.  Ends with "typed_map_check ok".
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../../smallz4_amd/csrc/sz4_typed_map.h"

int main()
{
  const uint32_t widths[4] = {1, 2, 4, 8};
  std::vector<uint32_t> lengths;
  for (uint32_t n = 0; n <= 71; n++) lengths.push_back(n);
  for (uint32_t n = 4093; n <= 4100; n++) lengths.push_back(n);
  int bad = 0;
  for (uint32_t E : widths)
    for (uint32_t n : lengths) {
      const uint32_t m = n / E;
      std::vector<uint8_t> hit(n, 0);
      printf("%u %u:", E, n);
      for (uint32_t x = 0; x < n; x++) {
        const uint32_t a = sz4::typed_map<uint32_t>(x, m, E);
        const uint64_t b = sz4::typed_map<uint64_t>(x, m, E);
        printf(" %u", a);
        if (b != a) {
          fprintf(stderr, "E %u n %u x %u: %u in 32 bits, %llu in 64\n", E, n, x, a, (unsigned long long)b);
          bad++;
        }
        if (a >= n || hit[a]) {
          fprintf(stderr, "E %u n %u x %u: address %u is %s\n", E, n, x, a, a >= n ? "outside the item" : "taken twice");
          bad++;
        } else {
          hit[a] = 1;
        }
      }
      printf("\n");
    }
  // beyond 32 bits: the 64-bit form alone, at the edges of a 5 GiB item's planes
  const uint64_t big = (5ull << 30) + 3, bm = big / 8;
  for (uint64_t k = 0; k < 8; k++) {
    if (sz4::typed_map<uint64_t>(k * bm, bm, 8) != k || sz4::typed_map<uint64_t>(k * bm + bm - 1, bm, 8) != (bm - 1) * 8 + k) {
      fprintf(stderr, "plane %llu of a 5 GiB item\n", (unsigned long long)k);
      bad++;
    }
  }
  if (sz4::typed_map<uint64_t>(8 * bm + 2, bm, 8) != 8 * bm + 2) bad++;
  if (bad) return 1;
  printf("typed_map_check ok\n");
  return 0;
}
