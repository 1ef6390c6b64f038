// sz4_typed_map.h -- where a byte of a typed item's split lands in the item itself: the byte-plane merge
// (include/smallz4_amd.h, smallz4_amd/planes.py) as a map of positions.  The decode queue's decoders store
// and re-read every output byte through it, so a typed item needs neither a staging buffer nor a merge pass.
// Plain C++ as well as HIP: tests/cpp/typed_map_check.cpp checks it on the CPU.
#pragma once
#include <stdint.h>

#ifdef __HIP__
#define SZ4_HOST_DEVICE __host__ __device__
#else
#define SZ4_HOST_DEVICE
#endif

namespace sz4 {

// An item of n bytes and element width E (1, 2, 4 or 8) has m = n / E whole elements.  Position x of its
// split (plane k = x / m, element e = x mod m) is byte e * E + k of the item; the n mod E tail bytes from
// E * m on keep their place.  E = 1 and m = 0 (n < E) are the identity.  The plane comes from at most three
// compares against multiples of m -- E is a power of two -- instead of a division, and with m and E uniform
// across a wavefront (one item per wavefront) every product below is scalar work: a lane pays a compare and
// two selects per step, then a shift.  U: uint32_t on the device (an item decodes to less than 4 GiB, and
// every product is at most n), uint64_t elsewhere.
template <class U>
SZ4_HOST_DEVICE inline U typed_map(U x, U m, uint32_t E)
{
  if (E <= 1u || x >= (U)E * m) return x;
  U k = 0, base = 0;  // the plane and its first position, k * m
  uint32_t shift = 0;  // log2 E
  for (uint32_t h = E >> 1; h; h >>= 1, shift++) {
    const U step = m * (U)h;
    if (x >= base + step) {
      base += step;
      k += (U)h;
    }
  }
  return ((x - base) << shift) + k;
}

}  // namespace sz4
