// sz4_device.h -- small device helpers shared by the gfx950 kernel files.  Not part of the public ABI.
#pragma once
#include <stdint.h>

#include <hip/hip_runtime.h>

#include "sz4_internal.h"

namespace sz4 {

// getHash32 (smallz4.h:163-168)
__device__ __forceinline__ uint32_t ref_hash(uint32_t four)
{
  return ((four * kHashMul) >> (32 - kHashBits)) & ((1u << kHashBits) - 1);
}

// four bytes at any offset of a buffer whose allocation is padded by >= 8 bytes and 4-aligned
__device__ __forceinline__ uint32_t gload4(const uint8_t* base, uint64_t off)
{
  const uint32_t* w = reinterpret_cast<const uint32_t*>(base + (off & ~3ull));
  const uint32_t lo = w[0], hi = w[1];
  return __builtin_amdgcn_alignbyte(hi, lo, (uint32_t)(off & 3));
}

__device__ __forceinline__ uint32_t lane_id() { return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); }

// value of a lane chosen by a wave-uniform index (v_readlane: no LDS round trip)
__device__ __forceinline__ uint32_t rdlane(uint32_t v, uint32_t lane)
{
  return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)lane);
}

template <int kCtrl>
__device__ __forceinline__ uint32_t dpp(uint32_t v)
{
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, kCtrl, 0xF, 0xF, false);
}
constexpr int kQuadSwap1 = 0xB1;      // quad_perm [1,0,3,2]
constexpr int kQuadSwap2 = 0x4E;      // quad_perm [2,3,0,1]
constexpr int kRowHalfMirror = 0x141;
constexpr int kRowMirror = 0x140;
constexpr int kRowShr = 0x110;        // + n
constexpr int kWaveShr1 = 0x138;      // wave_shr:1 (whole 64-lane wavefront)
constexpr int kRowBcast15 = 0x142;    // lane 15 of each row to the next row
constexpr int kRowBcast31 = 0x143;    // lane 31 to rows 2 and 3

// every lane receives the min / max / sum of its 16-lane row
__device__ __forceinline__ uint32_t row_min(uint32_t v)
{
  v = min(v, dpp<kQuadSwap1>(v));
  v = min(v, dpp<kQuadSwap2>(v));
  v = min(v, dpp<kRowHalfMirror>(v));
  v = min(v, dpp<kRowMirror>(v));
  return v;
}
__device__ __forceinline__ uint32_t row_max(uint32_t v)
{
  v = max(v, dpp<kQuadSwap1>(v));
  v = max(v, dpp<kQuadSwap2>(v));
  v = max(v, dpp<kRowHalfMirror>(v));
  v = max(v, dpp<kRowMirror>(v));
  return v;
}
__device__ __forceinline__ uint32_t row_sum(uint32_t v)
{
  v += dpp<kQuadSwap1>(v);
  v += dpp<kQuadSwap2>(v);
  v += dpp<kRowHalfMirror>(v);
  v += dpp<kRowMirror>(v);
  return v;
}

// inclusive wavefront scans by DPP: row shifts 1, 2, 4, 8, then lane 15 of each row into the next row and
// lane 31 into rows 2-3, lanes without a source taking the identity (0 for + and unsigned max) -- six
// dependent VALU steps instead of six ds_bpermute round trips
__device__ __forceinline__ uint32_t wave_incl_scan_add(uint32_t v)
{
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, kRowShr + 1, 0xF, 0xF, false);
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, kRowShr + 2, 0xF, 0xF, false);
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, kRowShr + 4, 0xF, 0xF, false);
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, kRowShr + 8, 0xF, 0xF, false);
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, kRowBcast15, 0xA, 0xF, false);
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, kRowBcast31, 0xC, 0xF, false);
  return v;
}

__device__ __forceinline__ uint32_t wave_incl_scan_max(uint32_t v)
{
  v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, kRowShr + 1, 0xF, 0xF, false));
  v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, kRowShr + 2, 0xF, 0xF, false));
  v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, kRowShr + 4, 0xF, 0xF, false));
  v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, kRowShr + 8, 0xF, 0xF, false));
  v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, kRowBcast15, 0xA, 0xF, false));
  v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, kRowBcast31, 0xC, 0xF, false));
  return v;
}

// The path through a 64-position window.  Lane l's successor is succ (a lane above l, or 64 when the step
// from l leaves the window); the path starts at the wave-uniform lane `entry` and follows the successors.
// Every lane at or above `entry` receives the last path position at or below itself, so the lanes that
// receive their own index are the path and lane 63 holds its last position.  A lane below `entry` receives
// `entry`, which is above it: it never finds itself.  F[k] is the 2^k-th successor by doubling (five
// ds_bpermute), then binary lifting from the entry: take the 32-step, 16-step .. 1-step jump whenever it
// does not pass the lane (five more).
__device__ __forceinline__ uint32_t wave_path(uint32_t succ, uint32_t entry, uint32_t lane)
{
  uint32_t F[6];
  F[0] = succ;
#pragma unroll
  for (int k = 1; k < 6; k++) {
    const uint32_t g = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(F[k - 1] << 2), (int)F[k - 1]);
    F[k] = F[k - 1] >= 64u ? 64u : g;
  }
  uint32_t x = entry;
  {
    const uint32_t y = rdlane(F[5], entry);
    x = y <= lane ? y : x;
  }
#pragma unroll
  for (int k = 4; k >= 0; k--) {
    const uint32_t y = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(x << 2), (int)F[k]);
    x = y <= lane ? y : x;
  }
  return x;
}

}  // namespace sz4
