// A stand-in for <hip/hip_runtime.h> with the few calls smallz4_amd/csrc/sz4_mem.h makes, backed by malloc:
// tests/cpp/mem_check.cpp puts this directory first on its include path and links no HIP library.  The
// "device" has a settable capacity; an allocation past it fails with hipErrorOutOfMemory.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

#include <unordered_map>

typedef enum { hipSuccess = 0, hipErrorInvalidValue = 1, hipErrorOutOfMemory = 2 } hipError_t;
enum { hipHostMallocDefault = 0 };

namespace fakehip {
struct State {
  uint64_t capacity = 0;  // 0: none
  uint64_t inUse = 0;
  uint64_t mallocs = 0, failed = 0, frees = 0;  // hipMalloc calls, the ones that failed, hipFree calls
  std::unordered_map<void*, uint64_t> live;     // device allocations and their sizes
  uint64_t hostLive = 0;
  int device = 0;
  hipError_t last = hipSuccess;
};
inline State& state()
{
  static State s;
  return s;
}
}  // namespace fakehip

inline hipError_t hipMalloc(void** p, size_t bytes)
{
  fakehip::State& s = fakehip::state();
  s.mallocs++;
  if (s.capacity && s.inUse + bytes > s.capacity) {
    s.failed++;
    return s.last = hipErrorOutOfMemory;
  }
  *p = malloc(bytes ? bytes : 1);
  if (!*p) return s.last = hipErrorOutOfMemory;
  s.live[*p] = bytes;
  s.inUse += bytes;
  return hipSuccess;
}

inline hipError_t hipFree(void* p)
{
  fakehip::State& s = fakehip::state();
  s.frees++;
  auto it = s.live.find(p);
  if (it == s.live.end()) return s.last = hipErrorInvalidValue;  // not a live device allocation (or freed twice)
  s.inUse -= it->second;
  s.live.erase(it);
  free(p);
  return hipSuccess;
}

inline hipError_t hipGetLastError()
{
  fakehip::State& s = fakehip::state();
  const hipError_t e = s.last;
  s.last = hipSuccess;
  return e;
}

inline hipError_t hipHostMalloc(void** p, size_t bytes, unsigned)
{
  *p = malloc(bytes ? bytes : 1);
  if (!*p) return hipErrorOutOfMemory;
  fakehip::state().hostLive++;
  return hipSuccess;
}

inline hipError_t hipHostFree(void* p)
{
  fakehip::state().hostLive--;
  free(p);
  return hipSuccess;
}

inline hipError_t hipGetDevice(int* d)
{
  *d = fakehip::state().device;
  return hipSuccess;
}

inline hipError_t hipSetDevice(int d)
{
  fakehip::state().device = d;
  return hipSuccess;
}
