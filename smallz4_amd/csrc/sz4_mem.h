// sz4_mem.h -- the host driver's memory holders: device scratch with its accounting (Budget, DevBuf),
// pinned host buffers (HostBuf) and the device guard of a call.  Used by sz4_host.cpp only.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

namespace sz4 {

// Device scratch accounting of one context: the bytes it holds, an optional limit, and a call counter.
// A buffer records the call that last reserved it; buffers of earlier calls (another kind of call: the
// stream path's staging, dictionary tables, decoder images) are the ones a growing call may release.
struct DevBuf;
struct Budget {
  uint64_t used = 0;   // bytes held by the context's DevBufs
  uint64_t limit = 0;  // 0: none (sz4_set_device_limit)
  uint64_t gen = 1;    // the current call
  std::vector<DevBuf*> bufs;  // every DevBuf constructed on this budget, in construction order
  uint64_t shedCount = 0;  // buffers released by shed()
  void (*onShed)(void*) = nullptr;
  void* owner = nullptr;
  inline uint64_t shed();  // releases every buffer the current call has not reserved; returns the bytes freed
  // Test hooks, read once by sz4_create and inert at 0: they make a growth fail as an
  // allocator's out-of-memory would, and change no size, plan or launch.  testAllocCap: a growth that would
  // take `used` above it fails; testFailReserve: the growth with this number (counted from 1) fails, once.
  uint64_t testAllocCap = 0;
  uint64_t testFailReserve = 0;
  uint64_t testFreeBytes = 0;  // the free device memory the batch piece sizing is to assume (it alone reads this)
  uint64_t growths = 0;  // growths that reached the allocator since the budget was created
  uint64_t injected = 0;  // ... of them, the ones whose first attempt a hook failed
  // the allocator as a growth sees it; `inject`: this growth is testFailReserve's (all its attempts fail)
  hipError_t alloc(void** p, size_t bytes, bool inject)
  {
    if (inject || (testAllocCap && used + bytes > testAllocCap)) return hipErrorOutOfMemory;
    return hipMalloc(p, bytes);
  }
};

// A grow-only device buffer.  It belongs to the budget it is constructed on and enters that budget's list
// itself, so accounting, shedding, trim and destroy see every buffer that exists; it stays where it was
// constructed (the list holds its address) and must not outlive the budget's owner.
struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  Budget& bud;
  uint64_t lastGen = 0;
  // held: a buffer whose address something outside the context's calls keeps (a decode queue's scratch, which
  // a captured graph names): counted and bounded like any other, but neither shed() nor sz4_trim releases it
  bool held = false;
  explicit DevBuf(Budget& b, bool keep = false) : bud(b), held(keep) { b.bufs.push_back(this); }
  // a buffer that ends before its budget's owner does leaves the list (decode queues; the context's own never do)
  void detach()
  {
    release();
    bud.bufs.erase(std::remove(bud.bufs.begin(), bud.bufs.end(), this), bud.bufs.end());
  }
  DevBuf(const DevBuf&) = delete;  // neither copied nor moved
  DevBuf& operator=(const DevBuf&) = delete;
  hipError_t reserve(size_t bytes)
  {
    lastGen = bud.gen;
    if (bytes <= cap) return hipSuccess;
    size_t want = bytes + bytes / 32 + 4096;  // slack: a slightly larger next call does not reallocate
    if (bud.limit) {
      if (bud.used - cap + want > bud.limit) want = bytes;
      if (bud.used - cap + want > bud.limit) bud.shed();
      if (bud.used - cap + want > bud.limit) {
        release();  // a failed reserve leaves the buffer empty, whichever branch failed
        return hipErrorOutOfMemory;
      }
    }
    release();
    const bool inject = ++bud.growths == bud.testFailReserve;
    if (inject || (bud.testAllocCap && bud.used + want > bud.testAllocCap)) bud.injected++;
    hipError_t e = bud.alloc(&p, want, inject);
    if (e == hipErrorOutOfMemory && bud.shed()) {
      (void)hipGetLastError();
      e = bud.alloc(&p, want, inject);
    }
    if (e == hipSuccess) {
      cap = want;
      bud.used += want;
    } else {
      p = nullptr;
      (void)hipGetLastError();  // the failure is returned, not left sticky for the next runtime call
    }
    return e;
  }
  void release()
  {
    if (p) hipFree(p);
    bud.used -= cap;
    p = nullptr;
    cap = 0;
  }
  // the context could grow this buffer to `bytes` without releasing any other buffer
  bool fits(size_t bytes) const { return bytes <= cap || !bud.limit || bud.used - cap + bytes <= bud.limit; }
  template <class T>
  T* as() const { return static_cast<T*>(p); }
};

inline uint64_t Budget::shed()
{
  uint64_t freed = 0;
  for (DevBuf* b : bufs)
    if (b->p && b->lastGen != gen && !b->held) {
      freed += b->cap;
      b->release();
      shedCount++;
    }
  if (freed && onShed) onShed(owner);
  return freed;
}

// pinned host memory (the stream path's chunk buffers), grow-only
struct HostBuf {
  void* p = nullptr;
  size_t cap = 0;
  hipError_t reserve(size_t bytes)
  {
    if (bytes <= cap) return hipSuccess;
    if (p) hipHostFree(p);
    p = nullptr;
    cap = 0;
    hipError_t e = hipHostMalloc(&p, bytes, hipHostMallocDefault);
    if (e == hipSuccess) cap = bytes;
    return e;
  }
  void release()
  {
    if (p) hipHostFree(p);
    p = nullptr;
    cap = 0;
  }
  template <class T>
  T* as() const { return static_cast<T*>(p); }
};

// makes the context's device current for the duration of a call and restores the caller's
struct DeviceGuard {
  int saved = -1;
  explicit DeviceGuard(int device)
  {
    if (hipGetDevice(&saved) != hipSuccess) saved = -1;
    if (saved != device) hipSetDevice(device);
  }
  ~DeviceGuard()
  {
    int now = -1;
    if (saved >= 0 && hipGetDevice(&now) == hipSuccess && now != saved) hipSetDevice(saved);
  }
};

}  // namespace sz4
