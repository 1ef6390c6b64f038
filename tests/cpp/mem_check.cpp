// mem_check.cpp -- the device memory accounting of smallz4_amd/csrc/sz4_mem.h (Budget, DevBuf) on the CPU, against
// a plain model written beside it.  <hip/hip_runtime.h> is tests/cpp/fakehip's stand-in (malloc with a settable
// capacity), so this is host code alone: built with the address and undefined-behaviour sanitizers and run
// stand-alone by tests/test_mem_host.py.
//
// Seeded random sequences of reserve / release / shed / detach / next call over a dozen buffers, some of them
// held, run with and without a limit, with and without a device capacity, and with the two failure hooks; after
// every step every field of every buffer and of the budget is compared with the model's.
#include <stdio.h>
#include <stdlib.h>

#include <memory>
#include <random>
#include <vector>

#include "sz4_mem.h"

using namespace sz4;

namespace {

#define CHECK(x)                                                                  \
  do {                                                                            \
    if (!(x)) {                                                                   \
      printf("mem_check FAILED at line %d: %s  [%s, step %d]\n", __LINE__, #x, g_what, g_step); \
      exit(1);                                                                    \
    }                                                                             \
  } while (0)

const char* g_what = "";
int g_step = 0;
int g_onShed = 0;

struct Config {
  const char* name;
  uint64_t limit, capacity, allocCap, failReserve;
};

// the model: what the accounting is defined to do, in the plainest words
struct MBuf {
  uint64_t cap = 0, lastGen = 0;
  bool held = false;
};
struct Model {
  std::vector<MBuf> b;  // in the budget's list order
  uint64_t gen = 1, limit = 0, capacity = 0, allocCap = 0, failReserve = 0;
  uint64_t growths = 0, injected = 0, shedCount = 0, onShed = 0;
  uint64_t mallocs = 0;  // calls that reach the device allocator
  uint64_t used() const
  {
    uint64_t u = 0;
    for (const MBuf& x : b) u += x.cap;
    return u;
  }
  uint64_t shed()
  {
    uint64_t freed = 0;
    for (MBuf& x : b)
      if (x.cap && x.lastGen != gen && !x.held) {
        freed += x.cap;
        x.cap = 0;
        shedCount++;
      }
    if (freed) onShed++;
    return freed;
  }
  // one attempt at the allocator for `want` bytes beside what is held now
  bool attempt(uint64_t want, bool inject)
  {
    if (inject || (allocCap && used() + want > allocCap)) return false;  // a hook fails it: the device is not asked
    mallocs++;
    return !(capacity && used() + want > capacity);
  }
  // returns success; *grew: the call went to the allocator
  bool reserve(size_t i, uint64_t bytes)
  {
    MBuf& m = b[i];
    m.lastGen = gen;
    if (bytes <= m.cap) return true;
    const uint64_t full = bytes + bytes / 32 + 4096;
    uint64_t want = full;
    if (limit) {
      if (used() - m.cap + want > limit) want = bytes;  // the slack goes only when the limit forces it
      if (used() - m.cap + want > limit) shed();
      if (used() - m.cap + want > limit) {
        m.cap = 0;
        return false;
      }
    }
    m.cap = 0;
    const bool inject = ++growths == failReserve;
    if (inject || (allocCap && used() + want > allocCap)) injected++;
    bool ok = attempt(want, inject);
    if (!ok && shed()) ok = attempt(want, inject);  // exactly one shed and one more try
    if (ok) m.cap = want;
    return ok;
  }
};

void on_shed(void* owner) { ++*static_cast<int*>(owner); }

void run(const Config& cfg, uint32_t seed)
{
  g_what = cfg.name;
  fakehip::State& dev = fakehip::state();
  CHECK(dev.inUse == 0 && dev.live.empty());
  dev.capacity = cfg.capacity;
  const uint64_t mallocs0 = dev.mallocs;
  std::mt19937 rng(seed);
  auto pick = [&](uint64_t n) { return (uint64_t)(rng() % n); };

  Budget bud;
  bud.limit = cfg.limit;
  bud.testAllocCap = cfg.allocCap;
  bud.testFailReserve = cfg.failReserve;
  bud.onShed = on_shed;
  bud.owner = &g_onShed;
  g_onShed = 0;
  Model M;
  M.limit = cfg.limit;
  M.capacity = cfg.capacity;
  M.allocCap = cfg.allocCap;
  M.failReserve = cfg.failReserve;

  const size_t kBufs = 12;
  std::vector<std::unique_ptr<DevBuf>> real;  // real[i] is M.b[i]: both follow the budget's list order
  for (size_t i = 0; i < kBufs; i++) {
    const bool held = i % 4 == 3;
    real.emplace_back(new DevBuf(bud, held));
    M.b.push_back(MBuf{0, 0, held});
  }

  auto compare = [&]() {
    CHECK(bud.bufs.size() == real.size() && M.b.size() == real.size());
    uint64_t sum = 0, liveBufs = 0;
    for (size_t i = 0; i < real.size(); i++) {
      const DevBuf& r = *real[i];
      CHECK(bud.bufs[i] == &r);
      CHECK(r.cap == M.b[i].cap);
      CHECK((r.p == nullptr) == (r.cap == 0));
      CHECK(r.lastGen == M.b[i].lastGen);
      CHECK(r.held == M.b[i].held);
      if (r.p) {
        auto it = dev.live.find(r.p);
        CHECK(it != dev.live.end() && it->second == r.cap);
        liveBufs++;
      }
      sum += r.cap;
    }
    CHECK(bud.used == sum);
    CHECK(dev.inUse == sum && dev.live.size() == liveBufs);  // nothing leaked, nothing freed twice
    CHECK(bud.gen == M.gen);
    CHECK(bud.shedCount == M.shedCount);
    CHECK((uint64_t)g_onShed == M.onShed);
    CHECK(bud.growths == M.growths && bud.injected == M.injected);
    CHECK(dev.mallocs - mallocs0 == M.mallocs);
    CHECK(hipGetLastError() == hipSuccess);  // a failure is returned, never left sticky
  };

  const int kSteps = 1500;
  for (g_step = 0; g_step < kSteps; g_step++) {
    const uint64_t op = pick(100);
    const size_t i = (size_t)pick(real.size());
    if (op < 62) {
      // sizes around what is held: below the capacity, just above it, far above it, and sometimes huge
      const uint64_t have = real[i]->cap;
      uint64_t bytes;
      switch (pick(5)) {
        case 0: bytes = have ? pick(have + 1) : 0; break;
        case 1: bytes = have + 1 + pick(64); break;
        case 2: bytes = 1 + pick(1 << 16); break;
        case 3: bytes = 1 + pick(1 << 20); break;
        default: bytes = 1 + pick(6 << 20); break;
      }
      const uint64_t usedBefore = bud.used, capBefore = real[i]->cap, mallocsBefore = dev.mallocs;
      const uint64_t shedBefore = M.onShed;
      void* const pBefore = real[i]->p;
      const bool expect = M.reserve(i, bytes);
      const hipError_t e = real[i]->reserve((size_t)bytes);
      CHECK((e == hipSuccess) == expect);
      CHECK(e == hipSuccess || e == hipErrorOutOfMemory);
      if (bytes <= capBefore) {  // a reserve of at most the capacity allocates nothing and moves nothing
        CHECK(dev.mallocs == mallocsBefore && real[i]->p == pBefore && real[i]->cap == capBefore && bud.used == usedBefore);
      } else if (e == hipSuccess) {
        const uint64_t full = bytes + bytes / 32 + 4096;
        CHECK(real[i]->cap == full || (real[i]->cap == bytes && cfg.limit && usedBefore - capBefore + full > cfg.limit));
        CHECK(!cfg.limit || bud.used <= cfg.limit);
        CHECK(!cfg.allocCap || bud.used <= cfg.allocCap);
        CHECK(!cfg.capacity || bud.used <= cfg.capacity);
      } else {
        CHECK(real[i]->p == nullptr && real[i]->cap == 0);
      }
      CHECK(dev.mallocs - mallocsBefore <= 2 && M.onShed - shedBefore <= 1);
    } else if (op < 72) {
      M.b[i].cap = 0;
      real[i]->release();
    } else if (op < 80) {
      const uint64_t expect = M.shed();
      CHECK(bud.shed() == expect);
    } else if (op < 94) {
      M.gen++;
      bud.gen++;
    } else if (op < 97) {
      // a buffer that ends before its budget (a queue's): it leaves the list, and a new one enters at the end
      const bool held = M.b[i].held;
      real[i]->detach();
      for (DevBuf* b : bud.bufs) CHECK(b != real[i].get());
      real.erase(real.begin() + (long)i);
      M.b.erase(M.b.begin() + (long)i);
      compare();
      real.emplace_back(new DevBuf(bud, !held));
      M.b.push_back(MBuf{0, 0, !held});
    } else {
      // fits(): growing without releasing any other buffer
      const uint64_t bytes = 1 + pick(4 << 20);
      const bool expect = bytes <= M.b[i].cap || !cfg.limit || M.used() - M.b[i].cap + bytes <= cfg.limit;
      CHECK(real[i]->fits((size_t)bytes) == expect);
    }
    compare();
  }
  if (cfg.failReserve) CHECK(bud.growths < cfg.failReserve || bud.injected >= 1);
  // the end of a context: everything released, held buffers too
  for (DevBuf* b : bud.bufs) b->release();
  CHECK(bud.used == 0 && dev.inUse == 0 && dev.live.empty());
  dev.capacity = 0;
}

// the pinned host buffers and the device guard, for completeness of the header
void host_side()
{
  g_what = "host";
  HostBuf h;
  CHECK(h.reserve(1000) == hipSuccess && h.cap == 1000);
  void* p = h.p;
  CHECK(h.reserve(10) == hipSuccess && h.p == p && h.cap == 1000);
  CHECK(h.reserve(5000) == hipSuccess && h.cap == 5000);
  h.release();
  CHECK(h.p == nullptr && h.cap == 0 && fakehip::state().hostLive == 0);
  fakehip::state().device = 2;
  {
    DeviceGuard g(5);
    CHECK(fakehip::state().device == 5);
  }
  CHECK(fakehip::state().device == 2);
}

}  // namespace

int main()
{
  const uint64_t MiB = 1 << 20;
  const Config configs[] = {
      {"plain", 0, 0, 0, 0},
      {"limit", 12 * MiB, 0, 0, 0},
      {"tight limit", 3 * MiB, 0, 0, 0},
      {"capacity", 0, 12 * MiB, 0, 0},
      {"limit above capacity", 16 * MiB, 10 * MiB, 0, 0},
      {"limit below capacity", 8 * MiB, 14 * MiB, 0, 0},
      {"alloc cap hook", 0, 0, 10 * MiB, 0},
      {"alloc cap hook under a limit", 14 * MiB, 0, 9 * MiB, 0},
      {"alloc cap hook and capacity", 0, 12 * MiB, 9 * MiB, 0},
      {"fail-reserve hook, first growth", 0, 0, 0, 1},
      {"fail-reserve hook", 0, 0, 0, 37},
      {"fail-reserve hook under a limit", 12 * MiB, 0, 0, 101},
      {"fail-reserve hook and capacity", 0, 12 * MiB, 0, 60},
  };
  int runs = 0;
  for (const Config& cfg : configs)
    for (uint32_t seed = 1; seed <= 6; seed++, runs++) run(cfg, seed * 7919u + 13u);
  host_side();
  CHECK(fakehip::state().live.empty() && fakehip::state().hostLive == 0);
  printf("%d runs, %llu device allocations, %llu of them refused\n", runs, (unsigned long long)fakehip::state().mallocs,
         (unsigned long long)fakehip::state().failed);
  printf("mem_check ok\n");
  return 0;
}
