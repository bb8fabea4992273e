// Host program for the registry layer of self-forcing_amd/csrc/sf_launch.h (plain C++, no HIP, no GPU):
//   c++ -std=c++17 -pthread -I self-forcing_amd/csrc tests/launch_registry_main.cpp -o launch_registry && ./launch_registry
// tests/test_launch_registry.py builds and runs it; with -fsanitize=thread it is the race check of the registry.
// A stand-in "runtime" keeps each (kernel, device)'s LDS cap behind its own lock, as the HIP runtime does; the
// injected setter writes it and a stand-in launch reads it.
#include <climits>
#include <cstdio>
#include <mutex>
#include <thread>
#include <vector>

#include "sf_launch.h"

static int failures = 0;
#define EXPECT(cond)                                                      \
  do {                                                                    \
    if (!(cond)) {                                                        \
      std::fprintf(stderr, "%s:%d: FAILED %s\n", __FILE__, __LINE__, #cond); \
      ++failures;                                                         \
    }                                                                     \
  } while (0)

namespace {

constexpr int CAP = 160 * 1024;
constexpr int MAX_DEV = 128;

struct FakeRuntime {   // one kernel's attribute on every device
  std::mutex lock;
  int cap[MAX_DEV] = {};
  int sets[MAX_DEV] = {};
  int set(int dev) {
    std::lock_guard<std::mutex> g(lock);
    cap[dev] = CAP;
    ++sets[dev];
    return 0;
  }
  int cap_at_launch(int dev) {
    std::lock_guard<std::mutex> g(lock);
    return cap[dev];
  }
  int sets_on(int dev) {
    std::lock_guard<std::mutex> g(lock);
    return sets[dev];
  }
};

// N threads x several devices, all released at once: every "launch" finds the cap registered on its device
void concurrent_first_use() {
  constexpr int THREADS = 8, DEVICES = 6, ROUNDS = 50;
  sf_lds_record rec;
  FakeRuntime rt;
  std::atomic<int> waiting{0}, bad_rc{0}, launched_early{0};
  std::vector<std::thread> pool;
  for (int t = 0; t < THREADS; ++t)
    pool.emplace_back([&, t] {
      waiting.fetch_add(1);
      while (waiting.load() < THREADS) std::this_thread::yield();
      for (int r = 0; r < ROUNDS; ++r)
        for (int i = 0; i < DEVICES; ++i) {
          const int dev = (i + t) % DEVICES;   // the threads start on different devices and meet on all of them
          if (sf_lds_register(rec, dev, [&] { return rt.set(dev); }) != 0) bad_rc.fetch_add(1);
          if (rt.cap_at_launch(dev) != CAP) launched_early.fetch_add(1);
        }
    });
  for (auto& th : pool) th.join();
  EXPECT(bad_rc.load() == 0);
  EXPECT(launched_early.load() == 0);
  for (int dev = 0; dev < DEVICES; ++dev) {
    const int n = rt.sets_on(dev);
    EXPECT(n >= 1 && n <= THREADS);   // racing first calls may both register; nobody registers twice
    EXPECT(sf_lds_register(rec, dev, [&] { return rt.set(dev); }) == 0);
    EXPECT(rt.sets_on(dev) == n);     // recorded: no further set
  }
  EXPECT(rt.sets_on(DEVICES) == 0);
}

// a failed registration is returned, not recorded, and tried again by the next call
void failure_is_retried() {
  sf_lds_record rec;
  int calls = 0;
  EXPECT(sf_lds_register(rec, 3, [&] { ++calls; return 719; }) == 719);
  EXPECT(sf_lds_register(rec, 3, [&] { ++calls; return 1; }) == 1);
  EXPECT(calls == 2);
  EXPECT(sf_lds_register(rec, 3, [&] { ++calls; return 0; }) == 0);
  EXPECT(calls == 3);
  EXPECT(sf_lds_register(rec, 3, [&] { ++calls; return 719; }) == 0);   // recorded now: the setter is not called
  EXPECT(calls == 3);
  EXPECT(sf_lds_register(rec, 4, [&] { ++calls; return 0; }) == 0);     // another device is another entry
  EXPECT(calls == 4);
}

// ordinals outside the record register on every call and leave the record alone
void ordinals_past_the_table() {
  sf_lds_record rec;
  int calls = 0;
  const int outside[] = {sf_lds_record::DEVICES, sf_lds_record::DEVICES + 1, 1000, -1, INT_MIN, INT_MAX};
  for (int round = 0; round < 2; ++round)
    for (int dev : outside) EXPECT(sf_lds_register(rec, dev, [&] { ++calls; return 0; }) == 0);
  EXPECT(calls == 12);
  EXPECT(rec.done.load() == 0);
  EXPECT(sf_lds_register(rec, 1000, [&] { ++calls; return 5; }) == 5);
  // the last ordinal inside it is tracked
  EXPECT(sf_lds_register(rec, sf_lds_record::DEVICES - 1, [&] { ++calls; return 0; }) == 0);
  EXPECT(sf_lds_register(rec, sf_lds_record::DEVICES - 1, [&] { ++calls; return 0; }) == 0);
  EXPECT(calls == 14);
  EXPECT(rec.done.load() == (uint64_t)1 << (sf_lds_record::DEVICES - 1));
}

// one kernel's record says nothing about another kernel's
void records_are_per_kernel() {
  sf_lds_record a, b;
  int calls_a = 0, calls_b = 0;
  EXPECT(sf_lds_register(a, 0, [&] { ++calls_a; return 0; }) == 0);
  EXPECT(sf_lds_register(b, 0, [&] { ++calls_b; return 0; }) == 0);
  EXPECT(sf_lds_register(a, 0, [&] { ++calls_a; return 0; }) == 0);
  EXPECT(sf_lds_register(b, 0, [&] { ++calls_b; return 0; }) == 0);
  EXPECT(calls_a == 1 && calls_b == 1);
}

}  // namespace

int main() {
  concurrent_first_use();
  failure_is_retried();
  ordinals_past_the_table();
  records_are_per_kernel();
  if (failures) {
    std::fprintf(stderr, "%d check(s) failed\n", failures);
    return 1;
  }
  std::puts("launch registry: all checks passed");
  return 0;
}
