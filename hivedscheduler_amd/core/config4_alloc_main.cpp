// Heap allocations of one HivedCore::schedule call, per kind of decision, on
// the flagship benchmark's stream (config 4, see config4_bench_main.cpp), and
// of what follows a bind: the commit (addAllocatedPod, handed the decision's own
// bind info handle as the fused schedule_pod(commit=True) does) and the release, by spec
// and bind info in even steps and by pod key in odd ones. The global operator
// new is replaced by a counting one; each count is taken around the one core
// call, after warm-up, so reusable scratch has its size.
// -DCONFIG4_NO_RELEASE_BY_KEY drives a core from before the release by key.
//
// The aim for a decision that waits because placement failed (reason ending in
// "when scheduling in physical cluster", or a guaranteed request whose intra-VC
// attempt failed) is one allocation: the reason string.
// Compile (one line, from hivedscheduler_amd/):
//   g++ -O2 -std=c++17 -o config4alloc core/config4_alloc_main.cpp
//       core/{cells,topo_sched,build,alloc,algorithm,debug}.cpp
// The same line with -O1 -g -fsanitize=address,undefined gives the sanitizer
// build; it runs on the CPU like this one.
// Run:
//   ./config4alloc [steps=20] [warmup=5]
#include <cstdio>
#include <cstdlib>
#include <map>
#include <new>
#include <string>
#include <vector>

#include "config4_stream.hpp"
#include "core.hpp"

namespace {
long gAllocations = 0;
}

void* operator new(std::size_t n) {
  gAllocations++;
  if (void* p = std::malloc(n ? n : 1)) return p;
  throw std::bad_alloc();
}
void* operator new[](std::size_t n) { return operator new(n); }
// the nothrow forms too (std::stable_sort's buffer uses them), so that every
// block the deletes below free came from malloc
void* operator new(std::size_t n, const std::nothrow_t&) noexcept {
  gAllocations++;
  return std::malloc(n ? n : 1);
}
void* operator new[](std::size_t n, const std::nothrow_t& t) noexcept { return operator new(n, t); }
void operator delete(void* p) noexcept { std::free(p); }
void operator delete[](void* p) noexcept { std::free(p); }
void operator delete(void* p, std::size_t) noexcept { std::free(p); }
void operator delete[](void* p, std::size_t) noexcept { std::free(p); }

using namespace hived;
using namespace config4;

namespace {

struct Tally {
  long n = 0, total = 0, lo = -1, hi = 0;
  void add(long a) {
    n++;
    total += a;
    if (lo < 0 || a < lo) lo = a;
    if (a > hi) hi = a;
  }
};

bool endsWith(const std::string& s, const char* tail) {
  std::string t(tail);
  return s.size() >= t.size() && s.compare(s.size() - t.size(), t.size(), t) == 0;
}

}  // namespace

int main(int argc, char** argv) {
  int steps = argc > 1 ? atoi(argv[1]) : 20;
  int warmup = argc > 2 ? atoi(argv[2]) : 5;

  HivedCore core(makeSpec());
  for (auto& n : core.allNodes()) core.setNodeHealthy(n, true);

  std::vector<PodSpec> specs(kNumRequests);
  std::vector<std::string> keys(kNumRequests);
  for (int i = 0; i < kNumRequests; i++) {
    keys[i] = "bench/p" + std::to_string(i);
    PodSpec& s = specs[i];
    s.vc = kRequests[i].vc;
    s.priority = kRequests[i].priority;
    s.leafCellNumber = kRequests[i].cells;
    s.groupName = keys[i];
    s.groupPodNums[s.leafCellNumber] = 1;
  }
  const std::set<std::string> suggested;  // ignoreK8sSuggestedNodes = true

  // category -> allocations per decision; a wait is filed under its reason
  // with the VC name cut off, so the categories are the same on every build
  std::map<std::string, Tally> tallies;
  for (int step = 0; step < warmup + steps; step++) {
    std::vector<std::pair<int, std::shared_ptr<const BindInfo>>> bound;
    for (int i = 0; i < kNumRequests; i++) {
      long before = gAllocations;
      ScheduleResult r = core.schedule(specs[i], keys[i], suggested, Phase::Filtering);
      long during = gAllocations - before;
      std::string what;
      switch (r.kind) {
        case ScheduleResult::Kind::Bind:
          what = "bind";
          {
            long beforeAdd = gAllocations;
            core.addAllocatedPod(specs[i], r.bindInfo, keys[i]);
            long add = gAllocations - beforeAdd;
            if (step >= warmup) {
              tallies["commit (addAllocatedPod)"].add(add);
              tallies["bind + commit"].add(during + add);
            }
          }
          bound.emplace_back(i, std::move(r.bindInfo));
          break;
        case ScheduleResult::Kind::Preempt:
          what = "preempt";
          break;
        case ScheduleResult::Kind::Wait:
          what = "wait: " + r.waitReason;
          if (!endsWith(r.waitReason, "physical cluster")) {
            what += kRequests[i].priority >= 0 ? " [guaranteed]" : " [opportunistic]";
          }
          break;
      }
      if (step >= warmup) tallies[what].add(during);
    }
#ifdef CONFIG4_NO_RELEASE_BY_KEY
    const bool byKey = false;
#else
    const bool byKey = step % 2 == 1;
#endif
    for (auto& [i, info] : bound) {
      long before = gAllocations;
#ifndef CONFIG4_NO_RELEASE_BY_KEY
      if (byKey) {
        if (!core.deleteAllocatedPodByKey(keys[i])) {
          fprintf(stderr, "unknown key %s\n", keys[i].c_str());
          return 1;
        }
      } else
#endif
        core.deleteAllocatedPod(specs[i], *info, keys[i]);
      if (step >= warmup) {
        tallies[byKey ? "release (deleteAllocatedPodByKey)" : "release (deleteAllocatedPod)"].add(
            gAllocations - before);
      }
    }
#ifndef CONFIG4_NO_RELEASE_BY_KEY
    // a released key is unknown, and asking again changes nothing
    for (auto& [i, info] : bound) {
      (void)info;
      if (core.deleteAllocatedPodByKey(keys[i])) {
        fprintf(stderr, "key %s known after its release\n", keys[i].c_str());
        return 1;
      }
    }
#endif
  }
  checkInvariants(core);

  printf("config4 heap allocations per core call: steps=%d warmup=%d\n", steps, warmup);
  for (auto& [what, t] : tallies) {
    printf("  n=%-5ld min=%-3ld max=%-3ld mean=%6.2f  %s\n", t.n, t.lo, t.hi,
           static_cast<double>(t.total) / static_cast<double>(t.n), what.c_str());
  }
  return 0;
}
