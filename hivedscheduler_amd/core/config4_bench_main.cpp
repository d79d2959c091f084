// Standalone driver of the flagship benchmark config (no Python): config 4,
// 64 mixed 1/2/4-GPU requests on a 4-node x 8-MI355X cluster with the VC
// quotas of bench.py. One step = schedule all 64 requests (a bind is committed
// at once with addAllocatedPod, handed the decision's own bind info handle as
// the fused schedule_pod(commit=True) of the simulation harness does), then delete
// every bound pod: by spec and bind info (deleteAllocatedPod) in even steps, by
// pod key (deleteAllocatedPodByKey) in odd ones, so both see the same stream.
// Reports the p50 of HivedCore::schedule per decision kind, of addAllocatedPod
// and of the two releases. -DCONFIG4_NO_RELEASE_BY_KEY drives a core from
// before the release by key (every step releases by spec and bind info).
//
// This is the "core time" of a decision. bench.py measures the same stream
// through the pybind11 boundary and the Python facade, so the difference
// between the two is what the boundary and the facade cost.
// Compile (one line, from hivedscheduler_amd/):
//   g++ -O2 -std=c++17 -o config4bench core/config4_bench_main.cpp
//       core/{cells,topo_sched,build,alloc,algorithm,debug}.cpp
// Run:
//   ./config4bench [steps=200] [warmup=5]
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "config4_stream.hpp"
#include "core.hpp"

using namespace hived;
using namespace config4;

namespace {

using Clock = std::chrono::steady_clock;
double usSince(Clock::time_point t0) {
  return std::chrono::duration<double, std::micro>(Clock::now() - t0).count();
}

struct Samples {
  std::vector<double> us;
  void report(const char* what) {
    if (us.empty()) {
      printf("  %-22s n=0\n", what);
      return;
    }
    std::sort(us.begin(), us.end());
    printf("  %-22s n=%-6zu p50=%7.2fus p99=%7.2fus\n", what, us.size(), us[us.size() / 2],
           us[std::min(us.size() - 1, static_cast<size_t>(us.size() * 0.99))]);
  }
};

}  // namespace

int main(int argc, char** argv) {
  int steps = argc > 1 ? atoi(argv[1]) : 200;
  int warmup = argc > 2 ? atoi(argv[2]) : 5;

  HivedCore core(makeSpec());
  for (auto& n : core.allNodes()) core.setNodeHealthy(n, true);

  // requests are built outside the timed calls, as bench.py builds its specs
  std::vector<PodSpec> specs(kNumRequests);
  std::vector<std::string> keys(kNumRequests);
  for (int i = 0; i < kNumRequests; i++) {
    keys[i] = "bench/p" + std::to_string(i);
    PodSpec& s = specs[i];
    s.vc = kRequests[i].vc;
    s.priority = kRequests[i].priority;
    s.leafCellNumber = kRequests[i].cells;
    s.groupName = keys[i];  // singleton group named after the pod
    s.groupPodNums[s.leafCellNumber] = 1;
  }
  const std::set<std::string> suggested;  // ignoreK8sSuggestedNodes = true

  Samples all, waitS, preemptS, bindS, addS, delS, delKeyS;
  std::vector<double> stepMs;
  long binds = 0, waits = 0, preempts = 0;
  for (int step = 0; step < warmup + steps; step++) {
    bool timed = step >= warmup;
    std::vector<std::pair<int, std::shared_ptr<const BindInfo>>> bound;
    auto ts = Clock::now();
    for (int i = 0; i < kNumRequests; i++) {
      auto t0 = Clock::now();
      ScheduleResult r = core.schedule(specs[i], keys[i], suggested, Phase::Filtering);
      double us = usSince(t0);
      double addUs = 0;
      if (r.kind == ScheduleResult::Kind::Bind) {
        auto t1 = Clock::now();
        core.addAllocatedPod(specs[i], r.bindInfo, keys[i]);
        addUs = usSince(t1);
        bound.emplace_back(i, std::move(r.bindInfo));
      }
      if (!timed) continue;
      all.us.push_back(us + addUs);  // what bench.py times: decision + commit
      switch (r.kind) {
        case ScheduleResult::Kind::Bind:
          bindS.us.push_back(us);
          addS.us.push_back(addUs);
          binds++;
          break;
        case ScheduleResult::Kind::Preempt:
          preemptS.us.push_back(us);
          preempts++;
          break;
        case ScheduleResult::Kind::Wait:
          waitS.us.push_back(us);
          waits++;
          break;
      }
    }
#ifdef CONFIG4_NO_RELEASE_BY_KEY
    const bool byKey = false;
#else
    const bool byKey = step % 2 == 1;
#endif
    for (auto& [i, info] : bound) {
      auto t0 = Clock::now();
#ifndef CONFIG4_NO_RELEASE_BY_KEY
      if (byKey) {
        if (!core.deleteAllocatedPodByKey(keys[i])) {
          fprintf(stderr, "unknown key %s\n", keys[i].c_str());
          return 1;
        }
      } else
#endif
        core.deleteAllocatedPod(specs[i], *info, keys[i]);
      double us = usSince(t0);
      if (timed) (byKey ? delKeyS : delS).us.push_back(us);
    }
    if (timed) stepMs.push_back(usSince(ts) / 1e3);
  }
  checkInvariants(core);

  int n = std::max(1, steps);
  printf("config4 core-only: steps=%d warmup=%d per step: binds=%ld waits=%ld preempts=%ld\n", steps,
         warmup, binds / n, waits / n, preempts / n);
  all.report("decision (+commit)");
  waitS.report("schedule -> wait");
  preemptS.report("schedule -> preempt");
  bindS.report("schedule -> bind");
  addS.report("addAllocatedPod");
  delS.report("deleteAllocatedPod");
  delKeyS.report("deleteAllocatedPodByKey");
  std::sort(stepMs.begin(), stepMs.end());
  if (!stepMs.empty()) printf("  ms_per_step p50=%.4f\n", stepMs[stepMs.size() / 2]);
  return 0;
}
