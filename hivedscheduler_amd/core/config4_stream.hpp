// The flagship benchmark's request stream and cluster (config 4), as data, for
// the stand-alone core drivers (config4_bench_main.cpp, config4_alloc_main.cpp).
#pragma once

#include <string>

#include "core.hpp"

namespace config4 {

using namespace hived;

struct Request {
  const char* vc;
  int cells;
  int priority;
};

// bench.py build_requests(seed=0, count=64), recorded as data
const Request kRequests[64] = {
    {"VC2", 2, -1}, {"VC2", 4, 1},  {"VC2", 2, 1},  {"VC2", 4, -1}, {"VC3", 1, 0},  {"VC1", 1, 0},
    {"VC3", 4, -1}, {"VC2", 1, -1}, {"VC3", 2, 1},  {"VC3", 1, 0},  {"VC2", 2, -1}, {"VC3", 2, 1},
    {"VC3", 2, -1}, {"VC3", 1, -1}, {"VC3", 2, -1}, {"VC3", 2, 0},  {"VC1", 2, -1}, {"VC1", 4, -1},
    {"VC1", 1, 1},  {"VC1", 1, 0},  {"VC3", 2, -1}, {"VC2", 4, 0},  {"VC3", 1, 0},  {"VC3", 1, 0},
    {"VC2", 1, 1},  {"VC2", 4, -1}, {"VC2", 1, -1}, {"VC1", 1, 0},  {"VC2", 1, -1}, {"VC3", 1, -1},
    {"VC1", 1, 1},  {"VC3", 4, 0},  {"VC3", 1, -1}, {"VC3", 4, 1},  {"VC3", 2, 1},  {"VC2", 2, -1},
    {"VC2", 4, -1}, {"VC2", 4, 0},  {"VC1", 1, -1}, {"VC3", 2, -1}, {"VC3", 1, 0},  {"VC1", 2, 1},
    {"VC1", 1, -1}, {"VC3", 1, -1}, {"VC3", 4, -1}, {"VC1", 1, -1}, {"VC3", 4, -1}, {"VC2", 1, 0},
    {"VC1", 1, -1}, {"VC1", 1, -1}, {"VC2", 1, -1}, {"VC3", 1, 1},  {"VC3", 1, 0},  {"VC1", 1, -1},
    {"VC3", 2, 0},  {"VC2", 1, -1}, {"VC3", 2, -1}, {"VC3", 1, 1},  {"VC1", 2, 0},  {"VC3", 2, -1},
    {"VC3", 1, -1}, {"VC3", 1, -1}, {"VC2", 4, 0},  {"VC1", 4, 1},
};
constexpr int kNumRequests = 64;
constexpr int kNumNodes = 4;

// The spec that sim.mi355x_cluster_config(num_nodes=4, vcs=...) hands to the
// core: the built-in MI355X chain with its 2- and 4-node pool types, four
// 8-GPU nodes, and the three VCs of bench.py.
inline ClusterSpec makeSpec() {
  ClusterSpec spec;
  spec.cellTypes["MI355X-PAIR"] = {"MI355X", 2, false};
  spec.cellTypes["MI355X-QUAD"] = {"MI355X-PAIR", 2, false};
  spec.cellTypes["MI355X-NODE"] = {"MI355X-QUAD", 2, true};
  spec.cellTypes["2-MI355X-NODE"] = {"MI355X-NODE", 2, false};
  spec.cellTypes["4-MI355X-NODE"] = {"MI355X-NODE", 4, false};
  for (int i = 0; i < kNumNodes; i++) {
    PhysCellSpec node;
    node.type = "MI355X-NODE";
    node.address = "node" + std::to_string(i + 1);
    int leafIdx = 0, pairIdx = 0;
    for (int q = 0; q < 2; q++) {
      PhysCellSpec quad;
      quad.type = "MI355X-QUAD";
      quad.address = std::to_string(q);
      for (int p = 0; p < 2; p++) {
        PhysCellSpec pair;
        pair.type = "MI355X-PAIR";
        pair.address = std::to_string(pairIdx++);
        for (int l = 0; l < 2; l++) {
          PhysCellSpec leaf;
          leaf.type = "MI355X";
          leaf.address = std::to_string(leafIdx++);
          pair.children.push_back(leaf);
        }
        quad.children.push_back(pair);
      }
      node.children.push_back(quad);
    }
    spec.physicalCells.push_back(node);
  }
  VCSpec vc1, vc2, vc3;
  vc1.virtualCells.push_back({"MI355X-NODE", 2});
  vc2.virtualCells.push_back({"MI355X-NODE", 1});
  vc2.virtualCells.push_back({"MI355X-NODE.MI355X-QUAD", 1});
  vc3.virtualCells.push_back({"MI355X-NODE.MI355X-QUAD", 1});
  spec.virtualClusters["VC1"] = vc1;
  spec.virtualClusters["VC2"] = vc2;
  spec.virtualClusters["VC3"] = vc3;
  return spec;
}

}  // namespace config4
