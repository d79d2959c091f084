// Cluster-spec compiler: normalized spec -> physical/virtual cell trees,
// free lists, VC accounting, schedulers. Semantics parity:
// pkg/algorithm/config.go (ParseConfig) + hived_algorithm.go:108-464 (init).
#include "core.hpp"

namespace hived {

namespace {

struct ChainMeta {
  std::vector<std::string> types;  // top-down type names, types.back() = leaf
  std::vector<bool> isNode;        // aligned with types
  int topLevel() const { return static_cast<int>(types.size()); }
  // level l (1=leaf) -> index into types: types[topLevel - l]
  const std::string& typeAt(int l) const { return types[topLevel() - l]; }
  bool isNodeAt(int l) const { return isNode[topLevel() - l]; }
  // a level is at-or-above node iff the chain's node level is at or below it
  bool atOrAboveNodeAt(int l) const {
    for (int ll = l; ll >= 1; ll--) {
      if (isNodeAt(ll)) return true;
    }
    return false;
  }
};

ChainMeta buildChainMeta(const std::map<std::string, CellTypeSpec>& cellTypes,
                         const std::string& topType) {
  ChainMeta m;
  std::string t = topType;
  std::set<std::string> seen;
  for (;;) {
    if (seen.count(t)) throw HivedError::BadRequest("cellTypes contains a cycle at " + t);
    seen.insert(t);
    auto it = cellTypes.find(t);
    bool leaf = (it == cellTypes.end()) || it->second.child.empty();
    m.types.push_back(t);
    m.isNode.push_back(it != cellTypes.end() && it->second.isNode);
    if (leaf) break;
    t = it->second.child;
  }
  return m;
}

int childCountAt(const std::map<std::string, CellTypeSpec>& cellTypes, const std::string& type) {
  auto it = cellTypes.find(type);
  if (it == cellTypes.end() || it->second.child.empty()) return 0;
  return it->second.childCount;
}

}  // namespace

struct BuildContext {
  HivedCore* h;
  const ClusterSpec& spec;
  std::map<std::string, ChainMeta> chainMeta;
  std::map<std::string, std::vector<PhysicalCell*>> nodeLeafCells;  // node -> leaf cells
  std::map<std::string, PhysicalCell*> pinnedCellsById;
  // (node, (a, b, gbps, healthy)) link specs deferred until leaf maps exist
  std::vector<std::pair<std::string, std::tuple<int, int, double, bool>>> pendingLinks;

  BuildContext(HivedCore* h_, const ClusterSpec& s) : h(h_), spec(s) {}

  PhysicalCell* buildPhysicalCell(const PhysCellSpec& cs, const ChainMeta& meta,
                                  ChainState* chainState, int level,
                                  const std::string& parentAddr, const std::string& nodeName) {
    const std::string& chain = chainState->name;
    auto cell = std::make_unique<PhysicalCell>();
    PhysicalCell* c = cell.get();
    h->cellStore_.push_back(std::move(cell));
    c->chain = chain;
    c->cs = chainState;
    c->level = level;
    c->typeName = meta.typeAt(level);
    c->isNodeLevel = meta.isNodeAt(level);
    c->atOrAboveNode = meta.atOrAboveNodeAt(level);
    std::string ownNodeName = nodeName;
    if (c->isNodeLevel) ownNodeName = cs.address;
    c->address = parentAddr.empty() ? cs.address : parentAddr + "/" + cs.address;
    if (!cs.pinnedId.empty()) {
      c->pinned = true;
      c->pinnedId = cs.pinnedId;
      if (!pinnedCellsById.emplace(cs.pinnedId, c).second) {
        throw HivedError::BadRequest("pinnedCellId " + cs.pinnedId + " used by multiple physical cells");
      }
    }
    // discovery-measured xGMI link table (node-level entries): applied after
    // construction, once nodeLeafCellsStorage_ is populated
    if (!cs.xgmiLinks.empty()) {
      for (auto& l : cs.xgmiLinks) pendingLinks.emplace_back(ownNodeName, l);
    }
    if (level == kLowestLevel) {
      if (ownNodeName.empty()) {
        // chain without a node level: the leaf's own address is the node name
        ownNodeName = c->address;
      }
      int leafIndex = 0;
      try {
        leafIndex = std::stoi(cs.address);
      } catch (...) {
        throw HivedError::BadRequest("leaf cell address must be an integer device index, got '" +
                                     cs.address + "'");
      }
      c->totalLeaf = 1;
      c->freeLeavesUnder = 1;  // all cells start Free
      c->nodes = {ownNodeName};
      c->leafIndices = {leafIndex};
      // measured per-GPU capacity from discovery when provided (a GPU
      // reporting less than the nominal 288 GB is a health signal and is
      // avoided by requests carrying hbmBytesPerCell), nominal otherwise
      c->hbmBytes = cs.hbmBytes > 0 ? cs.hbmBytes : 288LL * 1024 * 1024 * 1024;
      nodeLeafCells[ownNodeName].push_back(c);
    } else {
      int expected = childCountAt(spec.cellTypes, c->typeName);
      if (static_cast<int>(cs.children.size()) != expected) {
        throw HivedError::BadRequest("cell " + c->address + " of type " + c->typeName + " has " +
                                     std::to_string(cs.children.size()) + " children, expected " +
                                     std::to_string(expected));
      }
      for (const auto& childSpec : cs.children) {
        PhysicalCell* child =
            buildPhysicalCell(childSpec, meta, chainState, level - 1, c->address, ownNodeName);
        child->parent = c;
        c->children.push_back(child);
        c->totalLeaf += child->totalLeaf;
        c->freeLeavesUnder += child->freeLeavesUnder;
        c->hbmBytes += child->hbmBytes;
        for (auto& n : child->nodes) {
          if (std::find(c->nodes.begin(), c->nodes.end(), n) == c->nodes.end()) c->nodes.push_back(n);
        }
        for (int gi : child->leafIndices) c->leafIndices.push_back(gi);
      }
    }
    chainState->full.add(c, level);
    return c;
  }

  VirtualCell* buildVirtualCell(VCChainState* vcChain, const ChainMeta& meta, int level,
                                VirtualCell* preassigned, const std::string& addr,
                                const std::string& pinnedId, ChainCellList& fullList) {
    auto cell = std::make_unique<VirtualCell>();
    VirtualCell* c = cell.get();
    h->cellStore_.push_back(std::move(cell));
    c->vc = vcChain->vc;
    c->chain = vcChain->chain->name;
    c->cs = vcChain->chain;
    c->vcChain = vcChain;
    c->level = level;
    c->typeName = meta.typeAt(level);
    c->isNodeLevel = meta.isNodeAt(level);
    c->atOrAboveNode = meta.atOrAboveNodeAt(level);
    c->address = addr;
    c->pinnedId = pinnedId;
    c->preassigned = (preassigned == nullptr) ? c : preassigned;
    if (level == kLowestLevel) {
      c->totalLeaf = 1;
      c->freeLeavesUnder = 1;  // all cells start Free
    } else {
      int childNum = childCountAt(spec.cellTypes, c->typeName);
      for (int i = 0; i < childNum; i++) {
        VirtualCell* child = buildVirtualCell(vcChain, meta, level - 1, c->preassigned,
                                              addr + "/" + std::to_string(i), pinnedId, fullList);
        child->parent = c;
        c->children.push_back(child);
        c->totalLeaf += child->totalLeaf;
        c->freeLeavesUnder += child->freeLeavesUnder;
      }
    }
    fullList.add(c, level);
    return c;
  }

  // the VC's record on a chain, made on first use
  VCChainState* vcChainState(const std::string& vcName, ChainState* chainState) {
    auto& perChain = h->vcChainStates_[vcName];
    auto it = perChain.find(chainState->name);
    if (it != perChain.end()) return &it->second;
    VCChainState& vcc = perChain[chainState->name];
    vcc.vc = vcName;
    vcc.chain = chainState;
    vcc.free.assign(chainState->top + 1, 0);
    vcc.doomed.init(chainState->top);
    h->vcSchedulers_[vcName].byChain[chainState->index] = &vcc;
    return &vcc;
  }

  void build() {
    // --- physical cluster ---
    for (const auto& cs : spec.physicalCells) {
      const std::string& chain = cs.type;
      if (!chainMeta.count(chain)) chainMeta.emplace(chain, buildChainMeta(spec.cellTypes, chain));
      const ChainMeta& meta = chainMeta.at(chain);
      if (!h->chainStates_.count(chain)) {
        ChainState& st = h->chainStates_[chain];
        st.name = chain;
        st.top = meta.topLevel();
        st.full.init(st.top);
        st.free.init(st.top);
        st.badFree.init(st.top);
        st.levelType.assign(st.top + 1, std::string());
        for (int l = 1; l <= st.top; l++) st.levelType[l] = meta.typeAt(l);
        st.totalLeft.assign(st.top + 1, 0);
        st.allVCFree.assign(st.top + 1, 0);
        st.allVCDoomedBadCellNum.assign(st.top + 1, 0);
      }
      ChainState* st = &h->chainStates_.at(chain);
      PhysicalCell* top = buildPhysicalCell(cs, meta, st, meta.topLevel(), "", "");
      st->free.add(top, meta.topLevel());
    }
    {
      int index = 0;
      for (auto& [chain, st] : h->chainStates_) {
        (void)chain;
        st.index = index++;
      }
    }
    for (auto& [chain, meta] : chainMeta) {
      auto stIt = h->chainStates_.find(chain);
      if (stIt == h->chainStates_.end()) continue;
      h->cellChains_[meta.types.back()].push_back(&stIt->second);
      int leafNum = 1;
      for (int l = 1; l <= meta.topLevel(); l++) {
        h->leafCellNums_[chain][l] = leafNum;
        if (l < meta.topLevel()) {
          leafNum *= childCountAt(spec.cellTypes, meta.typeAt(l + 1));
        }
      }
    }

    // --- virtual clusters ---
    for (const auto& [vcName, vcSpec] : spec.virtualClusters) {
      IntraVCScheduler& vcs = h->vcSchedulers_[vcName];
      vcs.byChain.assign(h->chainStates_.size(), nullptr);
      int cellCounter = 0;
      for (const auto& vcell : vcSpec.virtualCells) {
        // resolve hierarchical type path "CHAIN.CHILD..." -> (chain, level)
        std::vector<std::string> parts;
        size_t start = 0;
        const std::string& path = vcell.typePath;
        while (start <= path.size()) {
          size_t dot = path.find('.', start);
          if (dot == std::string::npos) {
            parts.push_back(path.substr(start));
            break;
          }
          parts.push_back(path.substr(start, dot - start));
          start = dot + 1;
        }
        const std::string& chain = parts[0];
        auto metaIt = chainMeta.find(chain);
        if (metaIt == chainMeta.end() || !h->chainStates_.count(chain)) {
          throw HivedError::BadRequest("VC " + vcName + " virtual cell type " + path +
                                       ": chain " + chain + " does not exist in physical cluster");
        }
        const ChainMeta& meta = metaIt->second;
        for (size_t i = 1; i < parts.size(); i++) {
          if (i >= meta.types.size() || meta.types[i] != parts[i]) {
            throw HivedError::BadRequest("VC " + vcName + " virtual cell type path " + path +
                                         " does not match chain " + chain);
          }
        }
        int level = meta.topLevel() - static_cast<int>(parts.size()) + 1;
        if (!vcs.nonPinnedFull.count(chain)) {
          vcs.nonPinnedFull[chain].init(meta.topLevel());
          vcs.nonPinnedPreassigned[chain].init(meta.topLevel());
        }
        VCChainState* vcc = vcChainState(vcName, &h->chainStates_.at(chain));
        vcc->preassigned = &vcs.nonPinnedPreassigned[chain];
        for (int i = 0; i < vcell.number; i++) {
          std::string addr = vcName + "/" + chain + "/" + std::to_string(cellCounter++);
          VirtualCell* pre =
              buildVirtualCell(vcc, meta, level, nullptr, addr, "", vcs.nonPinnedFull[chain]);
          vcs.nonPinnedPreassigned[chain].add(pre, level);
        }
        vcc->free[level] += vcell.number;
      }
      // pinned cells: statically bound, scheduled by their own scheduler
      for (const auto& pinnedId : vcSpec.pinnedIds) {
        auto it = pinnedCellsById.find(pinnedId);
        if (it == pinnedCellsById.end()) {
          throw HivedError::BadRequest("VC " + vcName + " refers to unknown pinnedCellId " + pinnedId);
        }
        PhysicalCell* pc = it->second;
        if (h->pinnedPhysical_.count(vcName) == 0) h->pinnedPhysical_[vcName] = {};
        for (auto& [otherVc, ids] : h->pinnedPhysical_) {
          if (ids.count(pinnedId)) {
            throw HivedError::BadRequest("pinnedCellId " + pinnedId + " referred by multiple VCs");
          }
        }
        const ChainMeta& meta = chainMeta.at(pc->chain);
        ChainCellList& pinnedList = vcs.pinned[pinnedId];
        pinnedList.init(pc->level);
        std::string addr = vcName + "/" + pinnedId;
        VCChainState* vcc = vcChainState(vcName, pc->cs);
        buildVirtualCell(vcc, meta, pc->level, nullptr, addr, pinnedId, pinnedList);
        h->pinnedPhysical_[vcName][pinnedId] = pc;
        vcc->free[pc->level] += 1;
      }
      for (auto& [chain, ccl] : vcs.nonPinnedFull) {
        auto entered = vcs.nonPinnedSchedulers.emplace(
            chain, TopoScheduler(ccl, h->leafCellNums_[chain], true));
        vcs.byChain[h->chainStates_.at(chain).index]->topo = &entered.first->second;
      }
      for (auto& [pid, ccl] : vcs.pinned) {
        const std::string& chain = ccl.at(kLowestLevel)[0]->chain;
        vcs.pinnedSchedulers.emplace(pid, TopoScheduler(ccl, h->leafCellNums_[chain], true));
      }
    }
    for (auto& [chain, st] : h->chainStates_) {
      st.opportunistic = TopoScheduler(st.full, h->leafCellNums_[chain], false);
    }
  }
};

void HivedCore::buildFromSpec(const ClusterSpec& spec) {
  BuildContext ctx(this, spec);
  ctx.build();
  nodeLeafCellsStorage_.clear();
  for (auto& [node, cells] : ctx.nodeLeafCells) nodeLeafCellsStorage_[node] = cells;
  // apply the discovery-measured xGMI link table (records gbps; a link
  // reported unhealthy at config time degrades its pair/quad from the start)
  for (auto& [node, l] : ctx.pendingLinks) {
    setXgmiLinkHealthy(node, std::get<0>(l), std::get<1>(l), std::get<3>(l), std::get<2>(l));
  }
}

// Validates VC quota against the physical cluster and initializes the
// accounting maps (parity: hived_algorithm.go:369-409).
void HivedCore::initCellNums() {
  // Every physical chain has its accounting, even with no VC quota.
  for (auto& [chain, st] : chainStates_) {
    (void)chain;
    const ChainCellList& ccl = st.full;
    int top = st.top;
    st.totalLeft[top] = static_cast<int>(ccl.at(top).size());
    for (int l = top; l > kLowestLevel; l--) {
      int childNum = static_cast<int>(ccl.at(l)[0]->children.size());
      st.totalLeft[l - 1] = st.totalLeft[l] * childNum;
    }
  }
  // a chain's VCs in VC-name order: the order the doom checks visit them in
  for (auto& [vc, perChain] : vcChainStates_) {
    (void)vc;
    for (auto& [chain, vcc] : perChain) {
      (void)chain;
      ChainState* st = vcc.chain;
      st->vcs.push_back(&vcc);
      for (int l = kLowestLevel; l <= st->top; l++) st->allVCFree[l] += vcc.free[l];
    }
  }
  // Validate: the VCs' free cells fit into the physical cluster at every level.
  for (auto& [chain, st] : chainStates_) {
    const ChainCellList& ccl = st.full;
    int top = st.top;
    int available = static_cast<int>(ccl.at(top).size());
    for (int l = top; l >= kLowestLevel; l--) {
      int need = st.allVCFree[l];
      int left = available - need;
      if (left < 0) {
        throw HivedError::BadRequest(
            "Illegal initial VC assignment: insufficient physical cells at chain " + chain +
            " level " + std::to_string(l) + ": " + std::to_string(need) + " needed, " +
            std::to_string(available) + " available");
      }
      if (l > kLowestLevel) {
        int childNum = static_cast<int>(ccl.at(l)[0]->children.size());
        available = left * childNum;
      }
    }
  }
}

// Static bindings for pinned cells; removes them from the free list.
void HivedCore::initPinnedCells() {
  for (auto& [vcName, perId] : pinnedPhysical_) {
    for (auto& [pid, pc] : perId) {
      allocatePreassignedCell(pc, &vcChainStates_.at(vcName).at(pc->chain), false);
      ChainCellList& vlist = vcSchedulers_[vcName].pinned[pid];
      auto* pinnedVirtual = static_cast<VirtualCell*>(vlist.at(vlist.top())[0]);
      bindCell(pc, pinnedVirtual);
    }
  }
}

// All nodes start bad until the informer confirms them healthy.
void HivedCore::initBadNodes() {
  std::vector<std::string> nodes;
  for (auto& [node, cells] : nodeLeafCellsStorage_) nodes.push_back(node);
  for (auto& n : nodes) setNodeHealthy(n, false);
}

HivedCore::HivedCore(const ClusterSpec& spec) {
  buildFromSpec(spec);
  initCellNums();
  initPinnedCells();
  initBadNodes();
}

HivedCore::~HivedCore() = default;

std::vector<std::string> HivedCore::allNodes() const {
  std::vector<std::string> nodes;
  for (auto& [node, cells] : nodeLeafCellsStorage_) nodes.push_back(node);
  return nodes;
}

std::vector<std::string> HivedCore::chains() const {
  std::vector<std::string> out;
  for (auto& [chain, st] : chainStates_) out.push_back(chain);
  return out;
}

std::map<int, std::string> HivedCore::chainLevelTypes(const std::string& chain) const {
  std::map<int, std::string> out;
  auto it = chainStates_.find(chain);
  if (it == chainStates_.end()) return out;
  for (int l = kLowestLevel; l <= it->second.top; l++) out[l] = it->second.levelType[l];
  return out;
}

}  // namespace hived
