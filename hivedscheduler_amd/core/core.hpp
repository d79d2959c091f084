// MI355X-native gang-scheduler core: cell model, buddy allocation,
// topology-aware placement, VC-safety accounting, preemption lifecycle.
//
// This is a from-scratch C++ implementation of the scheduling semantics of
// microsoft/hivedscheduler's pkg/algorithm (Go), redesigned for:
//  - microsecond-scale Schedule() latency (the headline metric): pointer-based
//    cell trees, no per-call allocations on the hot path where avoidable;
//  - the CDNA4 cell chain (MI355X -> xGMI pair -> quad -> 8-GPU node -> pool)
//    with HBM capacity and link health as first-class cell attributes;
//  - a best-fit recursive descent for intra-node placement that directly
//    yields LCA-minimal placements (instead of combination backtracking).
//
// Behavioral parity references (semantics, not code):
//   cell model            ~ pkg/algorithm/cell.go
//   buddy alloc / binding ~ pkg/algorithm/cell_allocation.go
//   placement engine      ~ pkg/algorithm/topology_aware_scheduler.go
//   algorithm facade      ~ pkg/algorithm/hived_algorithm.go
//   state machines        ~ doc/design/state-machine.md
#pragma once

#include <algorithm>
#include <cstddef>
#include <map>
#include <memory>
#include <new>
#include <optional>
#include <random>
#include <set>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <vector>

namespace hived {

// ---------------------------------------------------------------------------
// Constants
// ---------------------------------------------------------------------------
constexpr int kMaxGuaranteedPriority = 1000;
constexpr int kMinGuaranteedPriority = 0;
constexpr int kOpportunisticPriority = -1;
constexpr int kFreePriority = -2;
constexpr int kLowestLevel = 1;
constexpr int kHighestLevel = 100;

enum class CState { Free, Used, Reserving, Reserved };
enum class GState { Allocated, Preempting, BeingPreempted };

const char* to_string(CState s);
const char* to_string(GState s);

// Error with an HTTP status code; translated to a Python exception.
struct HivedError : std::runtime_error {
  int code;
  HivedError(int code_, const std::string& msg) : std::runtime_error(msg), code(code_) {}
  static HivedError BadRequest(const std::string& msg) { return HivedError(400, msg); }
  static HivedError NotFound(const std::string& msg) { return HivedError(404, msg); }
  static HivedError Internal(const std::string& msg) { return HivedError(500, msg); }
};

// ---------------------------------------------------------------------------
// Small containers for the handful of cells one decision touches. The first N
// entries live inside the object (on the caller's stack or in reused scratch,
// no heap); a decision that needs more spills into the std container, so large
// gangs keep their O(1) lookups. Neither promises an iteration order; no
// caller depends on one.
// ---------------------------------------------------------------------------
template <class K, size_t N = 16>
class SmallPtrSet {
 public:
  bool empty() const { return n_ == 0 && big_.empty(); }
  size_t count(K* k) const {
    if (!big_.empty()) return big_.count(k);
    for (size_t i = 0; i < n_; i++) {
      if (inl_[i] == k) return 1;
    }
    return 0;
  }
  void insert(K* k) {
    if (count(k)) return;
    if (big_.empty() && n_ < N) {
      inl_[n_++] = k;
      return;
    }
    for (size_t i = 0; i < n_; i++) big_.insert(inl_[i]);
    n_ = 0;
    big_.insert(k);
  }
  void erase(K* k) {
    if (!big_.empty()) {
      big_.erase(k);
      return;
    }
    for (size_t i = 0; i < n_; i++) {
      if (inl_[i] == k) {
        inl_[i] = inl_[--n_];
        return;
      }
    }
  }

 private:
  K* inl_[N];
  size_t n_ = 0;
  std::unordered_set<K*> big_;
};

template <class K, class V, size_t N = 32>
class SmallPtrMap {
 public:
  bool empty() const { return n_ == 0 && big_.empty(); }
  // the value of k, or nullptr
  V* find(K* k) {
    if (!big_.empty()) {
      auto it = big_.find(k);
      return it == big_.end() ? nullptr : &it->second;
    }
    for (size_t i = 0; i < n_; i++) {
      if (inl_[i].first == k) return &inl_[i].second;
    }
    return nullptr;
  }
  const V* find(K* k) const { return const_cast<SmallPtrMap*>(this)->find(k); }
  size_t count(K* k) const { return find(k) != nullptr ? 1 : 0; }
  V& at(K* k) {
    V* v = find(k);
    if (v == nullptr) throw std::out_of_range("SmallPtrMap::at");
    return *v;
  }
  V& operator[](K* k) {
    if (V* v = find(k)) return *v;
    if (big_.empty() && n_ < N) {
      inl_[n_] = {k, V{}};
      return inl_[n_++].second;
    }
    for (size_t i = 0; i < n_; i++) big_.emplace(inl_[i].first, inl_[i].second);
    n_ = 0;
    return big_[k];
  }
  void erase(K* k) {
    if (!big_.empty()) {
      big_.erase(k);
      return;
    }
    for (size_t i = 0; i < n_; i++) {
      if (inl_[i].first == k) {
        inl_[i] = inl_[--n_];
        return;
      }
    }
  }
  void clear() {
    n_ = 0;
    big_.clear();
  }
  template <class F>
  void forEach(F f) const {
    for (size_t i = 0; i < n_; i++) f(inl_[i].first, inl_[i].second);
    for (auto& [k, v] : big_) f(k, v);
  }

 private:
  std::pair<K*, V> inl_[N];
  size_t n_ = 0;
  std::unordered_map<K*, V> big_;
};

// n values of a trivially copyable T, inline up to N, on the heap beyond.
template <class T, size_t N = 16>
class SmallBuf {
 public:
  explicit SmallBuf(size_t n, const T& init = T{}) : n_(n) {
    if (n > N) {
      heap_.assign(n, init);
      p_ = heap_.data();
    } else {
      p_ = inl_;
      for (size_t i = 0; i < n; i++) inl_[i] = init;
    }
  }
  SmallBuf(const SmallBuf&) = delete;
  SmallBuf& operator=(const SmallBuf&) = delete;
  T& operator[](size_t i) { return p_[i]; }
  const T& operator[](size_t i) const { return p_[i]; }
  T* begin() { return p_; }
  T* end() { return p_ + n_; }
  size_t size() const { return n_; }

 private:
  T inl_[N];
  std::vector<T> heap_;
  T* p_;
  size_t n_;
};

// A list of a trivially copyable T that grows by push_back: the first N values
// live inside the object, all of them on the heap once it outgrows N. For the
// mapper's candidate lists, which hold a handful of cells and are built anew
// at every level of its recursion (one list per depth, each on its own frame).
template <class T, size_t N = 16>
class SmallVec {
 public:
  SmallVec() {}
  SmallVec(const SmallVec&) = delete;
  SmallVec& operator=(const SmallVec&) = delete;
  size_t size() const { return n_; }
  bool empty() const { return n_ == 0; }
  T* begin() { return p_; }
  T* end() { return p_ + n_; }
  const T* begin() const { return p_; }
  const T* end() const { return p_ + n_; }
  T& operator[](size_t i) { return p_[i]; }
  const T& operator[](size_t i) const { return p_[i]; }
  T& back() { return p_[n_ - 1]; }
  void clear() { n_ = 0; }
  void pop_back() { n_--; }
  void push_back(const T& v) {
    if (n_ == cap_) grow();
    p_[n_++] = v;
  }

 private:
  void grow() {
    std::vector<T> bigger(2 * cap_);
    std::copy(p_, p_ + n_, bigger.begin());
    heap_.swap(bigger);
    p_ = heap_.data();
    cap_ = heap_.size();
  }
  T inl_[N];
  std::vector<T> heap_;
  T* p_ = inl_;
  size_t n_ = 0;
  size_t cap_ = N;
};

// Stable sort without std::stable_sort's heap-allocated merge buffer while
// the range is short (an insertion sort, which is stable too, so both give
// the same order).
template <class It, class Less>
void stableSortSmall(It first, It last, Less less) {
  if (last - first > 16) {
    std::stable_sort(first, last, less);
    return;
  }
  for (It i = first == last ? last : first + 1; i != last; ++i) {
    auto moving = *i;
    It j = i;
    for (; j != first && less(moving, *(j - 1)); --j) *j = *(j - 1);
    *j = moving;
  }
}

// ---------------------------------------------------------------------------
// Containers keyed by a pod's leaf-cell count. A group has one to three
// distinct counts and a node has 8 leaves, so these keep their entries inside
// the object and touch the heap only beyond that.
// ---------------------------------------------------------------------------

// int -> V for a handful of keys (a group's leaf-cell counts, the priorities in
// use under a cell), as a sorted small vector: the first N entries inline, all
// of them in a heap vector beyond N. Iteration is in ascending key order,
// exactly as std::map<int, V> gives it; generateResult emits memberBindInfo in
// that order. It has the part of std::map's interface its users need. Unlike
// std::map, an insertion or erasure moves the entries behind it: a reference
// or iterator is good only until the next one.
template <class V, size_t N = 4>
class FlatIntMap {
 public:
  using value_type = std::pair<int, V>;
  using iterator = value_type*;
  using const_iterator = const value_type*;

  FlatIntMap() {}
  FlatIntMap(const FlatIntMap& o) : spill_(o.spill_) {
    for (; n_ < o.n_; n_++) new (inl() + n_) value_type(o.inl()[n_]);
  }
  FlatIntMap(FlatIntMap&& o) noexcept : spill_(std::move(o.spill_)) {
    for (; n_ < o.n_; n_++) new (inl() + n_) value_type(std::move(o.inl()[n_]));
    o.clear();
  }
  FlatIntMap& operator=(const FlatIntMap& o) {
    if (this == &o) return *this;
    clear();
    for (; n_ < o.n_; n_++) new (inl() + n_) value_type(o.inl()[n_]);
    spill_ = o.spill_;
    return *this;
  }
  FlatIntMap& operator=(FlatIntMap&& o) noexcept {
    if (this == &o) return *this;
    clear();
    for (; n_ < o.n_; n_++) new (inl() + n_) value_type(std::move(o.inl()[n_]));
    spill_ = std::move(o.spill_);
    o.clear();
    return *this;
  }
  ~FlatIntMap() { clear(); }

  bool empty() const { return size() == 0; }
  size_t size() const { return spill_.empty() ? n_ : spill_.size(); }
  iterator begin() { return spill_.empty() ? inl() : spill_.data(); }
  iterator end() { return begin() + size(); }
  const_iterator begin() const { return spill_.empty() ? inl() : spill_.data(); }
  const_iterator end() const { return begin() + size(); }

  iterator find(int k) {
    iterator it = lowerBound(k);
    return it != end() && it->first == k ? it : end();
  }
  const_iterator find(int k) const { return const_cast<FlatIntMap*>(this)->find(k); }
  size_t count(int k) const { return find(k) != end() ? 1 : 0; }
  V& at(int k) {
    iterator it = find(k);
    if (it == end()) throw std::out_of_range("FlatIntMap::at");
    return it->second;
  }
  const V& at(int k) const { return const_cast<FlatIntMap*>(this)->at(k); }
  V& operator[](int k) {
    iterator it = lowerBound(k);
    if (it != end() && it->first == k) return it->second;
    const size_t pos = static_cast<size_t>(it - begin());
    if (spill_.empty() && n_ < N) {
      if (pos == n_) {
        new (inl() + n_) value_type(k, V{});
      } else {
        new (inl() + n_) value_type(std::move(inl()[n_ - 1]));
        for (size_t i = n_ - 1; i > pos; i--) inl()[i] = std::move(inl()[i - 1]);
        inl()[pos] = value_type(k, V{});
      }
      n_++;
      return inl()[pos].second;
    }
    if (spill_.empty()) {
      spill_.reserve(2 * N);
      for (size_t i = 0; i < n_; i++) spill_.push_back(std::move(inl()[i]));
      destroyInline();
    }
    return spill_.insert(spill_.begin() + static_cast<std::ptrdiff_t>(pos), value_type(k, V{}))
        ->second;
  }
  size_t erase(int k) {
    iterator it = find(k);
    if (it == end()) return 0;
    if (!spill_.empty()) {
      spill_.erase(spill_.begin() + (it - spill_.data()));
      return 1;
    }
    for (iterator j = it; j + 1 != end(); ++j) *j = std::move(*(j + 1));
    inl()[--n_].~value_type();
    return 1;
  }
  void clear() {
    destroyInline();
    spill_.clear();
  }

 private:
  iterator lowerBound(int k) {
    iterator it = begin();
    for (iterator e = end(); it != e && it->first < k; ++it) {
    }
    return it;
  }
  value_type* inl() { return reinterpret_cast<value_type*>(raw_); }
  const value_type* inl() const { return reinterpret_cast<const value_type*>(raw_); }
  void destroyInline() {
    while (n_ > 0) inl()[--n_].~value_type();
  }
  // the first n_ slots hold entries; an empty map has constructed nothing
  alignas(value_type) unsigned char raw_[N * sizeof(value_type)];
  size_t n_ = 0;  // entries in raw_; 0 while spill_ holds them
  std::vector<value_type> spill_;
};

// The map under the name its main users know it by: keyed by leaf-cell count.
template <class V, size_t N = 4>
using FlatLeafMap = FlatIntMap<V, N>;

// The leaf cells of one pod inside a PodCells block.
template <class P>
struct CellRow {
  P* p = nullptr;
  size_t n = 0;
  P* begin() const { return p; }
  P* end() const { return p + n; }
  size_t size() const { return n; }
  bool empty() const { return n == 0; }
  P& operator[](size_t i) const { return p[i]; }
};

// pods -> leaf cells for one leaf-cell count: a pods x leaves block of cell
// pointers in one piece, inline up to N pointers (one pod of a whole node),
// on the heap beyond. pods[pi][li], pods.size(), pods[pi].size() and the
// nested range-for read as they do on a vector of vectors; every pod of a
// block has the same number of leaves.
template <class T, size_t N = 8>
class PodCells {
 public:
  using Row = CellRow<T*>;
  using ConstRow = CellRow<T* const>;
  template <class P>
  class RowIter {
   public:
    RowIter(P* base, size_t cols, size_t i) : base_(base), cols_(cols), i_(i) {}
    CellRow<P>& operator*() const {
      row_ = CellRow<P>{base_ + i_ * cols_, cols_};
      return row_;
    }
    RowIter& operator++() {
      i_++;
      return *this;
    }
    bool operator!=(const RowIter& o) const { return i_ != o.i_; }
    bool operator==(const RowIter& o) const { return i_ == o.i_; }

   private:
    P* base_;
    size_t cols_;
    size_t i_;
    mutable CellRow<P> row_;
  };

  PodCells() {}
  PodCells(const PodCells& o) : heap_(o.heap_), rows_(o.rows_), cols_(o.cols_) { copyInline(o); }
  PodCells& operator=(const PodCells& o) {
    if (this == &o) return *this;
    heap_ = o.heap_;
    rows_ = o.rows_;
    cols_ = o.cols_;
    copyInline(o);
    return *this;
  }
  PodCells(PodCells&& o) noexcept : heap_(std::move(o.heap_)), rows_(o.rows_), cols_(o.cols_) {
    copyInline(o);
    o.clear();
  }
  PodCells& operator=(PodCells&& o) noexcept {
    if (this == &o) return *this;
    heap_ = std::move(o.heap_);
    rows_ = o.rows_;
    cols_ = o.cols_;
    copyInline(o);
    o.clear();
    return *this;
  }

  size_t size() const { return rows_; }
  bool empty() const { return rows_ == 0; }
  Row operator[](size_t pod) { return Row{data() + pod * cols_, cols_}; }
  ConstRow operator[](size_t pod) const { return ConstRow{data() + pod * cols_, cols_}; }
  RowIter<T*> begin() { return {data(), cols_, 0}; }
  RowIter<T*> end() { return {data(), cols_, rows_}; }
  RowIter<T* const> begin() const { return {data(), cols_, 0}; }
  RowIter<T* const> end() const { return {data(), cols_, rows_}; }

  void clear() {
    heap_.clear();
    rows_ = cols_ = 0;
  }
  // pods x leaves, every cell null
  void assign(size_t pods, size_t leaves) {
    clear();
    rows_ = pods;
    cols_ = leaves;
    if (pods * leaves > N) {
      heap_.assign(pods * leaves, nullptr);
    } else {
      std::fill(inl_, inl_ + pods * leaves, nullptr);
    }
  }
  // One more pod with `leaves` null cells; the caller fills the row handed out.
  T** appendPod(size_t leaves) {
    if (rows_ == 0) cols_ = leaves;
    if (leaves != cols_) throw std::logic_error("PodCells: pods of one block differ in size");
    const size_t have = rows_ * cols_;
    if (!heap_.empty() || have + cols_ > N) {
      if (heap_.empty()) heap_.assign(inl_, inl_ + have);
      heap_.resize(have + cols_, nullptr);
    } else {
      std::fill(inl_ + have, inl_ + have + cols_, nullptr);
    }
    rows_++;
    return data() + have;
  }

 private:
  T** data() { return heap_.empty() ? inl_ : heap_.data(); }
  T* const* data() const { return heap_.empty() ? inl_ : heap_.data(); }
  // after heap_ / rows_ / cols_ are o's: the cells o keeps inline
  void copyInline(const PodCells& o) {
    if (heap_.empty()) std::copy(o.inl_, o.inl_ + rows_ * cols_, inl_);
  }
  T* inl_[N];             // the first rows_ * cols_ are cells, the rest is unset
  std::vector<T*> heap_;  // all cells once they outgrow inl_
  size_t rows_ = 0;
  size_t cols_ = 0;
};

// A vector whose first N elements live inside the object; all of them move to
// the heap once it grows beyond N. Only what the pod slots of a group need.
template <class T, size_t N = 1>
class InlineVec {
 public:
  size_t size() const { return heap_.empty() ? n_ : heap_.size(); }
  bool empty() const { return size() == 0; }
  T* begin() { return heap_.empty() ? inl_ : heap_.data(); }
  T* end() { return begin() + size(); }
  const T* begin() const { return heap_.empty() ? inl_ : heap_.data(); }
  const T* end() const { return begin() + size(); }
  T& operator[](size_t i) { return begin()[i]; }
  const T& operator[](size_t i) const { return begin()[i]; }
  void resize(size_t n) {
    if (heap_.empty() && n <= N) {
      for (size_t i = n; i < n_; i++) inl_[i] = T{};
      n_ = n;
      return;
    }
    if (heap_.empty()) {
      heap_.reserve(n);
      for (size_t i = 0; i < n_; i++) {
        heap_.push_back(std::move(inl_[i]));
        inl_[i] = T{};
      }
      n_ = 0;
    }
    heap_.resize(n);
  }
  void clear() { resize(0); }

 private:
  T inl_[N];
  size_t n_ = 0;  // elements in inl_; 0 while heap_ holds them
  std::vector<T> heap_;
};

// ---------------------------------------------------------------------------
// Cell model
// ---------------------------------------------------------------------------
struct Group;
struct PhysicalCell;
struct VirtualCell;
struct ChainState;
struct VCChainState;

struct Cell {
  std::string chain;        // top-level cell type name identifying the chain
  ChainState* cs = nullptr; // that chain's record (see ChainState)
  int level = 0;            // 1 = leaf
  int totalLeaf = 0;        // number of leaf cells contained
  std::string address;      // unique address
  std::string typeName;     // cell type name at this level
  bool atOrAboveNode = false;
  bool isNodeLevel = false;
  Cell* parent = nullptr;
  std::vector<Cell*> children;
  int priority = kFreePriority;
  bool healthy = true;
  // priority -> used leaf-cell count (rolled up the ancestor path)
  FlatIntMap<int> usedLeafAtPriority;  // iterated in ascending priority
  // count of leaves under this cell at kFreePriority, maintained by
  // setCellPriority on leaf free<->used transitions. Together with
  // usedLeafAtPriority this gives the placement engine O(#priorities)
  // availability per node instead of an O(subtree) walk — the filter
  // hot path's dominant cost at cluster scale (gprof: availLeaves was
  // 100% of flat samples before this cache).
  int freeLeavesUnder = 0;

  explicit Cell(bool physical_) : physical(physical_) {}
  virtual ~Cell() = default;
  const bool physical;  // a PhysicalCell, else a VirtualCell
  bool isPhysical() const { return physical; }
  int usedAt(int p) const {
    auto it = usedLeafAtPriority.find(p);
    return it == usedLeafAtPriority.end() ? 0 : it->second;
  }
};

struct PhysicalCell : Cell {
  std::vector<std::string> nodes;  // node names covered (size 1 at/below node level)
  std::vector<int> leafIndices;    // leaf (GPU) indices, within-node
  CState state = CState::Free;
  bool split = false;   // children are in the free list instead of this cell
  bool pinned = false;
  std::string pinnedId;
  VirtualCell* virt = nullptr;       // bound virtual cell
  Group* usingGroup = nullptr;       // Allocated / BeingPreempted group (leaf only)
  Group* reservingGroup = nullptr;   // Preempting group (leaf only)
  std::string otVC;                  // VC using this cell opportunistically
  // MI355X hardware attributes (BASELINE north star: 288 GB HBM and
  // xGMI-link health as first-class cell attributes)
  long long hbmBytes = 0;
  // count of degraded xGMI links whose BOTH endpoints are leaves under this
  // cell (leaf cells: 0). Rolled up from setXgmiLinkHealthy: the LCA of the
  // link's endpoints and all its ancestors carry the count. A link-degraded
  // pair/quad stays usable for placements that avoid co-placing the two
  // endpoints (and for 1-GPU work) — unlike leaf badness, which removes the
  // GPU entirely. Extends the reference's healthiness seam (cell.go:302-312)
  // with a per-link dimension.
  int badLinksUnder = 0;
  // leaf cells only: peer leaves connected by a currently-degraded link
  std::vector<PhysicalCell*> badLinkPeers;
  PhysicalCell() : Cell(true) {}
};

// One xGMI link's measured state (node-local, endpoints are GPU indices).
struct XgmiLink {
  PhysicalCell* a = nullptr;  // leaf cells, a->leafIndices[0] < b->leafIndices[0]
  PhysicalCell* b = nullptr;
  double gbps = 0.0;          // measured bandwidth (0 = not measured)
  bool healthy = true;
};

struct VirtualCell : Cell {
  std::string vc;
  VirtualCell* preassigned = nullptr;  // root ancestor in the VC forest
  PhysicalCell* phys = nullptr;        // bound physical cell
  std::string pinnedId;                // non-empty if in a pinned pool
  // the record of this cell's VC on this cell's chain (see VCChainState)
  VCChainState* vcChain = nullptr;
  VirtualCell() : Cell(false) {}
};

// Level-indexed cell lists for one chain (index 1..top).
struct ChainCellList {
  std::vector<std::vector<Cell*>> byLevel;  // byLevel[0] unused
  int top() const { return static_cast<int>(byLevel.size()) - 1; }
  void init(int topLevel) { byLevel.assign(topLevel + 1, {}); }
  std::vector<Cell*>& at(int l) { return byLevel[l]; }
  const std::vector<Cell*>& at(int l) const { return byLevel[l]; }
  bool contains(Cell* c, int l) const {
    if (l < 0 || l >= static_cast<int>(byLevel.size())) return false;
    auto& v = byLevel[l];
    return std::find(v.begin(), v.end(), c) != v.end();
  }
  void remove(Cell* c, int l) {
    auto& v = byLevel[l];
    auto it = std::find(v.begin(), v.end(), c);
    if (it == v.end()) throw HivedError::Internal("cell not found in list when removing: " + c->address);
    *it = v.back();
    v.pop_back();
  }
  void add(Cell* c, int l) { byLevel[l].push_back(c); }
  ChainCellList shallowCopy() const { return *this; }
};

// ---------------------------------------------------------------------------
// Affinity groups
// ---------------------------------------------------------------------------
struct PodPlacementInfo {
  std::string node;
  std::vector<int> leafIndices;
  std::vector<std::string> preassignedTypes;
};
struct BindInfo {
  std::string node;
  std::vector<int> isolation;
  std::string chain;
  // one entry per distinct leafCellNumber; each has podPlacements
  std::vector<std::vector<PodPlacementInfo>> memberBindInfo;
};

struct AllocatedPod {
  bool present = false;
  std::string key;   // "ns/name"
  std::string node;
  // the group's full bind info as the deciding pod saw it; immutable, and
  // shared with the ScheduleResult it was decided in (see HivedCore::addAllocatedPod)
  std::shared_ptr<const BindInfo> bindInfo;
};
using PodSlots = InlineVec<AllocatedPod, 1>;

// Placement = leafCellNum -> pods -> leaf cells
template <class CellT>
using Placement = FlatLeafMap<PodCells<CellT>>;

struct LazyPreemptionStatus {
  std::string preemptor;
  std::string preemptionTime;
};

struct Group {
  std::string name;
  std::string vc;
  bool lazyPreemptionEnable = false;
  bool ignoreK8sSuggestedNodes = true;
  bool gangReleaseEnable = false;
  int priority = 0;
  GState state = GState::Allocated;
  FlatLeafMap<int> totalPodNums;  // leafCellNum -> pod count
  FlatLeafMap<PodSlots> allocatedPods;
  // leafCellNum -> pods -> leaf cells (entries may be null after reconfig)
  Placement<PhysicalCell> physPlacement;
  bool hasVirtualPlacement = true;  // false for opportunistic / lazy-preempted
  Placement<VirtualCell> virtPlacement;
  std::set<std::string> preemptingPods;  // pod keys (Preempting state only)
  std::optional<LazyPreemptionStatus> lazyStatus;
  // back to the state of a default-constructed Group; the strings keep their
  // capacity (HivedCore's group pool)
  void reset() {
    name.clear();
    vc.clear();
    lazyPreemptionEnable = false;
    ignoreK8sSuggestedNodes = true;
    gangReleaseEnable = false;
    priority = 0;
    state = GState::Allocated;
    totalPodNums.clear();
    allocatedPods.clear();
    physPlacement.clear();
    hasVirtualPlacement = true;
    virtPlacement.clear();
    preemptingPods.clear();
    lazyStatus.reset();
  }
};

// ---------------------------------------------------------------------------
// Normalized cluster spec (filled from Python)
// ---------------------------------------------------------------------------
struct CellTypeSpec {
  std::string child;  // empty = leaf
  int childCount = 0;
  bool isNode = false;
};
struct PhysCellSpec {
  std::string type;
  std::string address;
  std::string pinnedId;
  std::vector<PhysCellSpec> children;
  // measured per-GPU HBM capacity in bytes (0 = unknown); leaf entries only
  long long hbmBytes = 0;
  // measured xGMI links (a, b, gbps, healthy); node-level entries only,
  // emitted by rocm-topo-discover
  std::vector<std::tuple<int, int, double, bool>> xgmiLinks;
};
struct VirtCellSpec {
  std::string typePath;  // "TOP.CHILD....", chain = first component
  int number = 0;
};
struct VCSpec {
  std::vector<VirtCellSpec> virtualCells;
  std::vector<std::string> pinnedIds;
};
struct ClusterSpec {
  std::map<std::string, CellTypeSpec> cellTypes;
  std::vector<PhysCellSpec> physicalCells;
  std::map<std::string, VCSpec> virtualClusters;
};

// ---------------------------------------------------------------------------
// Scheduling request / result
// ---------------------------------------------------------------------------
struct PodSpec {
  std::string vc;
  int priority = 0;
  std::string pinnedCellId;
  std::string leafCellType;
  int leafCellNumber = 0;
  bool gangReleaseEnable = false;
  bool lazyPreemptionEnable = false;
  bool ignoreK8sSuggestedNodes = true;
  std::string groupName;
  FlatLeafMap<int> groupPodNums;  // leafCellNum -> pod count
  // optional: minimum measured HBM per leaf cell (bytes); leaves below are
  // unavailable for this request (MI355X: a GPU reporting < 288 GB is sick)
  long long hbmBytesPerCell = 0;
};

enum class Phase { Filtering, Preempting };

struct ScheduleResult {
  enum class Kind { Bind, Preempt, Wait } kind = Kind::Wait;
  // Bind: built once by the decision and never changed afterwards. The result
  // owns this handle; a commit that is handed the same handle stores it in the
  // pod's slot instead of copying, and whoever lets go last frees it.
  std::shared_ptr<const BindInfo> bindInfo;
  // Preempt: victims on one node (gang semantics: whole victim groups)
  std::string victimNode;
  std::vector<std::string> victimPodKeys;
  // Wait
  std::string waitReason;
};

// One globally consistent link-clean view of a chain's free capacity:
// `excluded` = the physical leaves dropped (per-node max independent set of
// the degraded-link graph restricted to free leaves); `caps` = per-level max
// in-world free capacity of any single physical cell.
struct CleanShapeWorld {
  // the scheduling tier this world models: in-world availability counts
  // leaves below this priority (kOpportunisticPriority = free cells only;
  // a request's own priority = free + preemptible)
  int priority = kOpportunisticPriority;
  std::map<int, int> caps;
  std::unordered_set<PhysicalCell*> excluded;
  // unbound physical cells per level, for hint resolution when no bound
  // ancestor scopes the candidates (see topo_sched.cpp pickLeavesWorld)
  std::map<int, std::vector<PhysicalCell*>> physByLevel;
};

class TopoScheduler;
struct IntraVCScheduler;

// One request on its way through the core. The strings and the pod-number map
// are the PodSpec's own (the request lives inside one HivedCore::schedule call,
// the spec outlives it), so building a request copies nothing.
struct SchedulingRequest {
  explicit SchedulingRequest(const PodSpec& s)
      : vc(s.vc),
        pinnedCellId(s.pinnedCellId),
        groupName(s.groupName),
        podLeafCellNums(s.groupPodNums),
        priority(s.priority) {}
  const std::string& vc;
  const std::string& pinnedCellId;
  const std::string& groupName;
  const FlatLeafMap<int>& podLeafCellNums;
  // the chain being tried
  ChainState* chain = nullptr;
  // the VC's scheduler, resolved once per request, and the placement engine
  // of the chain (or pinned cell) being tried, resolved once per chain: the
  // attempts themselves look nothing up by name
  IntraVCScheduler* vcScheduler = nullptr;
  const TopoScheduler* topo = nullptr;
  int priority = 0;
  const std::set<std::string>* suggestedNodes = nullptr;
  bool ignoreSuggestedNodes = true;
  long long hbmBytes = 0;  // minimum per-leaf HBM capacity (0 = any)
  // Clean-shape world, set only when the chain carries degraded xGMI links
  // and the gang needs >= 2 leaves: ONE globally consistent choice of
  // link endpoints to avoid. The virtual descent's link-honoring attempts
  // schedule inside this world (excluded leaves unavailable; unbound
  // subtrees capped by the best physical cell's in-world capacity; bound
  // subtrees min-capped by their physical region's in-world capacity), so
  // a request whose clean mapping needs a lower-affinity shape picks that
  // shape up front instead of falling to a dirty placement. Dirty rungs
  // run without the world, so capacity is never sacrificed.
  const CleanShapeWorld* cleanWorld = nullptr;
  // run only the link-honoring placement rungs (the caller iterates over
  // several clean-shape worlds and provides the dirty fallback itself)
  bool honorLinksOnly = false;
};

// ---------------------------------------------------------------------------
// Topology-aware placement engine
// ---------------------------------------------------------------------------
// Places pods onto a cluster view (list of node-level cells, or top-level cells
// below node level) sorted healthy > suggested > packing; inside a node, a
// best-fit recursive descent picks leaf cells with minimal LCA level.
class TopoScheduler {
 public:
  TopoScheduler() = default;
  TopoScheduler(const ChainCellList& ccl, std::map<int, int> levelLeafNum, bool crossPriorityPack);

  // Returns placement or empty with failedReason set. minHbmBytes > 0
  // filters out leaves whose measured HBM capacity falls short.
  // cleanWorld (optional): see SchedulingRequest::cleanWorld.
  // The engine places generic cells; a view holds cells of one kind, and the
  // caller names that kind (VirtualCell for a VC's view, PhysicalCell for the
  // opportunistic one) so that the placement is written typed, once.
  template <class CellT>
  bool Schedule(const FlatLeafMap<int>& podLeafCellNums, int priority,
                const std::set<std::string>& suggestedNodes, bool ignoreSuggestedNodes,
                Placement<CellT>* out, std::string* failedReason, long long minHbmBytes = 0,
                const CleanShapeWorld* cleanWorld = nullptr, bool honorOnly = false) const {
    PlacementSink sink{out, [](void* to) { static_cast<Placement<CellT>*>(to)->clear(); },
                       [](void* to, int leafNum, const std::vector<Cell*>& leaves) {
                         CellT** row = (*static_cast<Placement<CellT>*>(to))[leafNum].appendPod(
                             leaves.size());
                         for (size_t i = 0; i < leaves.size(); i++) {
                           row[i] = static_cast<CellT*>(leaves[i]);
                         }
                       }};
    return scheduleInto(podLeafCellNums, priority, suggestedNodes, ignoreSuggestedNodes, sink,
                        failedReason, minHbmBytes, cleanWorld, honorOnly);
  }

 private:
  struct NodeView {
    Cell* c = nullptr;
    int freeAtPriority = 0;
    int usedSamePriority = 0;
    int usedHigherPriority = 0;
    bool healthy = true;
    bool suggested = true;
  };
  // where a successful attempt writes its placement: one pod's leaves at a
  // time, filed under their number
  struct PlacementSink {
    void* to;
    void (*clear)(void* to);
    void (*addPod)(void* to, int leafNum, const std::vector<Cell*>& leaves);
  };
  bool scheduleInto(const FlatLeafMap<int>& podLeafCellNums, int priority,
                    const std::set<std::string>& suggestedNodes, bool ignoreSuggestedNodes,
                    const PlacementSink& out, std::string* failedReason, long long minHbmBytes,
                    const CleanShapeWorld* cleanWorld, bool honorOnly) const;
  bool tryScheduleAtPriority(const std::vector<int>& sortedLeafNums, int priority,
                             const std::set<std::string>& suggestedNodes, bool ignoreSuggestedNodes,
                             long long minHbmBytes, bool honorLinks,
                             const CleanShapeWorld* cleanWorld, const PlacementSink& out,
                             std::string* failedReason) const;

  std::vector<Cell*> viewCells_;
  std::map<int, int> levelLeafNum_;
  bool crossPriorityPack_ = false;
  // Reused by every Schedule call so that a failing decision allocates
  // nothing here (see the note on re-entrance in Schedule).
  struct Scratch {
    std::vector<NodeView> view;
    std::vector<int> sortedLeafNums;
    std::vector<int> pickedNodeIndices;
    std::vector<Cell*> leaves;  // of the pod being placed
  };
  mutable Scratch scratch_;
};

// ---------------------------------------------------------------------------
// Chain state
// ---------------------------------------------------------------------------
// Clean-shape worlds of one (chain, tier), validated against
// gWorldEpochCounter (bumped by every mutation that can change a world: leaf
// priorities, bindings, health, links). Wait-storms — the common case under
// contention: many failed filters with no allocation in between — reuse cached
// worlds instead of recomputing them per Schedule.
struct WorldCacheEntry {
  unsigned long long epoch = 0;
  std::vector<CleanShapeWorld> worlds;
};

// Everything the core keeps per chain, in one record that every cell of the
// chain points to (Cell::cs): the hot path reaches it from the cell in hand
// and looks nothing up by the chain's name. Built once by the cluster-spec
// compiler; HivedCore::chainStates_ owns the records and is the name-ordered
// index the cold paths (status, debug, health setters) iterate. The per-level
// vectors are indexed by level, 1..top; [0] is unused.
struct ChainState {
  std::string name;
  int index = 0;  // dense, in name order (IntraVCScheduler::byChain)
  int top = 0;
  ChainCellList full;     // every physical cell
  ChainCellList free;     // the buddy free list
  ChainCellList badFree;  // bad cells that are free (directly or via an unsplit ancestor)
  std::vector<std::string> levelType;  // cell type name
  std::vector<int> totalLeft;          // cells the free list can still produce
  std::vector<int> allVCFree;          // free preassigned cells, all VCs together
  std::vector<int> allVCDoomedBadCellNum;
  // the VCs with quota (or a pinned cell) in this chain, in VC-name order
  std::vector<VCChainState*> vcs;
  TopoScheduler opportunistic;  // placement engine over the physical cells
  std::map<int, WorldCacheEntry> worldCache;  // by tier
};

// One VC's share of one chain. Reached from the VC's scheduler
// (IntraVCScheduler::byChain) and from every virtual cell (VirtualCell::vcChain).
struct VCChainState {
  std::string vc;
  ChainState* chain = nullptr;
  std::vector<int> free;  // free preassigned cells by level
  ChainCellList doomed;   // bad physical cells bound to this VC's free cells
  // the VC's preassigned cells and its placement engine on this chain; null
  // where the VC has only a pinned cell there
  const ChainCellList* preassigned = nullptr;
  const TopoScheduler* topo = nullptr;
};

// ---------------------------------------------------------------------------
// Intra-VC scheduler
// ---------------------------------------------------------------------------
struct IntraVCScheduler {
  // by ChainState::index; null for a chain this VC has nothing in
  std::vector<VCChainState*> byChain;
  std::map<std::string, ChainCellList> nonPinnedFull;         // chain -> all virtual cells
  std::map<std::string, ChainCellList> nonPinnedPreassigned;  // chain -> preassigned cells
  std::map<std::string, ChainCellList> pinned;                // pinnedId -> subtree cells
  std::map<std::string, TopoScheduler> nonPinnedSchedulers;   // per chain
  std::map<std::string, TopoScheduler> pinnedSchedulers;      // per pinnedId

  bool schedule(const SchedulingRequest& sr, Placement<VirtualCell>* out, std::string* failedReason) const;
};

// A vertex in a cell-binding path: a tree of unbound virtual cells that need
// physical bindings, preserving intra-cell topology.
// The vertices of one mapping attempt belong to HivedCore::MapScratch.
struct BindingVertex {
  VirtualCell* cell = nullptr;
  std::vector<BindingVertex*> children;
};

// The pods a placement would evict, as (node, pod key) pairs: after seal() in
// ascending node order and, within a node, ascending key order, each pair once.
// That is the view a std::map<node, std::set<key>> gives: the victim node is
// picked by its position in node order, and the keys go out in key order. The
// strings are the victim groups' own (their AllocatedPod slots), which outlive
// the decision that collects them; the vector keeps its capacity between
// decisions, and one with no victims touches nothing.
class VictimList {
 public:
  bool empty() const { return pods_.empty(); }
  void clear() {
    pods_.clear();
    nodes_ = 0;
  }
  void add(const std::string& node, const std::string& key) { pods_.push_back({&node, &key}); }
  void seal() {
    auto less = [](const Entry& a, const Entry& b) {
      const int c = a.first->compare(*b.first);
      return c != 0 ? c < 0 : *a.second < *b.second;
    };
    auto same = [](const Entry& a, const Entry& b) {
      return *a.first == *b.first && *a.second == *b.second;
    };
    std::sort(pods_.begin(), pods_.end(), less);
    pods_.erase(std::unique(pods_.begin(), pods_.end(), same), pods_.end());
    nodes_ = 0;
    for (size_t i = 0; i < pods_.size(); i++) {
      if (i == 0 || *pods_[i].first != *pods_[i - 1].first) nodes_++;
    }
  }
  size_t nodeCount() const { return nodes_; }
  // the index-th node in name order and its pod keys in key order
  void nodeAt(size_t index, std::string* node, std::vector<std::string>* keys) const {
    size_t at = 0;
    size_t i = 0;
    for (; i < pods_.size(); i++) {
      if (i > 0 && *pods_[i].first != *pods_[i - 1].first) at++;
      if (at == index) break;
    }
    *node = *pods_[i].first;
    size_t last = i;
    while (last < pods_.size() && *pods_[last].first == *node) last++;
    keys->clear();
    keys->reserve(last - i);  // one allocation, whatever the number of keys
    for (; i < last; i++) keys->push_back(*pods_[i].second);
  }

 private:
  using Entry = std::pair<const std::string*, const std::string*>;
  std::vector<Entry> pods_;
  size_t nodes_ = 0;
};

// virtual cell -> the physical cell one mapping attempt gives it
using CellBindings = SmallPtrMap<VirtualCell, PhysicalCell*, 32>;

// ---------------------------------------------------------------------------
// The algorithm facade
// ---------------------------------------------------------------------------
class HivedCore {
 public:
  explicit HivedCore(const ClusterSpec& spec);
  ~HivedCore();

  // -- node health (informer events) --
  void setNodeHealthy(const std::string& node, bool healthy);
  // -- GPU/xGMI-level health (rocm-smi exporter / probe events): marks one
  // leaf cell; badness rolls up to pair/quad/node cells automatically --
  void setLeafCellHealthy(const std::string& node, int leafIndex, bool healthy);
  // -- xGMI link health: a degraded link between two GPUs of one node marks
  // the LINK (first-class), not the endpoint leaves: multi-GPU placements
  // avoid co-placing the endpoints while 1-GPU work still uses them --
  void setXgmiLinkHealthy(const std::string& node, int a, int b, bool healthy,
                          double gbps = 0.0);
  // per-node link table for inspect: (a, b, gbps, healthy)
  std::vector<std::tuple<int, int, double, bool>> xgmiLinks(const std::string& node) const;
  std::vector<std::string> allNodes() const;
  std::set<std::string> badNodes() const { return badNodes_; }

  // -- scheduling --
  ScheduleResult schedule(const PodSpec& s, const std::string& podKey,
                          const std::set<std::string>& suggestedNodes, Phase phase);
  void deleteUnallocatedPod(const PodSpec& s, const std::string& podKey);
  // Commits a pod. A bind info from outside (replay, a caller's own record) is
  // copied once into the pod's slot; the handle of the decision's own result is
  // stored as it is, so decision, result and slot share one BindInfo.
  void addAllocatedPod(const PodSpec& s, const BindInfo& info, const std::string& podKey);
  void addAllocatedPod(const PodSpec& s, const std::shared_ptr<const BindInfo>& info,
                       const std::string& podKey);
  void deleteAllocatedPod(const PodSpec& s, const BindInfo& info, const std::string& podKey);
  // deleteAllocatedPod for the spec and bind info the pod was added with, found
  // through podIndex_ instead of being handed back. Answers false, and changes
  // nothing, for a key the index does not hold (never added, already released,
  // or added to a core that has since been rebuilt and not yet replayed).
  bool deleteAllocatedPodByKey(const std::string& podKey);

  // -- inspect --
  const std::map<std::string, std::unique_ptr<Group>>& groups() const { return groups_; }
  const std::map<std::string, IntraVCScheduler>& vcSchedulers() const { return vcSchedulers_; }
  std::vector<std::string> chains() const;
  std::map<int, std::string> chainLevelTypes(const std::string& chain) const;

 private:
  friend struct BuildContext;

  // --- construction ---
  void buildFromSpec(const ClusterSpec& spec);
  void initCellNums();
  void initPinnedCells();
  void initBadNodes();

  // --- health ---
  void setBadCell(PhysicalCell* c);
  void setHealthyCell(PhysicalCell* c);
  void addBadFreeCell(PhysicalCell* c);
  void removeBadFreeCell(PhysicalCell* c);
  bool doomAllocationIsSafe(PhysicalCell* pc);
  // Doomed-bad checks are DEFERRED to the end of the enclosing top-level
  // operation (schedule commit, pod delete, health event): executing them
  // mid-operation re-enters free-list surgery against a half-updated list
  // and can consume cells an in-flight placement depends on (fuzz-found
  // corruption). tryBind/tryUnbind queue when an operation is active; the
  // bodies run from drainDoomChecks() once state is consistent.
  void tryBindDoomedBadCell(ChainState* chain, int level);
  void tryUnbindDoomedBadCell(ChainState* chain, int level);
  void doBindDoomedBadCell(ChainState* chain, int level);
  void doUnbindDoomedBadCell(ChainState* chain, int level);
  void drainDoomChecks();

  class OpGuard {
   public:
    explicit OpGuard(HivedCore* c)
        : c_(c), outer_(!c->inOperation_), exceptionsAtEntry_(std::uncaught_exceptions()) {
      c_->inOperation_ = true;
    }
    // On normal exit (including early returns) the outermost guard drains
    // the deferred doom checks; on exception unwind it only resets the flag
    // (queued checks stay pending and run at the next operation's end).
    ~OpGuard() noexcept(false) {
      if (!outer_) return;
      c_->inOperation_ = false;
      if (std::uncaught_exceptions() == exceptionsAtEntry_) c_->drainDoomChecks();
    }

   private:
    HivedCore* c_;
    bool outer_;
    int exceptionsAtEntry_;
  };

  // --- scheduling internals ---
  ScheduleResult generateResult(const Placement<PhysicalCell>& phys, bool hasVirtual,
                                const Placement<VirtualCell>& virt,
                                const VictimList& victims,
                                std::string&& waitReason, int currentLeafNum, int podIndex,
                                Group* group, const std::string& groupName);
  bool schedulePodFromExistingGroup(Group* g, const PodSpec& s,
                                    const std::set<std::string>& suggestedNodes, Phase phase,
                                    const std::string& podKey, Placement<PhysicalCell>* phys,
                                    bool* hasVirtual, Placement<VirtualCell>* virt,
                                    VictimList* victims,
                                    int* podIndex);
  Group* schedulePodFromNewGroup(const PodSpec& s, const std::set<std::string>& suggestedNodes,
                                 Phase phase, const std::string& podKey,
                                 Placement<PhysicalCell>* phys, bool* hasVirtual,
                                 Placement<VirtualCell>* virt,
                                 VictimList* victims,
                                 std::string* waitReason);
  bool scheduleNewAffinityGroup(const PodSpec& s, const std::set<std::string>& suggestedNodes,
                                const std::string& podKey, Placement<PhysicalCell>* phys,
                                bool* hasVirtual, Placement<VirtualCell>* virt,
                                std::string* failedReason);
  bool scheduleForLeafCellType(SchedulingRequest& sr, const std::string& leafCellType,
                               const std::vector<ChainState*>& chains,
                               const std::string& podKey, bool typeSpecified,
                               Placement<PhysicalCell>* phys, bool* hasVirtual,
                               Placement<VirtualCell>* virt, std::string* failedReason);
  bool handleSchedulingRequest(SchedulingRequest& sr, Placement<PhysicalCell>* phys,
                               bool* hasVirtual, Placement<VirtualCell>* virt,
                               std::string* failedReason);
  bool scheduleGuaranteedGroup(SchedulingRequest& sr, Placement<PhysicalCell>* phys,
                               Placement<VirtualCell>* virt, std::string* failedReason);
  static bool chainHasBadLinks(const ChainCellList& fullCells);
  bool scheduleOpportunisticGroup(const SchedulingRequest& sr, Placement<PhysicalCell>* phys,
                                  std::string* failedReason);
  void validateSchedulingRequest(SchedulingRequest& sr, const std::string& podKey);

  std::map<std::string, Placement<VirtualCell>> tryLazyPreempt(const Placement<VirtualCell>& p,
                                                               const std::string& groupName);

  // --- allocated-pod slots and their key index ---
  void addAllocatedPodShared(const PodSpec& s, const BindInfo& info,
                             const std::shared_ptr<const BindInfo>* shared,
                             const std::string& podKey);
  void setPodSlot(Group* g, int leafCellNum, int podIndex, bool releasable,
                  const std::string& podKey, std::shared_ptr<const BindInfo> info);
  void clearPodSlot(Group* g, int leafCellNum, int podIndex);
  void eraseGroup(Group* g);
  Group* insertNewGroup(const PodSpec& s, GState state);

  // --- group lifecycle ---
  Group* createAllocatedGroup(const PodSpec& s, const BindInfo& info, const std::string& podKey);
  void deleteAllocatedGroup(Group* g, const std::string& podKey);
  Group* createPreemptingGroup(const PodSpec& s, const Placement<PhysicalCell>& phys,
                               const Placement<VirtualCell>& virt, const std::string& podKey);
  void deletePreemptingGroup(Group* g, const std::string& podKey);
  void allocatePreemptingGroup(Group* g, const std::string& podKey);
  Placement<VirtualCell> lazyPreemptGroup(Group* victim, const std::string& preemptor);
  void lazyPreemptCell(VirtualCell* c, const std::string& preemptor);
  void revertLazyPreempt(Group* g, const Placement<VirtualCell>& virt);

  // --- leaf-cell allocate/release + safety accounting ---
  std::pair<PhysicalCell*, VirtualCell*> findAllocatedLeafCell(
      int index, const PodPlacementInfo& placement, const std::string& chain, const PodSpec& s,
      const IntraVCScheduler* vcs, const std::vector<PhysicalCell*>* nodeLeaves, Group* group,
      const std::string& podKey, bool* lazyPreempt, bool* isOpportunistic);
  std::pair<bool, std::string> allocateLeafCell(PhysicalCell* p, VirtualCell* v, int priority,
                                                const std::string& vc);
  void releaseLeafCell(PhysicalCell* p, const std::string& vc);
  std::pair<bool, std::string> allocatePreassignedCell(PhysicalCell* c, VCChainState* vc,
                                                       bool doomedBad);
  void releasePreassignedCell(PhysicalCell* c, VCChainState* vc, bool doomedBad);
  void allocateBadCell(PhysicalCell* c);
  void releaseBadCell(PhysicalCell* c);
  int removeCellFromFreeList(PhysicalCell* c);
  int addCellToFreeList(PhysicalCell* c);

  // --- mapping virtual -> physical (buddy allocation) ---
  // freeList / freeCellNum: the caller's working copies of the chain's free
  // list and allVCFree counts; both are consumed. Of nonPreassigned the
  // first nonPreassignedCount groups count.
  bool mapVirtualPlacementToPhysical(const std::vector<BindingVertex*>& preassigned,
                                     const std::vector<std::vector<BindingVertex*>>& nonPreassigned,
                                     size_t nonPreassignedCount, ChainCellList& freeList,
                                     std::vector<int>& freeCellNum,
                                     const std::set<std::string>& suggestedNodes,
                                     bool ignoreSuggestedNodes, CellBindings& bindings,
                                     long long minHbmBytes = 0, bool honorLinks = false,
                                     const CleanShapeWorld* world = nullptr);

  // What one mapping attempt of scheduleGuaranteedGroup builds and throws
  // away, kept between attempts so that its vectors and vertices are reused:
  // an attempt starts with reset(), attempts never nest (nothing an attempt
  // calls schedules), and nothing in here is read after the attempt ends.
  struct MapScratch {
    std::vector<std::unique_ptr<BindingVertex>> vertexPool;
    size_t verticesUsed = 0;
    std::vector<BindingVertex*> preassigned;
    std::vector<std::vector<BindingVertex*>> nonPreassigned;  // first ...Used count
    size_t nonPreassignedUsed = 0;
    std::vector<VirtualCell*> path;
    ChainCellList freeList;
    std::vector<int> freeCellNum;  // by level
    void reset() {
      verticesUsed = 0;
      preassigned.clear();
      nonPreassignedUsed = 0;
    }
    BindingVertex* newVertex(VirtualCell* cell) {
      if (verticesUsed == vertexPool.size()) vertexPool.push_back(std::make_unique<BindingVertex>());
      BindingVertex* v = vertexPool[verticesUsed++].get();
      v->cell = cell;
      v->children.clear();
      return v;
    }
    std::vector<BindingVertex*>& newNonPreassignedGroup() {
      if (nonPreassignedUsed == nonPreassigned.size()) nonPreassigned.emplace_back();
      std::vector<BindingVertex*>& g = nonPreassigned[nonPreassignedUsed++];
      g.clear();
      return g;
    }
  };
  MapScratch mapScratch_;
  VictimList victimScratch_;  // of the decision in progress (schedule never nests)

  // Erased groups, kept with their groups_ map node (the key string and the
  // Group object) so that the next group costs no allocation. eraseGroup is the
  // only way in, after every podIndex_ entry of the group is gone, and
  // insertNewGroup the only way out; Group::reset makes a recycled group equal
  // to a fresh one. Bounded: a burst of releases frees what exceeds it.
  using GroupNode = std::map<std::string, std::unique_ptr<Group>>::node_type;
  // (-DHIVED_GROUP_POOL_MAX=0 builds a core without the pool, to measure it)
#ifndef HIVED_GROUP_POOL_MAX
#define HIVED_GROUP_POOL_MAX 64
#endif
  static constexpr size_t kGroupPoolMax = HIVED_GROUP_POOL_MAX;
  std::vector<GroupNode> groupPool_;

 public:
  // state (public for inspect/bindings simplicity; external mutation forbidden)
  // chain name -> the chain's record; std::map nodes never move, so the
  // pointers the cells hold stay good. Iterated (in name order) by the cold
  // paths only.
  std::map<std::string, ChainState> chainStates_;
  // vc -> chain -> that VC's record on that chain, for the VCs with quota or
  // a pinned cell there
  std::map<std::string, std::map<std::string, VCChainState>> vcChainStates_;
  bool inOperation_ = false;
  std::vector<std::pair<ChainState*, int>> pendingDoomChecks_;  // (chain, level), FIFO
  std::map<std::string, IntraVCScheduler> vcSchedulers_;
  std::map<std::string, std::unique_ptr<Group>> groups_;
  // pod key -> the allocatedPods slot that holds it. Kept by setPodSlot /
  // clearPodSlot / eraseGroup, the only writers of a slot's `present`, so it
  // holds exactly the present slots (one entry per key: a key added again
  // points at the slot of its latest add). `releasable` is false for a pod
  // whose own bind info does not name its placement; deleteAllocatedPod leaves
  // such a pod alone, and so does the release by key.
  struct PodSlotRef {
    Group* group = nullptr;
    int leafCellNum = 0;
    int podIndex = 0;
    bool releasable = true;
  };
  std::unordered_map<std::string, PodSlotRef> podIndex_;

  std::set<std::string> badNodes_;
  // leaves individually marked bad (GPU/xGMI level), independent of node health
  std::set<PhysicalCell*> badLeafMarks_;
  // node -> (minIdx, maxIdx) -> link record (first-class xGMI link state)
  std::map<std::string, std::map<std::pair<int, int>, XgmiLink>> xgmiLinks_;
  // leaf type -> chains, in chain-name order
  std::map<std::string, std::vector<ChainState*>> cellChains_;
  std::map<std::string, std::map<int, int>> leafCellNums_;           // chain -> level -> leaf num
  // pinned: vc -> pinnedId -> physical cell
  std::map<std::string, std::map<std::string, PhysicalCell*>> pinnedPhysical_;

  // seeded PRNG for victim-node selection (deterministic for tests/fuzz,
  // spreads victim churn across nodes like the reference's rand)
  std::minstd_rand victimRng_{12345};
  // cell ownership
  std::vector<std::unique_ptr<Cell>> cellStore_;
  // node name -> leaf cells on that node (for health propagation)
  std::map<std::string, std::vector<PhysicalCell*>> nodeLeafCellsStorage_;
  long long scheduleCount_ = 0;
};

// helpers shared across translation units
extern unsigned long long gWorldEpochCounter;
void setCellPriority(Cell* c, int p);
void updateUsedLeafCellNumAtPriority(Cell* c, int p, bool increase);
void bindCell(PhysicalCell* pc, VirtualCell* vc);
void unbindCell(PhysicalCell* c);
VirtualCell* getUnboundVirtualCell(const std::vector<Cell*>& cl);
VirtualCell* getLowestPriorityVirtualCell(const std::vector<Cell*>& cl, int p);
VirtualCell* mapPhysicalCellToVirtual(PhysicalCell* c, const ChainCellList& vccl,
                                      int preassignedLevel, int p, std::string* message);
bool inFreeCellList(PhysicalCell* c);
void setCellState(PhysicalCell* c, CState s);
PhysicalCell* findPhysicalLeafCell(const std::map<std::string, ChainState>& chains,
                                   const std::string& chain, const std::string& node,
                                   int leafIndex);
Cell* ancestorNoHigherThanNode(Cell* c);
// the chain's clean-shape worlds: one per enumerated consistent endpoint
// choice (different max independent sets admit different clean shapes)
std::vector<CleanShapeWorld> computeCleanShapeWorlds(
    const ChainCellList& ccl, const std::set<std::string>* suggestedNodes,
    size_t maxWorlds = 4, int priority = kOpportunisticPriority);
void checkInvariants(const HivedCore& core);

}  // namespace hived
