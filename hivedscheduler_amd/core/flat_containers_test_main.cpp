// Stand-alone check of the leaf-count containers of core.hpp: FlatLeafMap
// against std::map<int, V> over random operations, PodCells against a vector
// of vectors, InlineVec and SmallVec against std::vector. No core object is linked.
// Compile and run (from hivedscheduler_amd/), on the CPU, with the sanitizers:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined
//       -o flatcontainerstest core/flat_containers_test_main.cpp && ./flatcontainerstest
// Exit status 0 and "flat containers OK" mean every comparison held.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "core.hpp"

using namespace hived;

namespace {

long gChecks = 0;

#define CHECK(cond)                                                        \
  do {                                                                     \
    gChecks++;                                                             \
    if (!(cond)) {                                                         \
      fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); \
      exit(1);                                                             \
    }                                                                      \
  } while (0)

// a value that owns heap memory twice over, so that the address sanitizer sees
// a double free, a use after free or a leak in the map's own bookkeeping
struct Owner {
  std::unique_ptr<std::string> text;
  std::vector<int> numbers;
  Owner() = default;
  explicit Owner(int v) : text(std::make_unique<std::string>(40, static_cast<char>('a' + v % 26))),
                          numbers(static_cast<size_t>(v % 5 + 1), v) {}
  Owner(const Owner& o)
      : text(o.text ? std::make_unique<std::string>(*o.text) : nullptr), numbers(o.numbers) {}
  Owner(Owner&&) = default;
  Owner& operator=(const Owner& o) {
    text = o.text ? std::make_unique<std::string>(*o.text) : nullptr;
    numbers = o.numbers;
    return *this;
  }
  Owner& operator=(Owner&&) = default;
  bool operator==(const Owner& o) const {
    if (static_cast<bool>(text) != static_cast<bool>(o.text)) return false;
    return (!text || *text == *o.text) && numbers == o.numbers;
  }
};

template <class V>
void expectSame(const FlatLeafMap<V>& flat, const std::map<int, V>& ref) {
  CHECK(flat.size() == ref.size());
  CHECK(flat.empty() == ref.empty());
  auto it = flat.begin();
  int last = 0;
  for (auto& [k, v] : ref) {  // ascending iteration, entry by entry
    CHECK(it != flat.end());
    CHECK(it->first == k);
    CHECK(it->first > last);
    CHECK(it->second == v);
    last = it->first;
    ++it;
  }
  CHECK(it == flat.end());
  for (int k = 0; k <= 13; k++) {
    CHECK(flat.count(k) == ref.count(k));
    auto found = flat.find(k);
    CHECK((found == flat.end()) == (ref.find(k) == ref.end()));
    if (found != flat.end()) CHECK(found->second == ref.at(k) && flat.at(k) == ref.at(k));
  }
}

template <class V, class Make>
void randomOperations(unsigned seed, int operations, Make make) {
  std::mt19937 rng(seed);
  FlatLeafMap<V> flat;
  std::map<int, V> ref;
  expectSame(flat, ref);
  for (int op = 0; op < operations; op++) {
    const int k = 1 + static_cast<int>(rng() % 12);
    switch (rng() % 10) {
      case 0:
      case 1:
      case 2:
      case 3: {  // insert or overwrite through operator[]
        V v = make(static_cast<int>(rng() % 1000));
        flat[k] = v;
        ref[k] = v;
        break;
      }
      case 4:  // operator[] alone: a missing key appears with a default value
        CHECK(flat[k] == ref[k]);
        break;
      case 5:
      case 6:
        CHECK(flat.erase(k) == ref.erase(k));
        break;
      case 7: {  // copy construction and copy assignment, over a non-empty target
        FlatLeafMap<V> copy(flat);
        expectSame(copy, ref);
        FlatLeafMap<V> target;
        target[3] = make(3);
        target[9] = make(9);
        target = copy;
        expectSame(target, ref);
        copy[k] = make(k);  // the copies own their values
        expectSame(flat, ref);
        flat = target;
        break;
      }
      case 8: {  // move construction and move assignment; the source is left empty
        FlatLeafMap<V> moved(std::move(flat));
        expectSame(moved, ref);
        CHECK(flat.empty() && flat.begin() == flat.end());
        flat[5] = make(5);  // a moved-from map is usable
        flat = std::move(moved);
        CHECK(moved.empty());
        break;
      }
      case 9:
        if (rng() % 4 == 0) {
          flat.clear();
          ref.clear();
        }
        try {
          flat.at(13);
          CHECK(false);
        } catch (const std::out_of_range&) {
        }
        break;
    }
    expectSame(flat, ref);
  }
}

// 0 entries, exactly the inline capacity, capacity + 1 (the spill) and back,
// with keys arriving in descending, ascending and mixed order
template <class V, class Make>
void capacityEdges(Make make) {
  const std::vector<std::vector<int>> orders = {
      {}, {4, 3, 2, 1}, {1, 2, 3, 4}, {4, 1, 5, 2, 3}, {5, 4, 3, 2, 1}, {2, 9, 1, 12, 7, 3, 11}};
  for (auto& order : orders) {
    FlatLeafMap<V> flat;
    std::map<int, V> ref;
    for (int k : order) {
      flat[k] = make(k);
      ref[k] = make(k);
      expectSame(flat, ref);
    }
    FlatLeafMap<V> copy = flat;
    expectSame(copy, ref);
    for (int k : order) {  // erase through the spill and back to nothing
      CHECK(flat.erase(k) == 1);
      ref.erase(k);
      expectSame(flat, ref);
    }
    CHECK(flat.erase(1) == 0);
    for (int k : order) flat[k] = make(k + 1);  // refill after emptying
    for (int k : order) ref[k] = make(k + 1);
    expectSame(flat, ref);
    expectSame(copy, [&] {
      std::map<int, V> m;
      for (int k : order) m[k] = make(k);
      return m;
    }());
  }
}

void podCells() {
  int cellsStore[64];
  std::mt19937 rng(3);
  for (size_t leaves : {0, 1, 2, 4, 5, 8}) {
    PodCells<int> block;
    std::vector<std::vector<int*>> ref;
    CHECK(block.empty() && block.begin() == block.end());
    for (size_t pod = 0; pod < 5; pod++) {  // 1 x 8 fills the inline part, more spills
      int** row = block.appendPod(leaves);
      ref.emplace_back();
      for (size_t i = 0; i < leaves; i++) {
        CHECK(row[i] == nullptr);
        row[i] = &cellsStore[rng() % 64];
        ref.back().push_back(row[i]);
      }
      CHECK(block.size() == ref.size());
      size_t pi = 0;
      for (auto& podCellsRow : block) {
        CHECK(podCellsRow.size() == leaves && podCellsRow.empty() == (leaves == 0));
        size_t li = 0;
        for (int* c : podCellsRow) CHECK(c == ref[pi][li++]);
        CHECK(li == leaves);
        pi++;
      }
      CHECK(pi == ref.size());
      const PodCells<int>& constBlock = block;
      for (size_t p = 0; p < ref.size(); p++) {
        for (size_t i = 0; i < leaves; i++) CHECK(constBlock[p][i] == ref[p][i]);
      }
      PodCells<int> copy = block;
      PodCells<int> assigned;
      assigned.assign(3, 7);
      assigned = copy;
      PodCells<int> moved = std::move(copy);
      CHECK(copy.empty());
      for (size_t p = 0; p < ref.size(); p++) {
        for (size_t i = 0; i < leaves; i++) {
          CHECK(moved[p][i] == ref[p][i] && assigned[p][i] == ref[p][i]);
        }
      }
      if (leaves > 0) {
        moved[0][0] = nullptr;  // a copy has its own cells
        CHECK(block[0][0] == ref[0][0]);
      }
    }
    if (leaves > 0) {
      try {
        block.appendPod(leaves + 1);
        CHECK(false);
      } catch (const std::logic_error&) {
      }
    }
    block.assign(2, 3);
    CHECK(block.size() == 2 && block[1].size() == 3 && block[1][2] == nullptr);
    block.assign(4, 6);  // 24 cells: on the heap
    CHECK(block.size() == 4 && block[3].size() == 6 && block[3][5] == nullptr);
    block.clear();
    CHECK(block.empty());
  }
}

void inlineVec() {
  std::mt19937 rng(4);
  InlineVec<Owner, 1> vec;
  std::vector<Owner> ref;
  for (int op = 0; op < 400; op++) {
    if (rng() % 3 == 0) {
      const size_t n = rng() % 5;
      vec.resize(n);
      ref.resize(n);
    } else if (!ref.empty()) {
      const size_t i = rng() % ref.size();
      vec[i] = Owner(op);
      ref[i] = Owner(op);
    }
    CHECK(vec.size() == ref.size() && vec.empty() == ref.empty());
    size_t i = 0;
    for (auto& v : vec) CHECK(v == ref[i++]);
    CHECK(i == ref.size());
    InlineVec<Owner, 1> copy = vec;
    InlineVec<Owner, 1> moved = std::move(copy);
    CHECK(moved.size() == ref.size());
    for (size_t j = 0; j < ref.size(); j++) CHECK(moved[j] == ref[j]);
  }
}

// SmallVec against std::vector: pushes across the inline capacity and two
// doublings beyond it, pops, clears (the heap block is kept and reused)
void smallVec() {
  std::mt19937 rng(5);
  SmallVec<int*, 4> vec;
  std::vector<int*> ref;
  int cells[64];
  for (int op = 0; op < 3000; op++) {
    const unsigned what = rng() % 16;
    if (what == 0) {
      vec.clear();
      ref.clear();
    } else if (what < 5 && !ref.empty()) {
      CHECK(vec.back() == ref.back());
      vec.pop_back();
      ref.pop_back();
    } else if (ref.size() < 20) {
      vec.push_back(&cells[op % 64]);
      ref.push_back(&cells[op % 64]);
    }
    CHECK(vec.size() == ref.size() && vec.empty() == ref.empty());
    CHECK(static_cast<size_t>(vec.end() - vec.begin()) == ref.size());
    size_t i = 0;
    for (int* c : vec) CHECK(c == ref[i++]);
    for (size_t j = 0; j < ref.size(); j++) CHECK(vec[j] == ref[j]);
  }
}

}  // namespace

int main() {
  for (unsigned seed = 1; seed <= 4; seed++) {
    randomOperations<int>(seed, 1500, [](int v) { return v; });
    randomOperations<Owner>(seed + 10, 1500, [](int v) { return Owner(v); });
  }
  capacityEdges<int>([](int v) { return v; });
  capacityEdges<Owner>([](int v) { return Owner(v); });
  podCells();
  inlineVec();
  smallVec();
  printf("flat containers OK (%ld checks)\n", gChecks);
  return 0;
}
