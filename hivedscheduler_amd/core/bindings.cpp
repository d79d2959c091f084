// pybind11 bindings for the scheduler core. Requests come in as the wire-format
// dict or as the API object itself (hivedscheduler_amd.api.types), results go
// out as dicts in the wire format, or from schedule_pod as a native
// ScheduleResult; all hot-path work happens in C++.
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <climits>
#include <cstring>
#include <functional>
#include <mutex>

#include "core.hpp"

namespace py = pybind11;
using namespace hived;

namespace {

std::string dstr(const py::dict& d, const char* key, const std::string& def = "") {
  if (!d.contains(key)) return def;
  py::object v = d[key];
  if (v.is_none()) return def;
  return py::cast<std::string>(py::str(v));
}
long long dint(const py::dict& d, const char* key, long long def = 0) {
  if (!d.contains(key)) return def;
  py::object v = d[key];
  if (v.is_none()) return def;
  return py::cast<long long>(v);
}
bool dbool(const py::dict& d, const char* key, bool def = false) {
  if (!d.contains(key)) return def;
  py::object v = d[key];
  if (v.is_none()) return def;
  return py::cast<bool>(v);
}

ClusterSpec parseClusterSpec(const py::dict& d) {
  ClusterSpec spec;
  if (d.contains("cellTypes")) {
    for (auto item : py::cast<py::dict>(d["cellTypes"])) {
      py::dict td = py::cast<py::dict>(item.second);
      CellTypeSpec ct;
      ct.child = dstr(td, "childCellType");
      ct.childCount = static_cast<int>(dint(td, "childCellNumber"));
      ct.isNode = dbool(td, "isNodeLevel");
      spec.cellTypes[py::cast<std::string>(item.first)] = ct;
    }
  }
  std::function<PhysCellSpec(const py::dict&)> parseCell = [&](const py::dict& cd) {
    PhysCellSpec c;
    c.type = dstr(cd, "cellType");
    c.address = dstr(cd, "cellAddress");
    c.pinnedId = dstr(cd, "pinnedCellId");
    if (cd.contains("hbmBytes") && !cd["hbmBytes"].is_none()) {
      c.hbmBytes = py::cast<long long>(cd["hbmBytes"]);
    }
    // discovery-measured xGMI link table (node-level entries):
    // [{a, b, gbps, healthy}, ...]
    if (cd.contains("xgmiLinks") && !cd["xgmiLinks"].is_none()) {
      for (auto lo : py::cast<py::list>(cd["xgmiLinks"])) {
        py::dict ld = py::cast<py::dict>(lo);
        double gbps = ld.contains("gbps") && !ld["gbps"].is_none() ? py::cast<double>(ld["gbps"]) : 0.0;
        c.xgmiLinks.emplace_back(static_cast<int>(dint(ld, "a")), static_cast<int>(dint(ld, "b")),
                                 gbps, dbool(ld, "healthy", true));
      }
    }
    if (cd.contains("cellChildren") && !cd["cellChildren"].is_none()) {
      for (auto child : py::cast<py::list>(cd["cellChildren"])) {
        c.children.push_back(parseCell(py::cast<py::dict>(child)));
      }
    }
    return c;
  };
  if (d.contains("physicalCells")) {
    for (auto cd : py::cast<py::list>(d["physicalCells"])) {
      spec.physicalCells.push_back(parseCell(py::cast<py::dict>(cd)));
    }
  }
  if (d.contains("virtualClusters")) {
    for (auto item : py::cast<py::dict>(d["virtualClusters"])) {
      py::dict vd = py::cast<py::dict>(item.second);
      VCSpec vc;
      if (vd.contains("virtualCells") && !vd["virtualCells"].is_none()) {
        for (auto vcell : py::cast<py::list>(vd["virtualCells"])) {
          py::dict vcd = py::cast<py::dict>(vcell);
          VirtCellSpec vs;
          vs.typePath = dstr(vcd, "cellType");
          vs.number = static_cast<int>(dint(vcd, "cellNumber"));
          vc.virtualCells.push_back(vs);
        }
      }
      if (vd.contains("pinnedCells") && !vd["pinnedCells"].is_none()) {
        for (auto pcell : py::cast<py::list>(vd["pinnedCells"])) {
          py::dict pcd = py::cast<py::dict>(pcell);
          vc.pinnedIds.push_back(dstr(pcd, "pinnedCellId"));
        }
      }
      spec.virtualClusters[py::cast<std::string>(item.first)] = vc;
    }
  }
  return spec;
}

// ---------------------------------------------------------------------------
// Hot-path marshalling (schedule / add / delete). Every decision crosses this
// boundary, so it avoids temporaries: key strings are interned once, each
// field costs one lookup, and str values are read in place.
// ---------------------------------------------------------------------------

// Interned key / attribute names and constant values. Created once at module
// initialisation (under the GIL) and never released, so interpreter shutdown
// has nothing to trip over.
struct Names {
  // PodSchedulingSpec
  PyObject* virtualCluster;
  PyObject* priority;
  PyObject* pinnedCellId;
  PyObject* leafCellType;
  PyObject* leafCellNumber;
  PyObject* gangReleaseEnable;
  PyObject* lazyPreemptionEnable;
  PyObject* ignoreK8sSuggestedNodes;
  PyObject* hbmBytesPerCell;
  PyObject* affinityGroup;
  PyObject* name;
  PyObject* members;
  PyObject* podNumber;
  // PodBindInfo
  PyObject* node;
  PyObject* cellChain;
  PyObject* leafCellIsolation;
  PyObject* affinityGroupBindInfo;
  PyObject* podPlacements;
  PyObject* physicalNode;
  PyObject* physicalLeafCellIndices;
  PyObject* preassignedCellTypes;
  // schedule result
  PyObject* kind;
  PyObject* bind;
  PyObject* preempt;
  PyObject* wait;
  PyObject* bindInfo;
  PyObject* victimNode;
  PyObject* victimPodKeys;
  PyObject* reason;
  // schedule_pod: argument names in positional order, phase values
  PyObject* pod_spec;
  PyObject* spec;  // the facade's name for pod_spec
  PyObject* pod_key;
  PyObject* suggested_nodes;
  PyObject* phase;
  PyObject* commit;
  PyObject* validate;
  PyObject* Filtering;
  PyObject* Preempting;
  PyObject* code;
};
Names N{};

PyObject* internName(const char* s) {
  PyObject* o = PyUnicode_InternFromString(s);
  if (o == nullptr) throw py::error_already_set();
  return o;
}

void initNames() {
#define HIVED_NAME(x) N.x = internName(#x)
  HIVED_NAME(virtualCluster);
  HIVED_NAME(priority);
  HIVED_NAME(pinnedCellId);
  HIVED_NAME(leafCellType);
  HIVED_NAME(leafCellNumber);
  HIVED_NAME(gangReleaseEnable);
  HIVED_NAME(lazyPreemptionEnable);
  HIVED_NAME(ignoreK8sSuggestedNodes);
  HIVED_NAME(hbmBytesPerCell);
  HIVED_NAME(affinityGroup);
  HIVED_NAME(name);
  HIVED_NAME(members);
  HIVED_NAME(podNumber);
  HIVED_NAME(node);
  HIVED_NAME(cellChain);
  HIVED_NAME(leafCellIsolation);
  HIVED_NAME(affinityGroupBindInfo);
  HIVED_NAME(podPlacements);
  HIVED_NAME(physicalNode);
  HIVED_NAME(physicalLeafCellIndices);
  HIVED_NAME(preassignedCellTypes);
  HIVED_NAME(kind);
  HIVED_NAME(bind);
  HIVED_NAME(preempt);
  HIVED_NAME(wait);
  HIVED_NAME(bindInfo);
  HIVED_NAME(victimNode);
  HIVED_NAME(victimPodKeys);
  HIVED_NAME(reason);
  HIVED_NAME(pod_spec);
  HIVED_NAME(spec);
  HIVED_NAME(pod_key);
  HIVED_NAME(suggested_nodes);
  HIVED_NAME(phase);
  HIVED_NAME(commit);
  HIVED_NAME(validate);
  HIVED_NAME(Filtering);
  HIVED_NAME(Preempting);
  HIVED_NAME(code);
#undef HIVED_NAME
}

// API classes (hivedscheduler_amd.api.types) and constants, looked up once at
// module initialisation and never released, like the names above.
struct ApiTypes {
  PyObject* PodSchedulingSpec;
  PyObject* AffinityGroupSpec;
  PyObject* AffinityGroupMemberSpec;
  PyObject* PodBindInfo;
  PyObject* AffinityGroupMemberBindInfo;
  PyObject* PodPlacementInfo;
  PyObject* WebServerError;
  PyObject* emptyTuple;
  PyObject* one;
};
ApiTypes T{};

void initApiTypes() {
  py::module_ types = py::module_::import("hivedscheduler_amd.api.types");
#define HIVED_TYPE(x) T.x = py::object(types.attr(#x)).release().ptr()
  HIVED_TYPE(PodSchedulingSpec);
  HIVED_TYPE(AffinityGroupSpec);
  HIVED_TYPE(AffinityGroupMemberSpec);
  HIVED_TYPE(PodBindInfo);
  HIVED_TYPE(AffinityGroupMemberBindInfo);
  HIVED_TYPE(PodPlacementInfo);
  HIVED_TYPE(WebServerError);
#undef HIVED_TYPE
  T.emptyTuple = PyTuple_New(0);
  T.one = PyLong_FromLong(1);
  if (T.emptyTuple == nullptr || T.one == nullptr) throw py::error_already_set();
}

// A request record about to be read field by field: the wire-format dict, or an
// API object. An object whose type is exactly PodSchedulingSpec,
// AffinityGroupSpec or AffinityGroupMemberSpec is a plain dataclass instance:
// its fields sit in its __dict__, and the class holds nothing that outranks
// them (no property, no __getattribute__), so a field found there is what
// getattr would give. Its __dict__ is fetched once and the fields are looked up
// in it by their interned names. A field not found there (deleted from the
// instance, so that the class default applies) and every other type (a
// subclass, which may carry properties; any other object) go through getattr.
class Record {
 public:
  explicit Record(py::handle rec) : rec_(rec.ptr()) {
    if (PyDict_Check(rec_)) {
      dict_ = rec_;
      wire_ = true;
      return;
    }
    PyObject* tp = reinterpret_cast<PyObject*>(Py_TYPE(rec_));
    if (tp == T.PodSchedulingSpec || tp == T.AffinityGroupMemberSpec ||
        tp == T.AffinityGroupSpec) {
      dict_ = ownedDict_ = PyObject_GenericGetDict(rec_, nullptr);
      if (dict_ == nullptr) PyErr_Clear();  // no __dict__ after all: getattr it is
    }
  }
  Record(const Record&) = delete;
  Record& operator=(const Record&) = delete;
  ~Record() { Py_XDECREF(ownedDict_); }
  py::handle object() const { return rec_; }

 private:
  friend class Field;
  PyObject* rec_;
  PyObject* dict_ = nullptr;       // the wire dict or the instance's __dict__
  PyObject* ownedDict_ = nullptr;  // the reference PyObject_GenericGetDict gave
  bool wire_ = false;
};

// One field of a record. A record is either the wire-format dict, read by key
// (borrowed reference), or an API object (PodSchedulingSpec, PodBindInfo and
// their members), read by attribute (owned reference). A missing key and a
// None value both read as absent; a failing lookup propagates, and so does a
// missing attribute: the API objects always carry all their fields.
class Field {
 public:
  Field(py::handle rec, PyObject* name) {
    if (PyDict_Check(rec.ptr())) {
      p_ = PyDict_GetItemWithError(rec.ptr(), name);
      if (p_ == nullptr && PyErr_Occurred()) throw py::error_already_set();
    } else {
      p_ = PyObject_GetAttr(rec.ptr(), name);
      if (p_ == nullptr) throw py::error_already_set();
      owned_ = true;
    }
  }
  Field(const Record& rec, PyObject* name) {
    if (rec.dict_ != nullptr) {
      p_ = PyDict_GetItemWithError(rec.dict_, name);
      if (p_ == nullptr && PyErr_Occurred()) throw py::error_already_set();
      if (rec.wire_) return;
      if (p_ != nullptr) {
        // owned, like an attribute: converting a value can run Python code
        // (__str__, __index__), which may drop the instance's own reference
        Py_INCREF(p_);
        owned_ = true;
        return;
      }
    }
    p_ = PyObject_GetAttr(rec.rec_, name);
    if (p_ == nullptr) throw py::error_already_set();
    owned_ = true;
  }
  Field(const Field&) = delete;
  Field& operator=(const Field&) = delete;
  ~Field() {
    if (owned_) Py_DECREF(p_);
  }
  explicit operator bool() const { return p_ != nullptr && p_ != Py_None; }
  py::handle get() const { return p_; }

 private:
  PyObject* p_ = nullptr;
  bool owned_ = false;
};

std::string toStdString(py::handle v) {
  if (PyUnicode_Check(v.ptr())) {
    Py_ssize_t n = 0;
    const char* s = PyUnicode_AsUTF8AndSize(v.ptr(), &n);
    if (s == nullptr) throw py::error_already_set();
    return std::string(s, static_cast<size_t>(n));
  }
  return py::cast<std::string>(py::str(v));
}
long long toLongLong(py::handle v) {
  if (PyLong_CheckExact(v.ptr())) {
    int overflow = 0;
    long long x = PyLong_AsLongLongAndOverflow(v.ptr(), &overflow);
    if (overflow == 0) {
      if (x == -1 && PyErr_Occurred()) throw py::error_already_set();
      return x;
    }
  }
  return py::cast<long long>(v);
}
int toInt(py::handle v) {
  if (PyLong_CheckExact(v.ptr())) {
    int overflow = 0;
    long x = PyLong_AsLongAndOverflow(v.ptr(), &overflow);
    if (overflow == 0 && x >= INT_MIN && x <= INT_MAX) {
      if (x == -1 && PyErr_Occurred()) throw py::error_already_set();
      return static_cast<int>(x);
    }
  }
  return py::cast<int>(v);
}
bool toBool(py::handle v) {
  if (v.ptr() == Py_True) return true;
  if (v.ptr() == Py_False) return false;
  return py::cast<bool>(v);
}

template <class Rec>
std::string fstr(const Rec& rec, PyObject* name) {
  Field f(rec, name);
  return f ? toStdString(f.get()) : std::string();
}
template <class Rec>
long long fint(const Rec& rec, PyObject* name) {
  Field f(rec, name);
  return f ? toLongLong(f.get()) : 0;
}
template <class Rec>
bool fbool(const Rec& rec, PyObject* name, bool def) {
  Field f(rec, name);
  return f ? toBool(f.get()) : def;
}

// Items of a list-valued field; any iterable is taken, as list(x) would.
class Items {
 public:
  explicit Items(py::handle v) : seq_(PySequence_Fast(v.ptr(), "expected a list")) {
    if (seq_ == nullptr) throw py::error_already_set();
  }
  Items(const Items&) = delete;
  Items& operator=(const Items&) = delete;
  ~Items() { Py_DECREF(seq_); }
  Py_ssize_t size() const { return PySequence_Fast_GET_SIZE(seq_); }
  py::handle operator[](Py_ssize_t i) const { return PySequence_Fast_GET_ITEM(seq_, i); }

 private:
  PyObject* seq_;
};

PodSpec parsePodSpec(py::handle spec) {
  Record d(spec);
  PodSpec s;
  s.vc = fstr(d, N.virtualCluster);
  s.priority = static_cast<int>(fint(d, N.priority));
  s.pinnedCellId = fstr(d, N.pinnedCellId);
  s.leafCellType = fstr(d, N.leafCellType);
  s.leafCellNumber = static_cast<int>(fint(d, N.leafCellNumber));
  s.gangReleaseEnable = fbool(d, N.gangReleaseEnable, false);
  s.lazyPreemptionEnable = fbool(d, N.lazyPreemptionEnable, false);
  s.ignoreK8sSuggestedNodes = fbool(d, N.ignoreK8sSuggestedNodes, true);
  s.hbmBytesPerCell = fint(d, N.hbmBytesPerCell);
  if (s.hbmBytesPerCell < 0) {
    throw HivedError::BadRequest("hbmBytesPerCell must be non-negative");
  }
  if (Field ag{d, N.affinityGroup}) {
    Record group(ag.get());
    s.groupName = fstr(group, N.name);
    if (Field members{group, N.members}) {
      Items ms(members.get());
      for (Py_ssize_t i = 0; i < ms.size(); i++) {
        Record member(ms[i]);
        s.groupPodNums[static_cast<int>(fint(member, N.leafCellNumber))] +=
            static_cast<int>(fint(member, N.podNumber));
      }
    }
  }
  if (s.groupPodNums.empty() && s.leafCellNumber > 0) {
    s.groupPodNums[s.leafCellNumber] = 1;  // singleton group default
  }
  return s;
}

void parseIntList(py::handle rec, PyObject* name, std::vector<int>* out) {
  if (Field f{rec, name}) {
    Items items(f.get());
    out->reserve(static_cast<size_t>(items.size()));
    for (Py_ssize_t i = 0; i < items.size(); i++) out->push_back(toInt(items[i]));
  }
}

BindInfo parseBindInfo(py::handle d) {
  BindInfo info;
  info.node = fstr(d, N.node);
  info.chain = fstr(d, N.cellChain);
  parseIntList(d, N.leafCellIsolation, &info.isolation);
  if (Field mbis{d, N.affinityGroupBindInfo}) {
    Items mbiItems(mbis.get());
    info.memberBindInfo.reserve(static_cast<size_t>(mbiItems.size()));
    for (Py_ssize_t m = 0; m < mbiItems.size(); m++) {
      std::vector<PodPlacementInfo> placements;
      if (Field pls{mbiItems[m], N.podPlacements}) {
        Items plItems(pls.get());
        placements.reserve(static_cast<size_t>(plItems.size()));
        for (Py_ssize_t p = 0; p < plItems.size(); p++) {
          py::handle plD = plItems[p];
          PodPlacementInfo pl;
          pl.node = fstr(plD, N.physicalNode);
          parseIntList(plD, N.physicalLeafCellIndices, &pl.leafIndices);
          if (Field types{plD, N.preassignedCellTypes}) {
            Items ts(types.get());
            pl.preassignedTypes.reserve(static_cast<size_t>(ts.size()));
            for (Py_ssize_t t = 0; t < ts.size(); t++) {
              pl.preassignedTypes.push_back(ts[t].is_none() ? std::string() : toStdString(ts[t]));
            }
          }
          placements.push_back(std::move(pl));
        }
      }
      info.memberBindInfo.push_back(std::move(placements));
    }
  }
  return info;
}

py::object pyStr(const std::string& s) {
  PyObject* o = PyUnicode_FromStringAndSize(s.data(), static_cast<Py_ssize_t>(s.size()));
  if (o == nullptr) throw py::error_already_set();
  return py::reinterpret_steal<py::object>(o);
}
py::object pyIntList(const std::vector<int>& v) {
  py::list l(v.size());
  for (size_t i = 0; i < v.size(); i++) {
    PyObject* o = PyLong_FromLong(v[i]);
    if (o == nullptr) throw py::error_already_set();
    PyList_SET_ITEM(l.ptr(), static_cast<Py_ssize_t>(i), o);
  }
  return std::move(l);
}
py::object pyStrList(const std::vector<std::string>& v) {
  py::list l(v.size());
  for (size_t i = 0; i < v.size(); i++) {
    PyList_SET_ITEM(l.ptr(), static_cast<Py_ssize_t>(i), pyStr(v[i]).release().ptr());
  }
  return std::move(l);
}
void setItem(py::dict& d, PyObject* key, py::handle value) {
  if (PyDict_SetItem(d.ptr(), key, value.ptr()) != 0) throw py::error_already_set();
}

// The str objects of the names a bind info is made of: node names, chain names
// and cell-type names (and the empty type of an opportunistic leaf). They are
// fixed when the core is built, so each is created once per core and every bind
// info handed out refers to it, instead of a new str per name and bind. A name
// the core does not know (a bind info that came from outside) gets a new str.
// Held by the core and by every result it gave out, so a result that outlives
// its core still finds it; built and released with the GIL held.
class NameStrs {
 public:
  NameStrs() { add(std::string()); }
  NameStrs(const NameStrs&) = delete;
  NameStrs& operator=(const NameStrs&) = delete;
  ~NameStrs() {
    for (auto& [name, o] : strs_) {
      (void)name;
      Py_DECREF(o);
    }
  }
  void add(const std::string& name) {
    if (strs_.count(name)) return;
    PyObject* o = PyUnicode_FromStringAndSize(name.data(), static_cast<Py_ssize_t>(name.size()));
    if (o == nullptr) throw py::error_already_set();
    strs_.emplace(name, o);
  }
  // a new reference
  PyObject* get(const std::string& name) const {
    auto it = strs_.find(name);
    if (it == strs_.end()) {
      PyObject* o = PyUnicode_FromStringAndSize(name.data(), static_cast<Py_ssize_t>(name.size()));
      if (o == nullptr) throw py::error_already_set();
      return o;
    }
    Py_INCREF(it->second);
    return it->second;
  }
  py::object str(const std::string& name) const {
    return py::reinterpret_steal<py::object>(get(name));
  }
  py::object strList(const std::vector<std::string>& v) const {
    py::list l(v.size());
    for (size_t i = 0; i < v.size(); i++) {
      PyList_SET_ITEM(l.ptr(), static_cast<Py_ssize_t>(i), get(v[i]));
    }
    return std::move(l);
  }

 private:
  std::unordered_map<std::string, PyObject*> strs_;
};

py::dict bindInfoToDict(const BindInfo& info, const NameStrs& names) {
  py::dict d;
  setItem(d, N.node, names.str(info.node));
  setItem(d, N.leafCellIsolation, pyIntList(info.isolation));
  setItem(d, N.cellChain, names.str(info.chain));
  py::list mbis(info.memberBindInfo.size());
  for (size_t m = 0; m < info.memberBindInfo.size(); m++) {
    auto& mbi = info.memberBindInfo[m];
    py::list placements(mbi.size());
    for (size_t p = 0; p < mbi.size(); p++) {
      auto& pl = mbi[p];
      py::dict pd;
      setItem(pd, N.physicalNode, names.str(pl.node));
      setItem(pd, N.physicalLeafCellIndices, pyIntList(pl.leafIndices));
      setItem(pd, N.preassignedCellTypes, names.strList(pl.preassignedTypes));
      PyList_SET_ITEM(placements.ptr(), static_cast<Py_ssize_t>(p), pd.release().ptr());
    }
    py::dict md;
    setItem(md, N.podPlacements, placements);
    PyList_SET_ITEM(mbis.ptr(), static_cast<Py_ssize_t>(m), md.release().ptr());
  }
  setItem(d, N.affinityGroupBindInfo, mbis);
  return d;
}

// The suggested_nodes argument takes what a std::vector<std::string> argument
// takes: a sequence other than str / bytes, a generator, a set or a dict view.
bool isNodeNameCollection(py::handle v) {
  PyObject* o = v.ptr();
  if (PySequence_Check(o) != 0) return !PyUnicode_Check(o) && !PyBytes_Check(o);
  if (PyGen_Check(o) != 0 || PyAnySet_Check(o) != 0) return true;
  if (PyType_Check(o)) return false;
  const char* tp = Py_TYPE(o)->tp_name;
  for (const char* ok : {"dict_keys", "dict_values", "dict_items", "map", "zip"}) {
    if (std::strcmp(tp, ok) == 0) return true;
  }
  return false;
}

std::set<std::string> toNodeNameSet(py::handle v) {
  std::set<std::string> out;
  Items items(v);
  for (Py_ssize_t i = 0; i < items.size(); i++) {
    py::handle item = items[i];
    if (!PyUnicode_Check(item.ptr()) && !PyBytes_Check(item.ptr())) {
      throw py::type_error("suggested_nodes must contain node names (str)");
    }
    out.insert(py::cast<std::string>(item));
  }
  return out;
}

// ---------------------------------------------------------------------------
// The fused decision (schedule_pod): validation and defaulting happen in the
// same pass that fills the PodSpec, and the answer goes out as a native
// ScheduleResult instead of a dict that Python unpacks again.
// ---------------------------------------------------------------------------

// An instance of a plain (dataclass) API class without running its __init__:
// object.__new__(cls); the caller then sets every field, in field order.
py::object newInstance(PyObject* cls) {
  PyTypeObject* tp = reinterpret_cast<PyTypeObject*>(cls);
  PyObject* o = tp->tp_new(tp, T.emptyTuple, nullptr);
  if (o == nullptr) throw py::error_already_set();
  return py::reinterpret_steal<py::object>(o);
}
void setAttr(py::handle o, PyObject* name, py::handle value) {
  if (PyObject_SetAttr(o.ptr(), name, value.ptr()) != 0) throw py::error_already_set();
}

// AffinityGroupSpec(name=key, members=[AffinityGroupMemberSpec(1, leafCellNumber)])
py::object defaultAffinityGroup(py::handle podKey, py::handle leafCellNumber) {
  py::object member = newInstance(T.AffinityGroupMemberSpec);
  setAttr(member, N.podNumber, T.one);
  setAttr(member, N.leafCellNumber, leafCellNumber);
  py::list members(1);
  PyList_SET_ITEM(members.ptr(), 0, member.release().ptr());
  py::object group = newInstance(T.AffinityGroupSpec);
  setAttr(group, N.name, podKey);
  setAttr(group, N.members, members);
  return group;
}

// parsePodSpec plus what validate_pod_scheduling_spec(spec, key) does, in one
// pass over the PodSchedulingSpec object: the singleton-group default is set
// on the spec first, then the same checks run in the same order with the same
// message texts. Nothing of the core is touched before the last check.
PodSpec parseValidatedPodSpec(py::handle spec, py::handle podKey, const std::string& key) {
  if (PyDict_Check(spec.ptr())) {
    throw py::type_error("schedule_pod validates a PodSchedulingSpec object, not a dict");
  }
  Record d(spec);
  PodSpec s;
  Field leaf(d, N.leafCellNumber);
  bool defaulted = false;
  {
    Field ag(d, N.affinityGroup);
    if (!ag) {
      setAttr(spec, N.affinityGroup, defaultAffinityGroup(podKey, leaf.get()));
      defaulted = true;
    }
  }
  s.vc = fstr(d, N.virtualCluster);
  if (s.vc.empty()) throw HivedError::BadRequest("VirtualCluster is empty");
  long long priority = fint(d, N.priority);
  if (priority < kOpportunisticPriority) {
    throw HivedError::BadRequest("Priority is less than " + std::to_string(kOpportunisticPriority));
  }
  if (priority > kMaxGuaranteedPriority) {
    throw HivedError::BadRequest("Priority is greater than " +
                                 std::to_string(kMaxGuaranteedPriority));
  }
  s.priority = static_cast<int>(priority);
  long long leafNum = leaf ? toLongLong(leaf.get()) : 0;
  if (leafNum <= 0) throw HivedError::BadRequest("LeafCellNumber is non-positive");
  s.leafCellNumber = static_cast<int>(leafNum);
  if (defaulted) {
    s.groupName = key;
    s.groupPodNums[s.leafCellNumber] = 1;
  } else {
    Field ag(d, N.affinityGroup);
    Record group(ag.get());
    s.groupName = fstr(group, N.name);
    if (s.groupName.empty()) throw HivedError::BadRequest("AffinityGroup.Name is empty");
    bool podInGroup = false;
    if (Field members{group, N.members}) {
      Items ms(members.get());
      for (Py_ssize_t i = 0; i < ms.size(); i++) {
        Record member(ms[i]);
        long long podNumber = fint(member, N.podNumber);
        if (podNumber <= 0) {
          throw HivedError::BadRequest("AffinityGroup.Members has non-positive PodNumber");
        }
        long long memberLeafNum = fint(member, N.leafCellNumber);
        if (memberLeafNum <= 0) {
          throw HivedError::BadRequest("AffinityGroup.Members has non-positive LeafCellNumber");
        }
        if (memberLeafNum == leafNum) podInGroup = true;
        s.groupPodNums[static_cast<int>(memberLeafNum)] += static_cast<int>(podNumber);
      }
    }
    if (!podInGroup) {
      throw HivedError::BadRequest("AffinityGroup.Members does not contain current Pod");
    }
  }
  s.pinnedCellId = fstr(d, N.pinnedCellId);
  s.leafCellType = fstr(d, N.leafCellType);
  s.gangReleaseEnable = fbool(d, N.gangReleaseEnable, false);
  s.lazyPreemptionEnable = fbool(d, N.lazyPreemptionEnable, false);
  s.ignoreK8sSuggestedNodes = fbool(d, N.ignoreK8sSuggestedNodes, true);
  s.hbmBytesPerCell = fint(d, N.hbmBytesPerCell);
  if (s.hbmBytesPerCell < 0) {
    throw HivedError::BadRequest("hbmBytesPerCell must be non-negative");
  }
  return s;
}

// C++ BindInfo -> PodBindInfo object, with no dict in between; equal to
// PodBindInfo.from_dict(bindInfoToDict(info, names)).
py::object bindInfoToObject(const BindInfo& info, const NameStrs& names) {
  py::list mbis(info.memberBindInfo.size());
  for (size_t m = 0; m < info.memberBindInfo.size(); m++) {
    auto& mbi = info.memberBindInfo[m];
    py::list placements(mbi.size());
    for (size_t p = 0; p < mbi.size(); p++) {
      auto& pl = mbi[p];
      py::object po = newInstance(T.PodPlacementInfo);
      setAttr(po, N.physicalNode, names.str(pl.node));
      setAttr(po, N.physicalLeafCellIndices, pyIntList(pl.leafIndices));
      setAttr(po, N.preassignedCellTypes, names.strList(pl.preassignedTypes));
      PyList_SET_ITEM(placements.ptr(), static_cast<Py_ssize_t>(p), po.release().ptr());
    }
    py::object mo = newInstance(T.AffinityGroupMemberBindInfo);
    setAttr(mo, N.podPlacements, placements);
    PyList_SET_ITEM(mbis.ptr(), static_cast<Py_ssize_t>(m), mo.release().ptr());
  }
  py::object o = newInstance(T.PodBindInfo);
  setAttr(o, N.node, names.str(info.node));
  setAttr(o, N.leafCellIsolation, pyIntList(info.isolation));
  setAttr(o, N.cellChain, names.str(info.chain));
  setAttr(o, N.affinityGroupBindInfo, mbis);
  return o;
}

// The Python-visible ScheduleResult: a plain C-API type (no pybind11 instance
// bookkeeping per decision) that keeps the core's result as it is and builds
// each attribute's Python value when it is first read. kind, victim_node and
// wait_reason are immutable; bind_info and victim_pod_keys are cached so that
// every read gives the same object. The type takes no part in cyclic GC: the
// only way to a cycle is to put the result into its own victim_pod_keys list.
struct PyScheduleResult {
  PyObject_HEAD
  PyObject* bindInfo;
  PyObject* victimNode;
  PyObject* victimPodKeys;
  PyObject* waitReason;
  hived::ScheduleResult r;
  std::shared_ptr<const NameStrs> names;  // of the core that decided
};

void resultDealloc(PyObject* self) {
  auto* o = reinterpret_cast<PyScheduleResult*>(self);
  Py_XDECREF(o->bindInfo);
  Py_XDECREF(o->victimNode);
  Py_XDECREF(o->victimPodKeys);
  Py_XDECREF(o->waitReason);
  o->r.~ScheduleResult();
  o->names.~shared_ptr();
  Py_TYPE(self)->tp_free(self);
}

// Runs `make` once into *slot and hands out a new reference to the cached
// object; C++ exceptions become the Python error the getter reports.
template <class Make>
PyObject* cachedAttr(PyObject** slot, Make make) {
  if (*slot == nullptr) {
    try {
      *slot = make().release().ptr();
    } catch (py::error_already_set& e) {
      e.restore();
      return nullptr;
    } catch (const std::exception& e) {
      PyErr_SetString(PyExc_RuntimeError, e.what());
      return nullptr;
    }
  }
  Py_INCREF(*slot);
  return *slot;
}

PyObject* resultKind(PyObject* self, void*) {
  PyObject* k = nullptr;
  switch (reinterpret_cast<PyScheduleResult*>(self)->r.kind) {
    case hived::ScheduleResult::Kind::Bind: k = N.bind; break;
    case hived::ScheduleResult::Kind::Preempt: k = N.preempt; break;
    case hived::ScheduleResult::Kind::Wait: k = N.wait; break;
  }
  Py_INCREF(k);
  return k;
}
PyObject* resultBindInfo(PyObject* self, void*) {
  auto* o = reinterpret_cast<PyScheduleResult*>(self);
  if (o->r.kind != hived::ScheduleResult::Kind::Bind) Py_RETURN_NONE;
  return cachedAttr(&o->bindInfo, [o] { return bindInfoToObject(*o->r.bindInfo, *o->names); });
}
PyObject* resultVictimNode(PyObject* self, void*) {
  auto* o = reinterpret_cast<PyScheduleResult*>(self);
  return cachedAttr(&o->victimNode, [o] { return pyStr(o->r.victimNode); });
}
PyObject* resultVictimPodKeys(PyObject* self, void*) {
  auto* o = reinterpret_cast<PyScheduleResult*>(self);
  return cachedAttr(&o->victimPodKeys, [o] { return pyStrList(o->r.victimPodKeys); });
}
PyObject* resultWaitReason(PyObject* self, void*) {
  auto* o = reinterpret_cast<PyScheduleResult*>(self);
  return cachedAttr(&o->waitReason, [o] { return pyStr(o->r.waitReason); });
}

PyObject* resultRepr(PyObject* self) {
  auto* o = reinterpret_cast<PyScheduleResult*>(self);
  switch (o->r.kind) {
    case hived::ScheduleResult::Kind::Bind: {
      PyObject* info = resultBindInfo(self, nullptr);
      if (info == nullptr) return nullptr;
      PyObject* node = PyObject_GetAttr(info, N.node);
      PyObject* cells = PyObject_GetAttr(info, N.leafCellIsolation);
      PyObject* out = (node != nullptr && cells != nullptr)
                          ? PyUnicode_FromFormat("ScheduleResult(bind node=%S cells=%S)", node, cells)
                          : nullptr;
      Py_XDECREF(node);
      Py_XDECREF(cells);
      Py_DECREF(info);
      return out;
    }
    case hived::ScheduleResult::Kind::Preempt: {
      PyObject* keys = resultVictimPodKeys(self, nullptr);
      if (keys == nullptr) return nullptr;
      PyObject* out = PyUnicode_FromFormat("ScheduleResult(preempt victims=%S)", keys);
      Py_DECREF(keys);
      return out;
    }
    case hived::ScheduleResult::Kind::Wait:
      break;
  }
  PyObject* reason = resultWaitReason(self, nullptr);
  if (reason == nullptr) return nullptr;
  PyObject* out = PyUnicode_FromFormat("ScheduleResult(wait reason=%R)", reason);
  Py_DECREF(reason);
  return out;
}

PyGetSetDef resultGetSet[] = {
    {"kind", resultKind, nullptr, "\"bind\", \"preempt\" or \"wait\"", nullptr},
    {"bind_info", resultBindInfo, nullptr, "PodBindInfo of a bind decision, else None", nullptr},
    {"victim_node", resultVictimNode, nullptr, "node whose pods a preempt decision evicts", nullptr},
    {"victim_pod_keys", resultVictimPodKeys, nullptr, "pod keys a preempt decision evicts", nullptr},
    {"wait_reason", resultWaitReason, nullptr, "why a wait decision waits", nullptr},
    {nullptr, nullptr, nullptr, nullptr, nullptr},
};

PyTypeObject ResultType = {PyVarObject_HEAD_INIT(nullptr, 0)};

void initResultType(py::module_& m) {
  ResultType.tp_name = "hivedscheduler_amd.hivedcore.ScheduleResult";
  ResultType.tp_doc = "One of bind / preempt / wait.";
  ResultType.tp_basicsize = sizeof(PyScheduleResult);
  ResultType.tp_flags = Py_TPFLAGS_DEFAULT;
  ResultType.tp_dealloc = resultDealloc;
  ResultType.tp_repr = resultRepr;
  ResultType.tp_getset = resultGetSet;
  if (PyType_Ready(&ResultType) != 0) throw py::error_already_set();
  m.add_object("ScheduleResult", reinterpret_cast<PyObject*>(&ResultType));
}

py::object makeResult(hived::ScheduleResult&& r, const std::shared_ptr<const NameStrs>& names) {
  PyScheduleResult* o = PyObject_New(PyScheduleResult, &ResultType);
  if (o == nullptr) throw py::error_already_set();
  o->bindInfo = o->victimNode = o->victimPodKeys = o->waitReason = nullptr;
  new (&o->r) hived::ScheduleResult(std::move(r));
  new (&o->names) std::shared_ptr<const NameStrs>(names);
  return py::reinterpret_steal<py::object>(reinterpret_cast<PyObject*>(o));
}

py::dict physicalCellStatus(PhysicalCell* c, bool withChildren = true) {
  py::dict d;
  d["cellType"] = c->typeName;
  d["cellAddress"] = c->address;
  d["isNodeLevel"] = c->isNodeLevel;
  d["cellState"] = to_string(c->state);
  d["cellHealthiness"] = c->healthy ? "Healthy" : "Bad";
  d["cellPriority"] = c->priority;
  if (!c->otVC.empty()) d["vc"] = c->otVC;
  if (c->virt != nullptr) {
    d["vc"] = c->virt->vc;
    d["virtualCell"] = c->virt->address;
  }
  if (c->level == kLowestLevel) {
    d["physicalNode"] = c->nodes.empty() ? "" : c->nodes[0];
    d["leafCellIndex"] = c->leafIndices.empty() ? -1 : c->leafIndices[0];
    d["hbmBytes"] = c->hbmBytes;
  } else if (c->badLinksUnder > 0) {
    // first-class xGMI link state: degraded links under this pair/quad/node
    // (the cell stays Healthy — its GPUs work — but multi-GPU placements
    // avoid co-placing the degraded link's endpoints)
    d["badXgmiLinksUnder"] = c->badLinksUnder;
  }
  if (withChildren && !c->children.empty()) {
    py::list children;
    for (Cell* child : c->children) {
      children.append(physicalCellStatus(static_cast<PhysicalCell*>(child)));
    }
    d["cellChildren"] = children;
  }
  return d;
}

py::dict virtualCellStatus(VirtualCell* c, bool withChildren = true) {
  py::dict d;
  d["cellType"] = c->typeName;
  d["cellAddress"] = c->address;
  CState state = c->phys != nullptr ? c->phys->state
                                    : (c->priority > kFreePriority ? CState::Used : CState::Free);
  d["cellState"] = to_string(state);
  d["cellHealthiness"] = (c->phys == nullptr || c->phys->healthy) ? "Healthy" : "Bad";
  d["cellPriority"] = c->priority;
  if (c->phys != nullptr) d["physicalCell"] = c->phys->address;
  if (withChildren && !c->children.empty()) {
    py::list children;
    for (Cell* child : c->children) {
      children.append(virtualCellStatus(static_cast<VirtualCell*>(child)));
    }
    d["cellChildren"] = children;
  }
  return d;
}

py::dict groupToDict(const Group* g) {
  py::dict d;
  d["name"] = g->name;
  d["vc"] = g->vc;
  d["priority"] = g->priority;
  d["state"] = to_string(g->state);
  if (g->lazyStatus.has_value()) {
    py::dict lp;
    lp["preemptor"] = g->lazyStatus->preemptor;
    lp["preemptionTime"] = g->lazyStatus->preemptionTime;
    d["lazyPreemptionStatus"] = lp;
  } else {
    d["lazyPreemptionStatus"] = py::none();
  }
  // physical placement: node -> leaf cell indices
  py::dict physD;
  for (auto& [leafNum, pods] : g->physPlacement) {
    (void)leafNum;
    for (auto& pod : pods) {
      for (PhysicalCell* c : pod) {
        if (c == nullptr) continue;
        std::string node = c->nodes.empty() ? "" : c->nodes[0];
        if (!physD.contains(py::str(node))) physD[py::str(node)] = py::list();
        py::cast<py::list>(physD[py::str(node)]).append(c->leafIndices[0]);
      }
    }
  }
  d["physicalPlacement"] = physD;
  // virtual placement: preassigned cell address -> leaf cell addresses
  py::dict virtD;
  if (g->hasVirtualPlacement) {
    for (auto& [leafNum, pods] : g->virtPlacement) {
      (void)leafNum;
      for (auto& pod : pods) {
        for (VirtualCell* v : pod) {
          if (v == nullptr) continue;
          std::string pre = v->preassigned->address;
          if (!virtD.contains(py::str(pre))) virtD[py::str(pre)] = py::list();
          py::cast<py::list>(virtD[py::str(pre)]).append(v->address);
        }
      }
    }
  }
  d["virtualPlacement"] = virtD;
  py::list allocated;
  for (auto& [ln, pods] : g->allocatedPods) {
    (void)ln;
    for (auto& p : pods) {
      if (p.present) allocated.append(p.key);
    }
  }
  d["allocatedPods"] = allocated;
  py::list preempting;
  for (auto& k : g->preemptingPods) preempting.append(k);
  d["preemptingPods"] = preempting;
  return d;
}

// The stretch of a call that reads or writes core state. With a GIL that
// stretch is whole already (see PyHivedCore::schedulePod) and this is nothing.
// A free-threaded interpreter (Py_GIL_DISABLED) has no such guarantee, so there
// the decision and the calls that change core state take a native mutex; the
// code inside a section is C++ only and never calls into Python, so the mutex
// cannot be held across a thread switch that needs it. (HIVED_CORE_MUTEX turns
// the mutex on in a GIL build, to compile and test this path.)
#if defined(Py_GIL_DISABLED) || defined(HIVED_CORE_MUTEX)
using CoreMutex = std::mutex;
using CoreSection = std::lock_guard<std::mutex>;
#else
struct CoreMutex {};
struct CoreSection {
  explicit CoreSection(CoreMutex&) {}
};
#endif

class PyHivedCore {
 public:
  explicit PyHivedCore(const py::dict& spec) : core_(parseClusterSpec(spec)) {
    auto names = std::make_shared<NameStrs>();
    for (auto& node : core_.allNodes()) {
      names->add(node);
      nodeNames_.push_back(names->str(node));
      allNodeSet_.insert(node);
    }
    for (auto& chain : core_.chains()) {
      names->add(chain);
      for (auto& [level, type] : core_.chainLevelTypes(chain)) {
        (void)level;
        names->add(type);
      }
    }
    nameStrs_ = std::move(names);
  }

  void setNodeHealthy(const std::string& node, bool healthy) {
    CoreSection section(coreMutex_);
    core_.setNodeHealthy(node, healthy);
  }
  void setLeafCellHealthy(const std::string& node, int leafIndex, bool healthy) {
    CoreSection section(coreMutex_);
    core_.setLeafCellHealthy(node, leafIndex, healthy);
  }
  void setXgmiLinkHealthy(const std::string& node, int a, int b, bool healthy, double gbps) {
    CoreSection section(coreMutex_);
    core_.setXgmiLinkHealthy(node, a, b, healthy, gbps);
  }
  py::list xgmiLinks(const std::string& node) const {
    py::list out;
    for (auto& [a, b, gbps, healthy] : core_.xgmiLinks(node)) {
      py::dict d;
      d["a"] = a;
      d["b"] = b;
      d["gbps"] = gbps;
      d["healthy"] = healthy;
      out.append(d);
    }
    return out;
  }
  // The node set is fixed at construction (buildFromSpec is the only writer
  // of the node table), so the name objects are built once; every call hands
  // out a fresh list of them.
  py::list allNodes() const {
    py::list out(nodeNames_.size());
    for (size_t i = 0; i < nodeNames_.size(); i++) {
      PyList_SET_ITEM(out.ptr(), static_cast<Py_ssize_t>(i), py::object(nodeNames_[i]).release().ptr());
    }
    return out;
  }
  std::vector<std::string> badNodes() const {
    auto s = core_.badNodes();
    return {s.begin(), s.end()};
  }

  // pod_spec / bind_info: the wire-format dict or the API object itself.
  py::dict schedule(py::handle spec, const std::string& podKey, py::handle suggestedNodes,
                    const std::string& phase) {
    if (!isNodeNameCollection(suggestedNodes)) {
      throw py::type_error("suggested_nodes must be a sequence of node names, not " +
                           std::string(Py_TYPE(suggestedNodes.ptr())->tp_name));
    }
    PodSpec s = parsePodSpec(spec);
    // The core reads the suggested set only where suggested nodes are not
    // ignored: for a new group the request's flag decides, for an existing
    // group of that name the group's own flag does. Otherwise the names are
    // never converted.
    bool needSuggested = !s.ignoreK8sSuggestedNodes;
    if (!needSuggested) {
      CoreSection section(coreMutex_);
      auto it = core_.groups().find(s.groupName);
      needSuggested = it != core_.groups().end() && !it->second->ignoreK8sSuggestedNodes;
    }
    std::set<std::string> suggested;
    if (needSuggested) suggested = toNodeNameSet(suggestedNodes);
    Phase ph = (phase == "Preempting") ? Phase::Preempting : Phase::Filtering;
    ScheduleResult r = [&] {
      CoreSection section(coreMutex_);
      return core_.schedule(s, podKey, suggested, ph);
    }();
    py::dict d;
    switch (r.kind) {
      case ScheduleResult::Kind::Bind:
        setItem(d, N.kind, N.bind);
        setItem(d, N.bindInfo, bindInfoToDict(*r.bindInfo, *nameStrs_));
        break;
      case ScheduleResult::Kind::Preempt:
        setItem(d, N.kind, N.preempt);
        setItem(d, N.victimNode, pyStr(r.victimNode));
        setItem(d, N.victimPodKeys, pyStrList(r.victimPodKeys));
        break;
      case ScheduleResult::Kind::Wait:
        setItem(d, N.kind, N.wait);
        setItem(d, N.reason, pyStr(r.waitReason));
        break;
    }
    return d;
  }

  // One filter decision in one call: validate and default the request
  // (validate), decide, commit a bind decision (commit), and hand out the
  // native result. suggested_nodes=None stands for every node of the cluster.
  //
  // This call is not under HivedAlgorithm's lock (the facade binds the native
  // method itself, see scheduleValidatedPodEntry). What keeps it whole is the
  // GIL: no method of this class releases it, and between the first read of
  // core state below (the group peek) and the last write (addAllocatedPod)
  // this function runs no Python code, so no other thread can get in between.
  // Everything that can run Python code sits outside that stretch: the spec is
  // parsed before it ("nothing of the core is touched before the last check"),
  // the result object is built after it, and the one conversion in between,
  // toNodeNameSet, runs only when the peek said the names are needed; should
  // another thread change the group meanwhile, the names are converted for
  // nothing, and the decision itself is taken in one piece afterwards. Without
  // a GIL (Py_GIL_DISABLED) a native mutex takes its place, see CoreSection.
  py::object schedulePod(py::handle spec, py::handle podKey, py::handle suggestedNodes,
                         py::handle phase, bool commit, bool validate) {
    if (!PyUnicode_Check(podKey.ptr())) throw py::type_error("pod_key must be a str");
    // phase: absent means Filtering; the two constants are interned strings,
    // so they are told apart by identity before anything is compared
    Phase ph = Phase::Filtering;
    if (phase.ptr() != nullptr && phase.ptr() != N.Filtering) {
      if (!PyUnicode_Check(phase.ptr())) throw py::type_error("phase must be a str");
      if (phase.ptr() == N.Preempting ||
          PyUnicode_CompareWithASCIIString(phase.ptr(), "Preempting") == 0) {
        ph = Phase::Preempting;
      }
    }
    if (!suggestedNodes.is_none() && !isNodeNameCollection(suggestedNodes)) {
      throw py::type_error("suggested_nodes must be a sequence of node names, not " +
                           std::string(Py_TYPE(suggestedNodes.ptr())->tp_name));
    }
    std::string key = toStdString(podKey);
    PodSpec s = validate ? parseValidatedPodSpec(spec, podKey, key) : parsePodSpec(spec);
    // as in schedule(): the suggested set is read only where the request, or
    // an existing group of that name, does not ignore suggested nodes
    bool needSuggested = !s.ignoreK8sSuggestedNodes;
    if (!needSuggested) {
      CoreSection section(coreMutex_);
      auto it = core_.groups().find(s.groupName);
      needSuggested = it != core_.groups().end() && !it->second->ignoreK8sSuggestedNodes;
    }
    std::set<std::string> given;
    const std::set<std::string>* suggested = &given;
    if (needSuggested) {
      if (suggestedNodes.is_none()) {
        suggested = &allNodeSet_;
      } else {
        given = toNodeNameSet(suggestedNodes);
      }
    }
    hived::ScheduleResult r = [&] {
      CoreSection section(coreMutex_);  // pure C++ in here: no Python call
      hived::ScheduleResult decided = core_.schedule(s, key, *suggested, ph);
      if (commit && decided.kind == hived::ScheduleResult::Kind::Bind) {
        core_.addAllocatedPod(s, decided.bindInfo, key);
      }
      return decided;
    }();
    return makeResult(std::move(r), nameStrs_);
  }

  void deleteUnallocatedPod(py::handle spec, const std::string& podKey) {
    PodSpec s = parsePodSpec(spec);
    CoreSection section(coreMutex_);
    core_.deleteUnallocatedPod(s, podKey);
  }
  void addAllocatedPod(py::handle spec, py::handle bindInfo, const std::string& podKey) {
    PodSpec s = parsePodSpec(spec);
    BindInfo info = parseBindInfo(bindInfo);
    CoreSection section(coreMutex_);
    core_.addAllocatedPod(s, info, podKey);
  }
  void deleteAllocatedPod(py::handle spec, py::handle bindInfo, const std::string& podKey) {
    PodSpec s = parsePodSpec(spec);
    BindInfo info = parseBindInfo(bindInfo);
    CoreSection section(coreMutex_);
    core_.deleteAllocatedPod(s, info, podKey);
  }

  // The release of a pod the core itself knows by key; false for a key it does
  // not know. Like schedulePod this is not under HivedAlgorithm's lock, and the
  // same argument holds: with a GIL no other thread runs between the lookup
  // and the last write, because nothing in here runs Python code (reading a
  // str's UTF-8 does not); without one the CoreSection's mutex covers the same
  // stretch. The key is copied inside the section, into a buffer that is
  // reused from call to call.
  bool deleteAllocatedPodByKey(py::handle podKey) {
    if (!PyUnicode_Check(podKey.ptr())) throw py::type_error("pod_key must be a str");
    Py_ssize_t n = 0;
    const char* utf8 = PyUnicode_AsUTF8AndSize(podKey.ptr(), &n);
    if (utf8 == nullptr) throw py::error_already_set();
    CoreSection section(coreMutex_);  // pure C++ in here: no Python call
    releaseKey_.assign(utf8, static_cast<size_t>(n));
    return core_.deleteAllocatedPodByKey(releaseKey_);
  }

  py::list getAllAffinityGroups() const {
    py::list out;
    for (auto& [name, g] : core_.groups()) {
      (void)name;
      out.append(groupToDict(g.get()));
    }
    return out;
  }

  py::dict getAffinityGroup(const std::string& name) const {
    auto it = core_.groups().find(name);
    if (it == core_.groups().end()) {
      throw HivedError::BadRequest("Affinity group " + name +
                                   " does not exist since it is not allocated or preempting");
    }
    return groupToDict(it->second.get());
  }

  py::dict getClusterStatus() {
    py::dict d;
    d["physicalCluster"] = getPhysicalClusterStatus();
    d["virtualClusters"] = getAllVirtualClustersStatus();
    return d;
  }

  py::list getPhysicalClusterStatus() {
    py::list out;
    for (auto& [chain, st] : core_.chainStates_) {
      (void)chain;
      const ChainCellList& ccl = st.full;
      int top = ccl.top();
      for (Cell* c : ccl.at(top)) {
        out.append(physicalCellStatus(static_cast<PhysicalCell*>(c)));
      }
    }
    return out;
  }

  py::dict getAllVirtualClustersStatus() {
    py::dict out;
    for (auto& [vcName, vcs] : core_.vcSchedulers_) {
      out[py::str(vcName)] = getVirtualClusterStatus(vcName);
    }
    return out;
  }

  py::list getVirtualClusterStatus(const std::string& vcName) {
    auto it = core_.vcSchedulers_.find(vcName);
    if (it == core_.vcSchedulers_.end()) {
      throw HivedError::NotFound("VC " + vcName + " not found");
    }
    py::list out;
    for (auto& [chain, ccl] : it->second.nonPinnedPreassigned) {
      (void)chain;
      for (int l = 1; l <= ccl.top(); l++) {
        for (Cell* c : ccl.at(l)) {
          out.append(virtualCellStatus(static_cast<VirtualCell*>(c)));
        }
      }
    }
    for (auto& [pid, ccl] : it->second.pinned) {
      (void)pid;
      int top = ccl.top();
      for (Cell* c : ccl.at(top)) {
        out.append(virtualCellStatus(static_cast<VirtualCell*>(c)));
      }
    }
    // opportunistic cells used by this VC, exposed as fake virtual cells
    for (auto& [chain, st] : core_.chainStates_) {
      (void)chain;
      for (Cell* c : st.full.at(kLowestLevel)) {
        auto* pc = static_cast<PhysicalCell*>(c);
        if (pc->otVC == vcName) {
          py::dict d;
          d["cellType"] = pc->typeName;
          d["cellAddress"] = pc->address + "-opp";
          d["cellState"] = to_string(CState::Used);
          d["cellHealthiness"] = pc->healthy ? "Healthy" : "Bad";
          d["cellPriority"] = kOpportunisticPriority;
          d["physicalCell"] = pc->address;
          out.append(d);
        }
      }
    }
    return out;
  }

  long long scheduleCount() const { return core_.scheduleCount_; }
  void checkInvariants() const { hived::checkInvariants(core_); }

  py::dict debugCounters() const {
    // safety-accounting introspection for tests/debugging: per chain+level
    // totalLeft / allVCFree / per-VC free / bad-free count
    py::dict d;
    for (auto& [chain, st] : core_.chainStates_) {
      py::dict cd;
      for (int level = kLowestLevel; level <= st.top; level++) {
        py::dict ld;
        ld["totalLeft"] = st.totalLeft[level];
        ld["allVCFree"] = st.allVCFree[level];
        py::dict vd;
        for (const VCChainState* vcc : st.vcs) {  // in VC-name order
          if (vcc->free[level] != 0) vd[py::str(vcc->vc)] = vcc->free[level];
        }
        ld["vcFree"] = vd;
        py::list fl;
        for (auto* fc : st.free.at(level)) fl.append(fc->address);
        ld["freeList"] = fl;
        if (st.allVCDoomedBadCellNum[level] != 0) ld["doomed"] = st.allVCDoomedBadCellNum[level];
        ld["badFree"] = static_cast<int>(st.badFree.at(level).size());
        cd[py::int_(level)] = ld;
      }
      d[py::str(chain)] = cd;
    }
    return d;
  }

 private:
  HivedCore core_;
  std::vector<py::object> nodeNames_;
  // node, chain and cell-type names as str objects, shared with every result
  std::shared_ptr<const NameStrs> nameStrs_;
  // every node name, for schedule_pod(suggested_nodes=None)
  std::set<std::string> allNodeSet_;
  CoreMutex coreMutex_;
  std::string releaseKey_;  // deleteAllocatedPodByKey's key, written under the section
};

// ---------------------------------------------------------------------------
// The direct entry of the fused decision. schedule_pod is called once per
// decision, and pybind11's generic dispatcher (overload record, argument-loader
// tuple, one caster per argument) costs more there than the arguments are
// worth, so the method is a hand-written vectorcall function
// (METH_FASTCALL | METH_KEYWORDS) set on the pybind11 class as a method
// descriptor; the descriptor checks that self is a HivedCore. Everything else
// of the class stays on pybind11.
//
//   schedule_pod(pod_spec, pod_key, suggested_nodes=None, phase="Filtering",
//                commit=False, validate=True)              errors: CoreError
//   schedule_validated_pod(spec, pod_key, suggested_nodes=None,
//                phase="Filtering", commit=False)           errors: WebServerError
//   delete_allocated_pod_by_key(pod_key) -> bool            errors: CoreError
//   delete_validated_pod_by_key(pod_key) -> bool            errors: WebServerError
//
// The second is the first with validate=True and the facade's error protocol:
// a core error leaves as WebServerError(code, text) with the CoreError as its
// __cause__, which is what HivedAlgorithm._call makes of it. HivedAlgorithm
// binds it as its schedule_pod, so no Python frame stands between a caller and
// the core.
// ---------------------------------------------------------------------------

PyObject* gCoreError = nullptr;   // the CoreError class, set at module init
PyTypeObject* gCoreType = nullptr;  // the HivedCore class

// CoreError(text) with .code; a new reference, or nullptr with an error set
PyObject* newCoreError(const HivedError& e) {
  PyObject* text = PyUnicode_FromString(e.what());
  if (text == nullptr) return nullptr;
  PyObject* inst = PyObject_CallFunctionObjArgs(gCoreError, text, nullptr);
  Py_DECREF(text);
  if (inst == nullptr) return nullptr;
  PyObject* code = PyLong_FromLong(e.code);
  if (code == nullptr || PyObject_SetAttr(inst, N.code, code) != 0) {
    Py_XDECREF(code);
    Py_DECREF(inst);
    return nullptr;
  }
  Py_DECREF(code);
  return inst;
}

// Leaves the Python error for a HivedError: CoreError, or for the facade's
// entry `raise WebServerError(e.code, str(e)) from e`.
void setCoreError(const HivedError& e, bool asWebServerError) {
  PyObject* inst = newCoreError(e);
  if (inst == nullptr) return;
  if (!asWebServerError) {
    PyErr_SetObject(gCoreError, inst);
    Py_DECREF(inst);
    return;
  }
  PyObject* web = PyObject_CallFunction(T.WebServerError, "is", e.code, e.what());
  if (web == nullptr) {
    Py_DECREF(inst);
    return;
  }
  Py_INCREF(inst);
  PyException_SetCause(web, inst);    // steals; also sets __suppress_context__
  PyException_SetContext(web, inst);  // steals
  PyErr_SetObject(T.WebServerError, web);
  Py_DECREF(web);
}

// A bool argument as pybind11's caster takes it: True / False, None as False,
// or anything with __bool__.
bool toFlag(PyObject* o, const char* name) {
  if (o == Py_True) return true;
  if (o == Py_False || o == Py_None) return false;
  PyNumberMethods* num = Py_TYPE(o)->tp_as_number;
  if (num != nullptr && num->nb_bool != nullptr) {
    int r = num->nb_bool(o);
    if (r < 0) throw py::error_already_set();
    return r != 0;
  }
  throw py::type_error(std::string(name) + " must be a bool");
}

PyHivedCore* coreOf(PyObject* self) {
  // instances of the class itself keep the C++ object at the head of
  // pybind11's simple layout; subclasses go through the caster
  if (Py_TYPE(self) == gCoreType) {
    auto* inst = reinterpret_cast<py::detail::instance*>(self);
    if (inst->simple_layout && inst->simple_value_holder[0] != nullptr) {
      return static_cast<PyHivedCore*>(inst->simple_value_holder[0]);
    }
  }
  return py::cast<PyHivedCore*>(py::handle(self));
}

// The Python error for the C++ exception in flight (call from a catch block).
void setErrorFromCurrentException(bool facade) {
  try {
    throw;
  } catch (py::error_already_set& e) {
    e.restore();
  } catch (const py::builtin_exception& e) {
    e.set_error();
  } catch (const HivedError& e) {
    setCoreError(e, facade);
  } catch (const std::bad_alloc&) {
    PyErr_NoMemory();
  } catch (const std::out_of_range& e) {
    PyErr_SetString(PyExc_IndexError, e.what());
  } catch (const std::exception& e) {
    PyErr_SetString(PyExc_RuntimeError, e.what());
  }
}

constexpr int kSchedulePodArgs = 6;

PyObject* schedulePodCall(PyObject* self, PyObject* const* args, Py_ssize_t nargs,
                          PyObject* kwnames, bool facade) {
  const char* fn = facade ? "schedule_validated_pod" : "schedule_pod";
  const int maxArgs = facade ? kSchedulePodArgs - 1 : kSchedulePodArgs;
  PyObject* const names[kSchedulePodArgs] = {facade ? N.spec : N.pod_spec, N.pod_key,
                                             N.suggested_nodes,            N.phase,
                                             N.commit,                     N.validate};
  PyObject* a[kSchedulePodArgs] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  Py_ssize_t nkw = kwnames == nullptr ? 0 : PyTuple_GET_SIZE(kwnames);
  if (nargs + nkw > maxArgs) {
    PyErr_Format(PyExc_TypeError, "%s() takes at most %d arguments (%zd given)", fn, maxArgs,
                 nargs + nkw);
    return nullptr;
  }
  for (Py_ssize_t i = 0; i < nargs; i++) a[i] = args[i];
  for (Py_ssize_t k = 0; k < nkw; k++) {
    PyObject* name = PyTuple_GET_ITEM(kwnames, k);
    int idx = -1;
    for (int j = 0; j < maxArgs; j++) {  // keyword names are interned as a rule
      if (name == names[j]) {
        idx = j;
        break;
      }
    }
    for (int j = 0; idx < 0 && j < maxArgs; j++) {
      int eq = PyObject_RichCompareBool(name, names[j], Py_EQ);
      if (eq < 0) return nullptr;
      if (eq) idx = j;
    }
    if (idx < 0) {
      PyErr_Format(PyExc_TypeError, "%s() got an unexpected keyword argument '%U'", fn, name);
      return nullptr;
    }
    if (a[idx] != nullptr) {
      PyErr_Format(PyExc_TypeError, "%s() got multiple values for argument '%U'", fn, name);
      return nullptr;
    }
    a[idx] = args[nargs + k];
  }
  for (int j = 0; j < 2; j++) {
    if (a[j] == nullptr) {
      PyErr_Format(PyExc_TypeError, "%s() missing required argument '%U' (pos %d)", fn, names[j],
                   j + 1);
      return nullptr;
    }
  }
  try {
    bool commit = a[4] != nullptr && toFlag(a[4], "commit");
    bool validate = a[5] == nullptr || toFlag(a[5], "validate");
    return coreOf(self)
        ->schedulePod(a[0], a[1], a[2] != nullptr ? a[2] : Py_None, a[3], commit, validate)
        .release()
        .ptr();
  } catch (...) {
    setErrorFromCurrentException(facade);
  }
  return nullptr;
}

// delete_allocated_pod_by_key(pod_key) -> bool. One argument, by position or
// by name; the error protocol is schedule_pod's.
PyObject* deleteByKeyCall(PyObject* self, PyObject* const* args, Py_ssize_t nargs,
                          PyObject* kwnames, bool facade) {
  const char* fn = facade ? "delete_validated_pod_by_key" : "delete_allocated_pod_by_key";
  Py_ssize_t nkw = kwnames == nullptr ? 0 : PyTuple_GET_SIZE(kwnames);
  if (nargs + nkw != 1) {
    PyErr_Format(PyExc_TypeError, "%s() takes exactly one argument 'pod_key' (%zd given)", fn,
                 nargs + nkw);
    return nullptr;
  }
  if (nkw == 1) {
    PyObject* name = PyTuple_GET_ITEM(kwnames, 0);
    int eq = name == N.pod_key ? 1 : PyObject_RichCompareBool(name, N.pod_key, Py_EQ);
    if (eq < 0) return nullptr;
    if (eq == 0) {
      PyErr_Format(PyExc_TypeError, "%s() got an unexpected keyword argument '%U'", fn, name);
      return nullptr;
    }
  }
  try {
    if (coreOf(self)->deleteAllocatedPodByKey(args[0])) Py_RETURN_TRUE;
    Py_RETURN_FALSE;
  } catch (...) {
    setErrorFromCurrentException(facade);
  }
  return nullptr;
}

PyObject* schedulePodEntry(PyObject* self, PyObject* const* args, Py_ssize_t nargs,
                           PyObject* kwnames) {
  return schedulePodCall(self, args, nargs, kwnames, false);
}
PyObject* scheduleValidatedPodEntry(PyObject* self, PyObject* const* args, Py_ssize_t nargs,
                                    PyObject* kwnames) {
  return schedulePodCall(self, args, nargs, kwnames, true);
}

PyObject* deleteByKeyEntry(PyObject* self, PyObject* const* args, Py_ssize_t nargs,
                           PyObject* kwnames) {
  return deleteByKeyCall(self, args, nargs, kwnames, false);
}
PyObject* deleteValidatedByKeyEntry(PyObject* self, PyObject* const* args, Py_ssize_t nargs,
                                    PyObject* kwnames) {
  return deleteByKeyCall(self, args, nargs, kwnames, true);
}

using FastCallWithKeywords = PyObject* (*)(PyObject*, PyObject* const*, Py_ssize_t, PyObject*);
PyCFunction asCFunction(FastCallWithKeywords f) {
  return reinterpret_cast<PyCFunction>(reinterpret_cast<void (*)()>(f));
}

PyMethodDef directMethods[] = {
    {"schedule_pod", asCFunction(schedulePodEntry), METH_FASTCALL | METH_KEYWORDS,
     "schedule_pod($self, /, pod_spec, pod_key, suggested_nodes=None, phase='Filtering', "
     "commit=False, validate=True)\n--\n\n"
     "One filter decision in one call: validate and default the request, decide,\n"
     "commit a bind decision, return the native ScheduleResult. Raises CoreError."},
    {"schedule_validated_pod", asCFunction(scheduleValidatedPodEntry),
     METH_FASTCALL | METH_KEYWORDS,
     "schedule_validated_pod($self, /, spec, pod_key, suggested_nodes=None, "
     "phase='Filtering', commit=False)\n--\n\n"
     "schedule_pod with validate=True whose core errors leave as\n"
     "WebServerError(code, text) with the CoreError as __cause__."},
    {"delete_allocated_pod_by_key", asCFunction(deleteByKeyEntry), METH_FASTCALL | METH_KEYWORDS,
     "delete_allocated_pod_by_key($self, /, pod_key)\n--\n\n"
     "Release the allocated pod the core holds under pod_key, as\n"
     "delete_allocated_pod does for the spec and bind info it was added with.\n"
     "False, and nothing changed, if the core holds no such pod. Raises CoreError."},
    {"delete_validated_pod_by_key", asCFunction(deleteValidatedByKeyEntry),
     METH_FASTCALL | METH_KEYWORDS,
     "delete_validated_pod_by_key($self, /, pod_key)\n--\n\n"
     "delete_allocated_pod_by_key whose core errors leave as\n"
     "WebServerError(code, text) with the CoreError as __cause__."},
};

void addDirectMethods(py::handle cls) {
  gCoreType = reinterpret_cast<PyTypeObject*>(cls.ptr());
  for (PyMethodDef& def : directMethods) {
    PyObject* descr = PyDescr_NewMethod(gCoreType, &def);
    if (descr == nullptr) throw py::error_already_set();
    int rc = PyObject_SetAttrString(cls.ptr(), def.ml_name, descr);
    Py_DECREF(descr);
    if (rc != 0) throw py::error_already_set();
  }
}

}  // namespace

PYBIND11_MODULE(hivedcore, m) {
  m.doc() = "MI355X-native gang scheduler core (C++)";
  initNames();
  initApiTypes();
  initResultType(m);

  static py::exception<HivedError> exc(m, "CoreError");
  gCoreError = exc.ptr();
  py::register_exception_translator([](std::exception_ptr p) {
    try {
      if (p) std::rethrow_exception(p);
    } catch (const HivedError& e) {
      py::object pyExc = exc;
      py::object inst = pyExc(e.what());
      inst.attr("code") = e.code;
      PyErr_SetObject(pyExc.ptr(), inst.ptr());
    }
  });

  py::class_<PyHivedCore> coreClass(m, "HivedCore");
  coreClass
      .def(py::init<const py::dict&>(), py::arg("spec"))
      .def("set_node_healthy", &PyHivedCore::setNodeHealthy, py::arg("node"), py::arg("healthy"))
      .def("set_xgmi_link_healthy", &PyHivedCore::setXgmiLinkHealthy, py::arg("node"),
           py::arg("a"), py::arg("b"), py::arg("healthy"), py::arg("gbps") = 0.0)
      .def("xgmi_links", &PyHivedCore::xgmiLinks, py::arg("node"))
      .def("set_leaf_cell_healthy", &PyHivedCore::setLeafCellHealthy, py::arg("node"),
           py::arg("leaf_index"), py::arg("healthy"))
      .def("all_nodes", &PyHivedCore::allNodes)
      .def("bad_nodes", &PyHivedCore::badNodes)
      .def("schedule", &PyHivedCore::schedule, py::arg("pod_spec"), py::arg("pod_key"),
           py::arg("suggested_nodes"), py::arg("phase"))
      .def("delete_unallocated_pod", &PyHivedCore::deleteUnallocatedPod, py::arg("pod_spec"),
           py::arg("pod_key"))
      .def("add_allocated_pod", &PyHivedCore::addAllocatedPod, py::arg("pod_spec"),
           py::arg("bind_info"), py::arg("pod_key"))
      .def("delete_allocated_pod", &PyHivedCore::deleteAllocatedPod, py::arg("pod_spec"),
           py::arg("bind_info"), py::arg("pod_key"))
      .def("get_all_affinity_groups", &PyHivedCore::getAllAffinityGroups)
      .def("get_affinity_group", &PyHivedCore::getAffinityGroup, py::arg("name"))
      .def("get_cluster_status", &PyHivedCore::getClusterStatus)
      .def("get_physical_cluster_status", &PyHivedCore::getPhysicalClusterStatus)
      .def("get_all_virtual_clusters_status", &PyHivedCore::getAllVirtualClustersStatus)
      .def("get_virtual_cluster_status", &PyHivedCore::getVirtualClusterStatus, py::arg("vc"))
      .def("schedule_count", &PyHivedCore::scheduleCount)
      .def("check_invariants", &PyHivedCore::checkInvariants)
      .def("debug_counters", &PyHivedCore::debugCounters);
  // schedule_pod, schedule_validated_pod and the two releases by key:
  // hand-written vectorcall methods
  addDirectMethods(coreClass);
}
