"""The fused decision: HivedCore.schedule_pod validates and defaults the
request, decides, commits a bind and builds a native ScheduleResult in one
call. It must mean exactly what the separate steps mean: Python
validate_pod_scheduling_spec, all_nodes(), schedule, PodBindInfo.from_dict and
add_allocated_pod.
"""
import copy
import gc
import random
import sys

import pytest

from hivedscheduler_amd import hivedcore
from hivedscheduler_amd.algorithm import FILTERING, PREEMPTING, ScheduleResult, normalize_spec
from hivedscheduler_amd.api.types import (
    AffinityGroupMemberBindInfo,
    AffinityGroupMemberSpec,
    AffinityGroupSpec,
    PodBindInfo,
    PodPlacementInfo,
    PodSchedulingSpec,
    WebServerError,
)
from hivedscheduler_amd.internal.pod import validate_pod_scheduling_spec
from hivedscheduler_amd.sim import SimScheduler, mi355x_cluster_config

# 2 nodes; VC1 owns a node, VC2 a quad; the second quad of node 2 belongs to
# nobody and is only reachable opportunistically
TWIN_VCS = {"VC1": [("MI355X-NODE", 1)], "VC2": [("MI355X-NODE.MI355X-QUAD", 1)]}


def twin_config():
    return mi355x_cluster_config(num_nodes=2, vcs=TWIN_VCS)


def make_core(config=None):
    core = hivedcore.HivedCore(normalize_spec(config or twin_config()))
    for n in core.all_nodes():
        core.set_node_healthy(n, True)
    return core


def make_spec(vc="VC1", priority=0, cells=1, group=None, members=None, ignore_suggested=True):
    spec = PodSchedulingSpec(virtualCluster=vc, priority=priority, leafCellNumber=cells,
                             ignoreK8sSuggestedNodes=ignore_suggested)
    if group is not None:
        spec.affinityGroup = AffinityGroupSpec(
            name=group,
            members=[AffinityGroupMemberSpec(podNumber=p, leafCellNumber=c) for p, c in members])
    return spec


def fill_opportunistic(core):
    """Opportunistic pods on all but two GPUs: a 1-GPU request still binds,
    VC2's guaranteed quad has to preempt, and 8 GPUs in VC2 exceed its quota."""
    for i, cells in enumerate((4, 4, 4, 2)):
        filler = make_spec(vc="VC1", priority=-1, cells=cells)
        assert core.schedule_pod(filler, f"ns/fill{i}", commit=True).kind == "bind"


# ---------------------------------------------------------------------------
# twin equivalence
# ---------------------------------------------------------------------------


def outcome(fn):
    """What a call gave: ("ok", value) or ("error", type, code, text)."""
    try:
        return ("ok", fn())
    except hivedcore.CoreError as e:
        return ("error", "CoreError", e.code, str(e))
    except WebServerError as e:
        return ("error", "CoreError", e.code, e.message)


class Twins:
    """Two cores driven by the same operations: `old` through the separate
    steps, `new` through schedule_pod(commit=True)."""

    def __init__(self):
        self.old = make_core()
        self.new = make_core()
        self.live = {}  # key -> (params, old spec, old info, new spec, new info)
        self.kinds = set()

    def schedule(self, key, params, suggested, phase):
        old_spec, new_spec = make_spec(**params), make_spec(**params)
        given = None if suggested is None else list(suggested)

        def old_path():
            validate_pod_scheduling_spec(old_spec, key)
            nodes = self.old.all_nodes() if given is None else given
            raw = self.old.schedule(old_spec, key, nodes, phase)
            info = None
            if raw["kind"] == "bind":
                info = PodBindInfo.from_dict(raw["bindInfo"])
                self.old.add_allocated_pod(old_spec, info, key)
            return raw, info

        old = outcome(old_path)
        new = outcome(lambda: self.new.schedule_pod(new_spec, key, given, phase, commit=True))
        assert old[0] == new[0], (key, params, old, new)
        assert old_spec.affinityGroup == new_spec.affinityGroup
        if old[0] == "error":
            assert old[1:] == new[1:]
            self.kinds.add("error")
            return "error", []
        (raw, info), r = old[1], new[1]
        assert type(r) is ScheduleResult
        assert r.kind == raw["kind"], (key, params, raw, r)
        assert r.bind_info == info
        assert r.victim_node == raw.get("victimNode", "")
        assert r.victim_pod_keys == raw.get("victimPodKeys", [])
        assert r.wait_reason == raw.get("reason", "")
        self.kinds.add(r.kind)
        if r.kind == "bind":
            self.live[key] = (params, old_spec, info, new_spec, r.bind_info)
        return r.kind, list(r.victim_pod_keys)

    def delete(self, key):
        _, old_spec, old_info, new_spec, new_info = self.live.pop(key)
        self.old.delete_allocated_pod(old_spec, old_info, key)
        self.new.delete_allocated_pod(new_spec, new_info, key)

    def delete_unallocated(self, key, params):
        old_spec, new_spec = make_spec(**params), make_spec(**params)
        validate_pod_scheduling_spec(old_spec, key)
        validate_pod_scheduling_spec(new_spec, key)
        self.old.delete_unallocated_pod(old_spec, key)
        self.new.delete_unallocated_pod(new_spec, key)

    def health(self, method, *args):
        getattr(self.old, method)(*args)
        getattr(self.new, method)(*args)

    def compare(self, full):
        assert self.old.get_all_affinity_groups() == self.new.get_all_affinity_groups()
        assert self.old.schedule_count() == self.new.schedule_count()
        if full:
            assert self.old.get_cluster_status() == self.new.get_cluster_status()
            self.old.check_invariants()
            self.new.check_invariants()


GANG_SHAPES = [
    [(2, 2)],          # 2 pods x 2 GPUs
    [(1, 4), (2, 1)],  # 1 pod x 4 GPUs + 2 pods x 1 GPU
]


def run_twin_script(seed, ops=300):
    rng = random.Random(seed)
    twins = Twins()
    nodes = twins.old.all_nodes()
    pending = []  # (key, params): asked, not bound
    serial = 0

    def new_requests():
        nonlocal serial
        serial += 1
        common = dict(vc=rng.choice(["VC1", "VC1", "VC2"]), priority=rng.choice([-1, 0, 0, 1]),
                      ignore_suggested=rng.random() < 0.6)
        if rng.random() < 0.65:
            return [(f"ns/s{serial}", dict(common, cells=rng.choice([1, 2, 2, 4, 8])))]
        members = rng.choice(GANG_SHAPES)
        group = f"gang{serial}"
        pods = [(f"ns/{group}-{cells}-{i}", dict(common, cells=cells, group=group, members=members))
                for pod_number, cells in members for i in range(pod_number)]
        rng.shuffle(pods)
        return pods

    def suggested_nodes():
        pick = rng.random()
        if pick < 0.4:
            return None
        if pick < 0.7:
            return nodes
        return [rng.choice(nodes)]

    for op in range(ops):
        if op == ops // 3:
            twins.health("set_node_healthy", "node2", False)
        if op == ops // 2:
            twins.health("set_leaf_cell_healthy", "node1", 3, False)
        if op == (2 * ops) // 3:
            twins.health("set_node_healthy", "node2", True)
        if op == (5 * ops) // 6:
            twins.health("set_leaf_cell_healthy", "node1", 3, True)

        roll = rng.random()
        if roll < 0.25 and twins.live:
            twins.delete(rng.choice(sorted(twins.live)))
        elif roll < 0.30 and pending:
            key, params = pending.pop(rng.randrange(len(pending)))
            twins.delete_unallocated(key, params)
        else:
            if pending and rng.random() < 0.5:
                key, params = pending.pop(rng.randrange(len(pending)))
            else:
                first, *rest = new_requests()
                pending.extend(rest)
                key, params = first
            phase = PREEMPTING if rng.random() < 0.4 else FILTERING
            kind, victims = twins.schedule(key, params, suggested_nodes(), phase)
            if kind in ("wait", "preempt"):
                pending.append((key, params))
            if kind == "preempt" and rng.random() < 0.7:
                for victim in victims:  # the cluster's part: evict the victims
                    if victim in twins.live:
                        twins.delete(victim)
        twins.compare(full=(op + 1) % 25 == 0)
    twins.compare(full=True)
    return twins


@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_twin_cores_agree(seed):
    twins = run_twin_script(seed)
    # the script is only worth something if it reached every kind of answer
    assert {"bind", "wait", "preempt"} <= twins.kinds, twins.kinds


# ---------------------------------------------------------------------------
# validation
# ---------------------------------------------------------------------------

GANG = dict(group="g", members=[(1, 2)], cells=2)

REJECTED = {
    "empty VC": make_spec(vc=""),
    "priority below": make_spec(priority=-2),
    "priority above": make_spec(priority=1001),
    "leaf number zero": make_spec(cells=0),
    "leaf number negative": make_spec(cells=-3),
    "empty group name": make_spec(**dict(GANG, group="")),
    "member pod number": make_spec(cells=2, group="g", members=[(0, 2)]),
    "member leaf number": make_spec(cells=2, group="g", members=[(1, 2), (1, 0)]),
    "group without pod": make_spec(cells=2, group="g", members=[(1, 4)]),
    # the first failing check wins
    "empty VC and bad priority": make_spec(vc="", priority=-5),
    "bad priority and leaf": make_spec(priority=2000, cells=0),
}


@pytest.mark.parametrize("case", sorted(REJECTED))
def test_rejections_match_the_python_validation(case):
    expected_spec = copy.deepcopy(REJECTED[case])
    with pytest.raises(WebServerError) as expected:
        validate_pod_scheduling_spec(expected_spec, "ns/bad")
    assert expected.value.code == 400

    sim = SimScheduler(twin_config())
    assert sim.schedule("ns/first", sim.pod_spec(leaf_cells=2)).kind == "bind"
    count = sim.alg.schedule_count()
    groups = sim.alg.get_all_affinity_groups()

    spec = copy.deepcopy(REJECTED[case])
    with pytest.raises(WebServerError) as got:
        sim.schedule("ns/bad", spec)
    assert got.value.code == 400
    assert got.value.message == expected.value.message
    assert str(got.value) == str(expected.value)
    assert spec.affinityGroup == expected_spec.affinityGroup
    assert sim.alg.schedule_count() == count
    assert sim.alg.get_all_affinity_groups() == groups
    assert "ns/bad" not in sim.pods

    assert sim.schedule("ns/after", sim.pod_spec(leaf_cells=2)).kind == "bind"
    sim.alg._core.check_invariants()


def test_core_error_carries_the_code_and_text():
    core = make_core()
    with pytest.raises(hivedcore.CoreError) as e:
        core.schedule_pod(make_spec(vc=""), "ns/bad")
    assert e.value.code == 400 and str(e.value) == "VirtualCluster is empty"
    assert core.schedule_count() == 0


# ---------------------------------------------------------------------------
# defaulting
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("vc,priority,cells,phase,kind", [
    ("VC1", 0, 2, FILTERING, "bind"),
    ("VC2", 0, 8, FILTERING, "wait"),
    ("VC2", 1, 4, FILTERING, "preempt"),
    ("VC2", 1, 4, PREEMPTING, "preempt"),
])
def test_absent_group_is_defaulted_for_every_kind(vc, priority, cells, phase, kind):
    core = make_core()
    if kind != "bind":
        fill_opportunistic(core)
    key = "ns/some-pod"
    spec = make_spec(vc=vc, priority=priority, cells=cells)
    expected = copy.deepcopy(spec)
    validate_pod_scheduling_spec(expected, key)
    result = core.schedule_pod(spec, key, None, phase)
    assert result.kind == kind
    assert spec.affinityGroup == expected.affinityGroup
    assert spec == expected
    assert type(spec.affinityGroup) is AffinityGroupSpec
    assert type(spec.affinityGroup.members[0]) is AffinityGroupMemberSpec
    assert spec.affinityGroup.name is key
    assert repr(spec.affinityGroup) == repr(expected.affinityGroup)


def test_defaulted_spec_can_be_replayed_on_another_core():
    core = make_core()
    spec = make_spec(cells=4)
    result = core.schedule_pod(spec, "ns/p", commit=True)
    other = make_core()
    other.add_allocated_pod(spec, result.bind_info, "ns/p")
    assert other.get_all_affinity_groups() == core.get_all_affinity_groups()
    other.check_invariants()


def test_present_group_is_left_alone():
    core = make_core()
    spec = make_spec(cells=2, group="g", members=[(2, 2)])
    group, members, member = spec.affinityGroup, spec.affinityGroup.members, spec.affinityGroup.members[0]
    before = copy.deepcopy(spec)
    assert core.schedule_pod(spec, "ns/g-0", commit=True).kind == "bind"
    assert spec.affinityGroup is group
    assert spec.affinityGroup.members is members and members[0] is member
    assert spec == before


def test_validate_false_leaves_the_spec_untouched():
    core, twin = make_core(), make_core()
    spec = make_spec(cells=2)
    result = core.schedule_pod(spec, "ns/p", None, FILTERING, commit=True, validate=False)
    assert spec.affinityGroup is None
    assert spec == make_spec(cells=2)
    # today's schedule semantics: an absent group means the empty group name
    raw = twin.schedule(make_spec(cells=2), "ns/p", twin.all_nodes(), FILTERING)
    twin.add_allocated_pod(make_spec(cells=2), raw["bindInfo"], "ns/p")
    assert result.bind_info == PodBindInfo.from_dict(raw["bindInfo"])
    assert core.get_all_affinity_groups() == twin.get_all_affinity_groups()
    assert core.get_all_affinity_groups()[0]["name"] == ""
    # and no checks
    assert core.schedule_pod(make_spec(vc="VC1", priority=5000, cells=1, group="x", members=[(1, 4)]),
                             "ns/q", validate=False).kind in ("bind", "wait", "preempt")


# ---------------------------------------------------------------------------
# suggested nodes
# ---------------------------------------------------------------------------

ONE_VC_TWO_NODES = {"VC1": [("MI355X-NODE", 2)]}


def two_node_core_with_one_full_node():
    core = make_core(mi355x_cluster_config(num_nodes=2, vcs=ONE_VC_TWO_NODES))
    filler = make_spec(cells=8)
    full = core.schedule_pod(filler, "ns/fill", commit=True).bind_info.node
    free = "node2" if full == "node1" else "node1"
    return core, full, free


def test_none_means_every_node_for_a_new_group():
    core, full, free = two_node_core_with_one_full_node()
    raw = core.schedule(make_spec(cells=8, group="ns/p", members=[(1, 8)], ignore_suggested=False),
                        "ns/p", core.all_nodes(), FILTERING)
    result = core.schedule_pod(make_spec(cells=8, ignore_suggested=False), "ns/p", None)
    assert raw["kind"] == "bind" and result.kind == "bind"
    assert result.bind_info == PodBindInfo.from_dict(raw["bindInfo"])
    assert result.bind_info.node == free


def test_explicit_list_without_the_only_fitting_node_waits():
    core, full, free = two_node_core_with_one_full_node()
    for suggested in ([full], (full,), {full}, [full, "no-such-node"]):
        spec = make_spec(cells=8, ignore_suggested=False)
        assert core.schedule_pod(spec, "ns/p", suggested).kind == "wait"
        assert core.schedule(spec, "ns/p", list(suggested), FILTERING)["kind"] == "wait"
    assert core.schedule_pod(make_spec(cells=8, ignore_suggested=False), "ns/p", [full, free]).kind == "bind"
    # ignored suggestions: the list is never read
    assert core.schedule_pod(make_spec(cells=8), "ns/p", [full]).kind == "bind"


def preempting_group_cores():
    """Two cores, each with a Preempting gang "g" created with
    ignoreK8sSuggestedNodes=False by its first pod."""
    config = mi355x_cluster_config(num_nodes=2, vcs={"VC1": [("MI355X-NODE.MI355X-QUAD", 2)],
                                                     "VC2": [("MI355X-NODE.MI355X-QUAD", 2)]})
    cores = []
    for _ in range(2):
        core = make_core(config)
        for key in ("ns/o1", "ns/o2"):
            assert core.schedule_pod(make_spec(vc="VC2", priority=-1, cells=8), key, commit=True).kind == "bind"
        first = make_spec(vc="VC1", priority=1, cells=2, group="g", members=[(2, 2)], ignore_suggested=False)
        assert core.schedule_pod(first, "ns/g-0", None, PREEMPTING).kind == "preempt"
        assert core.get_affinity_group("g")["state"] == "Preempting"
        cores.append(core)
    return cores


def test_none_means_every_node_for_an_existing_group_with_its_own_flag():
    """The request ignores suggestions, the existing group does not: the
    group's nodes are checked against the suggested set, and None has to
    stand for all nodes there too, or the reservation would be cancelled."""
    fused, stepwise = preempting_group_cores()

    def second():
        return make_spec(vc="VC1", priority=1, cells=2, group="g", members=[(2, 2)], ignore_suggested=True)

    raw = stepwise.schedule(second(), "ns/g-1", stepwise.all_nodes(), PREEMPTING)
    result = fused.schedule_pod(second(), "ns/g-1", None, PREEMPTING)
    assert raw["kind"] == "preempt" and result.kind == "preempt"
    assert result.victim_node == raw["victimNode"]
    assert result.victim_pod_keys == raw["victimPodKeys"]
    assert sorted(fused.get_affinity_group("g")["preemptingPods"]) == ["ns/g-0", "ns/g-1"]
    assert fused.get_all_affinity_groups() == stepwise.get_all_affinity_groups()

    # an explicit list that leaves the reserved nodes out cancels the group
    reserved = sorted(fused.get_affinity_group("g")["physicalPlacement"])
    others = [n for n in fused.all_nodes() if n not in reserved] or ["no-such-node"]
    raw = stepwise.schedule(second(), "ns/g-1", others, PREEMPTING)
    result = fused.schedule_pod(second(), "ns/g-1", others, PREEMPTING)
    assert result.kind == raw["kind"]
    assert fused.get_affinity_group("g")["preemptingPods"] == ["ns/g-1"]
    assert fused.get_all_affinity_groups() == stepwise.get_all_affinity_groups()
    fused.check_invariants()


@pytest.mark.parametrize("bad", ["node1", 7])
@pytest.mark.parametrize("ignore_suggested", [True, False])
@pytest.mark.parametrize("validate", [True, False])
def test_a_str_or_an_int_is_no_node_collection(bad, ignore_suggested, validate):
    core = make_core()
    spec = make_spec(cells=1, group="ns/p", members=[(1, 1)], ignore_suggested=ignore_suggested)
    with pytest.raises(TypeError):
        core.schedule(spec, "ns/p", bad, FILTERING)
    with pytest.raises(TypeError):
        core.schedule_pod(spec, "ns/p", bad, FILTERING, False, validate)
    assert core.schedule_count() == 0
    sim = SimScheduler(twin_config())
    with pytest.raises(TypeError):
        sim.schedule("ns/p", make_spec(ignore_suggested=ignore_suggested), bad)
    assert sim.alg.schedule_count() == 0


def test_facade_schedule_still_wants_a_node_collection():
    sim = SimScheduler(twin_config())
    spec = make_spec(cells=1, group="ns/p", members=[(1, 1)])
    with pytest.raises(TypeError):
        sim.alg.schedule(spec, "ns/p", None)
    assert sim.alg.schedule(spec, "ns/p", []).kind == "bind"
    assert sim.alg.get_all_affinity_groups() == []  # decided, not committed


# ---------------------------------------------------------------------------
# the result object
# ---------------------------------------------------------------------------


def three_results():
    """A bind, a wait and a preempt answer from one core, with the raw dicts a
    twin core gives for the same requests."""
    core, twin = make_core(), make_core()
    fill_opportunistic(core)
    fill_opportunistic(twin)
    requests = {
        "bind": ("ns/b", make_spec(vc="VC1", priority=-1, cells=1)),
        "wait": ("ns/w", make_spec(vc="VC2", priority=0, cells=8)),
        "preempt": ("ns/p", make_spec(vc="VC2", priority=1, cells=4)),
    }
    out = {}
    for kind, (key, spec) in requests.items():
        twin_spec = copy.deepcopy(spec)
        validate_pod_scheduling_spec(twin_spec, key)
        raw = twin.schedule(twin_spec, key, twin.all_nodes(), FILTERING)
        result = core.schedule_pod(spec, key)
        assert result.kind == raw["kind"] == kind
        out[kind] = (result, raw)
    return out


def test_result_attributes_per_kind():
    results = three_results()
    bind, raw = results["bind"]
    assert (bind.victim_node, bind.victim_pod_keys, bind.wait_reason) == ("", [], "")
    assert bind.bind_info == PodBindInfo.from_dict(raw["bindInfo"])
    wait, raw = results["wait"]
    assert (wait.bind_info, wait.victim_node, wait.victim_pod_keys) == (None, "", [])
    assert wait.wait_reason == raw["reason"] != ""
    preempt, raw = results["preempt"]
    assert (preempt.bind_info, preempt.wait_reason) == (None, "")
    assert preempt.victim_node == raw["victimNode"] != ""
    assert preempt.victim_pod_keys == raw["victimPodKeys"] != []
    for result, _ in results.values():
        assert result.kind is sys.intern(result.kind)
        assert type(result.victim_pod_keys) is list
        assert result.victim_pod_keys is result.victim_pod_keys
        assert result.bind_info is result.bind_info
        with pytest.raises(AttributeError):
            result.kind = "bind"
    # a fresh list per result
    other, _ = three_results()["preempt"]
    assert other.victim_pod_keys == preempt.victim_pod_keys
    assert other.victim_pod_keys is not preempt.victim_pod_keys
    preempt.victim_pod_keys.append("x")
    assert other.victim_pod_keys == raw["victimPodKeys"]


def test_result_repr_keeps_the_old_format():
    results = three_results()
    bind, _ = results["bind"]
    assert repr(bind) == (f"ScheduleResult(bind node={bind.bind_info.node} "
                          f"cells={bind.bind_info.leafCellIsolation})")
    preempt, _ = results["preempt"]
    assert repr(preempt) == f"ScheduleResult(preempt victims={preempt.victim_pod_keys})"
    wait, _ = results["wait"]
    assert repr(wait) == f"ScheduleResult(wait reason={wait.wait_reason!r})"
    assert repr(wait).startswith("ScheduleResult(wait reason='")


@pytest.mark.parametrize("shape", ["singleton", "gang"])
def test_bind_info_equals_from_dict_of_the_raw_result(shape):
    core, twin = make_core(), make_core()
    if shape == "singleton":
        pods = [("ns/one", dict(cells=4))]
    else:
        members = [(1, 4), (2, 1)]
        pods = [(f"ns/gang-{c}-{i}", dict(cells=c, group="gang", members=members))
                for p, c in members for i in range(p)]
    for key, params in pods:
        raw = twin.schedule(make_spec(**params) if shape == "gang" else
                            make_spec(group=key, members=[(1, 4)], **params),
                            key, twin.all_nodes(), FILTERING)
        result = core.schedule_pod(make_spec(**params), key, commit=True)
        expected = PodBindInfo.from_dict(raw["bindInfo"])
        twin.add_allocated_pod(make_spec(**params) if shape == "gang" else
                               make_spec(group=key, members=[(1, 4)], **params), expected, key)
        info = result.bind_info
        assert info is result.bind_info
        assert info == expected
        assert info.to_dict() == raw["bindInfo"]
        assert repr(info) == repr(expected)
        assert type(info) is PodBindInfo
        assert all(type(m) is AffinityGroupMemberBindInfo for m in info.affinityGroupBindInfo)
        assert all(type(p) is PodPlacementInfo
                   for m in info.affinityGroupBindInfo for p in m.podPlacements)
        assert all(type(i) is int for i in info.leafCellIsolation)
    if shape == "gang":
        assert len(info.affinityGroupBindInfo) == 2
        assert sorted(len(m.podPlacements) for m in info.affinityGroupBindInfo) == [1, 2]
    assert core.get_all_affinity_groups() == twin.get_all_affinity_groups()


def test_sim_keeps_spec_and_bind_info_of_a_committed_bind():
    sim = SimScheduler(twin_config())
    spec = sim.pod_spec(leaf_cells=2)
    result = sim.schedule("ns/p", spec)
    assert sim.pods["ns/p"] == (spec, result.bind_info)
    assert sim.pods["ns/p"][1] is result.bind_info
    uncommitted = sim.schedule("ns/q", sim.pod_spec(leaf_cells=2), commit=False)
    assert uncommitted.kind == "bind" and "ns/q" not in sim.pods
    assert [g["name"] for g in sim.alg.get_all_affinity_groups()] == ["ns/p"]
    sim.delete_pod("ns/p")
    sim.assert_empty()


# ---------------------------------------------------------------------------
# reference counts
# ---------------------------------------------------------------------------

N_REFCOUNT = 20000


def watched_objects(core, key):
    return ([PodSchedulingSpec, AffinityGroupSpec, AffinityGroupMemberSpec, PodBindInfo,
             AffinityGroupMemberBindInfo, PodPlacementInfo, ScheduleResult, key,
             sys.intern("bind"), sys.intern("preempt"), sys.intern("wait")]
            + core.all_nodes())


def refcounts(objects):
    gc.collect()
    return [sys.getrefcount(o) for o in objects]


@pytest.mark.parametrize("kind", ["bind", "wait", "preempt"])
def test_refcounts_are_steady_over_decisions(kind):
    core = make_core()
    fill_opportunistic(core)
    params = {"bind": dict(vc="VC1", priority=-1, cells=1),
              "wait": dict(vc="VC2", priority=0, cells=8),
              "preempt": dict(vc="VC2", priority=1, cells=4)}[kind]
    key = "ns/refcount-" + kind
    nodes = core.all_nodes()
    watched = watched_objects(core, key)
    before = refcounts(watched)
    for i in range(N_REFCOUNT):
        spec = make_spec(**params)
        suggested = None if i % 2 else nodes
        spec.ignoreK8sSuggestedNodes = bool(i % 4 < 2)
        result = core.schedule_pod(spec, key, suggested)
        assert result.kind == kind
        # read everything, twice
        for _ in range(2):
            result.bind_info, result.victim_node, result.victim_pod_keys, result.wait_reason
        repr(result)
    del spec, result, suggested
    assert refcounts(watched) == before


def test_refcounts_are_steady_over_committed_binds_and_rejections():
    core = make_core()
    key = "ns/refcount-commit"
    watched = watched_objects(core, key)
    before = refcounts(watched)
    for i in range(N_REFCOUNT):
        if i % 3 == 0:
            spec = make_spec(cells=2, group="g", members=[(1, 2)])
        else:
            spec = make_spec(cells=2)
        result = core.schedule_pod(spec, key, None, FILTERING, True)
        assert result.kind == "bind"
        if i % 2:
            core.delete_allocated_pod(spec, result.bind_info, key)
        else:  # the result outlives the bind info it handed out, and the other way round
            info = result.bind_info
            del result
            core.delete_allocated_pod(spec, info, key)
            del info
        if i % 5 == 0:
            with pytest.raises(hivedcore.CoreError):
                core.schedule_pod(make_spec(cells=0), key)
    del spec, result
    assert refcounts(watched) == before
    assert core.get_all_affinity_groups() == []
    core.check_invariants()
