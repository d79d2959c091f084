"""The Python <-> C++ boundary of the scheduling core (core/bindings.cpp).

The binding takes a request and a bind info either as the wire-format dict or
as the API object itself (PodSchedulingSpec / PodBindInfo, read by attribute).
Both forms must mean the same, keep the dict form's defaulting and errors, and
the suggested-node list must still be honoured wherever the core reads it,
although it is only converted on demand.
"""
import copy

import pytest

from hivedscheduler_amd import hivedcore
from hivedscheduler_amd.algorithm import normalize_spec
from hivedscheduler_amd.api.types import (
    AffinityGroupMemberSpec,
    AffinityGroupSpec,
    PodBindInfo,
    PodSchedulingSpec,
)
from hivedscheduler_amd.sim import mi355x_cluster_config

FILTERING = "Filtering"
PREEMPTING = "Preempting"


def make_core(num_nodes=1, vcs=None):
    core = hivedcore.HivedCore(normalize_spec(mi355x_cluster_config(num_nodes=num_nodes, vcs=vcs)))
    for n in core.all_nodes():
        core.set_node_healthy(n, True)
    return core


def make_spec(key, vc="VC1", priority=0, cells=1, group=None, members=None, ignore_suggested=True):
    """A validated-looking request: singleton group named after the pod unless
    a gang is given as members=[(podNumber, leafCellNumber), ...]."""
    return PodSchedulingSpec(
        virtualCluster=vc,
        priority=priority,
        leafCellNumber=cells,
        ignoreK8sSuggestedNodes=ignore_suggested,
        affinityGroup=AffinityGroupSpec(
            name=group or key,
            members=[AffinityGroupMemberSpec(podNumber=p, leafCellNumber=c)
                     for p, c in (members or [(1, cells)])],
        ),
    )


def as_form(form, spec):
    return spec.to_dict() if form == "dict" else spec


def info_as_form(form, raw_bind_info):
    return raw_bind_info if form == "dict" else PodBindInfo.from_dict(raw_bind_info)


# ---------------------------------------------------------------------------
# dict form and object form agree
# ---------------------------------------------------------------------------

TWO_VCS = {"VC1": [("MI355X-NODE", 1)], "VC2": [("MI355X-NODE", 1)]}


def run_script(form):
    """Guaranteed, opportunistic and a 2-pod gang through schedule -> add ->
    delete, plus one wait and one preempt answer. Returns every raw result and
    the group table at three points."""
    core = make_core(2, TWO_VCS)
    nodes = core.all_nodes()
    raws, tables, live = [], [], []

    def sched(key, spec, phase=FILTERING):
        raw = core.schedule(as_form(form, spec), key, nodes, phase)
        raws.append(raw)
        return raw

    def commit(key, spec, raw):
        assert raw["kind"] == "bind", raw
        core.add_allocated_pod(as_form(form, spec), info_as_form(form, raw["bindInfo"]), key)
        live.append((key, spec, raw["bindInfo"]))

    guaranteed = make_spec("ns/g1", vc="VC1", priority=0, cells=2)
    commit("ns/g1", guaranteed, sched("ns/g1", guaranteed))
    opportunistic = make_spec("ns/o1", vc="VC2", priority=-1, cells=8)
    commit("ns/o1", opportunistic, sched("ns/o1", opportunistic))
    for key in ("ns/gang-0", "ns/gang-1"):
        gang = make_spec(key, vc="VC1", priority=0, cells=2, group="gang", members=[(2, 2)])
        commit(key, gang, sched(key, gang))
    tables.append(core.get_all_affinity_groups())

    waiter = make_spec("ns/w", vc="VC1", priority=0, cells=8)
    assert sched("ns/w", waiter)["kind"] == "wait"
    core.delete_unallocated_pod(as_form(form, waiter), "ns/w")
    preemptor = make_spec("ns/p", vc="VC2", priority=1, cells=8)
    assert sched("ns/p", preemptor)["kind"] == "preempt"
    tables.append(core.get_all_affinity_groups())
    core.check_invariants()

    for key, spec, raw_info in live:
        core.delete_allocated_pod(as_form(form, spec), info_as_form(form, raw_info), key)
    tables.append(core.get_all_affinity_groups())
    assert tables[-1] == []
    core.check_invariants()
    return raws, tables


def test_dict_form_and_object_form_agree():
    dict_raws, dict_tables = run_script("dict")
    obj_raws, obj_tables = run_script("object")
    assert [r["kind"] for r in dict_raws] == ["bind"] * 4 + ["wait", "preempt"]
    assert obj_raws == dict_raws
    assert obj_tables == dict_tables


# ---------------------------------------------------------------------------
# defaults
# ---------------------------------------------------------------------------


def test_missing_keys_and_explicit_none_mean_the_defaults():
    explicit = {
        "virtualCluster": "VC1", "priority": 0, "pinnedCellId": "", "leafCellType": "",
        "leafCellNumber": 2, "gangReleaseEnable": False, "lazyPreemptionEnable": False,
        "ignoreK8sSuggestedNodes": True, "hbmBytesPerCell": 0,
        "affinityGroup": {"name": "", "members": [{"podNumber": 1, "leafCellNumber": 2}]},
    }
    missing = {"virtualCluster": "VC1", "leafCellNumber": 2}
    nones = {
        "virtualCluster": "VC1", "priority": None, "pinnedCellId": None, "leafCellType": None,
        "leafCellNumber": 2, "gangReleaseEnable": None, "lazyPreemptionEnable": None,
        "ignoreK8sSuggestedNodes": None, "hbmBytesPerCell": None, "affinityGroup": None,
    }
    members_none = dict(missing, affinityGroup={"name": None, "members": None})
    obj_nones = PodSchedulingSpec(
        virtualCluster="VC1", priority=None, pinnedCellId=None, leafCellType=None,
        leafCellNumber=2, gangReleaseEnable=None, lazyPreemptionEnable=None,
        ignoreK8sSuggestedNodes=None, hbmBytesPerCell=None, affinityGroup=None)
    obj_members_none = PodSchedulingSpec(
        virtualCluster="VC1", leafCellNumber=2,
        affinityGroup=AffinityGroupSpec(name=None, members=None))

    outcomes = []
    for spec in (explicit, missing, nones, members_none, obj_nones, obj_members_none):
        core = make_core(1)
        # ignoreK8sSuggestedNodes defaults to True: the unknown name is never read
        raw = core.schedule(spec, "ns/p", ["no-such-node"], FILTERING)
        assert raw["kind"] == "bind", (spec, raw)
        core.add_allocated_pod(spec, raw["bindInfo"], "ns/p")
        core.check_invariants()
        outcomes.append((raw, core.get_all_affinity_groups()))
    # the singleton-group default gives every form the same one-pod group
    assert all(o == outcomes[0] for o in outcomes[1:])
    assert outcomes[0][1][0]["allocatedPods"] == ["ns/p"]


@pytest.mark.parametrize("form", ["dict", "object"])
def test_bool_fields_take_0_and_1(form):
    for flag, suggested, expected in ((0, ["no-such-node"], "wait"), (1, ["no-such-node"], "bind"),
                                      (0, ["node1"], "bind")):
        core = make_core(1)
        spec = make_spec("ns/p", cells=8)
        spec.ignoreK8sSuggestedNodes = flag
        assert core.schedule(as_form(form, spec), "ns/p", suggested, FILTERING)["kind"] == expected


class VCName:
    """Not a str, but str() of it names a real VC."""

    def __str__(self):
        return "VC1"


@pytest.mark.parametrize("form", ["dict", "object"])
def test_non_str_string_field_goes_through_str(form):
    core = make_core(1)
    spec = make_spec("ns/p", cells=2)
    spec.virtualCluster = VCName()
    raw = core.schedule(as_form(form, spec), "ns/p", [], FILTERING)
    assert raw["kind"] == "bind"
    core.add_allocated_pod(as_form(form, spec), raw["bindInfo"], "ns/p")
    assert core.get_affinity_group("ns/p")["vc"] == "VC1"


# ---------------------------------------------------------------------------
# errors
# ---------------------------------------------------------------------------


def assert_still_usable(core):
    core.check_invariants()
    spec = make_spec("ns/after", cells=1)
    assert core.schedule(spec, "ns/after", [], FILTERING)["kind"] == "bind"


@pytest.mark.parametrize("form", ["dict", "object"])
def test_negative_hbm_is_a_400(form):
    core = make_core(1)
    spec = make_spec("ns/p")
    spec.hbmBytesPerCell = -1
    with pytest.raises(hivedcore.CoreError) as e:
        core.schedule(as_form(form, spec), "ns/p", [], FILTERING)
    assert e.value.code == 400
    assert_still_usable(core)


@pytest.mark.parametrize("form", ["dict", "object"])
def test_unknown_vc_is_a_400(form):
    core = make_core(1)
    spec = make_spec("ns/p", vc="NO-SUCH-VC")
    with pytest.raises(hivedcore.CoreError) as e:
        core.schedule(as_form(form, spec), "ns/p", [], FILTERING)
    assert e.value.code == 400
    assert_still_usable(core)


@pytest.mark.parametrize("form", ["dict", "object"])
@pytest.mark.parametrize("field", ["priority", "leafCellNumber", "hbmBytesPerCell"])
def test_wrong_type_for_int_field_raises_and_core_stays_usable(form, field):
    core = make_core(1)
    spec = make_spec("ns/p")
    setattr(spec, field, "three")
    request = as_form(form, spec)
    if form == "dict":
        request[field] = "three"  # to_dict() leaves a falsy hbmBytesPerCell out
    with pytest.raises(Exception):
        core.schedule(request, "ns/p", [], FILTERING)
    assert_still_usable(core)


def test_failing_lookup_is_not_swallowed():
    class Boom(Exception):
        pass

    class Spec:
        virtualCluster = "VC1"

        def __getattr__(self, name):
            raise Boom(name)

    core = make_core(1)
    with pytest.raises(Boom):
        core.schedule(Spec(), "ns/p", [], FILTERING)
    assert_still_usable(core)


# ---------------------------------------------------------------------------
# lazy suggested set
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("form", ["dict", "object"])
def test_suggested_list_is_read_when_the_request_does_not_ignore_it(form):
    # node1 is full, node2 is the only free node
    core = make_core(2, {"VC1": [("MI355X-NODE", 2)]})
    filler = make_spec("ns/fill", cells=8)
    raw = core.schedule(filler, "ns/fill", [], FILTERING)
    core.add_allocated_pod(filler, raw["bindInfo"], "ns/fill")
    full = raw["bindInfo"]["node"]
    free = "node2" if full == "node1" else "node1"

    spec = make_spec("ns/p", cells=8, ignore_suggested=False)
    assert core.schedule(as_form(form, spec), "ns/p", [full], FILTERING)["kind"] == "wait"
    raw = core.schedule(as_form(form, spec), "ns/p", (full, free), FILTERING)
    assert raw["kind"] == "bind" and raw["bindInfo"]["node"] == free


@pytest.mark.parametrize("form", ["dict", "object"])
def test_existing_preempting_group_is_governed_by_its_own_flag(form):
    """A Preempting group created with ignoreK8sSuggestedNodes=False is checked
    against the suggested list on every re-filter, whatever the re-filtering
    request's own flag says: inside the list it stays, outside it is cancelled
    and scheduled afresh."""
    core = make_core(2, {"VC1": [("MI355X-NODE.MI355X-QUAD", 2)],
                         "VC2": [("MI355X-NODE.MI355X-QUAD", 2)]})
    for key in ("ns/o1", "ns/o2"):
        filler = make_spec(key, vc="VC2", priority=-1, cells=8)
        raw = core.schedule(filler, key, [], FILTERING)
        core.add_allocated_pod(filler, raw["bindInfo"], key)

    def gang_pod(key, ignore_suggested):
        return as_form(form, make_spec(key, vc="VC1", priority=1, cells=2, group="g",
                                       members=[(2, 2)], ignore_suggested=ignore_suggested))

    both = ["node1", "node2"]
    assert core.schedule(gang_pod("ns/g-0", False), "ns/g-0", both, PREEMPTING)["kind"] == "preempt"
    group = core.get_affinity_group("g")
    assert group["state"] == "Preempting" and group["preemptingPods"] == ["ns/g-0"]
    reserved = sorted(group["physicalPlacement"])

    # the request ignores suggestions, the group does not: its nodes are
    # suggested, so the reservation stays and the second pod joins it
    assert core.schedule(gang_pod("ns/g-1", True), "ns/g-1", both, PREEMPTING)["kind"] == "preempt"
    group = core.get_affinity_group("g")
    assert sorted(group["preemptingPods"]) == ["ns/g-0", "ns/g-1"]
    assert sorted(group["physicalPlacement"]) == reserved

    # now the list leaves the reserved nodes out: cancelled and rescheduled,
    # so the group is a new one that only knows the re-filtering pod
    others = [n for n in both if n not in reserved] or ["no-such-node"]
    assert core.schedule(gang_pod("ns/g-1", True), "ns/g-1", others, PREEMPTING)["kind"] == "preempt"
    assert core.get_affinity_group("g")["preemptingPods"] == ["ns/g-1"]
    core.check_invariants()


@pytest.mark.parametrize("form", ["dict", "object"])
def test_unknown_names_change_nothing_when_suggestions_are_ignored(form):
    outcomes = []
    for suggested in (["node1", "node2"], ["x", "y", "z"], []):
        core = make_core(2, {"VC1": [("MI355X-NODE", 2)]})
        raws = []
        for i, cells in enumerate((4, 8, 2, 8)):
            spec = make_spec(f"ns/p{i}", cells=cells)
            raw = core.schedule(as_form(form, spec), f"ns/p{i}", suggested, FILTERING)
            if raw["kind"] == "bind":
                core.add_allocated_pod(as_form(form, spec), raw["bindInfo"], f"ns/p{i}")
            raws.append(raw)
        outcomes.append((raws, core.get_all_affinity_groups()))
    assert outcomes[1] == outcomes[0] and outcomes[2] == outcomes[0]


@pytest.mark.parametrize("form", ["dict", "object"])
@pytest.mark.parametrize("ignore_suggested", [True, False])
@pytest.mark.parametrize("bad", [None, "node1"])
def test_suggested_nodes_must_be_a_sequence_of_names(form, ignore_suggested, bad):
    core = make_core(1)
    spec = make_spec("ns/p", ignore_suggested=ignore_suggested)
    with pytest.raises(TypeError):
        core.schedule(as_form(form, spec), "ns/p", bad, FILTERING)
    assert_still_usable(core)


# ---------------------------------------------------------------------------
# all_nodes()
# ---------------------------------------------------------------------------


def test_all_nodes_returns_a_fresh_list_each_time():
    core = make_core(2, {"VC1": [("MI355X-NODE", 2)]})
    first = core.all_nodes()
    second = core.all_nodes()
    assert first == second == ["node1", "node2"]
    assert first is not second
    first.clear()
    second[0] = "mutated"
    assert core.all_nodes() == ["node1", "node2"]
    core.set_node_healthy("node1", False)
    assert core.bad_nodes() == ["node1"]
    assert core.all_nodes() == ["node1", "node2"]


# ---------------------------------------------------------------------------
# bind round trip
# ---------------------------------------------------------------------------

# get_affinity_group("ns/rt") for a 4-GPU guaranteed pod on an empty one-node
# cluster, recorded from the dict-only binding this file's subject replaced
ROUND_TRIP_BIND_INFO = {
    "node": "node1",
    "leafCellIsolation": [0, 1, 2, 3],
    "cellChain": "MI355X-NODE",
    "affinityGroupBindInfo": [{"podPlacements": [{
        "physicalNode": "node1",
        "physicalLeafCellIndices": [0, 1, 2, 3],
        "preassignedCellTypes": ["MI355X-NODE"] * 4,
    }]}],
}
ROUND_TRIP_GROUP = {
    "name": "ns/rt",
    "vc": "VC1",
    "priority": 0,
    "state": "Allocated",
    "lazyPreemptionStatus": None,
    "physicalPlacement": {"node1": [0, 1, 2, 3]},
    "virtualPlacement": {"VC1/MI355X-NODE/0": [
        "VC1/MI355X-NODE/0/0/0/0", "VC1/MI355X-NODE/0/0/0/1",
        "VC1/MI355X-NODE/0/0/1/0", "VC1/MI355X-NODE/0/0/1/1"]},
    "allocatedPods": ["ns/rt"],
    "preemptingPods": [],
}


@pytest.mark.parametrize("form", ["dict", "object"])
def test_bind_info_round_trip(form):
    core = make_core(1)
    spec = make_spec("ns/rt", cells=4)
    raw = core.schedule(as_form(form, spec), "ns/rt", [], FILTERING)
    assert raw == {"kind": "bind", "bindInfo": ROUND_TRIP_BIND_INFO}
    fed_back = info_as_form(form, copy.deepcopy(raw["bindInfo"]))
    core.add_allocated_pod(as_form(form, spec), fed_back, "ns/rt")
    assert core.get_affinity_group("ns/rt") == ROUND_TRIP_GROUP
    core.check_invariants()
    core.delete_allocated_pod(as_form(form, spec), fed_back, "ns/rt")
    assert core.get_all_affinity_groups() == []
    core.check_invariants()
