"""The core decides, and is left in, what it did before its leaf-count maps went
flat, a decision's bind info came to be shared and erased groups were pooled.

Golden replay: `tests/golden/data_layout_decisions.json` holds every decision of
five streams field by field, each with the affinity groups and the cluster
status the core was left in, recorded on the commit before that change.
Re-record (only ever on a commit whose decisions are the reference) with

    HIVED_DATA_LAYOUT_RECORD=1 python -m pytest tests/test_data_layout_golden.py -k golden

The bench stream runs to 1920 decisions; its first and last round are held in
full, every round as the SHA-256 of its decisions' canonical JSON.
"""
import gc
import hashlib
import json
import os

import pytest

import bench
from hivedscheduler_amd.algorithm import FILTERING, PREEMPTING
from hivedscheduler_amd.api.types import (AffinityGroupMemberBindInfo, PodBindInfo,
                                          PodPlacementInfo, WebServerError)
from hivedscheduler_amd.sim import SimScheduler, mi355x_cluster_config

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                      "data_layout_decisions.json")
ALL_NODES_VC = {"VC1": [("MI355X-NODE", 4)]}


def decision(sim, key, spec, phase=FILTERING):
    """One committed sim.schedule as a JSON-able record: kind, node, isolation,
    chain, full affinityGroupBindInfo, victim node, victim keys, wait reason."""
    try:
        r = sim.schedule(key, spec, None, phase, True)
    except WebServerError as e:
        return {"kind": "error", "code": e.code, "message": e.message}
    info = r.bind_info
    return {"kind": r.kind,
            "node": info.node if info else "",
            "isolation": list(info.leafCellIsolation) if info else [],
            "chain": info.cellChain if info else "",
            "affinityGroupBindInfo": info.to_dict()["affinityGroupBindInfo"] if info else None,
            "victimNode": r.victim_node,
            "victimPodKeys": list(r.victim_pod_keys),
            "waitReason": r.wait_reason}


def end_state(sim):
    sim.alg._core.check_invariants()
    return {"groups": sim.alg.get_all_affinity_groups(), "status": sim.alg.get_cluster_status()}


def digest(records):
    text = json.dumps(records, sort_keys=True, separators=(",", ":"))
    return hashlib.sha256(text.encode()).hexdigest()


# ---------------------------------------------------------------------------
# the streams
# ---------------------------------------------------------------------------

GANG5 = [(1, 4), (1, 1), (1, 5), (1, 2), (1, 3)]  # five leaf counts, out of order


def five_count_gang_stream():
    """More distinct leaf counts than a flat map holds inline. Every pod is
    scheduled, the gang is released in another order and scheduled again."""
    sim = SimScheduler(mi355x_cluster_config(num_nodes=4, vcs=ALL_NODES_VC))
    out = []

    def schedule_all(order):
        for cells in order:
            spec = sim.pod_spec(vc="VC1", priority=1, leaf_cells=cells, group="gang5",
                                members=GANG5)
            out.append(decision(sim, f"ns/gang5-{cells}", spec))

    schedule_all([4, 1, 5, 2, 3])
    mid = sim.alg.get_affinity_group("gang5")
    for cells in (3, 5, 1, 4, 2):
        sim.delete_pod(f"ns/gang5-{cells}")
    emptied = sim.alg.get_all_affinity_groups()
    schedule_all([2, 5, 3, 1, 4])
    return {"decisions": out, "mid": mid, "emptied": emptied, "end": end_state(sim)}


def bench_stream(rounds=30):
    """bench.py's 64 requests with release, round after round: groups are
    erased and come back under the same names."""
    sim = bench.make_sim()
    requests = bench.build_requests(seed=0, count=64)
    per_round = []
    for _ in range(rounds):
        records, bound = [], []
        for i, req in enumerate(requests):
            key = f"bench/p{i}"
            spec = sim.pod_spec(vc=req["vc"], priority=req["priority"], leaf_cells=req["cells"])
            records.append(decision(sim, key, spec))
            if records[-1]["kind"] == "bind":
                bound.append(key)
        per_round.append(records)
        for key in bound:
            sim.delete_pod(key)
    return {"decisions": per_round[0], "last_round": per_round[-1],
            "round_sha256": [digest(r) for r in per_round],
            "binds_per_round": [sum(d["kind"] == "bind" for d in r) for r in per_round],
            "end": end_state(sim)}


def pool_hygiene_stream():
    """A lazily preempted group is released; the next group, a guaranteed one
    under another name, must show nothing of it."""
    sim = bench.make_sim()
    out = [decision(sim, "ns/lazy", sim.pod_spec(vc="VC1", priority=0, leaf_cells=8,
                                                 group="lazy", lazy_preemption=True)),
           decision(sim, "ns/other", sim.pod_spec(vc="VC1", priority=0, leaf_cells=8,
                                                  group="other")),
           # VC1's two nodes are taken: the higher priority takes the lazy
           # group's virtual cells and lands on a free physical node
           decision(sim, "ns/high", sim.pod_spec(vc="VC1", priority=1, leaf_cells=8,
                                                 group="high"))]
    lazy = sim.alg.get_affinity_group("lazy")
    sim.delete_pod("ns/lazy")
    out.append(decision(sim, "ns/fresh", sim.pod_spec(vc="VC2", priority=0, leaf_cells=4,
                                                      group="fresh")))
    fresh = sim.alg.get_affinity_group("fresh")
    return {"decisions": out, "lazy": lazy, "fresh": fresh, "end": end_state(sim)}


def preempting_stream():
    """A Preempting-phase gang reserves cells on two nodes, its second pod
    joins, a higher priority cancels it, the victims go and the preemptor is
    bound. Victims sit on two nodes, so every preempt decision draws a node."""
    sim = bench.make_sim()
    out = []
    for i in range(8):
        out.append(decision(sim, f"ns/low{i}", sim.pod_spec(vc="VC1", priority=0, leaf_cells=2)))
    members = [(2, 8)]
    mid_spec = dict(vc="VC1", priority=1, leaf_cells=8, group="mid", members=members)
    out.append(decision(sim, "ns/mid-0", sim.pod_spec(**mid_spec), PREEMPTING))
    out.append(decision(sim, "ns/mid-1", sim.pod_spec(**mid_spec), PREEMPTING))
    reserved = sim.alg.get_all_affinity_groups()
    top_spec = dict(vc="VC1", priority=2, leaf_cells=8, group="top", members=members)
    out.append(decision(sim, "ns/top-0", sim.pod_spec(**top_spec), PREEMPTING))
    cancelled = sim.alg.get_all_affinity_groups()
    for _ in range(8):  # the cluster's part: evict the victims, ask again
        if out[-1]["kind"] != "preempt":
            break
        for victim in out[-1]["victimPodKeys"]:
            if victim in sim.pods:
                sim.delete_pod(victim)
        out.append(decision(sim, "ns/top-0", sim.pod_spec(**top_spec), PREEMPTING))
    out.append(decision(sim, "ns/top-1", sim.pod_spec(**top_spec)))
    return {"decisions": out, "reserved": reserved, "cancelled": cancelled, "end": end_state(sim)}


def extended_bind_info_stream():
    """add_allocated_pod with a bind info that carries a leaf count the group
    spec does not (the core tolerates it by extending the group); the pod is
    released and its key reused with a consistent spec."""
    sim = SimScheduler(mi355x_cluster_config(num_nodes=4, vcs=ALL_NODES_VC))

    def placement(node, cells):
        return PodPlacementInfo(physicalNode=node, physicalLeafCellIndices=cells,
                                preassignedCellTypes=["MI355X-NODE"] * len(cells))

    info = PodBindInfo(
        node="node1", leafCellIsolation=[0, 1], cellChain="MI355X-NODE",
        affinityGroupBindInfo=[
            AffinityGroupMemberBindInfo(podPlacements=[placement("node1", [0, 1])]),
            AffinityGroupMemberBindInfo(podPlacements=[placement("node1", [4, 5, 6, 7])]),
        ])
    spec = sim.pod_spec(vc="VC1", priority=0, leaf_cells=2, group="odd", members=[(1, 2)])
    sim.alg.add_allocated_pod(spec, info, "ns/odd")
    extended = sim.alg.get_affinity_group("odd")
    sim.alg._core.check_invariants()
    released = sim.alg.delete_allocated_pod_by_key("ns/odd")
    after_release = sim.alg.get_all_affinity_groups()
    out = [decision(sim, "ns/odd", sim.pod_spec(vc="VC1", priority=0, leaf_cells=2, group="odd",
                                                members=[(1, 2)]))]
    return {"decisions": out, "extended": extended, "released": released,
            "after_release": after_release, "end": end_state(sim)}


def record_all():
    return {
        "five-count-gang": five_count_gang_stream(),
        "bench": bench_stream(),
        "pool-hygiene": pool_hygiene_stream(),
        "preempting": preempting_stream(),
        "extended-bind-info": extended_bind_info_stream(),
    }


def check_not_hollow(recorded):
    """The streams reach what they are for, in the golden as in the replay."""
    gang = recorded["five-count-gang"]
    assert [d["kind"] for d in gang["decisions"]] == ["bind"] * 10
    for d in gang["decisions"]:
        counts = [len(m["podPlacements"][0]["physicalLeafCellIndices"])
                  for m in d["affinityGroupBindInfo"]]
        assert counts == [1, 2, 3, 4, 5], counts  # ascending by leaf count
    assert len(gang["mid"]["allocatedPods"]) == 5 and gang["emptied"] == []

    bench_rec = recorded["bench"]
    assert len(bench_rec["round_sha256"]) == 30
    assert bench_rec["binds_per_round"] == [16] * 30
    kinds = [d["kind"] for d in bench_rec["decisions"]]
    assert {"bind", "preempt", "wait"} <= set(kinds)

    hygiene = recorded["pool-hygiene"]
    assert [d["kind"] for d in hygiene["decisions"]] == ["bind"] * 4
    assert hygiene["lazy"]["lazyPreemptionStatus"] is not None
    assert hygiene["lazy"]["virtualPlacement"] == {}
    assert hygiene["fresh"]["lazyPreemptionStatus"] is None
    assert hygiene["fresh"]["virtualPlacement"] != {}

    pre = recorded["preempting"]
    kinds = [d["kind"] for d in pre["decisions"]]
    assert kinds[:8] == ["bind"] * 8 and kinds[8:11] == ["preempt"] * 3, kinds
    assert kinds[-2:] == ["bind", "bind"], kinds
    states = {g["name"]: g["state"] for g in pre["reserved"]}
    assert states["mid"] == "Preempting"
    assert sorted(g["preemptingPods"] for g in pre["reserved"] if g["name"] == "mid")[0] == \
        ["ns/mid-0", "ns/mid-1"]
    states = {g["name"]: g["state"] for g in pre["cancelled"]}
    assert "mid" not in states and states["top"] == "Preempting"
    assert len({d["victimNode"] for d in pre["decisions"] if d["kind"] == "preempt"}) == 2

    ext = recorded["extended-bind-info"]
    assert ext["released"] is True and ext["after_release"] == []
    assert sorted(len(v) for v in ext["extended"]["physicalPlacement"].values()) == [6]
    assert ext["decisions"][0]["kind"] == "bind"


@pytest.fixture(scope="module")
def recorded():
    # through JSON, so that what is compared is what a fixture can hold
    return json.loads(json.dumps(record_all()))


def test_golden_replay(recorded):
    check_not_hollow(recorded)
    if os.environ.get("HIVED_DATA_LAYOUT_RECORD") == "1":
        os.makedirs(os.path.dirname(GOLDEN), exist_ok=True)
        with open(GOLDEN, "w") as f:
            json.dump(recorded, f, separators=(",", ":"), sort_keys=True)
            f.write("\n")
    with open(GOLDEN) as f:
        golden = json.load(f)
    check_not_hollow(golden)
    assert sorted(recorded) == sorted(golden)
    for name, want in golden.items():
        got = recorded[name]
        assert sorted(got) == sorted(want), name
        assert len(got["decisions"]) == len(want["decisions"]), name
        for i, (g, w) in enumerate(zip(got["decisions"], want["decisions"])):
            assert g == w, (name, i)
        for field in want:
            assert got[field] == want[field], (name, field)


def test_bind_info_outlives_pod_and_group():
    """The result of a committed bind keeps its bind info alive by itself: it is
    first read after the pod is released, its group erased and recycled a
    hundred times over, and reads as the decision made it."""
    def first_bind(sim):
        # the core's own call: SimScheduler.schedule would read bind_info at once
        spec = sim.pod_spec(vc="VC1", priority=0, leaf_cells=4, group="keep",
                            members=[(1, 4), (1, 2)])
        return sim.alg.schedule_pod(spec, "ns/keep", None, FILTERING, True)

    witness = SimScheduler(mi355x_cluster_config(num_nodes=4, vcs=ALL_NODES_VC))
    expected = first_bind(witness).bind_info
    assert len(expected.affinityGroupBindInfo) == 2

    sim = SimScheduler(mi355x_cluster_config(num_nodes=4, vcs=ALL_NODES_VC))
    result = first_bind(sim)
    assert result.kind == "bind"
    assert sim.alg.delete_allocated_pod_by_key("ns/keep") is True
    assert sim.alg.get_all_affinity_groups() == []
    for i in range(100):
        key = f"ns/k{i % 4}"
        r = sim.schedule(key, sim.pod_spec(vc="VC1", priority=i % 2, leaf_cells=(1, 2, 4, 8)[i % 4]))
        assert r.kind == "bind", (i, r)
        if i % 4 == 3:
            for k in list(sim.pods):
                sim.delete_pod(k)
    gc.collect()
    info = result.bind_info  # built now, for the first time
    assert info == expected
    assert info.to_dict() == expected.to_dict()
    assert repr(result) == f"ScheduleResult(bind node={expected.node} " \
                           f"cells={expected.leafCellIsolation})"
    assert result.bind_info is info
