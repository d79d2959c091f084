"""Bind, preempt, commit and release give what they gave before they were made
leaner.

Golden replay: `tests/golden/lifecycle_decisions.json` holds every decision of
five streams, each with the affinity groups and the cluster status the core
was left in, recorded on the commit before the core's bind / preempt / commit
paths were made allocation-lean and pods came to be released by key. Re-record
(only ever on a commit whose decisions are the reference) with

    HIVED_LIFECYCLE_RECORD=1 python -m pytest tests/test_lifecycle_golden.py -k golden
"""
import hashlib
import json
import os
import random

import pytest

import bench
from hivedscheduler_amd.algorithm import FILTERING, PREEMPTING
from hivedscheduler_amd.api.types import WebServerError
from hivedscheduler_amd.sim import SimScheduler, mi355x_cluster_config

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                      "lifecycle_decisions.json")


def decision(sim, key, spec, suggested=None, phase=FILTERING, commit=True):
    """One sim.schedule as a JSON-able record: every field of the decision."""
    try:
        r = sim.schedule(key, spec, suggested, phase, commit)
    except WebServerError as e:
        return ["error", e.code, e.message]
    info = r.bind_info
    return [r.kind, info.node if info else "", list(info.leafCellIsolation) if info else [],
            r.victim_node, list(r.victim_pod_keys), r.wait_reason,
            info.to_dict() if info else None]


def end_state(sim):
    """What the core was left in: the groups in full, the cluster status as a
    digest of its canonical JSON (the status itself runs to tens of kB)."""
    sim.alg._core.check_invariants()
    status = json.dumps(sim.alg.get_cluster_status(), sort_keys=True, separators=(",", ":"))
    return {"groups": sim.alg.get_all_affinity_groups(),
            "status_sha256": hashlib.sha256(status.encode()).hexdigest()}


# ---------------------------------------------------------------------------
# the streams
# ---------------------------------------------------------------------------


def bench_stream():
    """bench.py's own stream on config 4, three steps; the last step's pods
    stay, so the end state is not the empty cluster."""
    sim = bench.make_sim()
    requests = bench.build_requests(seed=0, count=64)
    out = []
    for step in range(3):
        bound = []
        for i, req in enumerate(requests):
            key = f"bench/p{i}"
            spec = sim.pod_spec(vc=req["vc"], priority=req["priority"], leaf_cells=req["cells"])
            out.append(decision(sim, key, spec))
            if out[-1][0] == "bind":
                bound.append(key)
        if step < 2:
            for key in bound:
                sim.delete_pod(key)
    return {"decisions": out, "end": end_state(sim)}


GANGS = [[(2, 2)], [(1, 4), (2, 1)], [(2, 8)], [(3, 4)], [(2, 4)], [(1, 8), (1, 4)], [(4, 1)]]
FOUR_NODE_VCS = {
    "VC1": [("MI355X-NODE", 2)],
    "VC2": [("MI355X-NODE", 1), ("MI355X-NODE.MI355X-QUAD", 1)],
    "VC3": [("MI355X-NODE.MI355X-QUAD", 1)],
}


def mixed_stream(sim, seed, ops, vcs, gang_share=0.0, pinned_share=0.0, preempting_share=0.0,
                 lazy_share=0.0, events=None):
    """Seeded schedule / release / cancel operations on `sim`. Gang pods arrive
    one by one and in shuffled order, victims of a preempt decision are evicted
    most of the time, a waiting or preempting pod is cancelled now and then."""
    rng = random.Random(seed)
    pending = []  # (key, params): asked, not bound
    serial = 0
    out = []
    lazy_seen = []  # [operation, group] whenever a lazy-preempted group is in the core
    events = events or {}

    def new_requests():
        nonlocal serial
        serial += 1
        common = dict(vc=rng.choice(vcs), priority=rng.choice([-1, 0, 0, 1, 2]),
                      lazy_preemption=rng.random() < lazy_share)
        if rng.random() < pinned_share:
            common.update(vc="VC1", pinned_cell_id="VC1-PIN", priority=max(0, common["priority"]))
        if rng.random() >= gang_share:
            return [(f"ns/s{serial}", dict(common, leaf_cells=rng.choice([1, 2, 4, 8])))]
        members = rng.choice(GANGS)
        group = f"gang{serial}"
        pods = [(f"ns/{group}-{cells}-{i}", dict(common, leaf_cells=cells, group=group,
                                                 members=members))
                for pod_number, cells in members for i in range(pod_number)]
        rng.shuffle(pods)
        return pods

    for op in range(ops):
        if op in events:
            events[op](sim)
        roll = rng.random()
        if roll < 0.14 and sim.pods:
            sim.delete_pod(rng.choice(sorted(sim.pods)))
        elif roll < 0.18 and pending:
            key, params = pending.pop(rng.randrange(len(pending)))
            sim.delete_unallocated(key, sim.pod_spec(**params))
        else:
            if pending and rng.random() < 0.5:
                key, params = pending.pop(rng.randrange(len(pending)))
            else:
                first, *rest = new_requests()
                pending.extend(rest)
                key, params = first
            phase = PREEMPTING if rng.random() < preempting_share else FILTERING
            record = decision(sim, key, sim.pod_spec(**params), None, phase)
            out.append(record)
            if record[0] in ("wait", "preempt"):
                pending.append((key, params))
            if record[0] == "preempt" and rng.random() < 0.7:
                for victim in record[4]:  # the cluster's part: evict the victims
                    if victim in sim.pods:
                        sim.delete_pod(victim)
        if (op + 1) % 10 == 0:
            lazy_seen.extend([op, g["name"]] for g in sim.alg.get_all_affinity_groups()
                             if g["lazyPreemptionStatus"] is not None)
        if (op + 1) % 50 == 0:
            sim.alg._core.check_invariants()
    return {"decisions": out, "lazy_seen": lazy_seen, "end": end_state(sim)}


def gang_stream():
    sim = SimScheduler(mi355x_cluster_config(num_nodes=4, vcs=FOUR_NODE_VCS))
    return mixed_stream(sim, 11, 260, ["VC1", "VC1", "VC2", "VC3"], gang_share=0.6,
                        lazy_share=0.5)


def degraded_link_stream():
    """Degraded xGMI links on three of four nodes before and during the stream,
    so multi-GPU requests go through the clean-world rungs."""
    sim = SimScheduler(mi355x_cluster_config(num_nodes=4, vcs=FOUR_NODE_VCS))
    sim.alg.set_xgmi_link_healthy("node1", 0, 1, False, 12.0)
    sim.alg.set_xgmi_link_healthy("node2", 2, 3, False, 12.0)
    events = {
        60: lambda s: s.alg.set_xgmi_link_healthy("node3", 4, 6, False, 12.0),
        140: lambda s: s.alg.set_xgmi_link_healthy("node1", 0, 1, True, 150.0),
        170: lambda s: s.alg.set_bad_node("node4"),
        200: lambda s: s.alg.set_healthy_node("node4"),
    }
    return mixed_stream(sim, 12, 240, ["VC1", "VC1", "VC2", "VC3"], gang_share=0.35, events=events)


def pinned_stream(design_config):
    sim = SimScheduler(design_config)
    return mixed_stream(sim, 13, 240, ["VC1", "VC1", "VC2"], gang_share=0.3, pinned_share=0.3)


def preempting_stream():
    """Most decisions in the Preempting phase: preempting groups are created,
    joined, cancelled by a higher priority and by delete_unallocated."""
    sim = SimScheduler(mi355x_cluster_config(num_nodes=4, vcs=FOUR_NODE_VCS))
    return mixed_stream(sim, 14, 300, ["VC1", "VC1", "VC2", "VC3"], gang_share=0.3,
                        preempting_share=0.7, lazy_share=0.15)


def record_all(design_config):
    return {
        "bench": bench_stream(),
        "gangs": gang_stream(),
        "degraded-links": degraded_link_stream(),
        "pinned": pinned_stream(design_config),
        "preempting": preempting_stream(),
    }


def check_not_hollow(recorded):
    for name, stream in recorded.items():
        kinds = [d[0] for d in stream["decisions"]]
        for kind in ("bind", "preempt", "wait"):
            assert kinds.count(kind) >= 1, (name, kind)
        assert stream["end"]["groups"], name
    for name in ("gangs", "degraded-links", "pinned", "preempting"):
        # a multi-pod gang that got at least two of its pods bound
        gang_pods = {}
        for d in recorded[name]["decisions"]:
            if d[0] == "bind" and sum(len(m["podPlacements"])
                                      for m in d[6]["affinityGroupBindInfo"]) > 1:
                gang_pods.setdefault(json.dumps(d[6]["affinityGroupBindInfo"]), []).append(d)
        assert any(len(pods) >= 2 for pods in gang_pods.values()), name
    states = {g["state"] for g in recorded["preempting"]["end"]["groups"]}
    assert "Preempting" in states, states
    pinned = recorded["pinned"]["decisions"]
    assert any(d[0] == "bind" and d[1].endswith("n4") for d in pinned)
    assert recorded["gangs"]["lazy_seen"] or recorded["preempting"]["lazy_seen"]


@pytest.fixture(scope="module")
def recorded(design_config):
    # through JSON, so that what is compared is what a fixture can hold
    return json.loads(json.dumps(record_all(design_config)))


def test_golden_replay(recorded):
    check_not_hollow(recorded)
    if os.environ.get("HIVED_LIFECYCLE_RECORD") == "1":
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
        assert len(got["decisions"]) == len(want["decisions"]), name
        for i, (g, w) in enumerate(zip(got["decisions"], want["decisions"])):
            assert g == w, (name, i)
        assert got.get("lazy_seen") == want.get("lazy_seen"), name
        assert got["end"]["groups"] == want["end"]["groups"], name
        assert got["end"]["status_sha256"] == want["end"]["status_sha256"], name


def test_a_core_that_has_served_200_decisions_answers_like_a_new_one():
    """The reused-scratch check. Both cores hold the same committed pods; one
    then serves 200 mixed decisions that commit nothing. A fresh stream of
    uncommitted requests gets the same answers from both. (The fresh stream
    asks for single pods and the committed pods are single pods too, so a
    decision's victims sit on one node and the seeded victim draw picks that
    node however many draws went before; the 200 decisions include gangs.)"""
    def filled():
        sim = SimScheduler(mi355x_cluster_config(num_nodes=4, vcs=FOUR_NODE_VCS))
        rng = random.Random(5)
        for i in range(14):
            spec = sim.pod_spec(vc=rng.choice(["VC1", "VC2", "VC3"]), priority=rng.choice([-1, -1, 0]),
                                leaf_cells=rng.choice([1, 2, 4]))
            sim.schedule(f"ns/fill{i}", spec)
        return sim

    def request(sim, rng, i, gangs=True):
        leaf_cells = rng.choice([1, 2, 4, 8])
        if gangs and rng.random() < 0.3:
            members = rng.choice(GANGS)
            return f"ns/g{i}", sim.pod_spec(vc=rng.choice(["VC1", "VC2", "VC3"]),
                                            priority=rng.choice([-1, 0, 1, 2]),
                                            leaf_cells=members[0][1], group=f"g{i}", members=members)
        return f"ns/r{i}", sim.pod_spec(vc=rng.choice(["VC1", "VC2", "VC3"]),
                                        priority=rng.choice([-1, 0, 1, 2]), leaf_cells=leaf_cells)

    used, fresh = filled(), filled()
    rng = random.Random(6)
    kinds = [decision(used, *request(used, rng, i), commit=False)[0] for i in range(200)]
    assert {"bind", "preempt", "wait"} <= set(kinds), set(kinds)
    rng_used, rng_fresh = random.Random(7), random.Random(7)
    answers = []
    for i in range(60):
        got = decision(used, *request(used, rng_used, i, gangs=False), commit=False)
        assert got == decision(fresh, *request(fresh, rng_fresh, i, gangs=False),
                               commit=False), i
        answers.append(got[0])
    assert {"bind", "preempt", "wait"} <= set(answers), set(answers)
    assert used.alg.get_all_affinity_groups() == fresh.alg.get_all_affinity_groups()
    assert used.alg.get_cluster_status() == fresh.alg.get_cluster_status()
