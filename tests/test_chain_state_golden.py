"""The core decides, and is left in, what it did before a chain's state came to
be reached by pointer, the doom checks learned to cost nothing on a healthy
cluster and the mapper's candidate lists stopped growing on the heap.

Golden replay: `tests/golden/chain_state_decisions.json` holds four streams
that no other golden covers, recorded on the commit before that change: every
decision field by field (the bench stream as a SHA-256 per round), and at fixed
points of each stream the affinity groups, the cluster status, the debug
counters with the order of their keys, and the outcome of the invariant check.
Re-record (only ever on a commit whose decisions are the reference) with

    HIVED_CHAIN_STATE_RECORD=1 python -m pytest tests/test_chain_state_golden.py -k golden
"""
import hashlib
import json
import os

import pytest

import bench
from hivedscheduler_amd.algorithm import FILTERING, PREEMPTING
from hivedscheduler_amd.api import config as apicfg
from hivedscheduler_amd.api.types import WebServerError
from hivedscheduler_amd.sim import SimScheduler

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "chain_state_decisions.json")
DESIGN = os.path.join(os.path.dirname(HERE), "examples", "config", "design-heterogeneous.yaml")


def decision(sim, key, spec, phase=FILTERING):
    """One committed sim.schedule as a JSON-able record."""
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


def ordered(value):
    """Dicts as lists of [key, value] in their own order, so that the order of
    the debug counters' keys is part of what is compared."""
    if isinstance(value, dict):
        return [[k, ordered(v)] for k, v in value.items()]
    if isinstance(value, (list, tuple)):
        return [ordered(v) for v in value]
    return value


def digest(records):
    text = json.dumps(records, sort_keys=True, separators=(",", ":"))
    return hashlib.sha256(text.encode()).hexdigest()


def invariants(sim):
    try:
        sim.alg._core.check_invariants()
    except Exception as e:  # recorded, so that a replay must fail the same way
        return str(e)
    return "ok"


def snapshot(sim, full=False):
    """The state the core is left in. The counters and the invariant check are
    always held in full; groups and status in full where asked for, else as
    digests (a status of the config-4 cluster is 20 KB)."""
    groups = sim.alg.get_all_affinity_groups()
    status = sim.alg.get_cluster_status()
    snap = {"counters": ordered(sim.alg._core.debug_counters()),
            "invariants": invariants(sim),
            "groups_sha256": digest(groups),
            "status_sha256": digest(status)}
    if full:
        snap["groups"] = groups
        snap["status"] = status
    return snap


def counter_levels(snap):
    """(chain, level, fields as a dict) of a snapshot's recorded counters."""
    for chain, levels in snap["counters"]:
        for level, fields in levels:
            yield chain, level, dict((k, v) for k, v in fields)


def release(sim, out, keys):
    for key in keys:
        if key in sim.pods:
            sim.delete_pod(key)
            out.append({"kind": "release", "key": key})


# ---------------------------------------------------------------------------
# the streams
# ---------------------------------------------------------------------------

def health_flap_stream():
    """Nodes and single GPUs of the config-4 cluster go bad and heal between
    schedules, preemptions and releases. The VCs' quota is the whole cluster,
    so a bad free node dooms a VC's cell, and healing it lifts the doom."""
    sim = bench.make_sim()
    alg = sim.alg
    out, snaps = [], []
    requests = bench.build_requests(seed=0, count=64)

    def spec_of(req, **kw):
        return sim.pod_spec(vc=req["vc"], priority=req["priority"], leaf_cells=req["cells"], **kw)

    def wave(tag, reqs, phase=FILTERING):
        keys = []
        for i, req in enumerate(reqs):
            key = f"flap/{tag}{i}"
            out.append(decision(sim, key, spec_of(req), phase))
            if out[-1]["kind"] == "bind":
                keys.append(key)
        return keys

    snaps.append(snapshot(sim))
    # a free node goes bad on an empty cluster: doomed cells, bad free cells
    alg.set_bad_node("node1")
    snaps.append(snapshot(sim, full=True))
    first = wave("a", requests[:24])
    snaps.append(snapshot(sim))
    # one GPU of a used node goes bad, a second node goes bad under load
    alg.set_leaf_cell_healthy("node2", 3, False)
    alg.set_bad_node("node3")
    snaps.append(snapshot(sim))
    second = wave("b", requests[24:48])
    snaps.append(snapshot(sim))
    # guaranteed gangs preempt what sits on their cells
    for i, (vc, cells) in enumerate([("VC1", 8), ("VC2", 4), ("VC3", 4), ("VC1", 8)]):
        key = f"flap/gang{i}"
        spec = sim.pod_spec(vc=vc, priority=5, leaf_cells=cells)
        for _ in range(6):
            out.append(decision(sim, key, spec, PREEMPTING))
            if out[-1]["kind"] != "preempt":
                break
            release(sim, out, out[-1]["victimPodKeys"])
    snaps.append(snapshot(sim))
    # heal under load, release half, flap again
    alg.set_healthy_node("node1")
    snaps.append(snapshot(sim))
    release(sim, out, first[::2] + second[1::2])
    alg.set_leaf_cell_healthy("node2", 3, True)
    alg.set_leaf_cell_healthy("node4", 0, False)
    snaps.append(snapshot(sim))
    third = wave("c", requests[48:])
    alg.set_healthy_node("node3")
    alg.set_bad_node("node2")
    snaps.append(snapshot(sim))
    release(sim, out, list(sim.pods))
    snaps.append(snapshot(sim))
    alg.set_healthy_node("node2")
    alg.set_leaf_cell_healthy("node4", 0, True)
    fourth = wave("d", requests[:16])
    snaps.append(snapshot(sim))
    release(sim, out, third + fourth)
    snaps.append(snapshot(sim))
    return {"decisions": out, "snapshots": snaps}


def xgmi_flap_stream():
    """xGMI links degrade and heal between 2- and 4-GPU gangs: the clean-world
    path, its cache and the dirty fallback."""
    sim = bench.make_sim()
    alg = sim.alg
    out, snaps = [], []
    n = [0]

    def gangs(shapes):
        keys = []
        for vc, prio, cells, members in shapes:
            n[0] += 1
            group = f"x{n[0]}"
            for m in range(sum(p for p, _ in members)):
                key = f"xgmi/{group}-{m}"
                spec = sim.pod_spec(vc=vc, priority=prio, leaf_cells=cells, group=group,
                                    members=members)
                out.append(decision(sim, key, spec))
                if out[-1]["kind"] == "bind":
                    keys.append(key)
        return keys

    alg.set_xgmi_link_healthy("node1", 0, 1, False, 12.0)
    alg.set_xgmi_link_healthy("node2", 2, 3, False, 11.5)
    alg.set_xgmi_link_healthy("node2", 4, 6, False, 10.0)
    snaps.append(snapshot(sim))
    a = gangs([("VC1", 0, 2, [(1, 2)]), ("VC1", 0, 4, [(1, 4)]), ("VC2", 1, 2, [(2, 2)]),
               ("VC3", 0, 4, [(1, 4)]), ("VC1", 1, 1, [(1, 1)]), ("VC2", 0, 4, [(1, 4)]),
               ("VC1", -1, 2, [(1, 2)]), ("VC1", 0, 2, [(2, 2)])])
    snaps.append(snapshot(sim, full=True))
    alg.set_xgmi_link_healthy("node1", 0, 1, True)
    alg.set_xgmi_link_healthy("node3", 5, 7, False, 9.0)
    release(sim, out, a[::2])
    b = gangs([("VC1", 0, 4, [(2, 4)]), ("VC2", 0, 2, [(1, 2)]), ("VC3", 1, 2, [(2, 2)]),
               ("VC1", 0, 8, [(1, 8)]), ("VC2", -1, 4, [(1, 4)]), ("VC1", 2, 2, [(1, 2)])])
    snaps.append(snapshot(sim))
    for node, x, y in (("node2", 2, 3), ("node2", 4, 6), ("node3", 5, 7)):
        alg.set_xgmi_link_healthy(node, x, y, True)
    release(sim, out, b[1::2])
    gangs([("VC1", 0, 4, [(1, 4)]), ("VC2", 0, 2, [(1, 2)])])
    snaps.append(snapshot(sim))
    release(sim, out, list(sim.pods))
    snaps.append(snapshot(sim))
    return {"decisions": out, "snapshots": snaps}


def heterogeneous_stream():
    """Four chains, a pinned cell, leaf types given by name, a type the VC does
    not have and one the cluster does not have; a node of the pinned chain and
    a node of a rack flap in between."""
    sim = SimScheduler(apicfg.init_raw_config(DESIGN))
    alg = sim.alg
    out, snaps = [], [snapshot(sim, full=True)]

    def ask(key, phase=FILTERING, **kw):
        out.append(decision(sim, key, sim.pod_spec(**kw), phase))

    ask("het/pin-a", vc="VC1", leaf_cells=4, pinned_cell_id="VC1-PIN")
    ask("het/pin-b", vc="VC1", leaf_cells=4, pinned_cell_id="VC1-PIN", priority=1)
    ask("het/pin-c", vc="VC1", leaf_cells=2, pinned_cell_id="VC1-PIN")          # waits
    ask("het/pin-opp", vc="VC1", leaf_cells=1, pinned_cell_id="VC1-PIN", priority=-1)  # error
    ask("het/pin-none", vc="VC2", leaf_cells=1, pinned_cell_id="VC1-PIN")       # error
    ask("het/ct1-a", vc="VC2", leaf_cells=2, leaf_cell_type="CT1")
    ask("het/ct1-b", vc="VC2", leaf_cells=1, leaf_cell_type="CT1")
    ask("het/ct1-vc1", vc="VC1", leaf_cells=1, leaf_cell_type="CT1")            # VC lacks it
    ask("het/ct1-opp", vc="VC1", leaf_cells=1, leaf_cell_type="CT1", priority=-1)
    ask("het/nosuch", vc="VC1", leaf_cells=1, leaf_cell_type="H100")            # nobody has it
    ask("het/novc", vc="VC9", leaf_cells=1)
    ask("het/mi-a", vc="VC1", leaf_cells=8, leaf_cell_type="MI355X")
    ask("het/mi-b", vc="VC1", leaf_cells=8)
    ask("het/mi-c", vc="VC1", leaf_cells=8)
    ask("het/mi-d", vc="VC1", leaf_cells=8)                                      # quota spent
    ask("het/mi-e", vc="VC2", leaf_cells=4, leaf_cell_type="MI355X")
    ask("het/mi-f", vc="VC2", leaf_cells=8)
    ask("het/opp-a", vc="VC2", leaf_cells=2, priority=-1)
    ask("het/opp-b", vc="VC1", leaf_cells=4, priority=-1, leaf_cell_type="MI355X")
    snaps.append(snapshot(sim, full=True))
    alg.set_bad_node("n5")
    alg.set_bad_node("n2")
    alg.set_leaf_cell_healthy("c2", 1, False)
    snaps.append(snapshot(sim))
    release(sim, out, ["het/mi-b", "het/mi-e", "het/ct1-a", "het/pin-a"])
    ask("het/mi-g", vc="VC1", leaf_cells=8, priority=2, phase=PREEMPTING)
    ask("het/ct1-c", vc="VC2", leaf_cells=2, leaf_cell_type="CT1")
    ask("het/pin-d", vc="VC1", leaf_cells=4, pinned_cell_id="VC1-PIN", priority=3,
        phase=PREEMPTING)
    ask("het/mi-h", vc="VC2", leaf_cells=8, priority=1, phase=PREEMPTING)
    snaps.append(snapshot(sim))
    alg.set_healthy_node("n5")
    alg.set_healthy_node("n2")
    alg.set_leaf_cell_healthy("c2", 1, True)
    ask("het/mi-i", vc="VC2", leaf_cells=8, priority=1)
    ask("het/ct1-d", vc="VC2", leaf_cells=2, leaf_cell_type="CT1")
    snaps.append(snapshot(sim))
    release(sim, out, list(sim.pods))
    snaps.append(snapshot(sim))
    return {"decisions": out, "snapshots": snaps}


def bench_stream(rounds=30):
    """bench.py's 64 requests with release, round after round, as digests."""
    sim = bench.make_sim()
    requests = bench.build_requests(seed=0, count=64)
    shas, binds, snaps = [], [], []
    for rnd in range(rounds):
        records, bound = [], []
        for i, req in enumerate(requests):
            key = f"bench/p{i}"
            spec = sim.pod_spec(vc=req["vc"], priority=req["priority"], leaf_cells=req["cells"])
            records.append(decision(sim, key, spec))
            if records[-1]["kind"] == "bind":
                bound.append(key)
        if rnd in (0, rounds - 1):
            snaps.append(snapshot(sim))  # loaded
        for key in bound:
            sim.delete_pod(key)
        shas.append(digest(records))
        binds.append(len(bound))
    snaps.append(snapshot(sim))
    return {"decisions": [], "round_sha256": shas, "binds_per_round": binds, "snapshots": snaps}


def record_all():
    return {"health-flaps": health_flap_stream(),
            "xgmi-flaps": xgmi_flap_stream(),
            "heterogeneous": heterogeneous_stream(),
            "bench": bench_stream()}


def check_not_hollow(recorded):
    """The streams reach what they are for, in the golden as in the replay."""
    for name, stream in recorded.items():
        for i, snap in enumerate(stream["snapshots"]):
            assert snap["invariants"] == "ok", (name, i, snap["invariants"])

    flaps = recorded["health-flaps"]
    kinds = {d["kind"] for d in flaps["decisions"]}
    assert {"bind", "preempt", "wait", "release"} <= kinds, kinds
    doomed = [sum(f.get("doomed", 0) for _, _, f in counter_levels(s)) for s in flaps["snapshots"]]
    bad_free = [sum(f.get("badFree", 0) for _, _, f in counter_levels(s))
                for s in flaps["snapshots"]]
    first_doomed = next(i for i, n in enumerate(doomed) if n > 0)
    assert any(n == 0 for n in doomed[first_doomed + 1:]), doomed  # the doom is lifted again
    assert doomed[0] == 0 and doomed[-1] == 0, doomed
    assert max(bad_free) > 0, bad_free

    xgmi = recorded["xgmi-flaps"]
    binds = [d for d in xgmi["decisions"] if d["kind"] == "bind"]
    sizes = {len(d["isolation"]) for d in binds}
    assert {2, 4} <= sizes, sizes
    # while node1's 0<->1 link is degraded no gang is handed both of its ends
    for d in xgmi["decisions"]:
        if d["kind"] == "release":
            break
        if d["kind"] == "bind" and d["node"] == "node1":
            assert not {0, 1} <= set(d["isolation"]), d

    het = recorded["heterogeneous"]
    chains = {c for c, _, _ in counter_levels(het["snapshots"][0])}
    assert len(chains) >= 2, chains
    bound_chains = {d["chain"] for d in het["decisions"] if d["kind"] == "bind"}
    assert len(bound_chains) >= 3, bound_chains
    errors = [d["message"] for d in het["decisions"] if d["kind"] == "error"]
    assert any("which VC VC1 does not have" in m for m in errors), errors
    assert any("which the whole cluster does not have" in m for m in errors), errors
    assert any("does not have pinned cell" in m for m in errors), errors
    pinned = [d for d in het["decisions"] if d["kind"] == "bind" and d["node"] == "n4"]
    assert len(pinned) >= 2, pinned

    bench_rec = recorded["bench"]
    assert len(bench_rec["round_sha256"]) == 30
    assert bench_rec["binds_per_round"] == [16] * 30


@pytest.fixture(scope="module")
def recorded():
    # through JSON, so that what is compared is what a fixture can hold
    return json.loads(json.dumps(record_all()))


def test_golden_replay(recorded):
    check_not_hollow(recorded)
    if os.environ.get("HIVED_CHAIN_STATE_RECORD") == "1":
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
        assert len(got["snapshots"]) == len(want["snapshots"]), name
        for i, (g, w) in enumerate(zip(got["snapshots"], want["snapshots"])):
            for field in w:
                assert g[field] == w[field], (name, "snapshot", i, field)
        for field in want:
            assert got[field] == want[field], (name, field)
