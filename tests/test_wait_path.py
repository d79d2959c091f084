"""The waiting decision's path: a failing decision decides early and reuses its
scratch in the core, `schedule_pod` enters the core through a hand-written
vectorcall method, and `HivedAlgorithm.schedule_pod` is that method itself (no
Python frame, lock or `try` in between). None of it may change an answer.

Golden replay: `tests/golden/wait_path_decisions.json` holds every decision of
a set of seeded request streams as the commit before this change gave them.
To record it again (on a build whose answers are the reference):

    HIVED_WAIT_PATH_RECORD=1 python -m pytest tests/test_wait_path.py -k golden
"""
import copy
import json
import os
import random
import threading

import pytest

import bench
from hivedscheduler_amd import hivedcore
from hivedscheduler_amd.algorithm import FILTERING, PREEMPTING, HivedAlgorithm, ScheduleResult
from hivedscheduler_amd.api.types import (
    AffinityGroupMemberSpec,
    AffinityGroupSpec,
    WebServerError,
)
from hivedscheduler_amd.internal.pod import validate_pod_scheduling_spec
from hivedscheduler_amd.sim import SimScheduler, mi355x_cluster_config

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                      "wait_path_decisions.json")
GIB = 1 << 30

# Every wait-reason text the early exit, the sort and the scratch can touch
# and a caller can see. "... when scheduling in VC <vc>" is not among them: a
# guaranteed request whose intra-VC attempt fails leaves scheduleGuaranteedGroup
# with the mapping text below, which replaces the intra-VC reason. That is how
# the commit before this change answers, so it is what the fixture holds.
MAPPING_BAD = "Mapping the virtual placement would need to use at least one bad node"
MAPPING_BAD_OR_NON_SUGGESTED = ("Mapping the virtual placement would need to use at least one "
                                "bad or non-suggested node")
REASON_TEXTS = [
    "insufficient capacity when scheduling in physical cluster",
    "have to use at least one non-suggested node ",
    " when scheduling in physical cluster",
    MAPPING_BAD,
    MAPPING_BAD_OR_NON_SUGGESTED,
]


def decision(sim, key, spec, suggested=None, phase=FILTERING, commit=True):
    """One sim.schedule as a JSON-able record: kind, node, leaf cells, victim
    node, victim keys, wait reason; or the error it raised."""
    try:
        r = sim.schedule(key, spec, suggested, phase, commit)
    except WebServerError as e:
        return ["error", e.code, e.message]
    info = r.bind_info
    return [r.kind, info.node if info else "", list(info.leafCellIsolation) if info else [],
            r.victim_node, list(r.victim_pod_keys), r.wait_reason]


# ---------------------------------------------------------------------------
# the streams
# ---------------------------------------------------------------------------


def bench_stream():
    """bench.py's own stream on config 4, three steps."""
    sim = bench.make_sim()
    requests = bench.build_requests(seed=0, count=64)
    out = []
    for _ in range(3):
        bound = []
        for i, req in enumerate(requests):
            key = f"bench/p{i}"
            spec = sim.pod_spec(vc=req["vc"], priority=req["priority"], leaf_cells=req["cells"])
            out.append(decision(sim, key, spec))
            if out[-1][0] == "bind":
                bound.append(key)
        for key in bound:
            sim.delete_pod(key)
    sim.assert_empty()
    return out


GANGS = [[(2, 2)], [(1, 4), (2, 1)], [(2, 8)], [(3, 4)], [(2, 4)], [(1, 8), (1, 4)]]


def hbm_design_config(design_config):
    """design_config with measured HBM on node n7: GPU 0 reports half."""
    cfg = copy.deepcopy(design_config)

    def visit(cell, node):
        node = cell.cellAddress if cell.cellType == "MI355X-NODE" else node
        if cell.cellType == "MI355X" and node is not None and node.endswith("n7"):
            cell.hbmBytes = (144 if cell.cellAddress.endswith("/0") or cell.cellAddress == "0"
                             else 288) * GIB
        for child in cell.cellChildren:
            visit(child, node)

    for top in cfg.physicalCluster.physicalCells:
        visit(top, None)
    return cfg


def design_stream(design_config, seed, ops=300):
    """Mixed schedule / delete operations on the heterogeneous design cluster:
    gangs, the pinned cell, leafCellType, partial suggested lists, a bad node,
    a bad leaf, an HBM demand and one degraded xGMI link."""
    rng = random.Random(seed)
    sim = SimScheduler(hbm_design_config(design_config))
    nodes = sorted(sim.alg.all_nodes())
    pending = []  # (key, params): asked, not bound
    serial = 0
    out = []

    def new_requests():
        nonlocal serial
        serial += 1
        common = dict(vc=rng.choice(["VC1", "VC1", "VC2"]), priority=rng.choice([-1, 0, 0, 1, 2]),
                      ignore_suggested=rng.random() < 0.55)
        roll = rng.random()
        if roll < 0.10:
            common.update(vc="VC1", pinned_cell_id="VC1-PIN", priority=max(0, common["priority"]))
        elif roll < 0.22:
            common["leaf_cell_type"] = rng.choice(["MI355X", "CT1", "CT1"])
        elif roll < 0.32:
            common["hbm_bytes_per_cell"] = 200 * GIB
        if common.get("leaf_cell_type") == "CT1":
            return [(f"ns/c{serial}", dict(common, leaf_cells=rng.choice([1, 2])))]
        if rng.random() < 0.55:
            return [(f"ns/s{serial}", dict(common, leaf_cells=rng.choice([1, 2, 4, 8, 8])))]
        members = rng.choice(GANGS)
        group = f"gang{serial}"
        pods = [(f"ns/{group}-{cells}-{i}", dict(common, leaf_cells=cells, group=group,
                                                 members=members))
                for pod_number, cells in members for i in range(pod_number)]
        rng.shuffle(pods)
        return pods

    def suggested_nodes():
        pick = rng.random()
        if pick < 0.25:
            return None
        if pick < 0.45:
            return nodes
        return rng.sample(nodes, rng.choice([1, 2, 4, 6]))

    events = {
        ops // 10: lambda: sim.alg.set_xgmi_link_healthy(nodes[0], 0, 1, False, 12.0),
        ops // 5: lambda: sim.alg.set_bad_node(nodes[1]),
        ops // 3: lambda: sim.alg.set_leaf_cell_healthy(nodes[5], 3, False),
        (2 * ops) // 3: lambda: sim.alg.set_healthy_node(nodes[1]),
    }
    for op in range(ops):
        if op in events:
            events[op]()
        roll = rng.random()
        if roll < 0.12 and sim.pods:
            sim.delete_pod(rng.choice(sorted(sim.pods)))
        elif roll < 0.16 and pending:
            key, params = pending.pop(rng.randrange(len(pending)))
            sim.delete_unallocated(key, sim.pod_spec(**params))
        else:
            if pending and rng.random() < 0.45:
                key, params = pending.pop(rng.randrange(len(pending)))
            else:
                first, *rest = new_requests()
                pending.extend(rest)
                key, params = first
            phase = PREEMPTING if rng.random() < 0.35 else FILTERING
            record = decision(sim, key, sim.pod_spec(**params), suggested_nodes(), phase)
            out.append(record)
            if record[0] in ("wait", "preempt"):
                pending.append((key, params))
            if record[0] == "preempt" and rng.random() < 0.6:
                for victim in record[4]:  # the cluster's part: evict the victims
                    if victim in sim.pods:
                        sim.delete_pod(victim)
        if (op + 1) % 50 == 0:
            sim.alg._core.check_invariants()
    sim.alg._core.check_invariants()
    return out


ONE_VC = {"VC1": [("MI355X-NODE", 2)]}


def two_nodes_with_three_free_each():
    """Two nodes of one VC, five GPUs taken on each (a 4 and a 1)."""
    sim = SimScheduler(mi355x_cluster_config(num_nodes=2, vcs=ONE_VC))
    for node in ("node1", "node2"):
        for cells in (4, 1):
            spec = sim.pod_spec(leaf_cells=cells, ignore_suggested=False)
            assert sim.schedule(f"ns/fill-{node}-{cells}", spec, [node]).kind == "bind"
    return sim


def shape_cases():
    """The smallest shapes around the early exit; name -> list of decisions."""
    cases = {}

    # a single pod of 8 with one leaf taken: no node can host it
    for priority in (0, -1):
        sim = SimScheduler(mi355x_cluster_config(num_nodes=1))
        taken = [decision(sim, "ns/one", sim.pod_spec(leaf_cells=1, priority=priority))]
        cases[f"single pod of 8, one leaf taken, priority {priority}"] = taken + [
            decision(sim, "ns/eight", sim.pod_spec(leaf_cells=8, priority=priority))]

    # 2 pods x 4 leaves against 7 free leaves: the demand exceeds the sum
    for priority in (0, -1):
        sim = SimScheduler(mi355x_cluster_config(num_nodes=1))
        taken = [decision(sim, "ns/one", sim.pod_spec(leaf_cells=1, priority=priority))]
        gang = sim.pod_spec(leaf_cells=4, priority=priority, group="g", members=[(2, 4)])
        cases[f"gang 2x4 against 7 free, priority {priority}"] = taken + [
            decision(sim, "ns/g-0", gang)]

    # the demand fits the sum but not the nodes (3 + 3 free, pods of 4 and 2):
    # the greedy loop decides
    sim = two_nodes_with_three_free_each()
    gang = sim.pod_spec(leaf_cells=4, group="g", members=[(1, 4), (1, 2)])
    cases["gang 4+2 against 3+3 free"] = [decision(sim, "ns/g-4", gang)]
    gang = sim.pod_spec(leaf_cells=4, priority=-1, group="h", members=[(1, 4), (1, 2)])
    cases["gang 4+2 against 3+3 free, opportunistic"] = [decision(sim, "ns/h-4", gang)]

    # a non-suggested node with room is met: the reason names its address
    for priority in (0, -1):
        for suggested in (["node1"], ["node2"]):
            sim = two_nodes_with_three_free_each()
            gang = sim.pod_spec(leaf_cells=3, priority=priority, group="g", members=[(2, 3)],
                                ignore_suggested=False)
            cases[f"gang 2x3 against 3+3 free, only {suggested[0]} suggested, "
                  f"priority {priority}"] = [decision(sim, "ns/g-0", gang, suggested)]
            # ... and the same gang binds once both nodes are suggested
            cases[f"gang 2x3 against 3+3 free, both suggested after {suggested[0]}, "
                  f"priority {priority}"] = [
                decision(sim, "ns/g-0", gang, ["node1", "node2"], commit=False)]

    # waits at opportunistic priority, preempts at its own
    sim = SimScheduler(mi355x_cluster_config(num_nodes=1))
    records = [decision(sim, f"ns/opp{i}", sim.pod_spec(leaf_cells=4, priority=-1))
               for i in range(2)]
    records.append(decision(sim, "ns/opp-more", sim.pod_spec(leaf_cells=1, priority=-1)))
    records.append(decision(sim, "ns/own", sim.pod_spec(leaf_cells=4, priority=1)))
    records.append(decision(sim, "ns/own", sim.pod_spec(leaf_cells=8, priority=1),
                            phase=PREEMPTING, commit=False))
    cases["waits opportunistically, preempts at its own priority"] = records

    # two different requests back to back: the scratch carries nothing over
    sim = two_nodes_with_three_free_each()
    big = sim.pod_spec(leaf_cells=2, group="big", members=[(4, 2)])
    records = []
    for _ in range(2):
        records.append(decision(sim, "ns/big-0", big, commit=False))
        records.append(decision(sim, "ns/small", sim.pod_spec(leaf_cells=1), commit=False))
        records.append(decision(sim, "ns/eight", sim.pod_spec(leaf_cells=8), commit=False))
        records.append(decision(sim, "ns/three", sim.pod_spec(leaf_cells=3, group="t",
                                                              members=[(2, 3)]), commit=False))
        records.append(decision(sim, "ns/opp", sim.pod_spec(leaf_cells=4, priority=-1),
                                commit=False))
    cases["different requests back to back"] = records
    return cases


def record_all(design_config):
    return {
        "bench": bench_stream(),
        "design-1": design_stream(design_config, 1),
        "design-2": design_stream(design_config, 2),
        "shapes": shape_cases(),
    }


def all_decisions(recorded):
    out = list(recorded["bench"]) + list(recorded["design-1"]) + list(recorded["design-2"])
    for records in recorded["shapes"].values():
        out.extend(records)
    return out


def check_not_hollow(recorded):
    decisions = all_decisions(recorded)
    waits = [d for d in decisions if d[0] == "wait"]
    assert len(waits) * 3 >= len(decisions), (len(waits), len(decisions))
    for name in ("bench", "design-1", "design-2"):
        kinds = {d[0] for d in recorded[name]}
        assert {"bind", "wait", "preempt"} <= kinds, (name, kinds)
    assert {"error"} <= {d[0] for d in recorded["design-1"] + recorded["design-2"]}
    for text in REASON_TEXTS:
        assert any(text in d[5] for d in waits), text
    assert not any(" when scheduling in VC " in d[5] for d in waits)


@pytest.fixture(scope="module")
def recorded(design_config):
    return record_all(design_config)


def test_golden_replay(recorded):
    check_not_hollow(recorded)
    if os.environ.get("HIVED_WAIT_PATH_RECORD") == "1":
        os.makedirs(os.path.dirname(GOLDEN), exist_ok=True)
        with open(GOLDEN, "w") as f:
            json.dump(recorded, f, separators=(",", ":"), sort_keys=True)
            f.write("\n")
    with open(GOLDEN) as f:
        golden = json.load(f)
    check_not_hollow(golden)
    assert sorted(recorded) == sorted(golden)
    for name in ("bench", "design-1", "design-2"):
        assert len(recorded[name]) == len(golden[name]), name
        for i, (got, want) in enumerate(zip(recorded[name], golden[name])):
            assert got == want, (name, i)
    assert sorted(recorded["shapes"]) == sorted(golden["shapes"])
    for name, want in golden["shapes"].items():
        assert recorded["shapes"][name] == want, name


# ---------------------------------------------------------------------------
# the smallest shapes around the early exit
# ---------------------------------------------------------------------------


def test_shapes_around_the_early_exit(recorded):
    cases = recorded["shapes"]

    def last(name):
        return cases[name][-1]

    opportunistic = "insufficient capacity when scheduling in physical cluster"
    for priority, reason in ((0, MAPPING_BAD), (-1, opportunistic)):
        assert last(f"single pod of 8, one leaf taken, priority {priority}")[0::5] == ["wait", reason]
        assert last(f"gang 2x4 against 7 free, priority {priority}")[0::5] == ["wait", reason]
    assert last("gang 4+2 against 3+3 free")[0::5] == ["wait", MAPPING_BAD]
    assert last("gang 4+2 against 3+3 free, opportunistic")[0::5] == ["wait", opportunistic]
    for suggested, other in (("node1", "node2"), ("node2", "node1")):
        # the physical view names the node; the address is the one recorded
        # on the commit before this change (test_golden_replay compares it)
        got = last(f"gang 2x3 against 3+3 free, only {suggested} suggested, priority -1")
        assert got[0::5] == ["wait", f"have to use at least one non-suggested node {other} "
                                     "when scheduling in physical cluster"]
        got = last(f"gang 2x3 against 3+3 free, only {suggested} suggested, priority 0")
        assert got[0::5] == ["wait", MAPPING_BAD_OR_NON_SUGGESTED]
        for priority in (0, -1):
            assert last(f"gang 2x3 against 3+3 free, both suggested after {suggested}, "
                        f"priority {priority}")[0] == "bind"
    own = cases["waits opportunistically, preempts at its own priority"]
    assert [d[0] for d in own] == ["bind", "bind", "wait", "preempt", "preempt"]
    assert own[3][4] != [] and own[4][4] != []
    back = cases["different requests back to back"]
    assert back[:5] == back[5:]
    assert [d[0] for d in back[:5]] == ["wait", "bind", "wait", "bind", "wait"]


def test_reused_scratch_gives_what_a_fresh_core_gives():
    """Each request of a mixed sequence on one core against the same request
    as the first call on a core of its own."""
    def requests(sim):
        return [
            ("ns/big-0", sim.pod_spec(leaf_cells=2, group="big", members=[(4, 2)])),
            ("ns/one", sim.pod_spec(leaf_cells=1)),
            ("ns/gang-4", sim.pod_spec(leaf_cells=4, group="gang", members=[(1, 4), (1, 2)])),
            ("ns/opp", sim.pod_spec(leaf_cells=2, priority=-1, group="o", members=[(3, 2)])),
            ("ns/eight", sim.pod_spec(leaf_cells=8)),
            ("ns/pair", sim.pod_spec(leaf_cells=2, priority=2)),
        ]

    shared = two_nodes_with_three_free_each()
    for i in range(len(requests(shared))):
        key, spec = requests(shared)[i]
        fresh = two_nodes_with_three_free_each()
        assert decision(shared, key, spec, commit=False) == \
            decision(fresh, *requests(fresh)[i], commit=False), key
    assert shared.alg.get_all_affinity_groups() == \
        two_nodes_with_three_free_each().alg.get_all_affinity_groups()


# ---------------------------------------------------------------------------
# the direct entry
# ---------------------------------------------------------------------------


def twin_sim():
    return SimScheduler(mi355x_cluster_config(
        num_nodes=2, vcs={"VC1": [("MI355X-NODE", 1)], "VC2": [("MI355X-NODE.MI355X-QUAD", 1)]}))


def test_positional_keyword_and_default_calls_agree():
    sims = [twin_sim() for _ in range(6)]
    nodes = sims[0].alg.all_nodes()

    def spec():
        return SimScheduler.pod_spec(leaf_cells=2)

    results = [
        sims[0].alg.schedule_pod(spec(), "ns/p"),
        sims[1].alg.schedule_pod(spec(), "ns/p", None, FILTERING, False),
        sims[2].alg.schedule_pod(spec(), pod_key="ns/p", suggested_nodes=nodes, phase=FILTERING,
                                 commit=False),
        sims[3].alg.schedule_pod(spec=spec(), pod_key="ns/p", commit=False),
        sims[4].alg._core.schedule_pod(commit=False, phase=FILTERING, pod_key="ns/p",
                                       pod_spec=spec(), suggested_nodes=None, validate=True),
        sims[5].alg._core.schedule_pod(spec(), "ns/p", None, FILTERING, False, True),
    ]
    for sim, r in zip(sims, results):
        assert type(r) is ScheduleResult and r.kind == "bind"
        assert r.bind_info == results[0].bind_info
        assert sim.alg.get_all_affinity_groups() == []  # commit defaults to False
    # commit by position and by keyword
    assert sims[0].alg.schedule_pod(spec(), "ns/p", None, FILTERING, True).kind == "bind"
    assert sims[1].alg.schedule_pod(spec(), "ns/p", commit=True).kind == "bind"
    assert sims[0].alg.get_all_affinity_groups() == sims[1].alg.get_all_affinity_groups() != []
    # the phase is read: a preempting group exists only after a Preempting call
    sim = twin_sim()
    for i in range(2):
        assert sim.schedule(f"ns/o{i}", sim.pod_spec(leaf_cells=8, priority=-1)).kind == "bind"
    want = sim.pod_spec(vc="VC2", leaf_cells=4, priority=1)
    assert sim.alg.schedule_pod(want, "ns/w", None, FILTERING).kind == "preempt"
    assert len(sim.alg.get_all_affinity_groups()) == 2
    assert sim.alg.schedule_pod(want, "ns/w", phase=PREEMPTING).kind == "preempt"
    assert len(sim.alg.get_all_affinity_groups()) == 3
    # validate stays a core-only argument, off only on request
    core = sim.alg._core
    bad = SimScheduler.pod_spec(leaf_cells=0)
    with pytest.raises(hivedcore.CoreError):
        core.schedule_pod(bad, "ns/bad")
    assert core.schedule_pod(SimScheduler.pod_spec(priority=5000), "ns/q", validate=False).kind in (
        "bind", "wait", "preempt")


TYPE_ERRORS = {
    "str for nodes": (lambda s: (s.pod_spec(), "ns/p", "node1"),
                      "suggested_nodes must be a sequence of node names, not str"),
    "int for nodes": (lambda s: (s.pod_spec(), "ns/p", 7),
                      "suggested_nodes must be a sequence of node names, not int"),
    "int in nodes": (lambda s: (s.pod_spec(ignore_suggested=False), "ns/p", ["node1", 7]),
                     "suggested_nodes must contain node names (str)"),
    "key": (lambda s: (s.pod_spec(), 7), "pod_key must be a str"),
    "phase": (lambda s: (s.pod_spec(), "ns/p", None, 7), "phase must be a str"),
    "dict spec": (lambda s: ({"virtualCluster": "VC1", "leafCellNumber": 1}, "ns/p"),
                  "schedule_pod validates a PodSchedulingSpec object, not a dict"),
}


@pytest.mark.parametrize("case", sorted(TYPE_ERRORS))
def test_type_errors_keep_their_text(case):
    args, text = TYPE_ERRORS[case]
    sim = twin_sim()
    for call in (sim.alg.schedule_pod, sim.alg._core.schedule_pod):
        with pytest.raises(TypeError) as e:
            call(*args(sim))
        assert str(e.value) == text
    if case in ("str for nodes", "phase"):  # ... and through the harness
        with pytest.raises(TypeError) as e:
            sim.schedule("ns/p", sim.pod_spec(), "node1" if case == "str for nodes" else None,
                         7 if case == "phase" else FILTERING)
        assert str(e.value) == text
    assert sim.alg.schedule_count() == 0


def test_argument_count_and_names_are_checked():
    sim = twin_sim()
    for call in (sim.alg.schedule_pod, sim.alg._core.schedule_pod):
        with pytest.raises(TypeError):
            call()
        with pytest.raises(TypeError):
            call(sim.pod_spec())
        with pytest.raises(TypeError):
            call(sim.pod_spec(), "ns/p", None, FILTERING, False, True, 1)
        with pytest.raises(TypeError):
            call(sim.pod_spec(), "ns/p", pod_key="ns/p")
        with pytest.raises(TypeError):
            call(sim.pod_spec(), "ns/p", no_such_argument=1)
    assert sim.alg.schedule_count() == 0


def test_dict_specs_still_work_without_validation():
    core = twin_sim().alg._core
    raw = {"virtualCluster": "VC1", "priority": 0, "leafCellNumber": 2,
           "affinityGroup": {"name": "g", "members": [{"podNumber": 1, "leafCellNumber": 2}]}}
    r = core.schedule_pod(raw, "ns/p", None, FILTERING, True, False)
    assert r.kind == "bind"
    assert [g["name"] for g in core.get_all_affinity_groups()] == ["g"]


def test_errors_arrive_as_web_server_errors_with_their_cause():
    sim = twin_sim()
    # a 400 from validation
    with pytest.raises(WebServerError) as e:
        sim.alg.schedule_pod(sim.pod_spec(vc=""), "ns/bad")
    assert (e.value.code, e.value.message) == (400, "VirtualCluster is empty")
    assert type(e.value.__cause__) is hivedcore.CoreError
    assert e.value.__cause__.code == 400 and str(e.value.__cause__) == "VirtualCluster is empty"
    with pytest.raises(WebServerError) as expected:
        validate_pod_scheduling_spec(sim.pod_spec(vc=""), "ns/bad")
    assert str(e.value) == str(expected.value) and e.value.args == expected.value.args
    # a BadRequest from the core
    with pytest.raises(WebServerError) as e:
        sim.alg.schedule_pod(sim.pod_spec(vc="NOPE"), "ns/bad")
    assert (e.value.code, e.value.message) == (400, "[ns/bad]: VC NOPE does not exist!")
    assert type(e.value.__cause__) is hivedcore.CoreError
    assert str(e.value.__cause__) == e.value.message and e.value.__cause__.code == 400
    # the decide-only method and the core itself are what they were
    with pytest.raises(WebServerError) as e:
        sim.alg.schedule(sim.pod_spec(vc="NOPE", group="g"), "ns/bad", [])
    assert (e.value.code, e.value.message) == (400, "[ns/bad]: VC NOPE does not exist!")
    with pytest.raises(hivedcore.CoreError) as e:
        sim.alg._core.schedule_pod(sim.pod_spec(vc="NOPE"), "ns/bad")
    assert e.value.code == 400 and e.value.__cause__ is None
    assert sim.alg.schedule_count() == 3
    assert sim.alg.get_all_affinity_groups() == []
    assert sim.schedule("ns/after", sim.pod_spec(leaf_cells=2)).kind == "bind"


def test_absent_group_is_defaulted_on_the_spec():
    sim = twin_sim()
    key = "ns/some-pod"
    spec = sim.pod_spec(leaf_cells=2)
    expected = copy.deepcopy(spec)
    validate_pod_scheduling_spec(expected, key)
    assert sim.alg.schedule_pod(spec, key).kind == "bind"
    assert spec == expected
    assert type(spec.affinityGroup) is AffinityGroupSpec
    assert type(spec.affinityGroup.members[0]) is AffinityGroupMemberSpec
    assert spec.affinityGroup.name is key
    given = sim.pod_spec(leaf_cells=2, group="g", members=[(2, 2)])
    group = given.affinityGroup
    assert sim.alg.schedule_pod(given, "ns/g-0").kind == "bind"
    assert given.affinityGroup is group


# ---------------------------------------------------------------------------
# threads
# ---------------------------------------------------------------------------


def test_threads_commit_and_delete_without_the_lock():
    alg = HivedAlgorithm(mi355x_cluster_config(num_nodes=4))
    for n in alg.all_nodes():
        alg.set_healthy_node(n)
    errors = []
    start = threading.Barrier(8)

    def worker(t):
        try:
            start.wait()
            for i in range(300):
                key = f"ns/t{t}-{i}"
                spec = SimScheduler.pod_spec(leaf_cells=(1, 2, 4, 8)[(t + i) % 4],
                                             priority=(0, -1, 1)[i % 3])
                r = alg.schedule_pod(spec, key, None, FILTERING, True)
                if r.kind == "bind":
                    alg.delete_allocated_pod(spec, r.bind_info, key)
                elif r.kind == "wait":
                    assert r.wait_reason
        except BaseException as e:  # noqa: BLE001 - reported by the main thread
            errors.append(e)

    threads = [threading.Thread(target=worker, args=(t,)) for t in range(8)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert errors == []
    alg._core.check_invariants()
    assert alg.get_all_affinity_groups() == []
    assert alg.schedule_count() == 8 * 300
