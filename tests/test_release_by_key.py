"""A pod released by its key leaves the core exactly where releasing it by spec
and bind info leaves it.

Two SimSchedulers get the same seeded stream of operations. One releases
through SimScheduler.delete_pod (by key, the spec / info form only for a key
the core does not know), the other by spec and bind info as before. After
every operation both report the same cluster status, affinity groups and
safety counters, and both pass the invariant check.
"""
import random
import threading

import pytest

from hivedscheduler_amd import hivedcore
from hivedscheduler_amd.algorithm import FILTERING, PREEMPTING, HivedAlgorithm
from hivedscheduler_amd.api.types import WebServerError
from hivedscheduler_amd.sim import SimScheduler, mi355x_cluster_config

VCS = {
    "VC1": [("MI355X-NODE", 2)],
    "VC2": [("MI355X-NODE", 1), ("MI355X-NODE.MI355X-QUAD", 1)],
}


class BySpecScheduler(SimScheduler):
    """SimScheduler as it released pods before the release by key."""

    def delete_pod(self, key):
        spec, info = self.pods.pop(key)
        self.alg.delete_allocated_pod(spec, info, key)


def twins(num_nodes=4, vcs=VCS):
    config = mi355x_cluster_config(num_nodes=num_nodes, vcs=vcs)
    return SimScheduler(config), BySpecScheduler(config)


def state(sim):
    core = sim.alg._core
    core.check_invariants()
    return (sim.alg.get_cluster_status(), sim.alg.get_all_affinity_groups(), core.debug_counters())


def assert_same(by_key, by_spec, what=""):
    got, want = state(by_key), state(by_spec)
    assert got[1] == want[1], what
    assert got[2] == want[2], what
    assert got[0] == want[0], what
    assert sorted(by_key.pods) == sorted(by_spec.pods), what


def both(by_key, by_spec, op, what=""):
    """Run op(sim) on both and compare what it gave and the state after it."""
    a, b = op(by_key), op(by_spec)
    assert a == b, what
    assert_same(by_key, by_spec, what)
    return a


def schedule(key, phase=FILTERING, **params):
    def op(sim):
        r = sim.schedule(key, sim.pod_spec(**params), None, phase)
        info = r.bind_info
        return (r.kind, info.to_dict() if info else None, r.victim_node, list(r.victim_pod_keys),
                r.wait_reason)
    return op


def release(key):
    return lambda sim: sim.delete_pod(key)


def release_victims(victims):
    def op(sim):
        for victim in victims:
            if victim in sim.pods:
                sim.delete_pod(victim)
    return op


# ---------------------------------------------------------------------------
# the seeded stream
# ---------------------------------------------------------------------------


def test_seeded_stream_leaves_both_cores_in_the_same_state():
    """1/2/4/8-cell pods, a 2x4 gang released pod by pod, guaranteed requests
    that preempt opportunistic pods (with the victims' release), bad-node
    flaps, and lazy preemption."""
    by_key, by_spec = twins()
    rng = random.Random(21)
    nodes = sorted(by_key.alg.all_nodes())
    serial = 0
    seen = {"bind": 0, "preempt": 0, "wait": 0, "released": 0, "gang-released": 0, "flaps": 0,
            "lazy": 0}
    gangs = []  # keys of bound 2x4 gang pods, released one by one
    for op in range(260):
        roll = rng.random()
        what = f"op {op}"
        if roll < 0.05:
            node = rng.choice(nodes)
            bad = node in by_key.alg.bad_nodes()
            both(by_key, by_spec,
                 lambda sim: sim.alg.set_healthy_node(node) if bad else sim.alg.set_bad_node(node),
                 what)
            seen["flaps"] += 1
        elif roll < 0.30 and by_key.pods:
            key = rng.choice(sorted(by_key.pods))
            both(by_key, by_spec, release(key), what)
            seen["released"] += 1
            seen["gang-released"] += key in gangs
        elif roll < 0.40:
            serial += 1
            group = f"gang{serial}"
            for i in range(2):
                key = f"ns/{group}-{i}"
                r = both(by_key, by_spec,
                         schedule(key, vc="VC1", priority=rng.choice([0, 1]), leaf_cells=4,
                                  group=group, members=[(2, 4)]), what)
                seen[r[0]] += 1
                if r[0] == "bind":
                    gangs.append(key)
        else:
            serial += 1
            key = f"ns/p{serial}"
            params = dict(vc=rng.choice(["VC1", "VC1", "VC2"]), priority=rng.choice([-1, -1, 0, 1, 2]),
                          leaf_cells=rng.choice([1, 2, 4, 8]),
                          lazy_preemption=rng.random() < 0.4)
            phase = PREEMPTING if rng.random() < 0.4 else FILTERING
            r = both(by_key, by_spec, schedule(key, phase, **params), what)
            seen[r[0]] += 1
            if r[0] == "preempt":
                both(by_key, by_spec, release_victims(r[3]), what)
                r = both(by_key, by_spec, schedule(key, phase, **params), what)
                seen[r[0]] += 1
        seen["lazy"] += any(g["lazyPreemptionStatus"] is not None
                            for g in by_key.alg.get_all_affinity_groups())
    assert all(n > 0 for n in seen.values()), seen
    # drain: every pod goes, by key on one side and by spec on the other
    for key in sorted(by_key.pods):
        both(by_key, by_spec, release(key), f"drain {key}")
    assert by_key.pods == {}


# ---------------------------------------------------------------------------
# the smallest shapes that can go wrong
# ---------------------------------------------------------------------------


def gang_of_two(by_key, by_spec):
    for i in range(2):
        r = both(by_key, by_spec, schedule(f"ns/g-{i}", leaf_cells=4, group="g", members=[(2, 4)]))
        assert r[0] == "bind"


@pytest.mark.parametrize("first", [0, 1])
def test_gang_first_pod_keeps_the_group_and_last_pod_ends_it(first):
    by_key, by_spec = twins()
    gang_of_two(by_key, by_spec)
    both(by_key, by_spec, release(f"ns/g-{first}"))
    groups = by_key.alg.get_all_affinity_groups()
    assert [g["name"] for g in groups] == ["g"]
    assert groups[0]["allocatedPods"] == [f"ns/g-{1 - first}"]
    both(by_key, by_spec, release(f"ns/g-{1 - first}"))
    by_key.assert_empty()


def test_a_key_released_twice_or_never_added_is_unknown_and_changes_nothing():
    by_key, by_spec = twins()
    gang_of_two(by_key, by_spec)
    alg = by_key.alg
    assert alg.delete_allocated_pod_by_key("ns/never-added") is False
    assert_same(by_key, by_spec)
    assert alg.delete_allocated_pod_by_key("ns/g-0") is True
    by_key.pods.pop("ns/g-0")
    by_spec.delete_pod("ns/g-0")
    assert_same(by_key, by_spec)
    before = state(by_key)
    assert alg.delete_allocated_pod_by_key("ns/g-0") is False
    assert state(by_key) == before
    # the group's name is not a pod key, and a key of a group that is gone is none
    assert alg.delete_allocated_pod_by_key("g") is False
    both(by_key, by_spec, release("ns/g-1"))
    assert alg.delete_allocated_pod_by_key("ns/g-1") is False
    by_key.assert_empty()


def test_a_key_added_twice_is_released_once():
    by_key, by_spec = twins()
    r = both(by_key, by_spec, schedule("ns/p", leaf_cells=2))
    assert r[0] == "bind"
    for sim in (by_key, by_spec):  # the informer's add after the optimistic commit
        sim.alg.add_allocated_pod(*sim.pods["ns/p"], "ns/p")
    assert_same(by_key, by_spec)
    both(by_key, by_spec, release("ns/p"))
    assert by_key.alg.delete_allocated_pod_by_key("ns/p") is False
    by_key.assert_empty()


def test_a_pod_the_core_never_saw_committed_falls_back_to_spec_and_info():
    """What a restart looks like to the caller: the pod is in its books, the
    core answers "unknown" until the replay adds the pod."""
    by_key, by_spec = twins()
    r = both(by_key, by_spec, schedule("ns/p", leaf_cells=2))
    spec, info = by_key.pods["ns/p"]
    restarted = SimScheduler(by_key.config)
    restarted.pods["ns/p"] = (spec, info)
    restarted.delete_pod("ns/p")  # unknown key, nothing to release: no error
    restarted.assert_empty()
    restarted.alg.add_allocated_pod(spec, info, "ns/p")  # the replay
    restarted.pods["ns/p"] = (spec, info)
    assert restarted.alg.get_all_affinity_groups() == by_key.alg.get_all_affinity_groups()
    restarted.delete_pod("ns/p")
    restarted.assert_empty()
    assert restarted.alg.delete_allocated_pod_by_key("ns/p") is False
    assert r[0] == "bind"


def test_release_after_the_group_was_lazy_preempted():
    by_key, by_spec = twins(num_nodes=1, vcs={"VC1": [("MI355X-NODE.MI355X-QUAD", 1)],
                                              "VC2": [("MI355X-NODE.MI355X-QUAD", 1)]})
    r = both(by_key, by_spec, schedule("ns/lazy", vc="VC1", priority=1, leaf_cells=4, group="lazy",
                                       lazy_preemption=True))
    assert r[0] == "bind"
    r = both(by_key, by_spec, schedule("ns/g", vc="VC1", priority=2, leaf_cells=4, group="g"))
    groups = {g["name"]: g for g in by_key.alg.get_all_affinity_groups()}
    assert groups["lazy"]["lazyPreemptionStatus"] is not None, (r, groups)
    both(by_key, by_spec, release("ns/lazy"))
    assert [g["name"] for g in by_key.alg.get_all_affinity_groups()] == ["g"]
    both(by_key, by_spec, release("ns/g"))
    by_key.assert_empty()


def test_release_of_a_group_that_is_being_preempted():
    by_key, by_spec = twins(num_nodes=1, vcs={"VC1": [("MI355X-NODE", 1)]})
    for i in range(2):
        assert both(by_key, by_spec, schedule(f"ns/opp{i}", priority=-1, leaf_cells=4))[0] == "bind"
    r = both(by_key, by_spec, schedule("ns/own", PREEMPTING, priority=1, leaf_cells=8))
    assert r[0] == "preempt" and sorted(r[3]) == ["ns/opp0", "ns/opp1"]
    states = {g["name"]: g["state"] for g in by_key.alg.get_all_affinity_groups()}
    assert states == {"ns/opp0": "BeingPreempted", "ns/opp1": "BeingPreempted", "ns/own": "Preempting"}
    both(by_key, by_spec, release_victims(r[3]))
    assert both(by_key, by_spec, schedule("ns/own", priority=1, leaf_cells=8))[0] == "bind"
    both(by_key, by_spec, release("ns/own"))
    by_key.assert_empty()


# ---------------------------------------------------------------------------
# the entry itself
# ---------------------------------------------------------------------------


def test_arguments_and_errors_of_the_entry():
    sim, _ = twins()
    core = sim.alg._core
    assert sim.schedule("ns/p", sim.pod_spec(leaf_cells=1)).kind == "bind"
    for call in (core.delete_allocated_pod_by_key, core.delete_validated_pod_by_key,
                 sim.alg.delete_allocated_pod_by_key):
        with pytest.raises(TypeError, match="pod_key must be a str"):
            call(7)
        with pytest.raises(TypeError, match="exactly one argument"):
            call()
        with pytest.raises(TypeError, match="exactly one argument"):
            call("ns/p", "ns/q")
        with pytest.raises(TypeError, match="unexpected keyword argument 'key'"):
            call(key="ns/p")
    assert [g["name"] for g in sim.alg.get_all_affinity_groups()] == ["ns/p"]
    assert core.delete_allocated_pod_by_key(pod_key="ns/p") is True
    sim.assert_empty()
    with pytest.raises(TypeError):
        hivedcore.HivedCore.delete_allocated_pod_by_key(object(), "ns/p")
    # the three-argument form is still there and still takes objects and dicts
    spec = sim.pod_spec(leaf_cells=1)
    r = sim.alg.schedule_pod(spec, "ns/q", None, FILTERING, True)
    sim.alg.delete_allocated_pod(spec.to_dict(), r.bind_info.to_dict(), "ns/q")
    sim.assert_empty()
    assert core.delete_allocated_pod_by_key("ns/q") is False
    with pytest.raises(WebServerError):
        sim.alg.schedule_pod(sim.pod_spec(vc="NOPE"), "ns/bad")


def test_threads_commit_and_release_by_key_without_the_lock():
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
                    assert alg.delete_allocated_pod_by_key(key) is True
                    assert alg.delete_allocated_pod_by_key(key) is False
                elif r.kind == "wait":
                    assert r.wait_reason
                    assert alg.delete_allocated_pod_by_key(key) is False
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
