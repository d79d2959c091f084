"""The core reads a plain PodSchedulingSpec straight from its instance dict.
Whatever the form of a request, the answer is the one getattr would lead to.

The same seeded requests go to four cores in step, each in one form:

  plain     a PodSchedulingSpec (fields read from the instance dict)
  property  a subclass whose priority and affinityGroup are properties; the
            instance dict holds decoys under those names, which getattr never
            sees (a data descriptor outranks the instance dict)
  deleted   a PodSchedulingSpec with the fields that are at their class default
            deleted from the instance dict (the class default must be read)
  dict      the validated spec's wire-format dict, with validate=False
"""
import copy
import random

import pytest

from hivedscheduler_amd.algorithm import FILTERING, PREEMPTING
from hivedscheduler_amd.api.types import (
    AffinityGroupMemberSpec,
    AffinityGroupSpec,
    PodSchedulingSpec,
    WebServerError,
)
from hivedscheduler_amd.internal.pod import validate_pod_scheduling_spec
from hivedscheduler_amd.sim import SimScheduler, mi355x_cluster_config

VCS = {
    "VC1": [("MI355X-NODE", 2)],
    "VC2": [("MI355X-NODE", 1), ("MI355X-NODE.MI355X-QUAD", 1)],
}
FIELDS = list(PodSchedulingSpec.__dataclass_fields__)


class PropertySpec(PodSchedulingSpec):
    """priority and affinityGroup live under other names; the instance dict
    holds wrong values under the fields' own names."""

    @property
    def priority(self):
        return self.__dict__["_priority"]

    @priority.setter
    def priority(self, value):
        self.__dict__["_priority"] = value
        self.__dict__["priority"] = 1000 - max(value, 0)  # decoy

    @property
    def affinityGroup(self):
        return self.__dict__["_group"]

    @affinityGroup.setter
    def affinityGroup(self, value):
        self.__dict__["_group"] = value
        self.__dict__["affinityGroup"] = AffinityGroupSpec(  # decoy
            name="decoy", members=[AffinityGroupMemberSpec(podNumber=64, leafCellNumber=1)])


class PropertyMember(AffinityGroupMemberSpec):
    @property
    def podNumber(self):
        return self.__dict__["_pods"]

    @podNumber.setter
    def podNumber(self, value):
        self.__dict__["_pods"] = value
        self.__dict__["podNumber"] = value + 7  # decoy


def as_plain(spec):
    return copy.deepcopy(spec)


def as_property(spec):
    out = PropertySpec(**{f: copy.deepcopy(getattr(spec, f)) for f in FIELDS})
    if out.affinityGroup is not None:
        out.affinityGroup.members = [PropertyMember(m.podNumber, m.leafCellNumber)
                                     for m in out.affinityGroup.members]
    assert out.__dict__["priority"] != out.priority
    return out


def as_deleted(spec):
    out = copy.deepcopy(spec)
    default = PodSchedulingSpec()
    for f in FIELDS:
        if getattr(out, f) == getattr(default, f):
            del out.__dict__[f]
    if out.affinityGroup is not None:
        if not out.affinityGroup.name:
            del out.affinityGroup.__dict__["name"]
        for m in out.affinityGroup.members:
            for f in ("podNumber", "leafCellNumber"):
                if getattr(m, f) == 0:
                    del m.__dict__[f]
    return out


FORMS = {"plain": as_plain, "property": as_property, "deleted": as_deleted}


def result_tuple(r):
    info = r.bind_info
    return (r.kind, info.to_dict() if info else None, r.victim_node, list(r.victim_pod_keys),
            r.wait_reason)


def requests(seed, count):
    rng = random.Random(seed)
    out = []
    for i in range(count):
        params = dict(vc=rng.choice(["VC1", "VC1", "VC2"]), priority=rng.choice([-1, 0, 0, 1, 5]),
                      leaf_cells=rng.choice([1, 2, 4, 8]),
                      lazy_preemption=rng.random() < 0.2, ignore_suggested=rng.random() < 0.7,
                      hbm_bytes_per_cell=rng.choice([0, 0, 1 << 30]),
                      leaf_cell_type=rng.choice(["", "", "MI355X"]))
        if rng.random() < 0.4:
            params.update(group=f"g{i}", members=[(rng.choice([1, 2]), params["leaf_cells"]),
                                                  (1, rng.choice([1, 2]))])
        phase = PREEMPTING if rng.random() < 0.3 else FILTERING
        suggested = None if rng.random() < 0.5 else ["node1", "node2", "node4"]
        out.append((f"ns/p{i}", SimScheduler.pod_spec(**params), suggested, phase))
    return out


def test_four_forms_of_a_request_get_the_same_answer():
    config = mi355x_cluster_config(num_nodes=4, vcs=VCS)
    sims = {form: SimScheduler(config) for form in list(FORMS) + ["dict"]}
    kinds = set()
    deleted_fields = 0
    for key, spec, suggested, phase in requests(31, 120):
        expected = copy.deepcopy(spec)
        validate_pod_scheduling_spec(expected, key)  # what the defaulting must leave
        answers = {}
        for form, make in FORMS.items():
            given = make(spec)
            deleted_fields += form == "deleted" and len(FIELDS) - len(given.__dict__)
            answers[form] = result_tuple(sims[form].schedule(key, given, suggested, phase))
            # (compared as dicts: the property form's members are a subclass)
            assert given.affinityGroup.to_dict() == expected.affinityGroup.to_dict(), (key, form)
            if spec.affinityGroup is None:  # defaulted on the spec, named after the pod
                assert type(given.affinityGroup) is AffinityGroupSpec
                assert given.affinityGroup.name is key
        core = sims["dict"].alg._core
        wire = expected.to_dict()
        answers["dict"] = result_tuple(core.schedule_pod(
            wire, key, suggested if suggested is not None else core.all_nodes(), phase, True, False))
        assert wire == expected.to_dict()  # a dict is read, never written
        for form, answer in answers.items():
            assert answer == answers["plain"], (key, form)
        kinds.add(answers["plain"][0])
        states = {form: (sim.alg.get_all_affinity_groups(), sim.alg.get_cluster_status())
                  for form, sim in sims.items()}
        for form, state in states.items():
            assert state == states["plain"], (key, form)
    assert kinds == {"bind", "preempt", "wait"}
    assert deleted_fields > 300
    for sim in sims.values():
        sim.alg._core.check_invariants()


def bad_specs():
    def spec(**kw):
        return SimScheduler.pod_spec(**kw)

    def group(name, members, **kw):
        s = spec(**kw)
        s.affinityGroup = AffinityGroupSpec(
            name=name, members=[AffinityGroupMemberSpec(podNumber=p, leafCellNumber=c)
                                for p, c in members])
        return s

    hbm = spec()
    hbm.hbmBytesPerCell = -1
    return {
        "VirtualCluster is empty": spec(vc=""),
        "Priority is less than -1": spec(priority=-2),
        "Priority is greater than 1000": spec(priority=1001),
        "LeafCellNumber is non-positive": spec(leaf_cells=0),
        "AffinityGroup.Name is empty": group("", [(1, 1)]),
        "AffinityGroup.Members has non-positive PodNumber": group("g", [(0, 1)]),
        "AffinityGroup.Members has non-positive LeafCellNumber": group("g", [(1, 1), (1, 0)]),
        "AffinityGroup.Members does not contain current Pod": group("g", [(1, 2)]),
        "hbmBytesPerCell must be non-negative": hbm,
    }


@pytest.mark.parametrize("text", list(bad_specs()))
def test_validation_error_texts_are_unchanged(text):
    sim = SimScheduler(mi355x_cluster_config(num_nodes=1))
    spec = bad_specs()[text]
    if not text.startswith("hbmBytesPerCell"):  # that check is the core's own
        with pytest.raises(WebServerError) as expected:
            validate_pod_scheduling_spec(copy.deepcopy(spec), "ns/bad")
        assert expected.value.message == text
    for form, make in FORMS.items():
        with pytest.raises(WebServerError) as e:
            sim.alg.schedule_pod(make(spec), "ns/bad")
        assert (e.value.code, e.value.message) == (400, text), form
    assert sim.alg.get_all_affinity_groups() == []
    assert sim.alg.schedule_count() == 0


def test_other_records_still_go_through_getattr_or_getitem():
    """An object that is no dataclass at all, and a spec whose group and
    members are wire-format dicts."""
    sim = SimScheduler(mi355x_cluster_config(num_nodes=1))

    class Duck:
        virtualCluster = "VC1"
        priority = 0
        pinnedCellId = ""
        leafCellType = ""
        leafCellNumber = 2
        gangReleaseEnable = False
        lazyPreemptionEnable = False
        ignoreK8sSuggestedNodes = True
        hbmBytesPerCell = 0
        affinityGroup = None

    duck = Duck()
    assert sim.alg.schedule_pod(duck, "ns/duck", None, FILTERING, True).kind == "bind"
    assert duck.affinityGroup.name == "ns/duck"
    mixed = SimScheduler.pod_spec(leaf_cells=2)
    mixed.affinityGroup = {"name": "m", "members": [{"podNumber": 1, "leafCellNumber": 2}]}
    assert sim.alg.schedule_pod(mixed, "ns/mixed", None, FILTERING, True).kind == "bind"
    assert sorted(g["name"] for g in sim.alg.get_all_affinity_groups()) == ["m", "ns/duck"]
