"""Full-LDS march, host side (no GPU): the pattern and its checksum, record
summarising and per-CU attribution, agent verdicts and cadence, and the path
of `lds_bad_cus` through the scheduler to the inspect view."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from hivedscheduler_amd import ops
from hivedscheduler_amd.ops import (
    LDS_MARCH_WORDS,
    lds_march_block_checksum,
    lds_march_pattern,
    summarize_lds_march,
)

M32 = 0xFFFFFFFF
SEED, ROUNDS = 5, 2


def fmix32(h):
    """murmur3 finaliser on Python ints, written out independently."""
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & M32
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & M32
    return h ^ (h >> 16)


def pattern_word(seed, rnd, i):
    return fmix32(((seed + rnd * 0x9E3779B9) & M32) ^ ((i * 0x85EBCA6B) & M32))


def hw_word(xcc, se, sh, cu):
    return (xcc << 16) | (se << 13) | (sh << 12) | (cu << 8)


# 4 distinct CUs, one block (4 waves) each
CUS = [(0, 0, 0, 1), (0, 3, 1, 7), (5, 2, 0, 15), (7, 7, 1, 0)]


def as_i32(v):
    return int(np.uint32(v & M32).astype(np.int32))


def clean_records(seed=SEED, rounds=ROUNDS, cus=CUS):
    """[blocks*4, 8] records of a fault-free run: the block checksum is split
    unevenly over the four waves, as on hardware."""
    total = lds_march_block_checksum(seed, rounds)
    parts = [0x1234567, 0xFEDCBA98, 0x0F0F0F0F]
    parts.append((total - sum(parts)) & M32)
    rec = np.zeros((len(cus) * 4, 8), dtype=np.int32)
    for b, cu in enumerate(cus):
        for w in range(4):
            # low byte of HW_ID (wave and SIMD ids) differs per wave
            rec[4 * b + w] = (hw_word(*cu) | (w << 4) | w, 0, -1, -1, 0, 0, as_i32(parts[w]), 0)
    return rec


def summarize(rec, elapsed_ms=1.0, expected_cus=4):
    return summarize_lds_march(rec, elapsed_ms, ROUNDS, SEED, expected_cus)


def test_fmix32_known_values():
    # murmur3's finaliser fixes 0; the other two are its published values,
    # e.g. fmix32(1): 1 -> *0x85EBCA6B = 0x85EBCA6B -> ^>>13 = 0x85EFE535
    # -> *0xC2B2AE35 = 0x514E79F9 -> ^>>16 = 0x514E28B7
    assert fmix32(0) == 0
    assert fmix32(1) == 0x514E28B7
    assert fmix32(0xFFFFFFFF) == 0x81F16F39


def test_pattern_matches_hand_computed_words():
    assert LDS_MARCH_WORDS == 40960
    p = lds_march_pattern(1, 0)
    assert p.dtype == np.uint32 and p.shape == (40960,)
    # seed 1, round 0: word 0 is fmix32(1), word 1 is fmix32(1 ^ 0x85EBCA6B)
    assert int(p[0]) == 0x514E28B7
    assert int(p[1]) == fmix32(0x85EBCA6A)
    # round 1 of seed 0 starts from the golden-ratio increment
    assert int(lds_march_pattern(0, 1)[0]) == fmix32(0x9E3779B9)
    for seed, rnd, i in ((1, 0, 40959), (7, 3, 16384), (0xFFFFFFFF, 2, 12345), (123, 5, 4 * 77 + 3)):
        assert int(lds_march_pattern(seed, rnd)[i]) == pattern_word(seed, rnd, i)


def test_pattern_is_address_unique_and_varies():
    for rnd in range(3):
        assert len(np.unique(lds_march_pattern(SEED, rnd))) == LDS_MARCH_WORDS
    assert not np.array_equal(lds_march_pattern(SEED, 0), lds_march_pattern(SEED, 1))
    assert not np.array_equal(lds_march_pattern(SEED, 0), lds_march_pattern(SEED + 1, 0))
    # seed + round*inc wraps: the pattern depends on their sum mod 2^32 only
    assert np.array_equal(lds_march_pattern(0x9E3779B9, 0), lds_march_pattern(0, 1))


def test_block_checksum_against_direct_sum():
    for seed, rounds in ((1, 1), (5, 2), (0xDEADBEEF, 3)):
        direct = 0
        for r in range(rounds):
            direct += 2 * int(lds_march_pattern(seed, r).astype(np.uint64).sum())
        assert lds_march_block_checksum(seed, rounds) == direct % 2 ** 32
    assert lds_march_block_checksum(5, 1) != lds_march_block_checksum(5, 2)


def test_summarize_clean():
    s = summarize(clean_records(), elapsed_ms=2.0)
    assert s["blocks"] == 4 and s["cus_seen"] == 4
    assert s["mismatched_blocks"] == 0 and s["split_blocks"] == 0
    assert s["checksum_ok"] is True and s["bad_cus"] == []
    assert s["ok"] is True
    assert s["elapsed_ms"] == 2.0
    # blocks x rounds x 4 passes x (write + read) x 163840 B over 2 ms
    assert s["gbps"] == pytest.approx(4 * ROUNDS * 4 * 2 * 163840 / 2.0e-3 / 1e9, rel=1e-12)


def test_summarize_names_the_bad_cu():
    rec = clean_records()
    # block 2 (CUS[2]): wave 1 fails at pass 5 word 300, wave 3 earlier at
    # pass 2 word 20000; the top bit dropped in one, bit 0 raised in the other
    rec[9, 1:6] = (2, 5, 300, as_i32(0x80000000), 0)
    rec[11, 1:6] = (1, 2, 20000, 0, 1)
    s = summarize(rec)
    assert s["mismatched_blocks"] == 1
    assert s["bad_cus"] == [{"xcc": 5, "se": 2, "sh": 0, "cu": 15, "blocks": 1,
                             "mismatched_dwords": 3, "first_bad_pass": 2,
                             "first_bad_word": 20000, "dropped_mask": 0x80000000,
                             "raised_mask": 1}]
    assert s["checksum_ok"] is True and s["split_blocks"] == 0
    assert s["ok"] is False


def test_summarize_merges_blocks_of_one_cu_and_sorts():
    rec = clean_records(cus=CUS + [CUS[2]])  # blocks 2 and 4 share a CU
    rec[8, 1:6] = (1, 4, 77, 0x10, 0)
    rec[17, 1:6] = (2, 4, 12, 0, 0x200)    # same pass, lower word
    rec[2, 1:6] = (1, 0, 40959, 0x4, 0)    # CUS[0]
    s = summarize(rec)
    assert s["blocks"] == 5 and s["cus_seen"] == 4 and s["mismatched_blocks"] == 3
    assert s["bad_cus"] == [
        {"xcc": 0, "se": 0, "sh": 0, "cu": 1, "blocks": 1, "mismatched_dwords": 1,
         "first_bad_pass": 0, "first_bad_word": 40959, "dropped_mask": 0x4, "raised_mask": 0},
        {"xcc": 5, "se": 2, "sh": 0, "cu": 15, "blocks": 2, "mismatched_dwords": 3,
         "first_bad_pass": 4, "first_bad_word": 12, "dropped_mask": 0x10,
         "raised_mask": 0x200},
    ]
    assert s["ok"] is False


def test_summarize_wrong_checksum_is_not_ok():
    rec = clean_records()
    rec[6, 6] ^= 1
    s = summarize(rec)
    assert s["mismatched_blocks"] == 0 and s["bad_cus"] == []
    assert s["checksum_ok"] is False
    assert s["ok"] is False
    # the records of another seed or round count do not pass either
    assert summarize_lds_march(clean_records(), 1.0, ROUNDS, SEED + 1, 4)["checksum_ok"] is False
    assert summarize_lds_march(clean_records(), 1.0, ROUNDS + 1, SEED, 4)["checksum_ok"] is False


def test_summarize_split_block_is_not_ok():
    rec = clean_records()
    rec[5, 0] = hw_word(*CUS[0]) | 0x11  # one wave of block 1 names another CU
    s = summarize(rec)
    assert s["split_blocks"] == 1
    assert s["mismatched_blocks"] == 0 and s["checksum_ok"] is True and s["cus_seen"] == 4
    assert s["ok"] is False


def test_summarize_missing_cus_is_not_ok():
    s = summarize(clean_records(), expected_cus=5)
    assert s["cus_seen"] == 4 and s["mismatched_blocks"] == 0 and s["checksum_ok"] is True
    assert s["ok"] is False


def test_summarize_zero_elapsed_gives_zero_gbps():
    s = summarize(clean_records(), elapsed_ms=0.0)
    assert s["gbps"] == 0.0 and s["elapsed_ms"] == 0.0


BAD_CU = {"xcc": 5, "se": 2, "sh": 0, "cu": 15, "blocks": 1, "mismatched_dwords": 1,
          "first_bad_pass": 2, "first_bad_word": 16384, "dropped_mask": 0, "raised_mask": 8}


def canned_report(bad_cus, ok=None, gbps=41234.56):
    ok = (not bad_cus) if ok is None else ok
    return {
        "hbm_gbps": 5000.0, "mfma_ok": True, "cu_coverage": 256, "lds_errors": 0,
        "healthy": ok,
        "lds_march": {"gbps": gbps, "elapsed_ms": 1.0, "blocks": 512, "cus_seen": 256,
                      "mismatched_blocks": len(bad_cus), "checksum_ok": True,
                      "split_blocks": 0, "bad_cus": bad_cus, "ok": ok},
    }


@pytest.fixture()
def agent_health(monkeypatch):
    """collect_node_health over one fake GPU: returns the agent module and a
    dict holding the canned `report` to serve and the `calls` it received."""
    from hivedscheduler_amd.agent import health

    state = {"report": None, "calls": []}

    def fake_report(device=0, **kwargs):
        state["calls"].append(kwargs)
        rep = dict(state["report"])
        if not kwargs.get("lds_march"):
            rep.pop("lds_march")
            rep["healthy"] = True
        return rep

    monkeypatch.setattr(ops, "gpu_health_report", fake_report)
    monkeypatch.setattr(health, "_rocm_smi_gpu_state", lambda: {0: True})
    return health, state


def test_agent_march_verdicts(agent_health):
    health, state = agent_health
    state["report"] = canned_report([])
    g = health.collect_node_health(deep=True, lds_march=True)["gpus"]["0"]
    assert g["healthy"] is True and g["lds_march_ok"] is True and g["lds_bad_cus"] == []
    assert g["lds_gbps"] == 41234.6
    assert state["calls"][-1]["lds_march"] is True
    assert "burn" not in state["calls"][-1]
    assert "bad_cus" not in g  # that key stays the burn-in's
    # a named bad CU fails the GPU and is reported as a plain CU tuple
    state["report"] = canned_report([BAD_CU])
    g = health.collect_node_health(deep=True, lds_march=True)["gpus"]["0"]
    assert g["healthy"] is False and g["lds_march_ok"] is False
    assert g["lds_bad_cus"] == [{"xcc": 5, "se": 2, "sh": 0, "cu": 15}]
    # a march that failed without naming a CU (missing coverage, checksum) too
    state["report"] = canned_report([], ok=False)
    g = health.collect_node_health(deep=True, lds_march=True)["gpus"]["0"]
    assert g["healthy"] is False and g["lds_march_ok"] is False and g["lds_bad_cus"] == []
    # the throughput figure is reported, never judged
    state["report"] = canned_report([], gbps=0.04)
    g = health.collect_node_health(deep=True, lds_march=True)["gpus"]["0"]
    assert g["healthy"] is True and g["lds_gbps"] == 0.0


def test_agent_without_march_is_unchanged(agent_health):
    health, state = agent_health
    state["report"] = canned_report([BAD_CU])
    g = health.collect_node_health(deep=True)["gpus"]["0"]
    assert g == {"healthy": True, "hbm_gbps": 5000.0, "mfma_ok": True, "cu_coverage": 256,
                 "lds_errors": 0}
    assert "lds_march" not in state["calls"][-1]
    # not deep: the kernels do not run at all
    n = len(state["calls"])
    g = health.collect_node_health(deep=False, lds_march=True)["gpus"]["0"]
    assert g == {"healthy": True} and len(state["calls"]) == n


def test_agent_march_cadence(agent_health, monkeypatch):
    health, state = agent_health
    state["report"] = canned_report([BAD_CU])
    monkeypatch.setattr(health.NodeHealthAgent, "post_report", lambda self, r: True)
    monkeypatch.setattr(health.NodeHealthAgent, "run_placement_probes", lambda self: [])
    monkeypatch.setattr(health, "p2p_link_matrix", lambda: {"matrix": {}, "links": []})
    never = health.NodeHealthAgent("http://x", node_name="n", deep_every=1, probe_pairs=False,
                                   p2p_matrix_every=10 ** 9)
    assert never.lds_march_every == 0
    assert all("lds_march_ok" not in never.run_once()["gpus"]["0"] for _ in range(3))
    assert all("lds_march" not in c for c in state["calls"])
    agent = health.NodeHealthAgent("http://x", node_name="n", deep_every=1, probe_pairs=False,
                                   p2p_matrix_every=10 ** 9, lds_march_every=2)
    got = [agent.run_once()["gpus"]["0"] for _ in range(4)]
    assert ["lds_gbps" in g for g in got] == [True, False, True, False]
    assert [g["healthy"] for g in got] == [False, True, False, True]
    # only on deep sweeps: every 2nd round is a march round, every 4th deep
    agent = health.NodeHealthAgent("http://x", node_name="n", deep_every=4, probe_pairs=False,
                                   p2p_matrix_every=10 ** 9, lds_march_every=2)
    got = [agent.run_once()["gpus"]["0"] for _ in range(6)]
    assert ["lds_gbps" in g for g in got] == [True, False, False, False, True, False]


def test_cli_has_the_march_flags(monkeypatch, capsys):
    import json
    import sys

    from hivedscheduler_amd.agent import __main__ as cli
    from hivedscheduler_amd.agent import health

    seen = {}

    def fake_collect(**kwargs):
        seen.update(kwargs)
        return {"gpus": {}}

    monkeypatch.setattr(health, "collect_node_health", fake_collect)
    monkeypatch.setattr(sys, "argv", ["agent", "--local", "--lds-march", "--no-probe-pairs"])
    cli.main()
    assert seen["lds_march"] is True
    assert json.loads(capsys.readouterr().out) == {"gpus": {}}
    monkeypatch.setattr(sys, "argv", ["agent", "--local", "--no-probe-pairs"])
    cli.main()
    assert seen["lds_march"] is False

    made = {}

    class FakeAgent:
        def __init__(self, url, **kwargs):
            made.update(kwargs)

        def run_once(self):
            return {}

    monkeypatch.setattr(health, "NodeHealthAgent", FakeAgent)
    monkeypatch.setattr(sys, "argv", ["agent", "--scheduler", "http://x", "--once",
                                      "--lds-march-every", "6"])
    cli.main()
    assert made["lds_march_every"] == 6
    monkeypatch.setattr(sys, "argv", ["agent", "--scheduler", "http://x", "--once"])
    cli.main()
    assert made["lds_march_every"] == 0


def test_lds_bad_cus_reach_the_inspect_view():
    from hivedscheduler_amd.scheduler import HivedScheduler
    from hivedscheduler_amd.sim import mi355x_cluster_config

    sched = HivedScheduler(mi355x_cluster_config(num_nodes=1))
    node = sched.algorithm.all_nodes()[0]
    sched.on_node_add({"metadata": {"name": node, "uid": "n1"}, "spec": {},
                       "status": {"conditions": [{"type": "Ready", "status": "True"}]}})
    lds_bad_cus = [{"xcc": 5, "se": 2, "sh": 0, "cu": 15}]
    report = {"gpus": {"3": {"healthy": False, "lds_march_ok": False, "lds_gbps": 41234.6,
                             "lds_bad_cus": lds_bad_cus}}}
    assert sched.on_health_report(node, report)["applied"] == {"3": False}

    def leaves(c):
        kids = c.get("cellChildren") or []
        return [c] if not kids else [l for k in kids for l in leaves(k)]

    status = sched.get_physical_cluster_status()
    unhealthy = [c for c in leaves(status[0]) if c.get("cellHealthiness") != "Healthy"]
    assert len(unhealthy) == 1, [c.get("cellAddress") for c in unhealthy]
    gpu = sched.get_health_reports()[node]["gpus"]["3"]
    assert gpu["lds_bad_cus"] == lds_bad_cus
    assert gpu["lds_march_ok"] is False and gpu["lds_gbps"] == 41234.6
