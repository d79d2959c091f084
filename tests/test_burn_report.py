"""MFMA burn-in, host side (no GPU): record summarising and per-CU
attribution, operand construction, agent verdicts and the path of `bad_cus`
through the scheduler to the inspect view."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from hivedscheduler_amd import ops
from hivedscheduler_amd.ops import (
    _FP4_E2M1_VALUES,
    _burn_integers,
    burn_chain_limit,
    burn_operands,
    decode_hw_word,
    summarize_burn,
)

FMTS = ("bf16", "fp8", "mx8", "mx4")
K = {"bf16": 32, "fp8": 32, "mx8": 128, "mx4": 128}


def hw_word(xcc, se, sh, cu):
    return (xcc << 16) | (se << 13) | (sh << 12) | (cu << 8)


# 4 distinct CUs, 4 waves each
CUS = [(0, 0, 0, 1), (0, 3, 1, 7), (5, 2, 0, 15), (7, 7, 1, 0)]


def clean_records(checksum=0x1234):
    rec = np.zeros((16, 4), dtype=np.int32)
    for w in range(16):
        rec[w] = (hw_word(*CUS[w % 4]), 0, -1, checksum)
    return rec


def test_decode_hw_word_fields():
    for cu in CUS:
        # low byte of HW_ID (wave/SIMD ids) must not leak into the tuple
        assert decode_hw_word(hw_word(*cu) | 0xB7) == cu


def test_summarize_names_the_bad_cu():
    rec = clean_records()
    rec[6, 1], rec[6, 2] = 3, 2  # wave 6 sits on CUS[2]
    s = summarize_burn(rec, elapsed_ms=2.0, fmt="bf16", chain=8, rounds=5, expected_cus=4)
    assert s["waves"] == 16 and s["cus_seen"] == 4
    assert s["mismatched_waves"] == 1
    assert s["bad_cus"] == [{"xcc": 5, "se": 2, "sh": 0, "cu": 15, "waves": 1,
                             "mismatched_elements": 3, "first_bad_round": 2}]
    assert s["ok"] is False
    # 2*M*N*K flop per MFMA x 4 accumulators x chain x rounds x waves, over 2 ms
    assert s["tflops"] == pytest.approx(2 * 16 * 16 * 32 * 4 * 8 * 5 * 16 / 2.0e-3 / 1e12,
                                        rel=1e-12)
    # K=128 formats count 4x the flop per instruction
    s4 = summarize_burn(rec, 2.0, "mx4", 8, 5, 4)
    assert s4["tflops"] == pytest.approx(4 * s["tflops"], rel=1e-12)


def test_summarize_merges_waves_of_one_cu_and_sorts():
    rec = clean_records()
    rec[6, 1], rec[6, 2] = 3, 2    # CUS[2]
    rec[10, 1], rec[10, 2] = 5, 1  # CUS[2] again
    rec[0, 1], rec[0, 2] = 1, 4    # CUS[0]
    s = summarize_burn(rec, 1.0, "fp8", 1, 1, 4)
    assert s["mismatched_waves"] == 3
    assert s["bad_cus"] == [
        {"xcc": 0, "se": 0, "sh": 0, "cu": 1, "waves": 1, "mismatched_elements": 1,
         "first_bad_round": 4},
        {"xcc": 5, "se": 2, "sh": 0, "cu": 15, "waves": 2, "mismatched_elements": 8,
         "first_bad_round": 1},
    ]


def test_summarize_missing_cus_is_not_ok():
    s = summarize_burn(clean_records(), 1.0, "bf16", 4, 4, expected_cus=5)
    assert s["mismatched_waves"] == 0 and s["bad_cus"] == [] and not s["checksum_spread"]
    assert s["cus_seen"] == 4
    assert s["ok"] is False
    assert summarize_burn(clean_records(), 1.0, "bf16", 4, 4, expected_cus=4)["ok"] is True


def test_summarize_checksum_spread_is_not_ok():
    rec = clean_records()
    rec[9, 3] ^= 1
    s = summarize_burn(rec, 1.0, "bf16", 4, 4, expected_cus=4)
    assert s["mismatched_waves"] == 0
    assert s["checksum_spread"] is True
    assert s["ok"] is False


@pytest.mark.parametrize("fmt", FMTS)
def test_burn_operands_are_exact_small_integers(fmt):
    A, B, unit = burn_operands(fmt, seed=3)
    assert A.shape == (64, K[fmt]) and B.shape == (K[fmt], 16) and unit.shape == (4, 16, 16)
    assert unit.dtype == torch.float32
    if fmt == "mx4":
        assert A.dtype == torch.uint8 and B.dtype == torch.uint8
        lut = torch.tensor(_FP4_E2M1_VALUES, dtype=torch.float32)
        a, b = lut[A.long()], lut[B.long()]
    else:
        assert A.dtype == (torch.bfloat16 if fmt == "bf16" else torch.float8_e4m3fn)
        a, b = A.float(), B.float()
    # decoding the encoded operands gives back the integers that were drawn
    a_int, b_int = _burn_integers(fmt, seed=3)
    assert a_int.dtype == torch.int64 and b_int.dtype == torch.int64
    assert torch.equal(a, a_int.float()) and torch.equal(b, b_int.float())
    for t in (a, b):
        assert torch.equal(t, t.round()) and t.abs().max().item() == 2.0
        assert set(t.unique().tolist()) == {-2.0, -1.0, 0.0, 1.0, 2.0}
    if fmt in ("fp8", "mx8"):
        assert set(A.view(torch.uint8).unique().tolist()) == {192, 184, 0, 56, 64}
    if fmt == "mx4":
        assert set(A.unique().tolist()) == {12, 10, 0, 2, 4}
    # asymmetric B: a transposed layout cannot reproduce it
    assert not torch.equal(b[:16, :16], b[:16, :16].T)
    # expected tile, recomputed in exact integer arithmetic
    want = a.long().view(4, 16, K[fmt]) @ b.long()
    assert torch.equal(unit.long(), want) and torch.equal(unit, want.float())
    # no expected element is zero, so a wrong chain length or a dead lane
    # shows in every element
    assert bool((unit != 0).all())
    assert burn_chain_limit(fmt) * 4 * K[fmt] <= 2 ** 24
    assert (burn_chain_limit(fmt) + 1) * 4 * K[fmt] > 2 ** 24
    # a different seed draws different operands
    assert not torch.equal(burn_operands(fmt, seed=4)[2], unit)


def canned_report(bf16_tflops, bad_cus):
    fmt = {"tflops": bf16_tflops, "ok": not bad_cus, "bad_cus": bad_cus}
    return {
        "hbm_gbps": 5000.0, "mfma_ok": True, "cu_coverage": 256, "lds_errors": 0,
        "healthy": not bad_cus,
        "mfma_burn": {"formats": {"bf16": fmt, "mx4": {"tflops": 4 * bf16_tflops, "ok": True,
                                                       "bad_cus": []}},
                      "ok": not bad_cus,
                      "bad_cus": [{k: c[k] for k in ("xcc", "se", "sh", "cu")}
                                  for c in bad_cus]},
    }


BAD_CU = {"xcc": 5, "se": 2, "sh": 0, "cu": 15, "waves": 1, "mismatched_elements": 3,
          "first_bad_round": 2}


@pytest.fixture()
def agent_health(monkeypatch):
    """collect_node_health over fake GPUs: returns the agent module and a
    dict holding the canned `report` to serve and the `calls` it received."""
    from hivedscheduler_amd.agent import health

    state = {"report": None, "calls": []}

    def fake_report(device=0, **kwargs):
        state["calls"].append(kwargs)
        rep = dict(state["report"])
        if not kwargs.get("burn"):
            rep.pop("mfma_burn")
        return rep

    monkeypatch.setattr(ops, "gpu_health_report", fake_report)
    monkeypatch.setattr(health, "_rocm_smi_gpu_state", lambda: {0: True})
    return health, state


def test_agent_burn_verdicts(agent_health):
    health, state = agent_health
    state["report"] = canned_report(1000.0, [])
    g = health.collect_node_health(deep=True, burn=True, min_mfma_tflops=500.0)["gpus"]["0"]
    assert g["healthy"] is True and g["mfma_burn_ok"] is True and g["bad_cus"] == []
    assert g["mfma_tflops"] == {"bf16": 1000.0, "mx4": 4000.0}
    assert state["calls"][-1]["burn"] is True
    # below the bf16 floor
    g = health.collect_node_health(deep=True, burn=True, min_mfma_tflops=1000.5)["gpus"]["0"]
    assert g["healthy"] is False and g["mfma_burn_ok"] is True
    # no floor given: the figure alone never fails a GPU
    g = health.collect_node_health(deep=True, burn=True)["gpus"]["0"]
    assert g["healthy"] is True
    # a named bad CU fails it however fast it ran
    state["report"] = canned_report(1000.0, [BAD_CU])
    g = health.collect_node_health(deep=True, burn=True, min_mfma_tflops=1.0)["gpus"]["0"]
    assert g["healthy"] is False and g["mfma_burn_ok"] is False
    assert g["bad_cus"] == [{"xcc": 5, "se": 2, "sh": 0, "cu": 15}]


def test_agent_without_burn_is_unchanged(agent_health):
    health, state = agent_health
    state["report"] = canned_report(1000.0, [])
    g = health.collect_node_health(deep=True)["gpus"]["0"]
    assert g["healthy"] is True
    assert not {"mfma_tflops", "mfma_burn_ok", "bad_cus"} & set(g)
    assert "burn" not in state["calls"][-1]


def test_agent_burn_cadence(agent_health, monkeypatch):
    health, state = agent_health
    state["report"] = canned_report(1000.0, [])
    monkeypatch.setattr(health.NodeHealthAgent, "post_report", lambda self, r: True)
    monkeypatch.setattr(health.NodeHealthAgent, "run_placement_probes", lambda self: [])
    monkeypatch.setattr(health, "p2p_link_matrix", lambda: {"matrix": {}, "links": []})
    never = health.NodeHealthAgent("http://x", node_name="n", deep_every=1, probe_pairs=False,
                                   p2p_matrix_every=10 ** 9)
    assert never.burn_every == 0
    assert all("bad_cus" not in never.run_once()["gpus"]["0"] for _ in range(3))
    agent = health.NodeHealthAgent("http://x", node_name="n", deep_every=1, probe_pairs=False,
                                   p2p_matrix_every=10 ** 9, burn_every=2,
                                   min_mfma_tflops=2000.0)
    got = [agent.run_once()["gpus"]["0"] for _ in range(4)]
    assert ["mfma_tflops" in g for g in got] == [True, False, True, False]
    assert [g["healthy"] for g in got] == [False, True, False, True]


def test_bad_cus_reach_the_inspect_view():
    from hivedscheduler_amd.scheduler import HivedScheduler
    from hivedscheduler_amd.sim import mi355x_cluster_config

    sched = HivedScheduler(mi355x_cluster_config(num_nodes=1))
    node = sched.algorithm.all_nodes()[0]
    sched.on_node_add({"metadata": {"name": node, "uid": "n1"}, "spec": {},
                       "status": {"conditions": [{"type": "Ready", "status": "True"}]}})
    bad_cus = [{"xcc": 5, "se": 2, "sh": 0, "cu": 15}]
    report = {"gpus": {"5": {"healthy": False, "mfma_burn_ok": False, "bad_cus": bad_cus,
                             "mfma_tflops": {"bf16": 1000.0}}}}
    assert sched.on_health_report(node, report)["applied"] == {"5": False}

    def leaves(c):
        kids = c.get("cellChildren") or []
        return [c] if not kids else [l for k in kids for l in leaves(k)]

    status = sched.get_physical_cluster_status()
    unhealthy = [c for c in leaves(status[0]) if c.get("cellHealthiness") != "Healthy"]
    assert len(unhealthy) == 1, [c.get("cellAddress") for c in unhealthy]
    assert sched.get_health_reports()[node]["gpus"]["5"]["bad_cus"] == bad_cus
