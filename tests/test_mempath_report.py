"""CPU tests for the memory-path probe's host side: the summariser on synthetic
records, the invariants of the out-of-bounds offset table, and the flag
plumbing through the agent and the command line."""
import inspect

import numpy as np
import pytest

from hivedscheduler_amd import ops
from hivedscheduler_amd.ops import mempath_probe as mp

SEED, ROUNDS = 3, 2
WORD = (3 << 16) | (2 << 13) | (1 << 12) | (5 << 8)


def clean_records(section, blocks=2):
    rec = np.zeros((blocks * 4, 8), dtype=np.int64)
    rec[:, 0] = WORD + 256 * (np.arange(blocks * 4) // 4)  # one CU per block
    rec[:, 2:4] = -1
    rec[:, 6] = [ops.mempath_wave_checksum(section, SEED, w, ROUNDS) for w in range(blocks * 4)]
    rec[:, 7] = 2 if section == "lds" else 0
    return rec


@pytest.mark.parametrize("section", ops.MEMPATH_SECTIONS)
def test_summarize(section):
    n = len(ops.mempath_steps(section))
    rec = clean_records(section)
    s = ops.summarize_mempath(rec, 2.0, section, ROUNDS, SEED, expected_cus=2)
    assert s["ok"] is True and s["bad_cus"] == [] and s["cus_seen"] == 2 and s["gbps"] > 0
    assert s.get("lds_oob_writes_zero") == (False if section == "lds" else None)
    assert ops.summarize_mempath(rec, 2.0, section, ROUNDS, SEED, expected_cus=3)["ok"] is False
    bad = rec.copy()
    bad[5, 1:6] = (2, n + 1, 40, 0x10, 0x3)  # wave 1 of block 1
    bad[6, 1:6] = (1, n + 1, 8, 0x20, 0)
    s = ops.summarize_mempath(bad, 2.0, section, ROUNDS, SEED, expected_cus=2)
    assert s["ok"] is False and s["mismatched_blocks"] == 1 and s["checksum_ok"] is True
    assert s["bad_cus"] == [{"xcc": 3, "se": 2, "sh": 1, "cu": 6, "blocks": 1,
                             "mismatched_elements": 3, "first_bad_step": n + 1,
                             "first_bad_offset": 8, "dropped_mask": 0x30, "raised_mask": 0x3,
                             "first_bad_step_name": ops.mempath_steps(section)[1]}]
    split = rec.copy()
    split[2, 0] += 256
    s = ops.summarize_mempath(split, 2.0, section, ROUNDS, SEED, expected_cus=2)
    assert s["ok"] is False and s["split_blocks"] == 1 and s["bad_cus"] == []
    wrong = rec.copy()
    wrong[3, 6] ^= 1
    s = ops.summarize_mempath(wrong, 2.0, section, ROUNDS, SEED, expected_cus=2)
    assert s["ok"] is False and s["checksum_ok"] is False
    if section == "lds":  # waves that disagree on what an out-of-range lane does
        rec[1, 7] = 1
        s = ops.summarize_mempath(rec, 2.0, section, ROUNDS, SEED, expected_cus=2)
        assert s["ok"] is False and s["lds_oob_writes_zero"] is None


def test_pattern_and_checksum():
    p0, p1 = ops.mempath_pattern(SEED, 7, 0), ops.mempath_pattern(SEED, 7, 1)
    assert len(set(p0.tolist())) == 3072 and len(set(p1.tolist())) == 3072
    assert (p1 != ~p0).any() and (ops.mempath_pattern(SEED, 8, 0) != p0).all()
    # one round of the lds section, from the kernel comment: four whole copies
    # and the 32 in-range words of the last step, among sentinels
    want = 4 * (int(p0.sum(dtype=np.uint64)) + 1024 * mp.LDS_SENTINEL) \
        + int(p0[:32].sum(dtype=np.uint64)) + (4096 - 64) * mp.LDS_SENTINEL
    assert ops.mempath_wave_checksum("lds", SEED, 7, 1) == want & 0xFFFFFFFF
    assert ops.mempath_wave_checksum("lds", SEED, 7, 2) == want & 0xFFFFFFFF  # odd round: unsummed


def test_oob_case_invariants():
    cases = ops.mempath_oob_cases()
    assert len(cases) == 60 == len(ops.mempath_steps("oob")) - 1
    assert {c["length"] for c in cases} >= {12288, 12287, 12285, 4, 0}
    for c in cases:
        L, w = c["length"], c["width"]
        assert c["soffset"] == 0 and c["name"] == ops.mempath_steps("oob")[c["step"]]
        ins = [o for o, where in c["accesses"] if where == "in"]
        outs = [o for o, where in c["accesses"] if where == "out"]
        for o, _ in c["accesses"]:
            assert 0 <= o and o + w <= mp.ROW_BYTES and o % w == 0
            assert o + w <= L or o >= L  # no straddling access
        assert c["first_out"] + w <= mp.ROW_BYTES
        assert outs and min(outs) == c["first_out"]
        if L >= w:  # the window allows an access that ends at the last whole element
            assert ins and max(ins) == L // w * w - w
    for w in mp.OOB_WIDTHS:
        assert {c["length"] for c in cases if c["width"] == w} == set(mp.OOB_LENGTHS)
    assert all((mp.GUARD_SENTINEL >> s) & 0xFF for s in (0, 8, 16, 24))


def test_flag_plumbing(monkeypatch):
    from hivedscheduler_amd.agent import health

    assert inspect.signature(ops.gpu_health_report).parameters["mempath_probe"].default is False
    assert inspect.signature(health.collect_node_health).parameters[
        "mempath_probe"].default is False
    bad_cu = {"xcc": 1, "se": 0, "sh": 0, "cu": 4}
    probe = {"sections": {"buf": {"gbps": 123.45}}, "ok": False, "bad_cus": [dict(bad_cu)],
             "lds_oob_writes_zero": False}
    calls = []

    def fake_report(device=0, **kwargs):
        calls.append(kwargs)
        rep = {"hbm_gbps": 5000.0, "mfma_ok": True, "cu_coverage": 256, "lds_errors": 0,
               "healthy": True}
        if kwargs.get("mempath_probe"):
            rep.update(mempath_probe=probe, healthy=False)
        return rep

    monkeypatch.setattr(ops, "gpu_health_report", fake_report)
    monkeypatch.setattr(health, "_rocm_smi_gpu_state", lambda: {0: True})
    g = health.collect_node_health(deep=True)["gpus"]["0"]
    assert g["healthy"] is True and "mempath_probe" not in calls[-1]
    assert not any(k.startswith("mempath") for k in g)
    g = health.collect_node_health(deep=True, mempath_probe=True)["gpus"]["0"]
    assert g["healthy"] is False and g["mempath_probe_ok"] is False
    assert g["mempath_gbps"] == {"buf": 123.5} and g["mempath_bad_cus"] == [bad_cu]
    monkeypatch.setattr(health.NodeHealthAgent, "post_report", lambda self, r: True)
    monkeypatch.setattr(health.NodeHealthAgent, "run_placement_probes", lambda self: [])
    monkeypatch.setattr(health, "p2p_link_matrix", lambda: {"matrix": {}, "links": []})
    assert health.NodeHealthAgent("http://x").mempath_probe_every == 0
    agent = health.NodeHealthAgent("http://x", node_name="n", deep_every=1, probe_pairs=False,
                                   p2p_matrix_every=10 ** 9, mempath_probe_every=2)
    got = [agent.run_once()["gpus"]["0"] for _ in range(4)]
    assert ["mempath_probe_ok" in g for g in got] == [True, False, True, False]
    from hivedscheduler_amd.agent import __main__ as cli

    seen = {}
    monkeypatch.setattr(health, "collect_node_health", lambda **kw: seen.update(kw) or {"gpus": {}})
    monkeypatch.setattr("sys.argv", ["agent", "--local", "--mempath-probe", "--no-probe-pairs"])
    cli.main()
    assert seen["mempath_probe"] is True and seen["mx_scale_probe"] is False
    monkeypatch.setattr(health, "NodeHealthAgent",
                        lambda url, **kw: seen.update(kw) or type("A", (), {"run_once": lambda s: {}})())
    monkeypatch.setattr("sys.argv", ["agent", "--scheduler", "http://x", "--once",
                                     "--mempath-probe-every", "6"])
    cli.main()
    assert seen["mempath_probe_every"] == 6 and seen["mx_scale_probe_every"] == 0
