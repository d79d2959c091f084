"""HBM march, host side (no GPU): the pattern, record summarising (errors,
location, masks, coverage, per-XCD rates from device clocks), the skipped
case in gpu_health_report, agent verdicts and cadence, the CLI flags, and the
path of the new keys through the scheduler to the inspect view."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from hivedscheduler_amd import ops
from hivedscheduler_amd.ops import hbm_march_pattern, summarize_hbm_march

M32 = 0xFFFFFFFF
M64 = (1 << 64) - 1


def mix64(x):
    """splitmix64 finaliser on Python ints, written out independently."""
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def test_pattern_known_values():
    # the first output of splitmix64 seeded with 0 is mix64(0) (published)
    assert mix64(0) == 0xE220A8397B1DCDAF
    p = hbm_march_pattern(0, 0, 1)
    assert p.dtype == np.uint64 and p.shape == (1,)
    assert int(p[0]) == 0xE220A8397B1DCDAF
    assert int(hbm_march_pattern(0, 1, 1)[0]) == 0x910A2DEC89025CC1 == mix64(1)


def test_pattern_matches_independent_mix64():
    for seed, g in ((1, 0), (1, 2047), (3, 2 ** 32 + 1), (0xDEADBEEFCAFEF00D, 2 ** 33 + 12345),
                    (7, 2 ** 37 - 1), (M64, 2 ** 32)):
        assert int(hbm_march_pattern(seed, g, 1)[0]) == mix64(seed ^ g), (seed, g)
    # a run of values is the per-index pattern, also across 2^32
    start = 2 ** 32 - 3
    run = hbm_march_pattern(5, start, 8)
    assert [int(v) for v in run] == [mix64(5 ^ (start + i)) for i in range(8)]


def test_pattern_is_unique_and_seeded():
    p = hbm_march_pattern(1, 2 ** 32 - 2 ** 15, 2 ** 16)
    assert len(np.unique(p)) == 2 ** 16
    assert not np.array_equal(p, hbm_march_pattern(2, 2 ** 32 - 2 ** 15, 2 ** 16))
    # the complement of a value is never its own pattern value elsewhere here
    assert len(np.unique(np.concatenate([p, ~p]))) == 2 ** 17


# ---------------------------------------------------------------------------
# synthetic records: 2 chunks x 4 launches x 8 workgroups on 4 XCDs
# ---------------------------------------------------------------------------
CHUNKS, BLOCKS, XCDS = 2, 8, 4
TILES = 16                      # per chunk: 2 per workgroup
CHUNK_BYTES = TILES * 16384
CHUNK_QWORDS = CHUNK_BYTES // 8
# each XCD counts from a base of its own, far from the others'; XCD 0 starts
# just below a carry of the low word
XCD_BASE = [2 ** 32 - 5, 7 * 10 ** 12, 3 * 10 ** 9, 2 ** 40 + 17]


def lo_hi(v):
    v &= M64
    return (int(np.uint32(v & M32).astype(np.int32)), int(np.uint32(v >> 32).astype(np.int32)))


def hw_word(xcc, cu=3):
    return (xcc << 16) | (cu << 8)


def clean_result(chunks=CHUNKS):
    """A fault-free result. Workgroup b runs on XCD b % 4. In launch l the
    two workgroups of an XCD run [t0, t0+800] and [t0+100, t0+1000] ticks
    with t0 = base + 5000*l: the XCD's span is 1000 ticks = 10 us."""
    launches = 4 * chunks
    rec = np.zeros((launches, BLOCKS, 16), dtype=np.int32)
    for l in range(launches):
        for b in range(BLOCKS):
            x = b % XCDS
            t0 = XCD_BASE[x] + 5000 * l + (100 if b >= XCDS else 0)
            t1 = t0 + (900 if b >= XCDS else 800)
            rec[l, b, 0] = hw_word(x, cu=b)
            rec[l, b, 1] = TILES // BLOCKS
            rec[l, b, 2:4] = lo_hi(t0)
            rec[l, b, 4:6] = lo_hi(t1)
            if l % 2 == 1:
                rec[l, b, 8:10] = (-1, -1)
                rec[l, b, 14:16] = lo_hi(0x0123456789ABCDEF * (b + 1))
    return {
        "records": rec,
        "elapsed_ms": np.full(launches, 0.02),
        "log": np.zeros((0, 4), dtype=np.int64),
        "log_count": 0,
        "bytes_tested": chunks * CHUNK_BYTES,
        "chunk_bytes": CHUNK_BYTES,
        "chunks": chunks,
        "skipped": False,
    }


def add_fault(res, launch, block, index, want, got, mismatched=1):
    """One workgroup's verify record and one log row for a bad qword."""
    assert launch % 2 == 1
    rec = res["records"]
    pas = (launch // 2) % 2
    rec[launch, block, 6:8] = lo_hi(mismatched)
    rec[launch, block, 8:10] = lo_hi(index)
    rec[launch, block, 10:12] = lo_hi(want & ~got)
    rec[launch, block, 12:14] = lo_hi(got & ~want)
    row = np.array([[index, pas, want, got]], dtype=np.uint64).astype(np.int64)
    res["log"] = np.concatenate([res["log"], row])
    res["log_count"] += 1


def test_summarize_clean():
    s = summarize_hbm_march(clean_result(), expected_xcds=XCDS)
    assert s["bytes_tested"] == 2 * CHUNK_BYTES and s["chunks"] == 2 and s["skipped"] is False
    assert s["errors"] == 0 and s["errors_per_chunk"] == [0, 0]
    assert s["dropped_mask"] == 0 and s["raised_mask"] == 0 and s["bad_bits"] == []
    assert s["first_bad"] is None and s["bad_locations"] == []
    assert s["coverage_ok"] is True
    assert s["xcds_seen"] == XCDS and s["slow_xcds"] == []
    assert s["ok"] is True
    # event-timed, chip-wide: both passes of both chunks over four launches
    want = 2 * 2 * CHUNK_BYTES / (4 * 0.02e-3) / 1e9
    assert s["write_gbps"] == pytest.approx(want, rel=1e-12)
    assert s["verify_gbps"] == pytest.approx(want, rel=1e-12)


def test_summarize_one_fault_with_sign_bits():
    res = clean_result()
    index = CHUNK_QWORDS + 777          # chunk 1, found in pass 0 (launch 5)
    want = (1 << 63) | (1 << 31) | 0x1000
    got = 0x1000 | 0x4                  # bits 63 and 31 dropped, bit 2 raised
    add_fault(res, 5, 3, index, want, got)
    s = summarize_hbm_march(res, expected_xcds=XCDS)
    assert s["errors"] == 1 and s["errors_per_chunk"] == [0, 1]
    assert s["dropped_mask"] == (1 << 63) | (1 << 31)
    assert s["raised_mask"] == 0x4
    assert s["bad_bits"] == [2, 31, 63]
    assert s["first_bad"] == {"offset": 8 * index, "pass": 0}
    assert s["bad_locations"] == [{"offset": 8 * index, "chunk": 1, "pass": 0,
                                   "xor": (1 << 63) | (1 << 31) | 0x4}]
    assert s["coverage_ok"] is True and s["ok"] is False
    # masks whose low and high words both have the int32 sign bit set
    res = clean_result()
    add_fault(res, 1, 0, 5, want=M64, got=M64 ^ ((1 << 63) | (1 << 31)))
    s = summarize_hbm_march(res, expected_xcds=XCDS)
    assert s["dropped_mask"] == (1 << 63) | (1 << 31) and s["raised_mask"] == 0
    res = clean_result()
    add_fault(res, 1, 0, 5, want=0, got=(1 << 63) | (1 << 31))
    s = summarize_hbm_march(res, expected_xcds=XCDS)
    assert s["raised_mask"] == (1 << 63) | (1 << 31) and s["dropped_mask"] == 0
    assert s["bad_locations"][0]["xor"] == (1 << 63) | (1 << 31)


def test_summarize_faults_in_both_chunks_earliest_launch_wins():
    res = clean_result()
    # chunk 0: index 100 goes wrong only in pass 1 (launch 3), index 5000 in
    # pass 0 (launch 1, two workgroups see a bad qword, 5000 the lower);
    # chunk 1: three bad qwords in one workgroup in pass 1 (launch 7)
    add_fault(res, 3, 1, 100, want=0xF0, got=0xF1)
    add_fault(res, 1, 6, 5000, want=0x10, got=0x0)
    add_fault(res, 1, 2, 9000, want=0x10, got=0x0)
    add_fault(res, 7, 4, CHUNK_QWORDS + 1, want=0x8, got=0x0, mismatched=3)
    s = summarize_hbm_march(res, expected_xcds=XCDS)
    assert s["errors"] == 6 and s["errors_per_chunk"] == [3, 3]
    assert s["first_bad"] == {"offset": 8 * 5000, "pass": 0}
    assert s["dropped_mask"] == 0x18 and s["raised_mask"] == 0x1
    assert s["bad_bits"] == [0, 3, 4]
    # sorted by (pass, index)
    assert [(e["pass"], e["offset"] // 8, e["chunk"]) for e in s["bad_locations"]] == [
        (0, 5000, 0), (0, 9000, 0), (1, 100, 0), (1, CHUNK_QWORDS + 1, 1)]
    assert s["ok"] is False


def test_summarize_keeps_at_most_16_locations():
    res = clean_result()
    for i in range(20):
        add_fault(res, 1, i % BLOCKS, 1000 - i, want=1, got=0)
    s = summarize_hbm_march(res, expected_xcds=XCDS)
    assert [e["offset"] // 8 for e in s["bad_locations"]] == list(range(981, 997))


def test_summarize_short_coverage_is_not_ok():
    res = clean_result()
    res["records"][6, 2, 1] -= 1        # one tile of one write launch not visited
    s = summarize_hbm_march(res, expected_xcds=XCDS)
    assert s["errors"] == 0 and s["coverage_ok"] is False and s["ok"] is False
    # a missing launch is short coverage too
    res = clean_result()
    res["records"] = res["records"][:-1]
    res["elapsed_ms"] = res["elapsed_ms"][:-1]
    s = summarize_hbm_march(res, expected_xcds=XCDS)
    assert s["coverage_ok"] is False and s["ok"] is False


def test_summarize_missing_xcd_is_not_ok():
    res = clean_result()
    rec = res["records"]
    moved = (rec[:, :, 0] >> 16) == 2   # XCD 2 never ran anything
    rec[:, :, 0][moved] = hw_word(0, cu=9)
    s = summarize_hbm_march(res, expected_xcds=XCDS)
    assert s["xcds_seen"] == 3 and [x["xcc"] for x in s["xcds"]] == [0, 1, 3]
    assert s["errors"] == 0 and s["coverage_ok"] is True
    assert s["ok"] is False
    assert summarize_hbm_march(res, expected_xcds=3)["ok"] is True


def test_per_xcd_rates_from_device_clocks():
    s = summarize_hbm_march(clean_result(), expected_xcds=XCDS)
    # per launch and XCD: 2 workgroups x 2 tiles x 16 KiB in a 1000-tick span;
    # XCD 0's span runs across the carry of the low clock word, and no base
    # of one XCD is ever subtracted from another's
    want = 4 * 16384 / (1000 * 1e-8) / 1e9
    assert [x["xcc"] for x in s["xcds"]] == [0, 1, 2, 3]
    for x in s["xcds"]:
        assert x["blocks"] == 2 * 4 * CHUNKS
        assert x["write_gbps"] == pytest.approx(want, rel=1e-12)
        assert x["verify_gbps"] == pytest.approx(want, rel=1e-12)
    assert s["xcd_ratio"] == pytest.approx(1.0, rel=1e-12)


def test_slow_xcd_is_named_only_with_a_floor():
    res = clean_result()
    rec = res["records"]
    for l in (1, 3, 5, 7):              # XCD 2 needs twice as long to verify
        t0 = XCD_BASE[2] + 5000 * l
        rec[l, 6, 4:6] = lo_hi(t0 + 2000)
    s = summarize_hbm_march(res, expected_xcds=XCDS)
    rates = {x["xcc"]: x for x in s["xcds"]}
    assert rates[2]["verify_gbps"] == pytest.approx(rates[1]["verify_gbps"] / 2, rel=1e-12)
    assert rates[2]["write_gbps"] == pytest.approx(rates[1]["write_gbps"], rel=1e-12)
    assert s["xcd_ratio"] == pytest.approx(0.5, rel=1e-12)
    assert s["slow_xcds"] == [] and s["ok"] is True
    s = summarize_hbm_march(res, expected_xcds=XCDS, min_xcd_ratio=0.8)
    assert s["slow_xcds"] == [2] and s["ok"] is False
    s = summarize_hbm_march(res, expected_xcds=XCDS, min_xcd_ratio=0.45)
    assert s["slow_xcds"] == [] and s["ok"] is True


def test_workgroup_without_tiles_is_ignored_in_spans():
    res = clean_result()
    rec = res["records"]
    # workgroup 7 (XCD 3) got no tile; workgroup 3 (same XCD) took its two.
    # Its clocks are outlandish and must not stretch the XCD's span.
    rec[:, 7, 1] = 0
    rec[:, 3, 1] = 4
    rec[:, 7, 2:4] = lo_hi(1)
    rec[:, 7, 4:6] = lo_hi(2 ** 50)
    s = summarize_hbm_march(res, expected_xcds=XCDS)
    assert s["coverage_ok"] is True and s["ok"] is True
    x3 = s["xcds"][3]
    want = 4 * 16384 / (800 * 1e-8) / 1e9   # workgroup 3 alone: 800 ticks
    assert x3["verify_gbps"] == pytest.approx(want, rel=1e-12)
    assert x3["write_gbps"] == pytest.approx(want, rel=1e-12)
    assert x3["blocks"] == 2 * 4 * CHUNKS


def test_skipped_is_ok():
    res = clean_result(chunks=0)
    res["skipped"] = True
    assert res["records"].shape == (0, BLOCKS, 16) and res["bytes_tested"] == 0
    s = summarize_hbm_march(res, expected_xcds=8)
    assert s["skipped"] is True and s["ok"] is True
    assert s["errors"] == 0 and s["xcds"] == [] and s["first_bad"] is None
    assert s["write_gbps"] == 0.0 and s["verify_gbps"] == 0.0


class FakeOps:
    """The probes gpu_health_report runs, answering as a healthy GPU would."""

    def device_info(self, dev):
        return {"multiProcessorCount": 1}

    def hbm_triad_gbps(self, size_mb, iters):
        return 5000.0

    @staticmethod
    def _tiles(ref):
        return ref.unsqueeze(0).repeat(2, 1, 1)

    def mfma_check(self, A, B, blocks, repeats):
        return self._tiles(A.float() @ B.float())

    def mfma_check_fp8(self, A, B, blocks):
        return self._tiles(A.view(torch.float8_e4m3fn).float() @ B.view(torch.float8_e4m3fn).float())

    def mfma_check_mx(self, A, B, blocks, fmt):
        if fmt == 0:
            return self.mfma_check_fp8(A, B, blocks)
        lut = torch.tensor(ops._FP4_E2M1_VALUES, dtype=torch.float32)
        return self._tiles(lut[A.long()] @ lut[B.long()])

    def cu_coverage(self, blocks):
        return torch.tensor([hw_word(0)], dtype=torch.int32)

    def lds_check(self, blocks, seed):
        return 0


def test_health_report_skipped_march_does_not_flip_healthy(monkeypatch):
    monkeypatch.setattr(ops, "get_ops", lambda: FakeOps())
    monkeypatch.setattr(torch.cuda, "set_device", lambda d: None)
    monkeypatch.setattr(torch.Tensor, "cuda", lambda self, *a, **k: self)
    calls = []
    march = {}

    def fake_march_report(device=0, **kwargs):
        calls.append(device)
        return dict(march)

    monkeypatch.setattr(ops, "hbm_march_report", fake_march_report)
    plain = ops.gpu_health_report(0, quick=True)
    assert plain["healthy"] is True and "hbm_march" not in plain and calls == []
    # skipped: recorded, never judged (not even with a verdict of False)
    for ok in (True, False):
        march.update(skipped=True, ok=ok)
        rep = ops.gpu_health_report(0, quick=True, hbm_march=True)
        assert rep["hbm_march"] == march and rep["healthy"] is True
        assert set(rep) - set(plain) == {"hbm_march"}
    march.update(skipped=False, ok=False)
    assert ops.gpu_health_report(0, quick=True, hbm_march=True)["healthy"] is False
    march.update(skipped=False, ok=True)
    assert ops.gpu_health_report(0, quick=True, hbm_march=True)["healthy"] is True
    assert calls == [0, 0, 0, 0]


# ---------------------------------------------------------------------------
# agent wiring
# ---------------------------------------------------------------------------
def canned_march(errors=0, slow_rate=None, skipped=False, ok=None):
    xcds = [{"xcc": x, "blocks": 256, "write_gbps": 700.0, "verify_gbps": 650.04 + x}
            for x in (3, 0, 1, 2)]      # deliberately not in XCC order
    if slow_rate is not None:
        xcds[0]["verify_gbps"] = slow_rate
    bad = errors > 0
    return {
        "bytes_tested": 0 if skipped else 16 << 30, "chunks": 0 if skipped else 4,
        "skipped": skipped, "errors": errors, "errors_per_chunk": [errors, 0, 0, 0],
        "dropped_mask": (1 << 63) if bad else 0, "raised_mask": 0x4 if bad else 0,
        "bad_bits": [2, 63] if bad else [],
        "first_bad": {"offset": 2 ** 33 + 8, "pass": 1} if bad else None,
        "bad_locations": [], "coverage_ok": True, "write_gbps": 5400.0, "verify_gbps": 5200.0,
        "xcds": [] if skipped else xcds, "xcds_seen": 0 if skipped else 4, "xcd_ratio": 1.0,
        "slow_xcds": [], "ok": (not bad) if ok is None else ok,
    }


def canned_report(march):
    return {"hbm_gbps": 5000.0, "mfma_ok": True, "cu_coverage": 256, "lds_errors": 0,
            "healthy": bool(march["ok"] or march["skipped"]), "hbm_march": march}


@pytest.fixture()
def agent_health(monkeypatch):
    """collect_node_health over one fake GPU: returns the agent module and a
    dict holding the canned `report` to serve and the `calls` it received."""
    from hivedscheduler_amd.agent import health

    state = {"report": None, "calls": []}

    def fake_report(device=0, **kwargs):
        state["calls"].append(kwargs)
        rep = dict(state["report"])
        if not kwargs.get("hbm_march"):
            rep.pop("hbm_march")
            rep["healthy"] = True
        return rep

    monkeypatch.setattr(ops, "gpu_health_report", fake_report)
    monkeypatch.setattr(health, "_rocm_smi_gpu_state", lambda: {0: True})
    return health, state


def test_agent_march_verdicts(agent_health):
    health, state = agent_health
    state["report"] = canned_report(canned_march())
    g = health.collect_node_health(deep=True, hbm_march=True)["gpus"]["0"]
    assert g["healthy"] is True and g["hbm_march_ok"] is True and g["hbm_march_errors"] == 0
    assert g["hbm_bad_bits"] == [] and g["slow_xcds"] == []
    assert "hbm_first_bad_offset" not in g
    assert g["xcd_gbps"] == [650.0, 651.0, 652.0, 653.0]    # by XCC id, rounded to 0.1
    assert state["calls"][-1]["hbm_march"] is True
    assert "lds_march" not in state["calls"][-1] and "burn" not in state["calls"][-1]
    # a data error fails the GPU and says where and which bits
    state["report"] = canned_report(canned_march(errors=3))
    g = health.collect_node_health(deep=True, hbm_march=True)["gpus"]["0"]
    assert g["healthy"] is False and g["hbm_march_ok"] is False and g["hbm_march_errors"] == 3
    assert g["hbm_bad_bits"] == [2, 63]
    assert g["hbm_first_bad_offset"] == 2 ** 33 + 8 and isinstance(g["hbm_first_bad_offset"], int)
    # a march that failed without a data error (coverage, missing XCD) too
    state["report"] = canned_report(canned_march(ok=False))
    g = health.collect_node_health(deep=True, hbm_march=True)["gpus"]["0"]
    assert g["healthy"] is False and g["hbm_march_ok"] is False and g["hbm_march_errors"] == 0
    # a slow XCD is judged only against a floor the operator gave
    state["report"] = canned_report(canned_march(slow_rate=300.0))
    g = health.collect_node_health(deep=True, hbm_march=True)["gpus"]["0"]
    assert g["healthy"] is True and g["slow_xcds"] == [] and g["xcd_gbps"][3] == 300.0
    g = health.collect_node_health(deep=True, hbm_march=True, min_xcd_ratio=0.8)["gpus"]["0"]
    assert g["healthy"] is False and g["slow_xcds"] == [3] and g["hbm_march_ok"] is False
    g = health.collect_node_health(deep=True, hbm_march=True, min_xcd_ratio=0.4)["gpus"]["0"]
    assert g["healthy"] is True and g["slow_xcds"] == []
    # a skipped march does not mark the leaf bad
    state["report"] = canned_report(canned_march(skipped=True, ok=True))
    g = health.collect_node_health(deep=True, hbm_march=True, min_xcd_ratio=0.8)["gpus"]["0"]
    assert g["healthy"] is True and g["hbm_march_ok"] is True and g["xcd_gbps"] == []


def test_agent_without_march_is_unchanged(agent_health):
    health, state = agent_health
    state["report"] = canned_report(canned_march(errors=3))
    g = health.collect_node_health(deep=True)["gpus"]["0"]
    assert g == {"healthy": True, "hbm_gbps": 5000.0, "mfma_ok": True, "cu_coverage": 256,
                 "lds_errors": 0}
    assert "hbm_march" not in state["calls"][-1]
    # not deep: the kernels do not run at all
    n = len(state["calls"])
    g = health.collect_node_health(deep=False, hbm_march=True)["gpus"]["0"]
    assert g == {"healthy": True} and len(state["calls"]) == n


def test_agent_march_cadence(agent_health, monkeypatch):
    health, state = agent_health
    state["report"] = canned_report(canned_march(errors=1))
    monkeypatch.setattr(health.NodeHealthAgent, "post_report", lambda self, r: True)
    monkeypatch.setattr(health.NodeHealthAgent, "run_placement_probes", lambda self: [])
    monkeypatch.setattr(health, "p2p_link_matrix", lambda: {"matrix": {}, "links": []})
    never = health.NodeHealthAgent("http://x", node_name="n", deep_every=1, probe_pairs=False,
                                   p2p_matrix_every=10 ** 9)
    assert never.hbm_march_every == 0 and never.min_xcd_ratio is None
    assert all("hbm_march_ok" not in never.run_once()["gpus"]["0"] for _ in range(3))
    assert all("hbm_march" not in c for c in state["calls"])
    agent = health.NodeHealthAgent("http://x", node_name="n", deep_every=1, probe_pairs=False,
                                   p2p_matrix_every=10 ** 9, hbm_march_every=2)
    got = [agent.run_once()["gpus"]["0"] for _ in range(4)]
    assert ["xcd_gbps" in g for g in got] == [True, False, True, False]
    assert [g["healthy"] for g in got] == [False, True, False, True]
    # only on deep sweeps: every 2nd round is a march round, every 4th deep
    agent = health.NodeHealthAgent("http://x", node_name="n", deep_every=4, probe_pairs=False,
                                   p2p_matrix_every=10 ** 9, hbm_march_every=2)
    got = [agent.run_once()["gpus"]["0"] for _ in range(6)]
    assert ["xcd_gbps" in g for g in got] == [True, False, False, False, True, False]
    # the agent's floor reaches the verdict
    state["report"] = canned_report(canned_march(slow_rate=300.0))
    agent = health.NodeHealthAgent("http://x", node_name="n", deep_every=1, probe_pairs=False,
                                   p2p_matrix_every=10 ** 9, hbm_march_every=1,
                                   min_xcd_ratio=0.8)
    g = agent.run_once()["gpus"]["0"]
    assert g["slow_xcds"] == [3] and g["healthy"] is False


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
    monkeypatch.setattr(sys, "argv", ["agent", "--local", "--hbm-march", "--min-xcd-ratio", "0.9",
                                      "--no-probe-pairs"])
    cli.main()
    assert seen["hbm_march"] is True and seen["min_xcd_ratio"] == 0.9
    assert json.loads(capsys.readouterr().out) == {"gpus": {}}
    monkeypatch.setattr(sys, "argv", ["agent", "--local", "--no-probe-pairs"])
    cli.main()
    assert seen["hbm_march"] is False and seen["min_xcd_ratio"] is None

    made = {}

    class FakeAgent:
        def __init__(self, url, **kwargs):
            made.update(kwargs)

        def run_once(self):
            return {}

    monkeypatch.setattr(health, "NodeHealthAgent", FakeAgent)
    monkeypatch.setattr(sys, "argv", ["agent", "--scheduler", "http://x", "--once",
                                      "--hbm-march-every", "6", "--min-xcd-ratio", "0.85"])
    cli.main()
    assert made["hbm_march_every"] == 6 and made["min_xcd_ratio"] == 0.85
    monkeypatch.setattr(sys, "argv", ["agent", "--scheduler", "http://x", "--once"])
    cli.main()
    assert made["hbm_march_every"] == 0 and made["min_xcd_ratio"] is None


def test_march_keys_reach_the_inspect_view():
    from hivedscheduler_amd.scheduler import HivedScheduler
    from hivedscheduler_amd.sim import mi355x_cluster_config

    sched = HivedScheduler(mi355x_cluster_config(num_nodes=1))
    node = sched.algorithm.all_nodes()[0]
    sched.on_node_add({"metadata": {"name": node, "uid": "n1"}, "spec": {},
                       "status": {"conditions": [{"type": "Ready", "status": "True"}]}})
    gpu_report = {"healthy": False, "hbm_march_ok": False, "hbm_march_errors": 3,
                  "hbm_bad_bits": [2, 63], "hbm_first_bad_offset": 2 ** 33 + 8,
                  "xcd_gbps": [650.0, 651.0, 300.0, 653.0], "slow_xcds": [2]}
    assert sched.on_health_report(node, {"gpus": {"5": dict(gpu_report)}})["applied"] == {"5": False}

    def leaves(c):
        kids = c.get("cellChildren") or []
        return [c] if not kids else [l for k in kids for l in leaves(k)]

    status = sched.get_physical_cluster_status()
    unhealthy = [c for c in leaves(status[0]) if c.get("cellHealthiness") != "Healthy"]
    assert len(unhealthy) == 1, [c.get("cellAddress") for c in unhealthy]
    gpu = sched.get_health_reports()[node]["gpus"]["5"]
    for key, value in gpu_report.items():
        assert gpu[key] == value, key
