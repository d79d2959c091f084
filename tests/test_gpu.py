"""GPU tests (real MI355X, run via gpurun): HIP kernel numerics vs plain
PyTorch fp32 references, health probes, RCCL cell probe, end-to-end smoke."""
import json
import os
import subprocess
import sys

import pytest

torch = pytest.importorskip("torch")

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

needs_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")


# The one inexact MFMA case: bf16 randn/4 against a ramp has 16-bit products at
# many exponents, so fp32 cannot hold the sum exactly and the result depends on
# how the pipe accumulates. Per element, |tile - float64 product| must stay
# within BF16_RANDN_C * 2^-24 * (|A| @ |B|). Any-order fp32 accumulation with
# truncation would give about 2K = 64; the constant is the next power of two
# above four times the largest ratio measured on an MI355X over seeds 0..31
# (BF16_RANDN_MEASURED_RATIO, BENCHMARKS.md), the kernel being deterministic
# and the margin covering only the variation between seeds.
BF16_RANDN_MEASURED_RATIO = 0.782   # seed 7 itself: 0.339
BF16_RANDN_C = 4


def bf16_randn_operands(seed=7):
    """(A, B) bf16 on the CPU; asymmetric B catches transposed C-write layouts."""
    g = torch.Generator().manual_seed(seed)
    A = (torch.randn(16, 32, generator=g) / 4).bfloat16()
    B = (torch.arange(32 * 16, dtype=torch.float32).reshape(32, 16) / 997 - 0.25).bfloat16()
    return A, B


def bf16_error_ratio(tiles, A, B):
    """max over waves and elements of |tile - float64 product| in units of
    2^-24 * (|A| @ |B|)."""
    a, b = A.double().cpu(), B.double().cpu()
    unit = (a.abs() @ b.abs()) * 2.0 ** -24
    return ((tiles.double().cpu() - (a @ b).unsqueeze(0)).abs() / unit.unsqueeze(0)).max().item()


def assert_all_waves_equal(tiles, expected, what):
    """Every wave's tile equals the float64-derived one: no tolerance."""
    tiles = tiles.cpu()
    assert tiles.shape[1:] == expected.shape
    wrong = tiles != expected.unsqueeze(0)
    assert not wrong.any(), (
        f"{what}: {int(wrong.sum())} elements in {int(wrong.any(-1).any(-1).sum())} of "
        f"{tiles.shape[0]} waves differ, max |err| {(tiles - expected).abs().max().item()}")
    assert torch.equal(tiles, expected.expand_as(tiles))


@needs_gpu
def test_mfma_numerics_vs_fp32():
    """MFMA bf16 tile GEMM on inexact inputs vs a float64 reference of the
    same op, every wave, within the relative per-element bound above."""
    from hivedscheduler_amd.ops import get_ops

    ops = get_ops()
    A, B = bf16_randn_operands()
    tiles = ops.mfma_check(A.cuda(), B.cuda(), 64, 1)
    ratio = bf16_error_ratio(tiles, A, B)
    print(f"bf16 randn/4 error ratio {ratio} (bound {BF16_RANDN_C})")
    assert ratio <= BF16_RANDN_C, f"MFMA result deviates from float64 reference: ratio {ratio}"
    # every wave on every CU must produce the identical tile
    spread = (tiles - tiles[0].unsqueeze(0)).abs().max().item()
    assert spread == 0.0, f"cross-CU MFMA mismatch: {spread}"


@needs_gpu
def test_mfma_identity():
    """A = I (padded) recovers B's rows exactly."""
    from hivedscheduler_amd.ops import get_ops

    ops = get_ops()
    A = torch.zeros(16, 32)
    for i in range(16):
        A[i, i] = 1.0
    B = (torch.randn(32, 16) / 4)
    tiles = ops.mfma_check(A.bfloat16().cuda(), B.bfloat16().cuda(), 8, 1)
    assert_all_waves_equal(tiles, B.bfloat16().float()[:16], "identity check")


@needs_gpu
def test_mfma_fp8_numerics_vs_fp32():
    """fp8 e4m3 MFMA (v_mfma_f32_16x16x32_fp8_fp8) vs the float64 product
    decoded from the same raw e4m3 bytes, which fp32 holds exactly (sum
    |a||b| < 64 in multiples of 2^-18) and which stays inside the window the
    fp8 pipes keep (e4m3_within_group_window); exercises the CDNA4
    low-precision pipes the bf16 check cannot see."""
    from hivedscheduler_amd.ops import e4m3_within_group_window, exact_tile, get_ops

    ops = get_ops()
    torch.manual_seed(11)
    A8 = (torch.randn(16, 32) / 8).to(torch.float8_e4m3fn).view(torch.uint8)
    # asymmetric B catches transposed C-write layouts
    B8 = ((torch.arange(32 * 16, dtype=torch.float32).reshape(32, 16) / 997 - 0.25)
          .to(torch.float8_e4m3fn).view(torch.uint8))
    # bitwise only because no product falls below the window the pipe keeps
    assert e4m3_within_group_window("fp8", A8, B8).all()
    tiles = ops.mfma_check_fp8(A8.cuda(), B8.cuda(), 64)
    assert_all_waves_equal(tiles, exact_tile("fp8", A8, B8), "fp8 MFMA")


@needs_gpu
def test_mfma_mx_fp8_numerics_vs_fp32():
    """MX block-scaled fp8 (v_mfma_f32_16x16x128_f8f6f4, fmt=0, unit scales)
    vs the exact float64 product — the instruction behind the ~5 PF fp8
    headline rate."""
    from hivedscheduler_amd.ops import e4m3_within_group_window, exact_tile, get_ops

    ops = get_ops()
    torch.manual_seed(12)
    A8 = (torch.randn(16, 128) / 16).to(torch.float8_e4m3fn).view(torch.uint8)
    B8 = ((torch.arange(128 * 16, dtype=torch.float32).reshape(128, 16) / 4093 - 0.25)
          .to(torch.float8_e4m3fn).view(torch.uint8))
    assert e4m3_within_group_window("mx8", A8, B8).all()
    tiles = ops.mfma_check_mx(A8.cuda(), B8.cuda(), 64, 0)
    assert_all_waves_equal(tiles, exact_tile("mx8", A8, B8), "MX fp8 MFMA")


@needs_gpu
def test_mfma_mx_fp4_numerics_exact():
    """MX fp4 (e2m1 codes, fmt=4, unit scales): all products are multiples of
    0.25 with sums << 2^24, so the float64 product must match bit-for-bit."""
    from hivedscheduler_amd.ops import exact_tile, get_ops

    ops = get_ops()
    g = torch.Generator().manual_seed(13)
    A4 = torch.randint(0, 16, (16, 128), generator=g, dtype=torch.uint8)
    B4 = torch.randint(0, 16, (128, 16), generator=g, dtype=torch.uint8)
    tiles = ops.mfma_check_mx(A4.cuda(), B4.cuda(), 64, 4)
    assert_all_waves_equal(tiles, exact_tile("mx4", A4, B4), "MX fp4 MFMA")


@needs_gpu
def test_health_report_includes_lowprec():
    from hivedscheduler_amd.ops import gpu_health_report

    rep = gpu_health_report(0, quick=True)
    assert rep["mfma_fp8_ok"] and rep["mfma_mx8_ok"] and rep["mfma_fp4_ok"], rep
    assert rep["mfma_fp8_cross_cu_spread"] == 0.0
    assert rep["mfma_fp4_cross_cu_spread"] == 0.0
    assert rep["mfma_lowprec_ok"] and rep["healthy"]


@needs_gpu
def test_hbm_bandwidth_sane():
    from hivedscheduler_amd.ops import get_ops

    ops = get_ops()
    gbps = ops.hbm_triad_gbps(512, 5)
    # MI355X HBM3E: ~8 TB/s peak, ~6.3 achievable; anything below 2 TB/s on a
    # streaming triad means a sick GPU (or wrong kernel)
    assert gbps > 2000, f"HBM triad bandwidth too low: {gbps} GB/s"
    assert gbps < 10000, f"HBM triad bandwidth implausibly high: {gbps} GB/s"


@needs_gpu
def test_gpu_health_report():
    from hivedscheduler_amd.ops import gpu_health_report

    rep = gpu_health_report(0, quick=True)
    assert rep["healthy"], rep
    assert rep["mfma_cross_cu_spread"] == 0.0


@needs_gpu
def test_device_info_is_gfx950():
    from hivedscheduler_amd.ops import get_ops

    info = get_ops().device_info(0)
    assert "gfx950" in info["gcnArchName"], info
    assert info["warpSize"] == 64


@needs_gpu
def test_rccl_cell_probe_binary():
    from hivedscheduler_amd.probe import CellProbeRunner

    runner = CellProbeRunner()
    assert runner.available(), f"native probe binary missing at {runner.binary}"
    res = runner.probe_cell([0], size_mb=16, iters=3)
    assert res["ok"], res
    assert res["ndev"] == 1
    # single-device probe flags itself as an HBM copy, not an xGMI number
    assert res["hbm_copy"] is True
    if torch.cuda.device_count() >= 2:
        multi = runner.probe_cell([0, 1], size_mb=16, iters=3, p2p_matrix=True)
        assert multi["ok"] and multi["hbm_copy"] is False, multi
        assert "0-1" in multi.get("p2p_matrix", {}), multi


@needs_gpu
def test_rocm_topo_discover():
    """Discovery emits measured facts (VRAM, link table) and the output is
    consumed end-to-end: YAML -> Config -> live core with link state."""
    from hivedscheduler_amd.sim import SimScheduler
    from hivedscheduler_amd.topo.discover import (
        cluster_config_from_discovery,
        parse_discovery_output,
    )

    binary = os.path.join(REPO, "native", "rocm-topo-discover")
    assert os.path.exists(binary)
    out = subprocess.run([binary, "--node-name", "testnode"], capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 0, out.stderr
    assert "nodeName: testnode" in out.stdout
    assert "physicalCells:" in out.stdout
    doc = parse_discovery_output(out.stdout)
    n = int(doc["numGpus"])
    assert doc["gpus"][0]["vramBytes"] > 200 * 1024 ** 3, "measured VRAM missing"
    if n >= 2:
        # the measured per-link table is present and parses into core state
        links_yaml = doc["physicalCells"][0].get("xgmiLinks") or []
        assert links_yaml, "xgmiLinks table missing from discovery output"
        if n == 8:
            cfg = cluster_config_from_discovery([doc])
            sim = SimScheduler(cfg)
            links = sim.alg.get_xgmi_links("testnode")
            assert len(links) == 28, f"8-GPU full mesh should have 28 links: {len(links)}"
            assert all(l["healthy"] for l in links)
            sim.alg._core.check_invariants()


@needs_gpu
def test_smoke_entry():
    sys.path.insert(0, REPO)
    import __graft_entry__ as ge

    ge.smoke()


@needs_gpu
def test_bench_on_gpu():
    out = subprocess.run([sys.executable, "bench.py", "--steps", "3", "--warmup", "1", "--full"],
                         capture_output=True, text=True, timeout=600, cwd=REPO)
    assert out.returncode == 0, out.stderr[-3000:]
    result = json.loads(out.stdout.strip().splitlines()[-1])
    assert result["config"]["vc_safety_violations"] == 0
    # 1-GPU run: the local-copy probe is reported as hbm_copy_gbps (an HBM
    # health floor); rccl_busbw_gbps carries only true multi-GPU xGMI numbers
    assert result["config"]["hbm_copy_gbps"], "expected an HBM copy measurement on GPU"
    assert result["config"]["rccl_busbw_gbps"] == {}


@needs_gpu
def test_hbm_pattern_sweep():
    """Stuck-bit sweep over 8 GiB: zero errors on healthy HBM, bandwidth in
    the HBM class (not cache-resident: chunk 4 GiB >> 512 MB Infinity Cache)."""
    from hivedscheduler_amd.ops import get_ops

    ops = get_ops()
    r = ops.hbm_sweep(8, 4, 12345)
    assert r["bytes_tested"] == 8 << 30
    assert r["errors"] == 0, f"HBM corruption detected: {r}"
    assert r["write_gbps"] > 500 and r["verify_gbps"] > 500, r


@needs_gpu
def test_health_report_deep():
    from hivedscheduler_amd.ops import gpu_health_report

    rep = gpu_health_report(0, quick=True, deep=True)
    assert rep["hbm_sweep"]["errors"] == 0
    assert rep["healthy"]


@needs_gpu
def test_agent_end_to_end_on_hardware():
    """Hardware-in-the-loop: the node agent collects REAL GPU health (HIP
    kernels incl. the stuck-bit sweep) over the live uvicorn extender server;
    the scheduler applies it to the cell tree and serves it via inspect."""
    import socket
    import threading
    import time as _time

    import requests
    import uvicorn

    from hivedscheduler_amd.agent.health import NodeHealthAgent, collect_node_health
    from hivedscheduler_amd.scheduler import HivedScheduler
    from hivedscheduler_amd.sim import mi355x_cluster_config
    from hivedscheduler_amd.webserver import create_app

    node = socket.gethostname()
    # simulated view of this box as node "<hostname>" (1 node x 8 GPUs)
    sched = HivedScheduler(mi355x_cluster_config(num_nodes=1, node_prefix=""))
    # rename: config names the node ""+"1"; map hostname via health intake only
    first_node = sched.algorithm.all_nodes()[0]
    sched.on_node_add({"metadata": {"name": first_node, "uid": "n1"}, "spec": {},
                       "status": {"conditions": [{"type": "Ready", "status": "True"}]}})

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    server = uvicorn.Server(uvicorn.Config(create_app(sched), host="127.0.0.1",
                                           port=port, log_level="error"))
    th = threading.Thread(target=server.run, daemon=True)
    th.start()
    for _ in range(100):
        if server.started:
            break
        _time.sleep(0.05)
    try:
        # real kernels: deep + stuck-bit sweep (bounded 16 GiB)
        report = collect_node_health(deep=True, sweep=True)
        assert report["gpus"], report
        g0 = report["gpus"]["0"]
        assert g0["mfma_ok"] and g0["hbm_gbps"] > 2000, g0
        assert g0.get("hbm_sweep_errors", 0) == 0, g0
        # post as the agent does, against the node name the scheduler knows
        agent = NodeHealthAgent(f"http://127.0.0.1:{port}", node_name=first_node)
        assert agent.post_report(report)
        served = requests.get(f"http://127.0.0.1:{port}/v1/inspect/health",
                              timeout=10).json()
        assert first_node in served
        assert served[first_node]["gpus"]["0"]["mfma_ok"] is True
        # a degraded-GPU report marks the leaf bad in the live cell tree
        bad = {"gpus": {"5": {"healthy": False, "mfma_ok": False}}}
        r = requests.post(f"http://127.0.0.1:{port}/v1/health/nodes/{first_node}",
                          json=bad, timeout=10)
        assert r.status_code == 200 and r.json()["applied"] == {"5": False}
        from hivedscheduler_amd.sim import SimScheduler  # noqa: F401  (import check)
        status = sched.get_physical_cluster_status()
        def leaves(c):
            kids = c.get("cellChildren") or []
            return [c] if not kids else [l for k in kids for l in leaves(k)]
        unhealthy = [c for c in leaves(status[0]) if c.get("cellHealthiness") != "Healthy"]
        assert len(unhealthy) == 1, [c.get("cellAddress") for c in unhealthy]
    finally:
        server.should_exit = True
        th.join(timeout=5)


@needs_gpu
def test_cu_coverage_all_256():
    """The coverage grid must place waves on every CU of every XCD: 256
    distinct (xcc, se, sh, cu) tuples on MI355X (8 XCDs x 32 CUs)."""
    from hivedscheduler_amd.ops import get_ops

    ops = get_ops()
    words = ops.cu_coverage(4096).cpu().numpy()
    xccs = {int(w) >> 16 for w in words}
    cus = {(int(w) >> 16, (int(w) >> 13) & 0x7, (int(w) >> 12) & 0x1, (int(w) >> 8) & 0xF)
           for w in words}
    n = get_ops().device_info(0)["multiProcessorCount"]
    assert len(xccs) == 8, f"XCDs covered: {sorted(xccs)}"
    assert len(cus) >= n, f"CUs covered: {len(cus)} < {n}"


@needs_gpu
def test_lds_check_clean():
    """LDS slab write/read-verify across the chip: zero errors on healthy
    hardware, and the full health report includes it."""
    from hivedscheduler_amd.ops import get_ops, gpu_health_report

    assert get_ops().lds_check(2048, 99) == 0
    rep = gpu_health_report(0, quick=True)
    assert rep["lds_errors"] == 0 and rep["healthy"]
