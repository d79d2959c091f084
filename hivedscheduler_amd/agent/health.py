"""Node health agent (DaemonSet-style): grounds cell healthiness in measured
CDNA4 facts and reports GPU-level health to the scheduler.

Per SURVEY.md §2.2, this replaces the reference's K8s-NodeReady-only health
signal with: rocm-smi device state, HIP health-probe kernels (HBM bandwidth,
MFMA verification), and the RCCL xGMI pair probe. Degraded xGMI links mark
the PAIR cell bad (via its endpoint leaf), not the whole node.

Runs on each GPU node: `python -m hivedscheduler_amd.agent --scheduler URL`.
Reports POST to the scheduler's /v1/health/nodes/{node} endpoint:
  {"gpus": {"0": {"healthy": true, ...}, ...}}
"""
from __future__ import annotations

import json
import logging
import os
import socket
import subprocess
import time
from typing import Dict, List, Optional

log = logging.getLogger("hivedscheduler.agent")


def _rocm_smi_gpu_state() -> Dict[int, bool]:
    """GPU liveness via rocm-smi JSON (a GPU missing or erroring is bad)."""
    try:
        out = subprocess.run(["rocm-smi", "--showuse", "--json"], capture_output=True,
                             text=True, timeout=60)
        if out.returncode != 0:
            return {}
        data = json.loads(out.stdout)
        state = {}
        for key in data:
            if key.lower().startswith("card"):
                idx = int(key[4:])
                state[idx] = True
        return state
    except Exception as e:
        log.warning("rocm-smi query failed: %s", e)
        return {}


def _set_flags(**flags) -> dict:
    """The set flags as keyword arguments; none set leaves a call as it was."""
    return {name: True for name, on in flags.items() if on}


def collect_node_health(
    deep: bool = False,
    min_hbm_gbps: float = 2000.0,
    min_pair_busbw_gbps: float = 50.0,
    probe_pairs: bool = False,
    sweep: bool = False,
    burn: bool = False,
    min_mfma_tflops: Optional[float] = None,
    lds_march: bool = False,
    hbm_march: bool = False,
    min_xcd_ratio: Optional[float] = None,
    simd_probe: bool = False,
    scalar_probe: bool = False,
    atomic_probe: bool = False,
) -> dict:
    """One health sweep over all visible GPUs. deep=True also runs the HIP
    kernels (HBM + MFMA); sweep=True adds the 16 GiB HBM stuck-bit pattern
    sweep (any error => leaf bad); probe_pairs=True RCCL-probes each xGMI
    pair.

    burn=True (with deep) adds the sustained MFMA burn-in: per GPU it records
    `mfma_tflops` ({fmt: TFLOP/s}), `mfma_burn_ok` and `bad_cus` (the CUs of
    any wave whose result was wrong), and a failed burn marks the leaf bad.
    min_mfma_tflops is a floor on the bf16 figure; there is no default
    because the right value is site-measured (docs/user-manual.md).

    lds_march=True (with deep) adds the full-LDS march: per GPU it records
    `lds_march_ok`, `lds_gbps` (reported, not judged: there is no floor) and
    `lds_bad_cus` (the CUs whose LDS read back wrong; a key of its own, so
    `bad_cus` keeps meaning the burn-in's), and a failed march marks the leaf
    bad.

    hbm_march=True (with deep) adds the HBM march (both bit polarities, 16 B
    accesses, fault location, bandwidth per XCD): per GPU it records
    `hbm_march_ok`, `hbm_march_errors`, `hbm_bad_bits`,
    `hbm_first_bad_offset` (absent when nothing was wrong), `xcd_gbps` (the
    verify rate of each XCD, ordered by XCC id) and `slow_xcds`. A failed
    march marks the leaf bad; one skipped for lack of free memory does not.
    min_xcd_ratio marks a GPU bad when one XCD reads below that fraction of
    the median XCD; there is no default because the healthy spread is
    site-measured (docs/user-manual.md). Like the stuck-bit scan it holds up
    to 16 GiB while it runs, and the same warning applies.

    simd_probe=True (with deep) adds the SIMD probe (the exact VALU burn and
    the register-file march): per GPU it records `simd_probe_ok`,
    `valu_burn_ok`, `vgpr_march_ok` and `bad_simds` (the SIMDs of any wave
    that computed or read back wrong, as xcc, se, sh, cu, simd; a key of its
    own beside `bad_cus` and `lds_bad_cus`), and a failed probe marks the
    leaf bad. The march holds every SIMD's whole register file for about a
    millisecond, during which tenant waves wait.

    scalar_probe=True (with deep) adds the scalar probe (the exact SALU burn,
    the SGPR march and the scalar-load check): per GPU it records
    `scalar_probe_ok`, `salu_burn_ok`, `sgpr_march_ok`, `scalar_load_ok` and
    `scalar_bad_simds` (the SIMDs of any wave that computed, read back or
    loaded wrong, as xcc, se, sh, cu, simd; a key of its own beside
    `bad_simds`), and a failed probe marks the leaf bad.

    atomic_probe=True (with deep) adds the atomic probe (the exact atomic burn
    on cells each lane owns and the contended ticket, reduce and cmpswap
    sections on shared cells): per GPU it records `atomic_probe_ok`,
    `atomic_burn_ok`, `atomic_contend_ok`, `atomic_bad_cus` (the CUs of any
    wave whose atomics returned or left a wrong value, as xcc, se, sh, cu; a
    key of its own beside `bad_cus` and `lds_bad_cus`) and `atomic_bad_cells`
    (the shared cells that ended wrong, as cell, section, op), and a failed
    probe marks the leaf bad.

    The stuck-bit scan transiently holds up to 16 GiB of HBM; on a GPU
    running tenant jobs this can make the tenant's own allocations fail.
    Keep sweep on the low-frequency cadence and prefer idle GPUs (the
    scheduler knows which leaves are unallocated).
    """
    report: dict = {"node": socket.gethostname(), "time": time.time(), "gpus": {}}
    alive = _rocm_smi_gpu_state()
    try:
        import torch

        n = torch.cuda.device_count() if torch.cuda.is_available() else 0
    except Exception:
        n = 0
    n = max(n, len(alive))
    for i in range(n):
        gpu = {"healthy": alive.get(i, True)}
        report["gpus"][str(i)] = gpu
    if deep and n > 0:
        from ..ops import gpu_health_report, hbm_slow_xcds

        kwargs = _set_flags(burn=burn, lds_march=lds_march, hbm_march=hbm_march,
                            simd_probe=simd_probe, scalar_probe=scalar_probe,
                            atomic_probe=atomic_probe)
        for i in range(n):
            gpu = report["gpus"][str(i)]
            try:
                # best-of-3 bandwidth: a tenant job on the GPU can halve a
                # single triad sample (see profiles/interference_r01.md)
                rep = gpu_health_report(i, quick=True, deep=sweep, bw_samples=3, **kwargs)
                gpu.update(
                    hbm_gbps=round(rep["hbm_gbps"], 1),
                    mfma_ok=rep["mfma_ok"],
                    cu_coverage=rep["cu_coverage"],
                    lds_errors=rep["lds_errors"],
                )
                if "hbm_sweep" in rep:
                    gpu["hbm_sweep_errors"] = rep["hbm_sweep"]["errors"]
                if not rep["healthy"] or rep["hbm_gbps"] < min_hbm_gbps:
                    gpu["healthy"] = False
                if burn:
                    b = rep["mfma_burn"]
                    tflops = {f: round(s["tflops"], 1) for f, s in b["formats"].items()}
                    gpu.update(
                        mfma_tflops=tflops,
                        mfma_burn_ok=bool(b["ok"]),
                        bad_cus=b["bad_cus"],
                    )
                    bf16 = b["formats"].get("bf16", {}).get("tflops", 0.0)
                    slow = min_mfma_tflops is not None and bf16 < min_mfma_tflops
                    if not b["ok"] or b["bad_cus"] or slow:
                        gpu["healthy"] = False
                if lds_march:
                    m = rep["lds_march"]
                    gpu.update(
                        lds_march_ok=bool(m["ok"]),
                        lds_gbps=round(m["gbps"], 1),
                        lds_bad_cus=[{k: c[k] for k in ("xcc", "se", "sh", "cu")}
                                     for c in m["bad_cus"]],
                    )
                    if not m["ok"] or m["bad_cus"]:
                        gpu["healthy"] = False
                if hbm_march:
                    h = rep["hbm_march"]
                    slow = hbm_slow_xcds(h["xcds"], min_xcd_ratio)
                    gpu.update(
                        hbm_march_ok=bool(h["ok"] and not slow),
                        hbm_march_errors=int(h["errors"]),
                        hbm_bad_bits=list(h["bad_bits"]),
                        xcd_gbps=[round(x["verify_gbps"], 1)
                                  for x in sorted(h["xcds"], key=lambda x: x["xcc"])],
                        slow_xcds=slow,
                    )
                    if h["first_bad"] is not None:
                        gpu["hbm_first_bad_offset"] = int(h["first_bad"]["offset"])
                    if not h["skipped"] and (not h["ok"] or slow):
                        gpu["healthy"] = False
                if simd_probe:
                    p = rep["simd_probe"]
                    gpu.update(
                        simd_probe_ok=bool(p["ok"]),
                        valu_burn_ok=bool(p["valu"]["ok"]),
                        vgpr_march_ok=bool(p["vgpr_march"]["ok"]),
                        bad_simds=[{k: c[k] for k in ("xcc", "se", "sh", "cu", "simd")}
                                   for c in p["bad_simds"]],
                    )
                    if not p["ok"] or p["bad_simds"]:
                        gpu["healthy"] = False
                if scalar_probe:
                    p = rep["scalar_probe"]
                    gpu.update(
                        scalar_probe_ok=bool(p["ok"]),
                        salu_burn_ok=bool(p["salu"]["ok"]),
                        sgpr_march_ok=bool(p["sgpr_march"]["ok"]),
                        scalar_load_ok=bool(p["scalar_load"]["ok"]),
                        scalar_bad_simds=[{k: c[k] for k in ("xcc", "se", "sh", "cu", "simd")}
                                          for c in p["bad_simds"]],
                    )
                    if not p["ok"] or p["bad_simds"]:
                        gpu["healthy"] = False
                if atomic_probe:
                    p = rep["atomic_probe"]
                    gpu.update(
                        atomic_probe_ok=bool(p["ok"]),
                        atomic_burn_ok=bool(p["burn"]["ok"]),
                        atomic_contend_ok=bool(p["contend"]["ok"]),
                        atomic_bad_cus=[{k: c[k] for k in ("xcc", "se", "sh", "cu")}
                                        for c in p["bad_cus"]],
                        atomic_bad_cells=[{k: c[k] for k in ("cell", "section", "op")}
                                          for c in p["bad_cells"]],
                    )
                    if not p["ok"] or p["bad_cus"] or p["bad_cells"]:
                        gpu["healthy"] = False
            except Exception as e:
                gpu.update(healthy=False, error=str(e)[:200])
    if probe_pairs and n >= 2:
        from ..probe import CellProbeRunner

        runner = CellProbeRunner(min_busbw_gbps=min_pair_busbw_gbps)
        if runner.available():
            report["pairs"] = {}
            links = []
            for p in range(n // 2):
                pair = [2 * p, 2 * p + 1]
                try:
                    res = runner.probe_cell(pair, size_mb=64, iters=10)
                    report["pairs"][f"{pair[0]}-{pair[1]}"] = res
                    if res.get("ok"):
                        # first-class LINK report: a degraded xGMI link marks
                        # the link (scheduler avoids co-placing the endpoints)
                        # while both GPUs stay schedulable for 1-GPU work
                        links.append({"a": pair[0], "b": pair[1],
                                      "healthy": bool(res.get("healthy", True)),
                                      "gbps": float(res.get("busbw_gbps") or 0.0)})
                except Exception as e:
                    report["pairs"][f"{pair[0]}-{pair[1]}"] = {"ok": False, "error": str(e)[:200]}
            if links:
                report["links"] = links
    return report


def p2p_link_matrix(n: Optional[int] = None, size_mb: int = 64, iters: int = 5,
                    min_link_gbps: float = 40.0) -> dict:
    """Measure the full xGMI p2p bandwidth matrix with the HIP copy kernel
    (ops.p2p_gbps) and derive per-link health. This is the cheapest way to
    localize a degraded link to ONE pair when a >=4-GPU collective probe
    reads low: every GPU pair on an 8x MI355X node is directly connected
    (7 links x ~153 GB/s per direction), so matrix[i][j] well below the
    floor indicts exactly link i<->j.

    Returns {"matrix": {"i-j": gbps}, "links": [{a, b, gbps, healthy}]}
    shaped for the scheduler's /v1/health/nodes intake.
    """
    import torch

    from ..ops import get_ops

    ops = get_ops()
    count = n if n is not None else (torch.cuda.device_count() if torch.cuda.is_available() else 0)
    out: dict = {"matrix": {}, "links": []}
    for i in range(count):
        for j in range(i + 1, count):
            try:
                # per-direction copies; a link is as sick as its worse direction
                fwd = ops.p2p_gbps(i, j, size_mb, iters)
                rev = ops.p2p_gbps(j, i, size_mb, iters)
                gbps = min(fwd, rev)
            except Exception as e:
                log.warning("p2p probe %d<->%d failed: %s", i, j, e)
                out["links"].append({"a": i, "b": j, "healthy": False, "gbps": 0.0,
                                     "error": str(e)[:200]})
                continue
            out["matrix"][f"{i}-{j}"] = round(gbps, 1)
            out["links"].append({"a": i, "b": j, "healthy": bool(gbps >= min_link_gbps),
                                 "gbps": round(gbps, 1)})
    return out


class NodeHealthAgent:
    """Periodic health loop posting reports to the scheduler."""

    def __init__(self, scheduler_url: str, node_name: Optional[str] = None,
                 interval_s: float = 60.0, deep_every: int = 10,
                 sweep_every: int = 60, probe_pairs: bool = True,
                 p2p_matrix_every: int = 30, burn_every: int = 0,
                 min_mfma_tflops: Optional[float] = None, lds_march_every: int = 0,
                 hbm_march_every: int = 0, min_xcd_ratio: Optional[float] = None,
                 simd_probe_every: int = 0, scalar_probe_every: int = 0,
                 atomic_probe_every: int = 0):
        self.scheduler_url = scheduler_url.rstrip("/")
        self.node_name = node_name or socket.gethostname()
        self.interval_s = interval_s
        self.deep_every = deep_every
        # stuck-bit HBM sweep cadence (GPU must be idle-ish; 16 GiB ~ 5 s/GPU)
        self.sweep_every = sweep_every
        # pair probes default ON: the xGMI checks are the point of the agent
        self.probe_pairs = probe_pairs
        # full p2p matrix cadence (28 pairs x 2 directions, ~1 min on 8 GPUs):
        # localizes a degraded link to one pair when collective probes read low
        self.p2p_matrix_every = p2p_matrix_every
        # sustained MFMA burn-in cadence, same pattern as sweep_every; 0 = never
        # (four formats x tens of ms per GPU, and it saturates the matrix
        # cores of a GPU a tenant may be using)
        self.burn_every = burn_every
        self.min_mfma_tflops = min_mfma_tflops
        # full-LDS march cadence, same pattern; 0 = never (about a millisecond
        # per GPU, but it takes every CU's whole LDS while it runs)
        self.lds_march_every = lds_march_every
        # HBM march cadence, same pattern; 0 = never. Like the stuck-bit sweep
        # it transiently holds up to 16 GiB of HBM (and takes about four times
        # as long: two polarities, written and verified), which on a GPU
        # running tenant jobs can make the tenant's own allocations fail:
        # keep it on a low-frequency cadence and prefer idle GPUs
        self.hbm_march_every = hbm_march_every
        self.min_xcd_ratio = min_xcd_ratio
        # SIMD probe cadence (VALU burn + register-file march), same pattern;
        # 0 = never (tens of milliseconds per GPU, and the march takes every
        # SIMD's whole register file for about one of them)
        self.simd_probe_every = simd_probe_every
        # scalar probe cadence (SALU burn + SGPR march + scalar-load check),
        # same pattern; 0 = never (tens of milliseconds per GPU, during which
        # it keeps every CU's scalar unit busy)
        self.scalar_probe_every = scalar_probe_every
        # atomic probe cadence (atomic burn + contended sections), same
        # pattern; 0 = never (tens of milliseconds per GPU, during which the
        # contended sections load the L2 and memory-side atomic units of
        # every XCD)
        self.atomic_probe_every = atomic_probe_every
        self._rounds = 0

    def post_report(self, report: dict) -> bool:
        import requests

        url = f"{self.scheduler_url}/v1/health/nodes/{self.node_name}"
        try:
            r = requests.post(url, json=report, timeout=30)
            return r.status_code < 300
        except Exception as e:
            log.warning("health report post failed: %s", e)
            return False

    def run_placement_probes(self) -> List[dict]:
        """Poll post-bind probe tasks for this node, run the native RCCL
        probe over each placement's GPUs, and post the results back."""
        import requests

        from ..probe import CellProbeRunner

        url = f"{self.scheduler_url}/v1/health/probes/{self.node_name}"
        try:
            tasks = requests.get(url, timeout=30).json()
        except Exception as e:
            log.warning("probe poll failed: %s", e)
            return []
        runner = CellProbeRunner()
        results = []
        for task in tasks:
            cells = [int(i) for i in task.get("leafCellIndices", [])]
            if runner.available():
                res = runner.probe_cell(cells, size_mb=64, iters=10)
            else:
                res = {"ok": False, "error": "rccl-cell-probe binary missing"}
            res.update(group=task.get("group", ""), node=self.node_name,
                       leafCellIndices=cells)
            try:
                requests.post(f"{self.scheduler_url}/v1/health/probes", json=res, timeout=30)
            except Exception as e:
                log.warning("probe result post failed: %s", e)
            results.append(res)
        return results

    def _due(self, every: int) -> bool:
        """Is a cadence of one in `every` rounds due this round? 0 = never."""
        return every > 0 and (self._rounds % every) == 0

    def run_once(self) -> dict:
        deep = (self._rounds % self.deep_every) == 0
        sweep = self._due(self.sweep_every)
        matrix = (self._rounds % self.p2p_matrix_every) == 0
        # the opt-in probes ride on the deep rounds
        kwargs = _set_flags(burn=deep and self._due(self.burn_every),
                            lds_march=deep and self._due(self.lds_march_every),
                            hbm_march=deep and self._due(self.hbm_march_every),
                            simd_probe=deep and self._due(self.simd_probe_every),
                            scalar_probe=deep and self._due(self.scalar_probe_every),
                            atomic_probe=deep and self._due(self.atomic_probe_every))
        self._rounds += 1
        if "burn" in kwargs:
            kwargs["min_mfma_tflops"] = self.min_mfma_tflops
        if "hbm_march" in kwargs:
            kwargs["min_xcd_ratio"] = self.min_xcd_ratio
        report = collect_node_health(deep=deep, probe_pairs=self.probe_pairs and deep,
                                     sweep=sweep and deep, **kwargs)
        report["node"] = self.node_name
        if matrix and deep:
            try:
                m = p2p_link_matrix()
                if m["links"]:
                    report["p2p_matrix"] = m["matrix"]
                    # matrix verdicts override pair-probe verdicts (finer)
                    report["links"] = m["links"]
            except Exception as e:
                log.warning("p2p matrix sweep failed: %s", e)
        self.post_report(report)
        report["placement_probes"] = self.run_placement_probes()
        return report

    def run_forever(self) -> None:  # pragma: no cover
        while True:
            try:
                self.run_once()
            except Exception as e:
                log.error("health sweep failed: %s", e)
            time.sleep(self.interval_s)
