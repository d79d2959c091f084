"""HIP (gfx950) GPU health-probe kernels.

Import `get_ops()` to obtain the compiled extension. On a GPU box the native
extension is REQUIRED: failure to load raises (no silent eager fallback).
"""
from __future__ import annotations

import os
import sys

_ops = None


def get_ops():
    """Load the hived_ops HIP extension, building it if necessary."""
    global _ops
    if _ops is None:
        from .build import build

        _ops = build(verbose=False)
    return _ops


def gpu_health_report(device: int = 0, quick: bool = True, deep: bool = False,
                      bw_samples: int = 1, burn: bool = False) -> dict:
    """Run the health-probe kernels on one GPU and return measured facts.

    Feeds leaf-cell healthiness: HBM bandwidth deficit, MFMA mismatch, or
    (deep=True) any stuck-bit error in the HBM pattern sweep marks the GPU's
    leaf cell bad. The deep sweep scans a bounded span (16 GiB quick / 64 GiB
    otherwise) of the 288 GB HBM3E in 4 GiB chunks.

    bw_samples: take the BEST of N triad samples. On a GPU busy with a tenant
    job a single sample can read under half the real bandwidth (measured:
    1.53 TB/s vs 4.6 TB/s idle on the same healthy GPU — profiles/
    interference_r01.md); genuinely sick HBM is low in EVERY sample. Agents
    probing live nodes should use bw_samples>=3.

    burn=True adds the sustained MFMA burn-in (`mfma_burn_report`, tens of
    milliseconds per format) as report["mfma_burn"] and ANDs its verdict
    into `healthy`. Off by default: the report is then unchanged.
    """
    import torch

    ops = get_ops()
    torch.cuda.set_device(device)
    size_mb = 256 if quick else 2048
    iters = 5 if quick else 20
    report = {"device": device, "info": ops.device_info(device)}
    samples = [ops.hbm_triad_gbps(size_mb, iters) for _ in range(max(1, bw_samples))]
    report["hbm_gbps"] = max(samples)
    if len(samples) > 1:
        report["hbm_gbps_samples"] = [round(s, 1) for s in samples]

    torch.manual_seed(0)
    A = (torch.randn(16, 32, dtype=torch.float32) / 8).bfloat16().cuda(device)
    B = (torch.randn(32, 16, dtype=torch.float32) / 8).bfloat16().cuda(device)
    tiles = ops.mfma_check(A, B, 2048, 1)  # 8192 waves >> 256 CUs
    ref = (A.float() @ B.float())
    max_err = (tiles - ref.unsqueeze(0)).abs().max().item()
    tile_spread = (tiles - tiles[0].unsqueeze(0)).abs().max().item()
    report["mfma_max_err_vs_fp32"] = max_err
    report["mfma_cross_cu_spread"] = tile_spread  # must be exactly 0
    report["mfma_ok"] = bool(tile_spread == 0.0 and max_err < 0.1)
    # Low-precision pipes (MI355X's headline datapaths): fp8 e4m3 MFMA, the
    # MX block-scaled fp8 path (K=128), and MX fp4. A GPU whose bf16 pipes
    # work but whose fp8/fp4 units are broken passes the bf16 check alone.
    for key, fn in (("mfma_fp8", _mfma_fp8_probe), ("mfma_mx8", _mfma_mx_probe_fp8),
                    ("mfma_fp4", _mfma_mx_probe_fp4)):
        err, spread = fn(ops, device)
        report[f"{key}_max_err_vs_fp32"] = err
        report[f"{key}_cross_cu_spread"] = spread
        report[f"{key}_ok"] = bool(spread == 0.0 and err < 0.1)
    report["mfma_lowprec_ok"] = bool(report["mfma_fp8_ok"] and report["mfma_mx8_ok"]
                                     and report["mfma_fp4_ok"])
    # CU coverage: a big grid must place waves on every CU of every XCD; a
    # fused-off / hung CU shows up as missing (xcc, se, sh, cu) tuples
    words = ops.cu_coverage(4096).cpu().numpy()
    cus = {(int(w) >> 16, (int(w) >> 13) & 0x7, (int(w) >> 12) & 0x1, (int(w) >> 8) & 0xF)
           for w in words}
    report["cu_coverage"] = len(cus)
    expected_cus = report["info"]["multiProcessorCount"]
    report["cu_coverage_ok"] = bool(len(cus) >= expected_cus)
    report["lds_errors"] = int(ops.lds_check(2048, 7))
    report["healthy"] = bool(report["mfma_ok"] and report["mfma_lowprec_ok"]
                             and report["cu_coverage_ok"]
                             and report["lds_errors"] == 0
                             and report["hbm_gbps"] > 1000.0)
    if deep:
        sweep = ops.hbm_sweep(16 if quick else 64, 4, 1)
        report["hbm_sweep"] = sweep
        # A skipped (zero-byte) sweep is not evidence of health, but neither
        # is it evidence of sickness (a busy tenant GPU can leave too little
        # free HBM): record it, don't flip `healthy` on it.
        if not sweep.get("skipped"):
            report["healthy"] = bool(report["healthy"] and sweep["errors"] == 0)
    if burn:
        report["mfma_burn"] = mfma_burn_report(device)
        report["healthy"] = bool(report["healthy"] and report["mfma_burn"]["ok"])
    return report


_FP4_E2M1_VALUES = [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0,
                    -0.0, -0.5, -1.0, -1.5, -2.0, -3.0, -4.0, -6.0]


def _mfma_fp8_probe(ops, device):
    """fp8 e4m3 16x16x32 MFMA vs a torch fp32 reference decoded from the
    same raw e4m3 bytes. Returns (max_err, cross_cu_spread)."""
    import torch

    torch.manual_seed(1)
    A8 = (torch.randn(16, 32) / 8).to(torch.float8_e4m3fn).cuda(device)
    B8 = (torch.randn(32, 16) / 8).to(torch.float8_e4m3fn).cuda(device)
    tiles = ops.mfma_check_fp8(A8.view(torch.uint8), B8.view(torch.uint8), 2048)
    ref = A8.float() @ B8.float()
    return ((tiles - ref.unsqueeze(0)).abs().max().item(),
            (tiles - tiles[0].unsqueeze(0)).abs().max().item())


def _mfma_mx_probe_fp8(ops, device):
    """MX block-scaled fp8 (16x16x128 f8f6f4, fmt=0) with unit scales."""
    import torch

    torch.manual_seed(2)
    A8 = (torch.randn(16, 128) / 16).to(torch.float8_e4m3fn).cuda(device)
    B8 = (torch.randn(128, 16) / 16).to(torch.float8_e4m3fn).cuda(device)
    tiles = ops.mfma_check_mx(A8.view(torch.uint8), B8.view(torch.uint8), 2048, 0)
    ref = A8.float() @ B8.float()
    return ((tiles - ref.unsqueeze(0)).abs().max().item(),
            (tiles - tiles[0].unsqueeze(0)).abs().max().item())


def _mfma_mx_probe_fp4(ops, device):
    """MX block-scaled fp4 (e2m1 codes, fmt=4) with unit scales. Values are
    exactly representable and the K=128 dot products stay small, so the fp32
    reference matches bit-for-bit on healthy hardware."""
    import torch

    g = torch.Generator().manual_seed(3)
    A4 = torch.randint(0, 16, (16, 128), generator=g, dtype=torch.uint8).cuda(device)
    B4 = torch.randint(0, 16, (128, 16), generator=g, dtype=torch.uint8).cuda(device)
    lut = torch.tensor(_FP4_E2M1_VALUES, dtype=torch.float32).cuda(device)
    tiles = ops.mfma_check_mx(A4, B4, 2048, 4)
    ref = lut[A4.long()] @ lut[B4.long()]
    return ((tiles - ref.unsqueeze(0)).abs().max().item(),
            (tiles - tiles[0].unsqueeze(0)).abs().max().item())


# ---------------------------------------------------------------------------
# Sustained MFMA burn-in (ops.mfma_burn): exact by construction, timed, and
# attributed per CU. See the kernel comment in hived_ops.hip.
# ---------------------------------------------------------------------------
BURN_FORMATS = ("bf16", "fp8", "mx8", "mx4")
_BURN_K = {"bf16": 32, "fp8": 32, "mx8": 128, "mx4": 128}
_BURN_NACC = 4
_BURN_DEFAULT_CHAIN = 1024
# e2m1 codes of the integers -2..2 (index = value + 2), see _FP4_E2M1_VALUES
_BURN_FP4_CODES = [12, 10, 0, 2, 4]


def burn_chain_limit(fmt: str) -> int:
    """Largest `chain` for which the burn stays exact: operands are integers
    of magnitude <= 2, so a partial sum is an integer <= 4*K*chain, which
    fp32 holds exactly up to 2^24."""
    return (1 << 24) // (4 * _BURN_K[fmt])


def _burn_integers(fmt: str, seed: int = 0):
    """The int64 operands (A [64,K], B [K,16]) behind burn_operands.

    A is random in {-2..2}; B is a fixed asymmetric pattern (B[k][n] !=
    B[n][k]) so a transposed fragment or C layout cannot pass. Rows of A are
    redrawn until no element of A @ B is zero: a zeroed output lane, or an
    accumulator that stopped accumulating, then differs from the expected
    value in every element rather than only where the product is non-zero.
    """
    import torch

    K = _BURN_K[fmt]
    g = torch.Generator().manual_seed(seed)
    k = torch.arange(K, dtype=torch.int64).unsqueeze(1)
    n = torch.arange(16, dtype=torch.int64).unsqueeze(0)
    b_int = (3 * k + n + seed) % 5 - 2
    a_int = torch.randint(-2, 3, (_BURN_NACC * 16, K), generator=g, dtype=torch.int64)
    while True:
        redraw = ((a_int @ b_int) == 0).any(dim=1)
        if not redraw.any():
            return a_int, b_int
        a_int[redraw] = torch.randint(-2, 3, (int(redraw.sum()), K), generator=g,
                                      dtype=torch.int64)


def burn_operands(fmt: str, seed: int = 0):
    """Integer operands in {-2..2} for one burn format, on the CPU.

    Returns (A [64,K], B [K,16], expected_unit [4,16,16] fp32) where A and B
    are encoded for `fmt` (bf16 tensor; float8_e4m3fn tensor for fp8/mx8;
    uint8 e2m1 codes one per byte for mx4) and expected_unit[i] is the exact
    fp32 product A[16i:16i+16] @ B, i.e. the expected tile for chain = 1.
    """
    import torch

    K = _BURN_K[fmt]
    a_int, b_int = _burn_integers(fmt, seed)
    expected_unit = (a_int.float().view(_BURN_NACC, 16, K) @ b_int.float()).contiguous()
    if fmt == "bf16":
        A, B = a_int.to(torch.bfloat16), b_int.to(torch.bfloat16)
    elif fmt in ("fp8", "mx8"):
        A = a_int.float().to(torch.float8_e4m3fn)
        B = b_int.float().to(torch.float8_e4m3fn)
    else:
        codes = torch.tensor(_BURN_FP4_CODES, dtype=torch.uint8)
        A, B = codes[a_int + 2], codes[b_int + 2]
    return A.contiguous(), B.contiguous(), expected_unit


def decode_hw_word(word) -> tuple:
    """(XCC_ID<<16 | HW_ID) placement word -> (xcc, se, sh, cu)."""
    w = int(word)
    return (w >> 16, (w >> 13) & 0x7, (w >> 12) & 0x1, (w >> 8) & 0xF)


def summarize_burn(records, elapsed_ms: float, fmt: str, chain: int, rounds: int,
                   expected_cus: int) -> dict:
    """Turn the per-wave records of one ops.mfma_burn launch into a verdict.

    records: [waves, 4] int32 rows {hw word, mismatched elements, first bad
    round (-1 if none), xor checksum}. Pure numpy; needs no GPU.
    """
    import numpy as np

    rec = np.asarray(records).reshape(-1, 4).astype(np.int64)
    waves = int(rec.shape[0])
    flop = 2.0 * 16 * 16 * _BURN_K[fmt] * _BURN_NACC * chain * rounds * waves
    tflops = flop / (elapsed_ms * 1e-3) / 1e12 if elapsed_ms > 0 else 0.0
    cus_seen = len({decode_hw_word(w) for w in np.unique(rec[:, 0])})
    bad: dict = {}
    for word, mism, first, _ in rec[rec[:, 1] != 0]:
        e = bad.setdefault(decode_hw_word(word),
                           {"waves": 0, "mismatched_elements": 0, "first_bad_round": int(first)})
        e["waves"] += 1
        e["mismatched_elements"] += int(mism)
        e["first_bad_round"] = min(e["first_bad_round"], int(first))
    bad_cus = [dict(xcc=key[0], se=key[1], sh=key[2], cu=key[3], **bad[key])
               for key in sorted(bad)]
    mismatched_waves = int((rec[:, 1] != 0).sum())
    values, counts = np.unique(rec[:, 3], return_counts=True)
    majority = values[counts.argmax()] if waves else 0
    checksum_spread = bool((rec[:, 3] != majority).any())
    return {
        "tflops": tflops,
        "elapsed_ms": float(elapsed_ms),
        "waves": waves,
        "cus_seen": cus_seen,
        "mismatched_waves": mismatched_waves,
        "bad_cus": bad_cus,
        "checksum_spread": checksum_spread,
        "ok": bool(mismatched_waves == 0 and not checksum_spread and cus_seen >= expected_cus),
    }


def mfma_burn_report(device: int = 0, fmts=BURN_FORMATS, blocks: int = 2048,
                     chain: int = None, rounds: int = 64, inject=None) -> dict:
    """Run the MFMA burn-in for each format on one GPU.

    Returns {"formats": {fmt: summarize_burn(...)}, "ok", "bad_cus"} where
    `ok` is the AND and `bad_cus` the union ((xcc, se, sh, cu) dicts, sorted)
    over formats. `inject=(wave, round)` flips one accumulator bit in that
    wave at that round (a harmless register-only fault) to exercise the
    detection path on healthy hardware.
    """
    import torch

    ops = get_ops()
    torch.cuda.set_device(device)
    chain = _BURN_DEFAULT_CHAIN if chain is None else int(chain)
    inject_wave, inject_round = (-1, -1) if inject is None else inject
    expected_cus = ops.device_info(device)["multiProcessorCount"]
    out: dict = {"blocks": blocks, "chain": chain, "rounds": rounds, "formats": {}}
    bad = set()
    for fmt in fmts:
        A, B, unit = burn_operands(fmt, seed=0)
        if A.dtype != torch.bfloat16:
            A, B = A.view(torch.uint8), B.view(torch.uint8)
        records, ms = ops.mfma_burn(A.cuda(device), B.cuda(device), (unit * chain).cuda(device),
                                    fmt, blocks, chain, rounds, inject_wave, inject_round)
        s = summarize_burn(records.cpu().numpy(), ms, fmt, chain, rounds, expected_cus)
        out["formats"][fmt] = s
        bad.update((c["xcc"], c["se"], c["sh"], c["cu"]) for c in s["bad_cus"])
    out["ok"] = all(s["ok"] for s in out["formats"].values())
    out["bad_cus"] = [dict(xcc=x, se=se, sh=sh, cu=cu) for x, se, sh, cu in sorted(bad)]
    return out
