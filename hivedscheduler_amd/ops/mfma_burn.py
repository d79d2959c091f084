"""Sustained MFMA burn-in (ops.mfma_burn): exact by construction, timed, and
attributed per CU. See the kernel comment in hived_ops.hip.
"""
from __future__ import annotations

from .records import (BadUnits, checksum_outliers, decode_hw_word, place_dicts, place_keys,
                      units_seen)

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
    cus_seen = units_seen(rec[:, 0], decode_hw_word)
    bad = BadUnits()
    for word, mism, first, _ in rec[rec[:, 1] != 0]:
        bad.add(decode_hw_word(word), {"waves": 1, "mismatched_elements": mism}, (int(first),))
    bad_cus = bad.entries(("first_bad_round",))
    mismatched_waves = int((rec[:, 1] != 0).sum())
    checksum_spread = bool(checksum_outliers(rec[:, 3]).any())
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

    from . import _ops_on

    ops = _ops_on(device)
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
        bad |= place_keys(s["bad_cus"], 4)
    out["ok"] = all(s["ok"] for s in out["formats"].values())
    out["bad_cus"] = place_dicts(bad)
    return out
