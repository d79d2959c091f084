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
                      bw_samples: int = 1, burn: bool = False, lds_march: bool = False) -> dict:
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

    lds_march=True adds the full-LDS march (`lds_march_report`, about a
    millisecond) as report["lds_march"] and ANDs its verdict into `healthy`.
    Off by default, and the report is then unchanged; `lds_errors` stays the
    64 KiB single-pass check either way.
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
    if lds_march:
        report["lds_march"] = lds_march_report(device)
        report["healthy"] = bool(report["healthy"] and report["lds_march"]["ok"])
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


# ---------------------------------------------------------------------------
# Full-LDS march (ops.lds_march): all 160 KiB of a CU, both bit polarities,
# ds_read_b32 and ds_read_b128 read-back, timed, attributed per CU. See the
# kernel comment in hived_ops.hip.
# ---------------------------------------------------------------------------
LDS_MARCH_WORDS = 40960  # 163840 B, the whole LDS of a CU
_LDS_MARCH_BYTES = 4 * LDS_MARCH_WORDS
# default rounds per workgroup, and workgroups per CU of the default grid
# (BENCHMARKS.md "LDS march")
_LDS_MARCH_DEFAULT_ROUNDS = 8
_LDS_MARCH_BLOCKS_PER_CU = 2


def _fmix32(h):
    """murmur3 32-bit finaliser on a numpy uint32 array."""
    import numpy as np

    h = h ^ (h >> np.uint32(16))
    h = h * np.uint32(0x85EBCA6B)
    h = h ^ (h >> np.uint32(13))
    h = h * np.uint32(0xC2B2AE35)
    return h ^ (h >> np.uint32(16))


def lds_march_pattern(seed: int, round: int):
    """The np.uint32[40960] pattern p(round, i) the kernel writes in the true
    polarity: fmix32((seed + round*0x9E3779B9) ^ (i*0x85EBCA6B)). Every step
    is a bijection on 32 bits, so the 40960 values of a round are distinct.
    The complement passes write ~p."""
    import numpy as np

    rs = np.uint32((int(seed) + int(round) * 0x9E3779B9) & 0xFFFFFFFF)
    i = np.arange(LDS_MARCH_WORDS, dtype=np.uint32)
    return _fmix32(rs ^ (i * np.uint32(0x85EBCA6B)))


def lds_march_block_checksum(seed: int, rounds: int) -> int:
    """Expected sum of record field [6] over the four waves of a block: every
    word of p is read once in phase 0 and once in phase 2 of each round, so
    2 * sum_round sum_i p(round, i) mod 2^32."""
    import numpy as np

    total = sum(int(lds_march_pattern(seed, r).sum(dtype=np.uint64)) for r in range(rounds))
    return (2 * total) & 0xFFFFFFFF


def summarize_lds_march(records, elapsed_ms: float, rounds: int, seed: int,
                        expected_cus: int) -> dict:
    """Turn the per-wave records of one ops.lds_march launch into a verdict.

    records: [blocks*4, 8] int32 rows {hw word, mismatched dwords, first bad
    global pass (-1), lowest bad word in that pass (-1), dropped mask (bits
    that should be 1 and read 0), raised mask (should be 0, read 1), sum of
    the dwords read in phases 0 and 2, reserved}. The four waves of a block
    (wave // 4) are combined; a block is attributed to the CU of its first
    wave, and a block whose waves name different CUs is counted in
    `split_blocks` (one workgroup runs on one CU, so that is a fault in
    itself). Pure numpy; needs no GPU.
    """
    import numpy as np

    rec = np.asarray(records).reshape(-1, 4, 8).astype(np.int64)
    blocks = int(rec.shape[0])
    nbytes = float(blocks) * rounds * 4 * 2 * _LDS_MARCH_BYTES
    gbps = nbytes / (elapsed_ms * 1e-3) / 1e9 if elapsed_ms > 0 else 0.0
    want_sum = lds_march_block_checksum(seed, rounds)
    cus_seen = len({decode_hw_word(w) for w in np.unique(rec[:, :, 0])})
    mismatched_blocks = split_blocks = 0
    checksum_ok = True
    bad: dict = {}
    for blk in rec:
        cus = [decode_hw_word(w) for w in blk[:, 0]]
        if len(set(cus)) != 1:
            split_blocks += 1
        if (int(blk[:, 6].sum()) & 0xFFFFFFFF) != want_sum:
            checksum_ok = False
        mism = int(blk[:, 1].sum())
        if mism == 0:
            continue
        mismatched_blocks += 1
        first = min((int(w[2]), int(w[3])) for w in blk if w[1] != 0)
        dropped = int(np.bitwise_or.reduce(blk[:, 4])) & 0xFFFFFFFF
        raised = int(np.bitwise_or.reduce(blk[:, 5])) & 0xFFFFFFFF
        e = bad.setdefault(cus[0], {"blocks": 0, "mismatched_dwords": 0, "first": first,
                                    "dropped_mask": 0, "raised_mask": 0})
        e["blocks"] += 1
        e["mismatched_dwords"] += mism
        e["first"] = min(e["first"], first)
        e["dropped_mask"] |= dropped
        e["raised_mask"] |= raised
    bad_cus = []
    for key in sorted(bad):
        e = bad[key]
        bad_cus.append(dict(xcc=key[0], se=key[1], sh=key[2], cu=key[3], blocks=e["blocks"],
                            mismatched_dwords=e["mismatched_dwords"],
                            first_bad_pass=e["first"][0], first_bad_word=e["first"][1],
                            dropped_mask=e["dropped_mask"], raised_mask=e["raised_mask"]))
    return {
        "gbps": gbps,
        "elapsed_ms": float(elapsed_ms),
        "blocks": blocks,
        "cus_seen": cus_seen,
        "mismatched_blocks": mismatched_blocks,
        "checksum_ok": checksum_ok,
        "split_blocks": split_blocks,
        "bad_cus": bad_cus,
        "ok": bool(mismatched_blocks == 0 and checksum_ok and split_blocks == 0
                   and cus_seen >= expected_cus),
    }


def lds_march_report(device: int = 0, blocks: int = None, rounds: int = None, seed: int = 1,
                     inject=None) -> dict:
    """Run the full-LDS march on one GPU and summarise it.

    The kernel takes all 160 KiB of LDS, so one workgroup is resident per CU;
    the default grid is two workgroups per CU (every CU is then covered on an
    idle GPU) and the default rounds keep the launch at about a millisecond.
    `inject=(block, word, pass, bit)` flips that bit of that LDS word in that
    block after the write of that global pass (round*4 + phase): a harmless
    store into the workgroup's own LDS that exercises detection and
    attribution on healthy hardware.
    """
    import torch

    ops = get_ops()
    torch.cuda.set_device(device)
    expected_cus = ops.device_info(device)["multiProcessorCount"]
    blocks = _LDS_MARCH_BLOCKS_PER_CU * expected_cus if blocks is None else int(blocks)
    rounds = _LDS_MARCH_DEFAULT_ROUNDS if rounds is None else int(rounds)
    inject_args = (-1, -1, -1, 0) if inject is None else tuple(int(v) for v in inject)
    records, ms = ops.lds_march(blocks, rounds, seed, *inject_args)
    out = summarize_lds_march(records.cpu().numpy(), ms, rounds, seed, expected_cus)
    out["rounds"] = rounds
    return out
