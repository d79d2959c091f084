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
                      bw_samples: int = 1, burn: bool = False, lds_march: bool = False,
                      hbm_march: bool = False, simd_probe: bool = False) -> dict:
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

    hbm_march=True adds the HBM march (`hbm_march_report`: up to 16 GiB held
    while it runs, both bit polarities, fault location, bandwidth per XCD) as
    report["hbm_march"] and ANDs its verdict into `healthy` unless the march
    was skipped for lack of free memory. Off by default, and the report is
    then unchanged; `hbm_sweep` (deep=True) stays as it is either way.

    simd_probe=True adds the SIMD probe (`simd_probe_report`: the exact VALU
    burn per section, tens of milliseconds, and the register-file march,
    about a millisecond during which it holds every SIMD's whole register
    file) as report["simd_probe"] and ANDs its verdict into `healthy`. Off by
    default, and the report is then unchanged.
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
    if hbm_march:
        report["hbm_march"] = hbm_march_report(device)
        # as for the sweep: a skipped march is no evidence either way
        if not report["hbm_march"]["skipped"]:
            report["healthy"] = bool(report["healthy"] and report["hbm_march"]["ok"])
    if simd_probe:
        report["simd_probe"] = simd_probe_report(device)
        report["healthy"] = bool(report["healthy"] and report["simd_probe"]["ok"])
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


# ---------------------------------------------------------------------------
# HBM march (ops.hbm_march): a bounded span of HBM, both bit polarities,
# 16 B per lane, a pattern unique across the whole sweep, every launch timed
# by events and by device clocks per workgroup. See the kernel comment in
# hived_ops.hip.
# ---------------------------------------------------------------------------
HBM_MARCH_TILE_BYTES = 16384  # 256 threads x 16 B x 4 accesses
_HBM_MARCH_TILE_QWORDS = HBM_MARCH_TILE_BYTES // 8
# the realtime clock of the records ticks at 100 MHz
_HBM_MARCH_TICK_S = 1e-8
_HBM_MARCH_MAX_LOCATIONS = 16
_HBM_MARCH_MAX_LOG = 64
_M64 = (1 << 64) - 1


def _mix64(x):
    """splitmix64 finaliser on a numpy uint64 array (wraps mod 2^64)."""
    import numpy as np

    x = x + np.uint64(0x9E3779B97F4A7C15)
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def hbm_march_pattern(seed: int, start: int, count: int):
    """The np.uint64[count] pattern p(seed, start + i) = mix64(seed ^ g) the
    kernel writes in pass 0 at the global qword indices g = start + i (byte
    offset in the sweep / 8). mix64(seed ^ .) is a bijection on 64 bits, so
    all values of a sweep are distinct. Pass 1 writes ~p."""
    import numpy as np

    g = np.arange(int(count), dtype=np.uint64) + np.uint64(int(start) & _M64)
    return _mix64(g ^ np.uint64(int(seed) & _M64))


def _u64_fields(rec, lo):
    """Fields [lo], [lo+1] of int32 records (lo word, hi word) as np.uint64."""
    import numpy as np

    low = (rec[..., lo].astype(np.int64) & 0xFFFFFFFF).astype(np.uint64)
    high = (rec[..., lo + 1].astype(np.int64) & 0xFFFFFFFF).astype(np.uint64)
    return (high << np.uint64(32)) | low


def hbm_slow_xcds(xcds, min_xcd_ratio) -> list:
    """XCC ids whose verify_gbps is below min_xcd_ratio x the median over the
    XCDs; empty when min_xcd_ratio is None."""
    import numpy as np

    if min_xcd_ratio is None or not xcds:
        return []
    floor = float(min_xcd_ratio) * float(np.median([x["verify_gbps"] for x in xcds]))
    return sorted(int(x["xcc"]) for x in xcds if x["verify_gbps"] < floor)


def summarize_hbm_march(result: dict, expected_xcds: int, min_xcd_ratio=None) -> dict:
    """Turn the result of one ops.hbm_march call into a verdict.

    result: the dict hbm_march returns, tensors already numpy. `records` is
    [launches, blocks, 16] int32 in launch order (chunk-major, then pass,
    then write before verify), rows {hw word, tiles, clock at start lo/hi,
    clock at end lo/hi, and for verify launches mismatched qwords lo/hi,
    lowest bad global qword index lo/hi (-1,-1), dropped mask lo/hi, raised
    mask lo/hi, sum of the qwords read lo/hi}. Pure numpy; needs no GPU.

    A rate per XCD is the bytes of that XCD's workgroups' tiles over all
    launches of one kind, divided by the sum over those launches of the XCD's
    own span (latest end minus earliest start among ITS workgroups that had a
    tile, in 10 ns ticks): clocks of different XCDs are never subtracted from
    each other. `blocks` of an XCD counts its workgroups over all launches.
    """
    import numpy as np

    bytes_tested = int(result["bytes_tested"])
    chunks = int(result["chunks"])
    chunk_bytes = int(result["chunk_bytes"])
    skipped = bool(result["skipped"])
    rec = np.asarray(result["records"]).astype(np.int64)
    rec = rec.reshape(-1, rec.shape[-2] if rec.ndim >= 2 else 0, 16)
    elapsed = np.asarray(result["elapsed_ms"], dtype=np.float64).reshape(-1)
    launches = int(rec.shape[0])
    is_verify = (np.arange(launches) % 2) == 1
    chunk_of = np.arange(launches) // 4
    pass_of = (np.arange(launches) // 2) % 2

    mism = _u64_fields(rec, 6)
    first = _u64_fields(rec, 8)
    per_launch = [int(mism[l].sum()) if is_verify[l] else 0 for l in range(launches)]
    errors = sum(per_launch)
    errors_per_chunk = [sum(e for l, e in enumerate(per_launch) if chunk_of[l] == c)
                        for c in range(chunks)]
    dropped = raised = 0
    first_bad = None
    for l in range(launches):
        if not per_launch[l]:
            continue
        bad = mism[l] != 0
        dropped |= int(np.bitwise_or.reduce(_u64_fields(rec[l], 10)[bad]))
        raised |= int(np.bitwise_or.reduce(_u64_fields(rec[l], 12)[bad]))
        if first_bad is None:
            first_bad = {"offset": 8 * int(first[l][bad].min()), "pass": int(pass_of[l])}
    bad_bits = [b for b in range(64) if ((dropped | raised) >> b) & 1]

    log = np.asarray(result["log"]).astype(np.int64).reshape(-1, 4)
    rows = sorted((int(r[1]), int(r[0]) & _M64, (int(r[2]) ^ int(r[3])) & _M64) for r in log)
    bad_locations = [{"offset": 8 * idx, "chunk": (8 * idx) // chunk_bytes if chunk_bytes else 0,
                      "pass": pas, "xor": xor}
                     for pas, idx, xor in rows[:_HBM_MARCH_MAX_LOCATIONS]]

    # every launch must have visited every tile of its chunk: a loop that
    # compared nothing cannot pass
    tiles = rec[:, :, 1]
    coverage_ok = bool(launches == 4 * chunks and
                       (tiles.sum(axis=1) * _HBM_MARCH_TILE_QWORDS == chunk_bytes // 8).all())

    def chip_gbps(kind):
        ms = float(elapsed[is_verify == kind].sum())
        return 2.0 * bytes_tested / (ms * 1e-3) / 1e9 if ms > 0 else 0.0

    start = _u64_fields(rec, 2)
    end = _u64_fields(rec, 4)
    xcc = rec[:, :, 0] >> 16
    xcds = []
    for x in sorted(int(v) for v in np.unique(xcc)):
        entry = {"xcc": x, "blocks": int((xcc == x).sum())}
        for kind, key in ((False, "write_gbps"), (True, "verify_gbps")):
            nbytes = ticks = 0
            for l in np.nonzero(is_verify == kind)[0]:
                sel = (xcc[l] == x) & (tiles[l] > 0)
                if not sel.any():
                    continue
                nbytes += int(tiles[l][sel].sum()) * HBM_MARCH_TILE_BYTES
                ticks += int(end[l][sel].max()) - int(start[l][sel].min())
            entry[key] = nbytes / (ticks * _HBM_MARCH_TICK_S) / 1e9 if ticks > 0 else 0.0
        xcds.append(entry)
    rates = [x["verify_gbps"] for x in xcds]
    median = float(np.median(rates)) if rates else 0.0
    xcd_ratio = min(rates) / median if median > 0 else 0.0
    slow_xcds = hbm_slow_xcds(xcds, min_xcd_ratio)
    ok = skipped or bool(errors == 0 and coverage_ok and len(xcds) >= expected_xcds
                         and not slow_xcds)
    return {
        "bytes_tested": bytes_tested,
        "chunks": chunks,
        "skipped": skipped,
        "errors": errors,
        "errors_per_chunk": errors_per_chunk,
        "dropped_mask": dropped,
        "raised_mask": raised,
        "bad_bits": bad_bits,
        "first_bad": first_bad,
        "bad_locations": bad_locations,
        "coverage_ok": coverage_ok,
        "write_gbps": chip_gbps(False),
        "verify_gbps": chip_gbps(True),
        "xcds": xcds,
        "xcds_seen": len(xcds),
        "xcd_ratio": xcd_ratio,
        "slow_xcds": slow_xcds,
        "ok": ok,
    }


def hbm_march_report(device: int = 0, max_gib: int = 16, chunk_gib: int = 4, seed: int = 1,
                     blocks: int = 2048, inject=None, min_xcd_ratio=None,
                     max_bytes: int = None, chunk_bytes: int = None) -> dict:
    """Run the HBM march on one GPU and summarise it.

    Marches up to max_gib GiB in chunk_gib chunks (all held until the end,
    like hbm_sweep, with the same 8 GiB headroom): four launches per chunk,
    write p / verify / write ~p / verify. max_bytes and chunk_bytes override
    the GiB arguments; they exist for small test shapes. `inject=(index,
    pass, bit)` xors that bit of the qword at that global index between the
    write and the verify of that pass: a plain store into the march's own
    allocation that exercises detection and location on healthy hardware.
    min_xcd_ratio has no default: the healthy spread between XCDs is
    site-measured (docs/user-manual.md).
    """
    import torch

    ops = get_ops()
    torch.cuda.set_device(device)
    max_bytes = int(max_gib) << 30 if max_bytes is None else int(max_bytes)
    chunk_bytes = int(chunk_gib) << 30 if chunk_bytes is None else int(chunk_bytes)
    inject_args = (-1, -1, 0) if inject is None else tuple(int(v) for v in inject)
    expected_xcds = max(1, ops.device_info(device)["multiProcessorCount"] // 32)
    res = dict(ops.hbm_march(max_bytes, chunk_bytes, seed, blocks, _HBM_MARCH_MAX_LOG,
                             *inject_args))
    for key in ("records", "elapsed_ms", "log"):
        res[key] = res[key].cpu().numpy()
    out = summarize_hbm_march(res, expected_xcds, min_xcd_ratio)
    out["expected_xcds"] = expected_xcds
    out["blocks"] = blocks
    out["elapsed_ms"] = float(res["elapsed_ms"].sum())
    return out


# ---------------------------------------------------------------------------
# SIMD probe: the exact VALU burn (ops.valu_burn) and the register-file march
# (ops.vgpr_march), attributed per SIMD. See the kernel comments in
# hived_ops.hip.
# ---------------------------------------------------------------------------
VALU_SECTIONS = ("int", "f32", "f64", "xlane", "trans")
# sections a host mirror reproduces bit for bit; "trans" is consensus only
VALU_EXACT_SECTIONS = ("int", "f32", "f64", "xlane")
_VALU_SECTION_ID = {s: i for i, s in enumerate(VALU_SECTIONS)}
_VALU_DEFAULT_CHAIN = 1024
# odd: every round ends in the same state, so the xor checksum over an even
# number of rounds cancels to zero and a consensus check compares nothing
_VALU_DEFAULT_ROUNDS = 33
_M32 = 0xFFFFFFFF

VGPR_MARCH_FIRST_REG = 32   # v0..v31 stay the compiler's
VGPR_MARCH_REGS = 480       # v32..v255 and a0..a255, marched per pass
# register indices R (0..255 architectural, 256..511 accumulators) that
# inject target 0 and target 1 flip a bit of
VGPR_MARCH_INJECT_VGPR = 77
VGPR_MARCH_INJECT_AGPR = 256 + 141
_VGPR_MARCH_BLOCKS_PER_CU = 2
# default rounds per workgroup (BENCHMARKS.md "SIMD probe")
_VGPR_MARCH_DEFAULT_ROUNDS = 16


def decode_hw_simd(word) -> tuple:
    """(XCC_ID<<16 | HW_ID) placement word -> (xcc, se, sh, cu, simd), with
    SIMD_ID at HW_ID[5:4] as in the gfx9-family layout."""
    w = int(word)
    return decode_hw_word(w) + ((w >> 4) & 0x3,)


def valu_fma_exact(section: str, a, b, c):
    """a*b + c on integers, as the f32 / f64 section's fma computes it, after
    asserting the bound that makes the floating-point fma exact: a, b < 2^12,
    c < 2^13 and a result <= 2^24 for "f32"; a, b < 2^26, c < 2^52 and a
    result < 2^53 for "f64". Works on Python ints and numpy uint64 arrays."""
    import numpy as np

    ab_bits, c_bits = {"f32": (12, 13), "f64": (26, 52)}[section]
    a, b, c = (np.asarray(v, dtype=np.uint64) for v in (a, b, c))
    if (a >> np.uint64(ab_bits)).any() or (b >> np.uint64(ab_bits)).any() \
            or (c >> np.uint64(c_bits)).any():
        raise AssertionError(f"{section} fma operand too wide for an exact result")
    r = a * b + c
    limit = (1 << 24) + 1 if section == "f32" else 1 << 53
    if (r >= np.uint64(limit)).any():
        raise AssertionError(f"{section} fma result not exactly representable")
    return r


def _rotl32(x, k):
    import numpy as np

    return (x << np.uint32(k)) | (x >> np.uint32(32 - k))


def _valu_seed_states(section: str, seed: int):
    """The 64 seeded states of a section as np.uint64 (the u32 sections use
    the low word only)."""
    import numpy as np

    lane = np.arange(64, dtype=np.uint32)
    start = np.uint32((int(seed) + _VALU_SECTION_ID[section] * 0x9E3779B9) & _M32)
    lo = _fmix32(start + lane * np.uint32(0x85EBCA6B))
    hi = _fmix32(lo ^ np.uint32(0xC2B2AE35))
    if section != "f64":
        return lo.astype(np.uint64)
    return (hi.astype(np.uint64) << np.uint64(32)) | lo.astype(np.uint64)


def _valu_step(section: str, s, c: int):
    """One step of the kernel's ValuStep<section> on the 64 lanes at once,
    integer arithmetic only. s: np.uint32[64], np.uint64[64] for "f64"."""
    import numpy as np

    u32, u64 = np.uint32, np.uint64
    if section == "int":
        lo = s * u32(0x9E3779B1)
        hi = ((s.astype(u64) * u64(0x85EBCA6B)) >> u64(32)).astype(u32)
        # v_mad_u64_u32: 32 x 32 -> 64 plus a 64-bit addend, wrapping at 2^64
        m = lo.astype(u64) * (hi | u32(1)).astype(u64) \
            + ((hi.astype(u64) << u64(32)) | s.astype(u64))
        t = (m.astype(u32) ^ (m >> u64(32)).astype(u32)) + lo
        bfe = (hi >> u32(7)) & u32(0x7FF)
        pop = np.array([bin(int(v)).count("1") for v in lo], dtype=u32)
        return (_rotl32(t, 13) ^ bfe) + pop
    if section == "f32":
        w = s.astype(u64)

        def f(shift, bits):
            return (w >> u64(shift)) & u64((1 << bits) - 1)

        # the 2^k scaling around the scalar fma is exact and leaves no trace
        r0 = valu_fma_exact("f32", f(0, 12), f(12, 12), f(19, 13))
        r1 = valu_fma_exact("f32", f(3, 12), f(16, 12), f(7, 13))
        r2 = valu_fma_exact("f32", f(9, 12), f(1, 12), f(13, 13))
        mix = (r0 + (r1 << u64(5)) + (r2 << u64(9))).astype(u32)
        return (s * u32(0x9E3779B1) + u32(0x7F4A7C15)) ^ mix
    if section == "f64":
        m26 = u64(0x3FFFFFF)
        # ch*2^26 + cl with ch, cl < 2^26: a power-of-two product and a sum
        # below 2^52, exact
        cc = ((s >> u64(38)) << u64(26)) + ((s >> u64(7)) & m26)
        r = valu_fma_exact("f64", s & m26, (s >> u64(26)) & m26, cc)
        return (s * u64(0x9E3779B97F4A7C15) + u64(0xBF58476D1CE4E5B9)) ^ r ^ (r << u64(11))
    if section == "xlane":
        l = np.arange(64)
        x = _rotl32(s, 5) + s[l ^ 1]                          # quad_perm:[1,0,3,2]
        x = _rotl32(x, 7) ^ x[np.where(l % 16 == 0, l, l - 1)]  # row_shr:1
        x = x + _rotl32(x[l ^ 15], 13)                        # row_mirror
        y = _rotl32(x, 3)
        # v_permlane32_swap: x's lanes 32-63 swap with y's lanes 0-31
        nx = np.where(l < 32, x, y[(l - 32) % 64])
        ny = np.where(l < 32, x[(l + 32) % 64], y)
        x = nx + (ny ^ u32(0x9E3779B9))
        x = _rotl32(x, 9) ^ x[(l * 13 + 7) & 63]              # ds_bpermute
        return x + x[(int(c) * 11 + 5) & 63]                  # v_readlane
    raise ValueError(f"section {section!r} has no host mirror")


def valu_burn_expected(section: str, seed: int, chain: int):
    """The 64 states (np.uint64, one per lane) every wave of ops.valu_burn
    must hold after `chain` steps: the host mirror of the kernel, on integers
    only. The f32 and f64 sections assert at every step the bound that makes
    their fma exact (valu_fma_exact). "trans" has no mirror: its low bits are
    hardware-defined."""
    import numpy as np

    if section not in VALU_EXACT_SECTIONS:
        raise ValueError(f"section {section!r} has no host mirror")
    s = _valu_seed_states(section, seed)
    if section != "f64":
        s = s.astype(np.uint32)
    for c in range(int(chain)):
        s = _valu_step(section, s, c)
    return s.astype(np.uint64)


def valu_burn_checksum(section: str, seed: int, chain: int, rounds: int) -> int:
    """The 64-bit xor checksum (record fields [4] low, [5] high) of a healthy
    wave: every round ends in the same state, so it is the xor over the lanes
    for odd `rounds` and 0 for even."""
    import numpy as np

    if int(rounds) % 2 == 0:
        return 0
    return int(np.bitwise_xor.reduce(valu_burn_expected(section, seed, chain)))


def vgpr_march_pattern(seed: int, round: int):
    """The np.uint32[512, 64] pattern p(round, R, lane) the march writes in
    the true polarity: ((R*64 + lane) * 0x9E3779B1 mod 2^32) ^ rs with
    rs = fmix32(seed + round*0x9E3779B9); rows 0..255 are the architectural
    registers, 256..511 the accumulators. The multiply by an odd constant and
    the xor are bijections on 32 bits, so all 32768 values are distinct. The
    complement pass writes ~p. Rows below VGPR_MARCH_FIRST_REG are not
    marched."""
    import numpy as np

    start = np.array([(int(seed) + int(round) * 0x9E3779B9) & _M32], dtype=np.uint32)
    rs = _fmix32(start)[0]
    idx = np.arange(512 * 64, dtype=np.uint32).reshape(512, 64)
    return (idx * np.uint32(0x9E3779B1)) ^ rs


def vgpr_march_wave_sum(seed: int, rounds: int) -> int:
    """Expected record field [6] of every wave: the sum mod 2^32 of the 480
    marched registers x 64 lanes of p over the pattern passes of all rounds."""
    import numpy as np

    total = sum(int(vgpr_march_pattern(seed, r)[VGPR_MARCH_FIRST_REG:].sum(dtype=np.uint64))
                for r in range(int(rounds)))
    return total & _M32


def _simd_entry(key, fields: dict) -> dict:
    return dict(xcc=key[0], se=key[1], sh=key[2], cu=key[3], simd=key[4], **fields)


def summarize_valu_burn(records, elapsed_ms: float, section: str, chain: int, rounds: int,
                        expected_simds: int) -> dict:
    """Turn the per-wave records of one ops.valu_burn launch into a verdict.

    records: [waves, 8] int32 rows {hw word, mismatched lane-rounds, first bad
    round (-1), lowest bad lane in it (-1), xor checksum low / high word, two
    reserved}. A wave is bad when it mismatched or when its checksum is not
    the majority's (all a "trans" run can show); it is attributed to the SIMD
    of its hw word. Pure numpy; needs no GPU.
    """
    import numpy as np

    rec = np.asarray(records).reshape(-1, 8).astype(np.int64)
    waves = int(rec.shape[0])
    simds_seen = len({decode_hw_simd(w) for w in np.unique(rec[:, 0])})
    checksum = _u64_fields(rec, 4)
    values, counts = np.unique(checksum, return_counts=True)
    majority = values[counts.argmax()] if waves else 0
    odd = checksum != majority
    bad: dict = {}
    for row in rec[(rec[:, 1] != 0) | odd]:
        e = bad.setdefault(decode_hw_simd(row[0]),
                           {"waves": 0, "mismatched_lane_rounds": 0, "first": None})
        e["waves"] += 1
        e["mismatched_lane_rounds"] += int(row[1])
        if row[1] != 0:
            first = (int(row[2]), int(row[3]))
            e["first"] = first if e["first"] is None else min(e["first"], first)
    bad_simds = []
    for key in sorted(bad):
        e = bad[key]
        first = e["first"] or (-1, -1)
        bad_simds.append(_simd_entry(key, {
            "waves": e["waves"], "mismatched_lane_rounds": e["mismatched_lane_rounds"],
            "first_bad_round": first[0], "first_bad_lane": first[1]}))
    mismatched_waves = int((rec[:, 1] != 0).sum())
    checksum_spread = bool(odd.any())
    return {
        "section": section,
        "chain": int(chain),
        "rounds": int(rounds),
        "elapsed_ms": float(elapsed_ms),
        "waves": waves,
        "simds_seen": simds_seen,
        "mismatched_waves": mismatched_waves,
        "checksum_spread": checksum_spread,
        "bad_simds": bad_simds,
        "ok": bool(mismatched_waves == 0 and not checksum_spread
                   and simds_seen >= expected_simds),
    }


def summarize_vgpr_march(records, elapsed_ms: float, rounds: int, seed: int,
                         expected_simds: int) -> dict:
    """Turn the per-wave records of one ops.vgpr_march launch into a verdict.

    records: [blocks*4, 8] int32 rows {hw word, mismatched (register, lane)
    pairs, first bad global pass (-1), lowest bad register in it (-1), dropped
    mask, raised mask, sum of the values read in the pattern passes, registers
    marched per pass}. A wave is bad when it counted a mismatch or, which
    would contradict a zero count, reports a dropped or raised bit; it is
    attributed to the SIMD of its hw word.
    At one wave per SIMD the four waves of a block share a CU and hold four
    different SIMD ids; a block that does not is counted in `split_blocks`
    and fails the run (it is also what confirms on hardware that SIMD_ID sits
    at HW_ID[5:4]). `checksum_ok` requires every wave's read sum to be the
    mirror's and every wave to have marched VGPR_MARCH_REGS registers. Pure
    numpy; needs no GPU.
    """
    import numpy as np

    rec = np.asarray(records).reshape(-1, 4, 8).astype(np.int64)
    blocks = int(rec.shape[0])
    want_sum = vgpr_march_wave_sum(seed, rounds)
    simds_seen = len({decode_hw_simd(w) for w in np.unique(rec[:, :, 0])})
    checksum_ok = bool(((rec[:, :, 6] & _M32) == want_sum).all()
                       and (rec[:, :, 7] == VGPR_MARCH_REGS).all())
    split_blocks = 0
    bad: dict = {}
    for blk in rec:
        places = [decode_hw_simd(w) for w in blk[:, 0]]
        if len({p[:4] for p in places}) != 1 or len({p[4] for p in places}) != 4:
            split_blocks += 1
        for place, row in zip(places, blk):
            # a set mask bit with a zero count contradicts itself: bad as well
            if row[1] == 0 and row[4] == 0 and row[5] == 0:
                continue
            e = bad.setdefault(place, {"waves": 0, "mismatched_registers": 0, "first": None,
                                       "dropped_mask": 0, "raised_mask": 0})
            e["waves"] += 1
            e["mismatched_registers"] += int(row[1])
            if row[2] >= 0:
                first = (int(row[2]), int(row[3]))
                e["first"] = first if e["first"] is None else min(e["first"], first)
            e["dropped_mask"] |= int(row[4]) & _M32
            e["raised_mask"] |= int(row[5]) & _M32
    bad_simds = []
    for key in sorted(bad):
        e = bad[key]
        first = e["first"] or (-1, -1)
        bad_simds.append(_simd_entry(key, {
            "waves": e["waves"], "mismatched_registers": e["mismatched_registers"],
            "first_bad_pass": first[0], "first_bad_reg": first[1],
            "dropped_mask": e["dropped_mask"], "raised_mask": e["raised_mask"]}))
    mismatched_waves = int(((rec[:, :, 1] != 0) | (rec[:, :, 4] != 0)
                            | (rec[:, :, 5] != 0)).sum())
    return {
        "elapsed_ms": float(elapsed_ms),
        "blocks": blocks,
        "waves": 4 * blocks,
        "simds_seen": simds_seen,
        "mismatched_waves": mismatched_waves,
        "checksum_ok": checksum_ok,
        "split_blocks": split_blocks,
        "bad_simds": bad_simds,
        "ok": bool(mismatched_waves == 0 and checksum_ok and split_blocks == 0
                   and simds_seen >= expected_simds),
    }


def _simd_keys(entries) -> set:
    return {(e["xcc"], e["se"], e["sh"], e["cu"], e["simd"]) for e in entries}


def _simd_dicts(keys) -> list:
    return [dict(xcc=x, se=se, sh=sh, cu=cu, simd=simd) for x, se, sh, cu, simd in sorted(keys)]


def valu_burn_report(device: int = 0, sections=VALU_SECTIONS, blocks: int = 2048,
                     chain: int = None, rounds: int = None, seed: int = 1,
                     inject=None) -> dict:
    """Run the VALU burn for each section on one GPU.

    Returns {"sections": {section: summarize_valu_burn(...)}, "ok",
    "bad_simds"} where `ok` is the AND and `bad_simds` the union ((xcc, se,
    sh, cu, simd) dicts, sorted) over sections. The exact sections compare
    against the host mirror; "trans" is consensus between waves only: it can
    name a SIMD that disagrees, not a fault common to all of them, and it
    needs an odd `rounds` (the default is; the extension refuses an even one
    too) because the xor checksum of an even number of identical rounds is
    zero. `inject=(wave, round, lane,
    bit)` xors that bit into that lane's state in that wave at that round (a
    harmless register-only fault) to exercise the detection path on healthy
    hardware.
    """
    import torch

    chain = _VALU_DEFAULT_CHAIN if chain is None else int(chain)
    rounds = _VALU_DEFAULT_ROUNDS if rounds is None else int(rounds)
    if "trans" in sections and rounds % 2 == 0:
        raise ValueError("section 'trans' needs an odd number of rounds")
    ops = get_ops()
    torch.cuda.set_device(device)
    inject_args = (-1, -1, -1, -1) if inject is None else tuple(int(v) for v in inject)
    expected_simds = 4 * ops.device_info(device)["multiProcessorCount"]
    out: dict = {"blocks": blocks, "chain": chain, "rounds": rounds, "sections": {}}
    bad = set()
    for section in sections:
        if section in VALU_EXACT_SECTIONS:
            want = valu_burn_expected(section, seed, chain)
            expected = torch.from_numpy(want.view("int64").copy()).cuda(device)
        else:
            expected = torch.empty(0, dtype=torch.int64)
        records, ms = ops.valu_burn(expected, section, seed, blocks, chain, rounds, *inject_args)
        s = summarize_valu_burn(records.cpu().numpy(), ms, section, chain, rounds, expected_simds)
        out["sections"][section] = s
        bad |= _simd_keys(s["bad_simds"])
    out["ok"] = all(s["ok"] for s in out["sections"].values())
    out["bad_simds"] = _simd_dicts(bad)
    return out


def vgpr_march_report(device: int = 0, blocks: int = None, rounds: int = None, seed: int = 1,
                      inject=None) -> dict:
    """Run the register-file march on one GPU and summarise it.

    The kernel allocates all 512 vector registers per lane, so one wave is
    resident per SIMD (the extension asserts it; `blocks_per_cu` is what the
    occupancy query said) and marches 480 of them: v0..v31 hold the kernel's
    own values and are exercised by the VALU burn instead. The default grid is
    two workgroups per CU and the default rounds keep the launch at about a
    millisecond, during which tenant waves wait for a SIMD. `inject=(wave,
    target, lane, bit, pass)` flips that bit of that lane of register
    VGPR_MARCH_INJECT_VGPR (target 0) or VGPR_MARCH_INJECT_AGPR (target 1) in
    that wave between the write and the read of that global pass (round*2 +
    polarity): registers only, to exercise detection and attribution on
    healthy hardware.
    """
    import torch

    ops = get_ops()
    torch.cuda.set_device(device)
    cus = ops.device_info(device)["multiProcessorCount"]
    blocks = _VGPR_MARCH_BLOCKS_PER_CU * cus if blocks is None else int(blocks)
    rounds = _VGPR_MARCH_DEFAULT_ROUNDS if rounds is None else int(rounds)
    inject_args = (-1, 0, 0, 0, -1) if inject is None else tuple(int(v) for v in inject)
    records, ms, per_cu = ops.vgpr_march(blocks, rounds, seed, *inject_args)
    out = summarize_vgpr_march(records.cpu().numpy(), ms, rounds, seed, 4 * cus)
    out["rounds"] = rounds
    out["registers_per_pass"] = VGPR_MARCH_REGS
    out["blocks_per_cu"] = int(per_cu)
    return out


def simd_probe_report(device: int = 0) -> dict:
    """Both SIMD probes at their default shapes: {"valu": valu_burn_report,
    "vgpr_march": vgpr_march_report, "ok", "bad_simds"}, `ok` the AND and
    `bad_simds` the union of the two."""
    valu = valu_burn_report(device)
    march = vgpr_march_report(device)
    bad = _simd_keys(valu["bad_simds"]) | _simd_keys(march["bad_simds"])
    return {"valu": valu, "vgpr_march": march, "ok": bool(valu["ok"] and march["ok"]),
            "bad_simds": _simd_dicts(bad)}
