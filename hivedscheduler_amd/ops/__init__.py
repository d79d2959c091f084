"""HIP (gfx950) GPU health-probe kernels.

Import `get_ops()` to obtain the compiled extension. On a GPU box the native
extension is REQUIRED: failure to load raises (no silent eager fallback).

Here: the loader, `gpu_health_report` and the single-tile MFMA checks. Each
opt-in probe has a module of its own (mfma_burn, lds_march, hbm_march,
simd_probe, scalar_probe, atomic_probe) on top of `records`, and the
single-tile checks' operands and verdict are in mfma_tiles; their public names
are re-exported here, and their report functions reach the extension through
`_ops_on` below.
"""
from __future__ import annotations

from .atomic_probe import (ATOMIC_CELLS, ATOMIC_FP_OPS, ATOMIC_INT_OPS,  # noqa: F401
                           ATOMIC_LDS_MAX_CHAIN, ATOMIC_SECTIONS, ATOMIC_STEP_OPS,
                           CONTEND_CELL_BYTES, CONTEND_SECTIONS, REDUCE_OPS,
                           REDUCE_OR_CONTRIBUTIONS, REDUCE_PK_CONTRIBUTIONS,
                           atomic_burn_checksum, atomic_burn_expected, atomic_burn_outcomes,
                           atomic_burn_report, atomic_cas_cap, atomic_cas_expected,
                           atomic_contend_report, atomic_fp_exact, atomic_probe_report,
                           atomic_reduce_contributions, atomic_reduce_expected,
                           contend_lanes_on_cell, summarize_atomic_burn,
                           summarize_atomic_contend)
from .hbm_march import (HBM_MARCH_TILE_BYTES, hbm_march_pattern, hbm_march_report,  # noqa: F401
                        hbm_slow_xcds, summarize_hbm_march)
from .lds_march import (LDS_MARCH_WORDS, lds_march_block_checksum, lds_march_pattern,  # noqa: F401
                        lds_march_report, summarize_lds_march)
from .mfma_tiles import (E4M3_GROUP_WINDOW_BITS, E4M3_NAN_CODES, TILE_FORMATS,  # noqa: F401
                         TILE_K, TILE_PROBE_SEEDS, _FP4_E2M1_VALUES, decode_tile_operand,
                         e4m3_values, e4m3_within_group_window, encode_tile_operand, exact_tile,
                         judge_mfma_tiles, mfma_tile_operands, mfma_tile_probe, run_mfma_tile,
                         tile_operand_invariants, tile_product)
from .mfma_burn import (BURN_FORMATS, _burn_integers, burn_chain_limit, burn_operands,  # noqa: F401
                        mfma_burn_report, summarize_burn)
from .records import decode_hw_simd, decode_hw_word  # noqa: F401
from .scalar_probe import (SALU_CHAINS, SALU_SECTIONS, SGPR_MARCH_FIRST_REG,  # noqa: F401
                           SGPR_MARCH_INJECT_REG, SGPR_MARCH_REGS, salu_burn_checksum,
                           salu_burn_expected, salu_burn_report, salu_ctl_arms,
                           scalar_load_pattern, scalar_load_report, scalar_probe_report,
                           sgpr_march_pattern, sgpr_march_report, sgpr_march_wave_sum,
                           summarize_salu_burn, summarize_scalar_load, summarize_sgpr_march)
from .simd_probe import (VALU_EXACT_SECTIONS, VALU_SECTIONS, VGPR_MARCH_FIRST_REG,  # noqa: F401
                         VGPR_MARCH_INJECT_AGPR, VGPR_MARCH_INJECT_VGPR, VGPR_MARCH_REGS,
                         simd_probe_report, summarize_valu_burn, summarize_vgpr_march,
                         valu_burn_checksum, valu_burn_expected, valu_burn_report,
                         valu_fma_exact, vgpr_march_pattern, vgpr_march_report,
                         vgpr_march_wave_sum)

_ops = None


def get_ops():
    """Load the hived_ops HIP extension, building it if necessary."""
    global _ops
    if _ops is None:
        from .build import build

        _ops = build(verbose=False)
    return _ops


def _ops_on(device: int):
    """The extension (through whatever `get_ops` is now), `device` made current."""
    import torch

    ops = get_ops()
    torch.cuda.set_device(device)
    return ops


def gpu_health_report(device: int = 0, quick: bool = True, deep: bool = False,
                      bw_samples: int = 1, burn: bool = False, lds_march: bool = False,
                      hbm_march: bool = False, simd_probe: bool = False,
                      scalar_probe: bool = False, atomic_probe: bool = False) -> dict:
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

    scalar_probe=True adds the scalar probe (`scalar_probe_report`: the exact
    SALU burn per section, tens of milliseconds, the SGPR march over the 70
    registers of every wave and the scalar-load check in five widths) as
    report["scalar_probe"] and ANDs its verdict into `healthy`. Off by
    default, and the report is then unchanged.

    atomic_probe=True adds the atomic probe (`atomic_probe_report`: the exact
    atomic burn per section on cells each lane owns, tens of milliseconds, and
    the contended ticket, reduce and cmpswap sections on cells every workgroup
    shares, a few milliseconds) as report["atomic_probe"] and ANDs its verdict
    into `healthy`. Off by default, and the report is then unchanged.
    """
    ops = _ops_on(device)
    size_mb = 256 if quick else 2048
    iters = 5 if quick else 20
    report = {"device": device, "info": ops.device_info(device)}
    samples = [ops.hbm_triad_gbps(size_mb, iters) for _ in range(max(1, bw_samples))]
    report["hbm_gbps"] = max(samples)
    if len(samples) > 1:
        report["hbm_gbps_samples"] = [round(s, 1) for s in samples]

    # Single-tile MFMA checks (mfma_tiles): operands whose product fp32 holds
    # exactly, every wave's tile compared with it bitwise. bf16 first, then the
    # low-precision pipes (MI355X's headline datapaths): fp8 e4m3 MFMA, the
    # MX block-scaled fp8 path (K=128), and MX fp4. A GPU whose bf16 pipes
    # work but whose fp8/fp4 units are broken passes the bf16 check alone.
    for key, fn in (("mfma", _mfma_bf16_probe), ("mfma_fp8", _mfma_fp8_probe),
                    ("mfma_mx8", _mfma_mx_probe_fp8), ("mfma_fp4", _mfma_mx_probe_fp4)):
        err, spread, ok = fn(ops, device)
        report[f"{key}_max_err_vs_fp32"] = err  # must be exactly 0
        report[f"{key}_cross_cu_spread"] = spread  # must be exactly 0
        report[f"{key}_ok"] = bool(ok and err == 0.0 and spread == 0.0)
    report["mfma_lowprec_ok"] = bool(report["mfma_fp8_ok"] and report["mfma_mx8_ok"]
                                     and report["mfma_fp4_ok"])
    # CU coverage: a big grid must place waves on every CU of every XCD; a
    # fused-off / hung CU shows up as missing (xcc, se, sh, cu) tuples
    words = ops.cu_coverage(4096).cpu().numpy()
    cus = {decode_hw_word(w) for w in words}
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
    if scalar_probe:
        report["scalar_probe"] = scalar_probe_report(device)
        report["healthy"] = bool(report["healthy"] and report["scalar_probe"]["ok"])
    if atomic_probe:
        report["atomic_probe"] = atomic_probe_report(device)
        report["healthy"] = bool(report["healthy"] and report["atomic_probe"]["ok"])
    return report


def _mfma_bf16_probe(ops, device):
    """bf16 16x16x32 MFMA on every CU against the exact tile of
    mfma_tile_operands("bf16", 0). Returns (max_err, cross_cu_spread, ok)."""
    return mfma_tile_probe(ops, device, "bf16")


def _mfma_fp8_probe(ops, device):
    """fp8 e4m3 16x16x32 MFMA against the exact product of the same raw e4m3
    bytes."""
    return mfma_tile_probe(ops, device, "fp8")


def _mfma_mx_probe_fp8(ops, device):
    """MX block-scaled fp8 (16x16x128 f8f6f4, fmt=0) with unit scales."""
    return mfma_tile_probe(ops, device, "mx8")


def _mfma_mx_probe_fp4(ops, device):
    """MX block-scaled fp4 (e2m1 codes, fmt=4) with unit scales."""
    return mfma_tile_probe(ops, device, "mx4")
