"""GEMM probe (ops.gemm_pipe, ops.lds_tr_read): a tiled bf16 / fp8 GEMM that
keeps direct-to-LDS loads, LDS fragment reads and MFMAs busy together, exact by
construction, compared bitwise in the kernel and attributed per CU; and the
host mirror of the LDS transpose reads underneath it. See the kernel comment in
hived_ops.hip. Pure numpy / torch on the CPU apart from the report function.
"""
from __future__ import annotations

from .records import (BadUnits, _fmix32, checksum_outliers, decode_hw_word, place_dicts,
                      place_keys, units_seen)

GEMM_PROBE_FORMATS = ("bf16", "fp8")
GEMM_PROBE_LAYOUTS = ("kn", "nk")
GEMM_PROBE_CASES = tuple((f, b) for f in GEMM_PROBE_FORMATS for b in GEMM_PROBE_LAYOUTS)
GEMM_TILE = 128
LDS_TR_WIDTHS = (16, 8, 4, 6)
_ELEM_BYTES = {"bf16": 2, "fp8": 1}
_STEP_BYTES = 128  # bytes of K per row and K step
# default shape and rounds of the three tiled GEMM probes (BENCHMARKS.md "GEMM
# probe", "MX GEMM probe", "MX6 GEMM probe"): 1024 workgroups, four per CU of
# an MI355X; 99 rounds put every MX6 case's timed launch at 27 to 31 ms, inside
# what the GEMM probe's cases take; an odd number keeps the xor checksum
# non-zero
_DEFAULT_MNK = (4096, 4096, 8192)
_DEFAULT_ROUNDS = 99


def gemm_probe_bk(fmt: str) -> int:
    """Elements of K per step: 128 bytes per row."""
    return _STEP_BYTES // _ELEM_BYTES[fmt]


def gemm_probe_period(fmt: str) -> int:
    """K period of the probe's operands: four K steps. With two LDS stages a
    stale stage holds step k-2, which a period of two steps would hide."""
    return 4 * gemm_probe_bk(fmt)


# --- the transpose-read mirror ---------------------------------------------
def lds_tr_span(width: int) -> tuple:
    """(bytes a lane reads, alignment the wrapper requires) of one read."""
    return (12, 16) if width == 6 else (8, 8)


def lds_tr_expected(width: int, image, addrs):
    """What ops.lds_tr_read returns, from the description of the instructions
    (LLVM AMDGPU ds.read.tr*, ck_tile's LaneGroupTransposeTraits): np.int32
    [64,2] ([64,3] for width 6).

    Each group of 16 lanes addresses a block of R rows of 16 elements of
    `width` bits, R = 64/width (16 for width 6); with P = 16/R lanes per row,
    lane i of the group supplies the 16/P elements of row i//P that start at
    element (16/P)*(i%P), from the 8 (12) bytes at its own address, element 0
    in the lowest bits. Lane i receives column i of the block, row 0 lowest.
    """
    import numpy as np

    data = np.ascontiguousarray(np.asarray(image)).view(np.uint8)
    addrs = [int(a) for a in np.asarray(addrs).reshape(64)]
    span, _ = lds_tr_span(width)
    rows = 16 if width in (4, 6) else 64 // width
    per_row = 16 // rows          # lanes per row
    per_lane = 16 // per_row      # elements a lane supplies
    mask = (1 << width) - 1
    lanes = [int.from_bytes(bytes(data[a:a + span]), "little") for a in addrs]
    out = np.zeros((64, span // 4), dtype=np.uint32)
    for lane in range(64):
        group, i = lane // 16 * 16, lane % 16
        value = 0
        for row in range(rows):
            src = lanes[group + per_row * row + i // per_lane]
            value |= ((src >> (width * (i % per_lane))) & mask) << (width * row)
        for w in range(span // 4):
            out[lane, w] = (value >> (32 * w)) & 0xFFFFFFFF
    return out.view(np.int32)


def lds_tr_tile_addrs(width: int, row_stride: int, base: int = 0, group_rows: int = None):
    """np.int32[64]: lane addresses that read, per group of 16 lanes, a block
    of consecutive rows of a row-major tile whose rows are `row_stride` bytes
    apart, group g starting at row g*group_rows (default: the block's own
    height). The GEMM reads B this way with row_stride 256, group_rows 8
    (tr_b16) and row_stride 128, group_rows 16 (tr_b8)."""
    import numpy as np

    span, _ = lds_tr_span(width)
    rows = 16 if width in (4, 6) else 64 // width
    per_row = 16 // rows
    group_rows = rows if group_rows is None else group_rows
    lane = np.arange(64)
    i = lane % 16
    row = (lane // 16) * group_rows + i // per_row
    return (base + row * row_stride + (i % per_row) * span).astype(np.int32)


def lds_tr_image(words: int, seed: int = 1, complement: bool = False):
    """np.int32[words]: fmix32(seed ^ i*0x85EBCA6B), optionally complemented."""
    import numpy as np

    i = np.arange(words, dtype=np.uint32) * np.uint32(0x85EBCA6B)
    v = _fmix32(np.uint32(seed & 0xFFFFFFFF) ^ i)
    return (~v if complement else v).view(np.int32)


# --- operands ----------------------------------------------------------------
def gemm_probe_encode(ints, fmt: str):
    """An integer tensor with values in {-2..2} as the op takes it: bfloat16
    for bf16, raw e4m3 bytes (uint8) for fp8."""
    import torch

    if fmt == "bf16":
        return ints.to(torch.bfloat16).contiguous()
    return ints.float().to(torch.float8_e4m3fn).view(torch.uint8).contiguous()


def _gemm_probe_units(fmt: str, seed: int = 0):
    """int64 (a_unit [128,P], b_unit [P,128]). b_unit is a fixed asymmetric
    pattern, as in _burn_integers; rows of a_unit are redrawn until no element
    of a_unit @ b_unit is zero, so a dead accumulator differs everywhere."""
    import torch

    P = gemm_probe_period(fmt)
    g = torch.Generator().manual_seed(seed)
    k = torch.arange(P, dtype=torch.int64).unsqueeze(1)
    n = torch.arange(GEMM_TILE, dtype=torch.int64).unsqueeze(0)
    b_unit = (3 * k + n + seed) % 5 - 2
    a_unit = torch.randint(-2, 3, (GEMM_TILE, P), generator=g, dtype=torch.int64)
    while True:
        redraw = ((a_unit @ b_unit) == 0).any(dim=1)
        if not redraw.any():
            return a_unit, b_unit
        a_unit[redraw] = torch.randint(-2, 3, (int(redraw.sum()), P), generator=g,
                                       dtype=torch.int64)


def gemm_probe_operands(fmt: str, b_layout: str, M: int, N: int, K: int, seed: int = 0):
    """(A [M,K], B [K,N] or [N,K], expected [128,128] fp32) on the CPU, encoded
    for `fmt`. A and B repeat the units with period 128 in M and N and period
    P = 4 K steps in K: every workgroup streams its own addresses, and every
    tile of C is (K/P) * (a_unit @ b_unit), an integer of at most 4*K."""
    import torch

    P = gemm_probe_period(fmt)
    if fmt not in GEMM_PROBE_FORMATS or b_layout not in GEMM_PROBE_LAYOUTS:
        raise ValueError(f"unknown case {fmt}/{b_layout}")
    if M % GEMM_TILE or N % GEMM_TILE or K % P or min(M, N, K) <= 0:
        raise ValueError(f"M, N must be multiples of 128 and K of {P}; got {M}, {N}, {K}")
    a_unit, b_unit = _gemm_probe_units(fmt, seed)
    expected = ((K // P) * (a_unit @ b_unit)).to(torch.float32).contiguous()
    A = gemm_probe_encode(a_unit, fmt).repeat(M // GEMM_TILE, K // P)
    b_enc = gemm_probe_encode(b_unit if b_layout == "kn" else b_unit.t(), fmt)
    B = b_enc.repeat(K // P, N // GEMM_TILE) if b_layout == "kn" \
        else b_enc.repeat(N // GEMM_TILE, K // P)
    return A.contiguous(), B.contiguous(), expected


def gemm_probe_wave_checksums(expected, rounds: int):
    """np.uint32[4]: record field [4] of the waves of a workgroup (wave w holds
    rows 64*(w>>1).., columns 64*(w&1)..): the xor of its block's fp32 bits,
    once per round."""
    import numpy as np

    bits = np.ascontiguousarray(np.asarray(expected, dtype=np.float32)).view(np.uint32)
    out = np.zeros(4, dtype=np.uint32)
    if rounds & 1:
        for w in range(4):
            block = bits[64 * (w >> 1):64 * (w >> 1) + 64, 64 * (w & 1):64 * (w & 1) + 64]
            out[w] = np.bitwise_xor.reduce(block.ravel())
    return out


def _summarize_tiled_gemm(records, ms: float, M: int, N: int, K: int, rounds: int,
                          expected_cus: int, steps: int, step_bytes: int) -> dict:
    """The verdict of one launch of a tiled GEMM probe (gemm_pipe, mx_gemm_pipe,
    mx6_gemm_pipe: the same records). `steps` K steps per round, in each of which
    a workgroup loads `step_bytes`."""
    import numpy as np

    rec = np.asarray(records).reshape(-1, 4, 8).astype(np.int64)
    grid = int(rec.shape[0])
    sec = ms * 1e-3
    flop = 2.0 * M * N * K * rounds
    loaded = float(grid) * steps * step_bytes * rounds
    bad = BadUnits()
    flat = rec.reshape(-1, 8)
    for word, mism, first, index in flat[flat[:, 1] != 0][:, :4]:
        bad.add(decode_hw_word(word), {"waves": 1, "mismatched_elements": mism},
                (int(first), int(index)))
    mismatched_waves = int((flat[:, 1] != 0).sum())
    # the four waves of a workgroup hold different blocks: consensus per position
    checksum_spread = bool(any(checksum_outliers(rec[:, w, 4]).any() for w in range(4)))
    cus_seen = units_seen(flat[:, 0], decode_hw_word)
    return {
        "tflops": flop / sec / 1e12 if ms > 0 else 0.0,
        "operand_gbps": loaded / sec / 1e9 if ms > 0 else 0.0,
        "elapsed_ms": float(ms),
        "waves": grid * 4,
        "cus_seen": cus_seen,
        "mismatched_waves": mismatched_waves,
        "bad_cus": bad.entries(("first_bad_round", "first_bad_index")),
        "checksum_spread": checksum_spread,
        "ok": bool(mismatched_waves == 0 and not checksum_spread and cus_seen >= expected_cus),
    }


def summarize_gemm_probe(records, ms: float, fmt: str, b_layout: str, M: int, N: int, K: int,
                         rounds: int, expected_cus: int) -> dict:
    """Turn the per-wave records of one ops.gemm_pipe launch into a verdict.

    records: [grid*4, 8] int32 rows {hw word, mismatched elements, first bad
    round (-1), first bad element of the wave's 64x64 block (-1), xor checksum,
    0, 0, 0}. `operand_gbps` is the bytes the workgroups load into LDS over the
    time, not HBM bandwidth: L2 and the Infinity Cache serve the reuse. The
    rates are reported, never judged. Pure numpy; needs no GPU.
    """
    return _summarize_tiled_gemm(records, ms, M, N, K, rounds, expected_cus,
                                 K // gemm_probe_bk(fmt), 2 * GEMM_TILE * _STEP_BYTES)


def lds_tr_map_report(device: int = 0) -> dict:
    """Every transpose-read width against the mirror, on the GEMM's tile
    addressing and on another stride and base, a pattern and its complement:
    {str(width): bool}."""
    import numpy as np
    import torch

    from . import _ops_on

    ops = _ops_on(device)
    out = {}
    for width in LDS_TR_WIDTHS:
        ok = True
        for complement in (False, True):
            image = lds_tr_image(4096, seed=width, complement=complement)
            for addrs in (lds_tr_tile_addrs(width, 256 if width == 16 else 128,
                                            group_rows=8 if width == 16 else 16),
                          lds_tr_tile_addrs(width, 80, base=1040)):
                got = ops.lds_tr_read(width, torch.from_numpy(image).cuda(device),
                                      torch.from_numpy(addrs))
                ok = ok and np.array_equal(got.cpu().numpy(),
                                           lds_tr_expected(width, image, addrs))
        out[str(width)] = bool(ok)
    return out


def _tiled_gemm_report(device: int, cases, M, N, K, rounds, inject, op: str, operands,
                       summarize, case_name) -> dict:
    """What the three tiled GEMM probes' report functions share: every case's
    `operands(*case, M, N, K)` through ops.<op>, its records through
    `summarize`, under `case_name(*case)`; `ok` the AND and `bad_cus` the union
    over the cases."""
    from . import _ops_on

    ops = _ops_on(device)
    M = _DEFAULT_MNK[0] if M is None else int(M)
    N = _DEFAULT_MNK[1] if N is None else int(N)
    K = _DEFAULT_MNK[2] if K is None else int(K)
    rounds = _DEFAULT_ROUNDS if rounds is None else int(rounds)
    inject_block, inject_round = (-1, -1) if inject is None else inject
    expected_cus = ops.device_info(device)["multiProcessorCount"]
    out: dict = {"M": M, "N": N, "K": K, "rounds": rounds, "cases": {}}
    bad = set()
    for case in cases:
        tensors = operands(*case, M, N, K)
        records, _, ms = getattr(ops, op)(*(t.cuda(device) for t in tensors), *case, rounds,
                                          False, inject_block, inject_round)
        s = summarize(records.cpu().numpy(), ms, *case, M, N, K, rounds, expected_cus)
        out["cases"][case_name(*case)] = s
        bad |= place_keys(s["bad_cus"], 4)
    out["ok"] = bool(all(s["ok"] for s in out["cases"].values()))
    out["bad_cus"] = place_dicts(bad)
    return out


def gemm_probe_report(device: int = 0, cases=GEMM_PROBE_CASES, M: int = None, N: int = None,
                      K: int = None, rounds: int = None, inject=None) -> dict:
    """Run the GEMM probe's cases and the transpose-read map on one GPU.

    Returns {"cases": {"<fmt>_<layout>": summarize_gemm_probe(...)}, "tr_map":
    {width: bool}, "ok", "bad_cus"} where `ok` is the AND and `bad_cus` the
    union ((xcc, se, sh, cu) dicts, sorted). `inject=(block, round)` flips one
    accumulator bit in wave 0 of that workgroup in that round (register
    arithmetic only) to exercise detection on healthy hardware.
    """
    out = _tiled_gemm_report(device, cases, M, N, K, rounds, inject, "gemm_pipe",
                             gemm_probe_operands, summarize_gemm_probe, "{}_{}".format)
    ok, bad_cus = out.pop("ok"), out.pop("bad_cus")  # they follow tr_map, as ever
    out["tr_map"] = lds_tr_map_report(device)
    out["ok"] = bool(ok and all(out["tr_map"].values()))
    out["bad_cus"] = bad_cus
    return out
