"""MX GEMM probe (ops.mx_gemm_pipe): the GEMM probe's pipeline feeding the
block-scaled MFMA, as an MXFP8 / MXFP4 tenant's GEMM does: direct-to-LDS
loads, LDS fragment reads (4- and 8-bit transpose reads for B kn), E8M0 scale
bytes streamed from memory per 32 elements of K, and
v_mfma_scale_f32_16x16x128_f8f6f4, exact by construction, compared bitwise in
the kernel and attributed per CU. See the kernel comment in hived_ops.hip.
Pure numpy / torch on the CPU apart from the report function.
"""
from __future__ import annotations

from .gemm_probe import GEMM_TILE, _summarize_tiled_gemm, _tiled_gemm_report
from .mfma_tiles import _lossless
from .mx_scale import MX_SCALE_SPREAD, mx_encode, mx_scaled_product

MX_GEMM_FORMATS = ("mxfp8", "mxfp4")
MX_GEMM_LAYOUTS = ("kn", "nk")
MX_GEMM_CASES = tuple((f, b) for f in MX_GEMM_FORMATS for b in MX_GEMM_LAYOUTS)
_MX_CODE = {"mxfp8": 0, "mxfp4": 4}     # the instruction's format codes (mx_scale.py)
_PACK = {"mxfp8": 1, "mxfp4": 2}        # codes per byte
_STEP_BYTES = 128                       # bytes of K per row and K step
# in units of 2^-4 (two scales of 2^-2) a term is an integer of at most
# 2*2 * 2^8, so a partial sum is at most K * 2^10: fp32 holds it up to 2^24
MX_GEMM_MAX_K = (1 << 24) >> (2 + 4 * MX_SCALE_SPREAD)


def mx_gemm_bk(fmt: str) -> int:
    """Elements of K per step: 128 bytes per row."""
    return _STEP_BYTES * _PACK[fmt]


def mx_gemm_period(fmt: str) -> int:
    """K period of the probe's operands: four K steps, for the reason
    gemm_probe_period gives (a stale LDS stage holds step k-2)."""
    return 4 * mx_gemm_bk(fmt)


def mx_gemm_pack(codes, fmt: str, axis: int = -1):
    """One code per byte to the op's bytes: mxfp8 unchanged; mxfp4 two codes
    per byte along `axis`, the even element in the low nibble."""
    import torch

    codes = codes.to(torch.uint8)
    if _PACK[fmt] == 1:
        return codes.contiguous()
    c = codes.movedim(axis, -1)
    assert c.shape[-1] % 2 == 0 and int(c.max()) < 16, "e2m1 codes, an even number along axis"
    return (c[..., 0::2] | (c[..., 1::2] << 4)).movedim(-1, axis).contiguous()


def mx_gemm_unpack(packed, fmt: str, axis: int = -1):
    """The inverse of mx_gemm_pack."""
    import torch

    if _PACK[fmt] == 1:
        return packed.contiguous()
    p = packed.movedim(axis, -1)
    c = torch.stack((p & 15, p >> 4), dim=-1).flatten(-2)
    return c.movedim(-1, axis).contiguous()


def mx_gemm_reference(fmt: str, b_layout: str, A, B, scale_a, scale_b):
    """The float64 product [M,N] of the operands as the op takes them."""
    a = mx_gemm_unpack(A, fmt)
    b = mx_gemm_unpack(B, fmt)
    if b_layout == "nk":
        b, scale_b = b.t(), scale_b.t()
    return mx_scaled_product(_MX_CODE[fmt], _MX_CODE[fmt], a, b, scale_a, scale_b)


def _mx_encode_ints(ints, code: int):
    """Integers in {-2..2} as codes of the format with the instruction's format
    code `code`, one per byte."""
    import torch

    table = mx_encode(code, torch.arange(-2, 3).double())
    return table[ints.long() + 2]


def mx_gemm_encode(ints, fmt: str):
    """Integers in {-2..2} as codes of the format, one per byte."""
    return _mx_encode_ints(ints, _MX_CODE[fmt])


def mx_gemm_layout(fmt: str, b_layout: str, a, b, sa, sb):
    """Integer operands a [M,K], b [K,N] in {-2..2} and scale bytes sa [M,K/32],
    sb [K/32,N] as the op takes them: (A, B, scale_a, scale_b)."""
    A = mx_gemm_pack(mx_gemm_encode(a, fmt), fmt)
    b, sb = (b, sb) if b_layout == "kn" else (b.t(), sb.t())
    return A, mx_gemm_pack(mx_gemm_encode(b, fmt), fmt), sa.contiguous(), sb.contiguous()


def _mx_units(code_a: int, code_b: int, P: int, seed: int = 0):
    """One period of the operands, the sides in the formats with the
    instruction's codes code_a and code_b: int64 a [128,P], b [P,128] in
    {-2..2} and uint8 scales sa [128,P/32], sb [P/32,128] in 127 +-
    MX_SCALE_SPREAD, drawn per (row, block) and (block, column), and the unit
    tile. b is the fixed asymmetric pattern of _gemm_probe_units; rows of a are
    redrawn until no element of the scaled product is zero, so a dead
    accumulator differs everywhere."""
    import torch

    g = torch.Generator().manual_seed(seed)
    k = torch.arange(P, dtype=torch.int64).unsqueeze(1)
    n = torch.arange(GEMM_TILE, dtype=torch.int64).unsqueeze(0)
    b = (3 * k + n + seed) % 5 - 2
    lo, hi = 127 - MX_SCALE_SPREAD, 127 + MX_SCALE_SPREAD + 1
    sa = torch.randint(lo, hi, (GEMM_TILE, P // 32), generator=g, dtype=torch.uint8)
    sb = torch.randint(lo, hi, (P // 32, GEMM_TILE), generator=g, dtype=torch.uint8)
    a = torch.randint(-2, 3, (GEMM_TILE, P), generator=g, dtype=torch.int64)
    b_codes = _mx_encode_ints(b, code_b)
    while True:
        unit = mx_scaled_product(code_a, code_b, _mx_encode_ints(a, code_a), b_codes, sa, sb)
        redraw = (unit == 0).any(dim=1)
        if not redraw.any():
            return a, b, sa, sb, unit
        a[redraw] = torch.randint(-2, 3, (int(redraw.sum()), P), generator=g, dtype=torch.int64)


def _mx_tiled_operands(code_a: int, code_b: int, P: int, layout, b_layout: str, M: int, N: int,
                       K: int, seed: int):
    """The operands of an MX tiled GEMM probe from one period's units:
    `layout(a, b, sa, sb)` brings the units into the op's form, and everything
    repeats with period 128 in M and N and P in K."""
    import torch

    if M % GEMM_TILE or N % GEMM_TILE or K % P or min(M, N, K) <= 0:
        raise ValueError(f"M, N must be multiples of 128 and K of {P}; got {M}, {N}, {K}")
    if K > MX_GEMM_MAX_K:
        raise ValueError(f"K {K} breaks fp32 exactness (need K * 2^10 <= 2^24)")
    a, b, sa, sb, unit = _mx_units(code_a, code_b, P, seed)
    expected = (K // P) * unit
    assert float(expected.abs().max()) * 16 <= K << 10 <= 1 << 24
    assert _lossless(expected.float(), expected) and not torch.equal(unit, unit.t())
    A, B, scale_a, scale_b = layout(a, b, sa, sb)
    tiles_b = (K // P, N // GEMM_TILE) if b_layout == "kn" else (N // GEMM_TILE, K // P)
    return (A.repeat(M // GEMM_TILE, K // P), B.repeat(*tiles_b),
            scale_a.repeat(M // GEMM_TILE, K // P), scale_b.repeat(*tiles_b),
            expected.float().contiguous())


def mx_gemm_operands(fmt: str, b_layout: str, M: int, N: int, K: int, seed: int = 0):
    """(A, B, scale_a, scale_b, expected [128,128] fp32) on the CPU, as the op
    takes them. Everything repeats with period 128 in M and N and P = 4 K
    steps in K: every workgroup streams its own addresses and every tile of C
    is (K/P) * the unit tile.

    Why the result is exact: operands are integers of magnitude <= 2 and each
    side's scale is 2^-2..2^2, so in units of 2^-4 every term is an integer of
    at most 4 * 2^8 and every partial sum, in any order, an integer of at most
    K * 2^10, which fp32 holds up to 2^24: K <= 16384. Inside a 32-block all
    products share one power of two, within the window the fp8 pipes keep
    inside a lane group (the regime mx_scale_burn_operands runs)."""
    if fmt not in MX_GEMM_FORMATS or b_layout not in MX_GEMM_LAYOUTS:
        raise ValueError(f"unknown case {fmt}/{b_layout}")
    return _mx_tiled_operands(_MX_CODE[fmt], _MX_CODE[fmt], mx_gemm_period(fmt),
                              lambda *units: mx_gemm_layout(fmt, b_layout, *units), b_layout,
                              M, N, K, seed)


def summarize_mx_gemm_probe(records, ms: float, fmt: str, b_layout: str, M: int, N: int, K: int,
                            rounds: int, expected_cus: int) -> dict:
    """summarize_gemm_probe for one ops.mx_gemm_pipe launch: the same records
    and fields. `operand_gbps` counts what the workgroups load per K step, 32
    KiB of operands and 256 rows' scale bytes, over the time. The rates are
    reported, never judged. Pure numpy; needs no GPU."""
    bk = mx_gemm_bk(fmt)
    return _summarize_tiled_gemm(records, ms, M, N, K, rounds, expected_cus, K // bk,
                                 2 * GEMM_TILE * (_STEP_BYTES + bk // 32))


def mx_gemm_probe_report(device: int = 0, cases=MX_GEMM_CASES, M: int = None, N: int = None,
                         K: int = None, rounds: int = None, inject=None) -> dict:
    """Run the MX GEMM probe's cases on one GPU.

    Returns {"cases": {"<fmt>_<layout>": summarize_mx_gemm_probe(...)}, "ok",
    "bad_cus"} where `ok` is the AND and `bad_cus` the union ((xcc, se, sh, cu)
    dicts, sorted). `inject=(block, round)` flips one accumulator bit in wave 0
    of that workgroup in that round (register arithmetic only) to exercise
    detection on healthy hardware.
    """
    return _tiled_gemm_report(device, cases, M, N, K, rounds, inject, "mx_gemm_pipe",
                              mx_gemm_operands, summarize_mx_gemm_probe, "{}_{}".format)
