"""MX6 GEMM probe (ops.mx6_gemm_pipe): the MX GEMM probe's pipeline for the
operands whose rows are not 128 bytes, as an MXFP6 / MXBF6 tenant's GEMM and a
W6A8 / W4A8 serving GEMM run it: 6-bit codes, four in three bytes (96-byte rows
of 128 elements, ds_read_b96_tr_b6 for B kn), and an MXFP8 A against MXFP6 or
MXFP4 weights in [N,K], two row pitches into one scaled MFMA. Exact by
construction, compared bitwise in the kernel and attributed per CU. See the
kernel comment in hived_ops.hip. Pure numpy / torch on the CPU apart from the
report function.
"""
from __future__ import annotations

from .gemm_probe import GEMM_TILE, _summarize_tiled_gemm, _tiled_gemm_report
from .mx_gemm_probe import (MX_GEMM_MAX_K, _mx_encode_ints,  # noqa: F401
                            _mx_tiled_operands, mx_gemm_pack, mx_gemm_unpack)
from .mx_scale import mx_scaled_product

# format name: (bits per code, the instruction's format code (mx_scale.py))
_MX6_FORMATS = {"mxfp8": (8, 0), "mxfp6": (6, 2), "mxbf6": (6, 3), "mxfp4": (4, 4)}
# (a_fmt, b_fmt, b_layout): what the kernel is instantiated for
MX6_GEMM_CASES = (("mxfp6", "mxfp6", "nk"), ("mxfp6", "mxfp6", "kn"),
                  ("mxbf6", "mxbf6", "nk"), ("mxbf6", "mxbf6", "kn"),
                  ("mxfp8", "mxfp6", "nk"), ("mxfp8", "mxfp4", "nk"))
MX6_GEMM_BK = 128                       # elements of K per step, in every case
MX6_GEMM_PERIOD = 4 * MX6_GEMM_BK       # as mx_gemm_period: a stale stage holds step k-2


def mx6_gemm_case_name(a_fmt: str, b_fmt: str, b_layout: str) -> str:
    """mxfp6_nk, mxbf6_kn, mxfp8xfp6_nk, ..."""
    return (a_fmt if a_fmt == b_fmt else f"{a_fmt}x{b_fmt[2:]}") + f"_{b_layout}"


def _check_case(a_fmt: str, b_fmt: str, b_layout: str):
    if (a_fmt, b_fmt, b_layout) not in MX6_GEMM_CASES:
        raise ValueError(f"unknown case {a_fmt} x {b_fmt} {b_layout}")


def mx6_pack6(codes, axis: int = -1):
    """One 6-bit code per byte to four codes in three bytes along `axis`: a
    little-endian bit stream, code j in bits [6j, 6j+6), as the MFMA takes it."""
    import torch

    c = codes.to(torch.int32).movedim(axis, -1)
    assert c.shape[-1] % 4 == 0 and int(c.max()) < 64, "6-bit codes, a multiple of four along axis"
    c = c.reshape(*c.shape[:-1], -1, 4)
    word = c[..., 0] | (c[..., 1] << 6) | (c[..., 2] << 12) | (c[..., 3] << 18)
    out = torch.stack((word & 255, (word >> 8) & 255, word >> 16), dim=-1).flatten(-2)
    return out.to(torch.uint8).movedim(-1, axis).contiguous()


def mx6_unpack6(packed, axis: int = -1):
    """The inverse of mx6_pack6."""
    import torch

    p = packed.to(torch.int32).movedim(axis, -1)
    p = p.reshape(*p.shape[:-1], -1, 3)
    word = p[..., 0] | (p[..., 1] << 8) | (p[..., 2] << 16)
    out = torch.stack([(word >> (6 * j)) & 63 for j in range(4)], dim=-1).flatten(-2)
    return out.to(torch.uint8).movedim(-1, axis).contiguous()


def _pack(codes, fmt: str, axis: int = -1):
    bits = _MX6_FORMATS[fmt][0]
    return mx6_pack6(codes, axis) if bits == 6 else \
        mx_gemm_pack(codes, "mxfp4" if bits == 4 else "mxfp8", axis)


def _unpack(packed, fmt: str, axis: int = -1):
    bits = _MX6_FORMATS[fmt][0]
    return mx6_unpack6(packed, axis) if bits == 6 else \
        mx_gemm_unpack(packed, "mxfp4" if bits == 4 else "mxfp8", axis)


def _encode(ints, fmt: str):
    return _mx_encode_ints(ints, _MX6_FORMATS[fmt][1])


def mx6_gemm_reference(a_fmt: str, b_fmt: str, b_layout: str, A, B, scale_a, scale_b):
    """The float64 product [M,N] of the operands as the op takes them."""
    a = _unpack(A, a_fmt)
    b = _unpack(B, b_fmt)
    if b_layout == "nk":
        b, scale_b = b.t(), scale_b.t()
    return mx_scaled_product(_MX6_FORMATS[a_fmt][1], _MX6_FORMATS[b_fmt][1], a, b, scale_a,
                             scale_b)


def mx6_gemm_layout(a_fmt: str, b_fmt: str, b_layout: str, a, b, sa, sb):
    """Integer operands a [M,K], b [K,N] in {-2..2} and scale bytes sa [M,K/32],
    sb [K/32,N] as the op takes them: (A, B, scale_a, scale_b)."""
    _check_case(a_fmt, b_fmt, b_layout)
    b, sb = (b, sb) if b_layout == "kn" else (b.t(), sb.t())
    return (_pack(_encode(a, a_fmt), a_fmt), _pack(_encode(b, b_fmt), b_fmt), sa.contiguous(),
            sb.contiguous())


def mx6_gemm_operands(a_fmt: str, b_fmt: str, b_layout: str, M: int, N: int, K: int,
                      seed: int = 0):
    """(A, B, scale_a, scale_b, expected [128,128] fp32) on the CPU, as the op
    takes them: period 128 in M and N and four K steps (512) in K, so every
    tile of C is (K/512) * the unit tile. Exact for the reason mx_gemm_operands
    gives, which does not depend on the format: integers of magnitude <= 2
    (exact codes in e4m3, e2m3, e3m2 and e2m1) under scales 2^-2..2^2, every
    partial sum an integer of at most K * 2^10 units of 2^-4: K <= 16384."""
    _check_case(a_fmt, b_fmt, b_layout)
    return _mx_tiled_operands(_MX6_FORMATS[a_fmt][1], _MX6_FORMATS[b_fmt][1], MX6_GEMM_PERIOD,
                              lambda *units: mx6_gemm_layout(a_fmt, b_fmt, b_layout, *units),
                              b_layout, M, N, K, seed)


def mx6_gemm_step_bytes(a_fmt: str, b_fmt: str, b_layout: str) -> int:
    """Bytes one workgroup loads per K step: 128 rows of 16 bytes per bit of
    width on each side (B kn: 128 bytes per k row, the dword loads fetch the
    padding word too) and 256 rows' four scale bytes."""
    b_row = 128 if b_layout == "kn" else 16 * _MX6_FORMATS[b_fmt][0]
    return GEMM_TILE * (16 * _MX6_FORMATS[a_fmt][0] + b_row) + 2 * GEMM_TILE * (MX6_GEMM_BK // 32)


def summarize_mx6_gemm_probe(records, ms: float, a_fmt: str, b_fmt: str, b_layout: str, M: int,
                             N: int, K: int, rounds: int, expected_cus: int) -> dict:
    """summarize_gemm_probe for one ops.mx6_gemm_pipe launch: the same records
    and fields. `operand_gbps` counts what the workgroups load per K step
    (mx6_gemm_step_bytes) over the time. The rates are reported, never judged.
    Pure numpy; needs no GPU."""
    return _summarize_tiled_gemm(records, ms, M, N, K, rounds, expected_cus, K // MX6_GEMM_BK,
                                 mx6_gemm_step_bytes(a_fmt, b_fmt, b_layout))


def mx6_gemm_probe_report(device: int = 0, cases=MX6_GEMM_CASES, M: int = None, N: int = None,
                          K: int = None, rounds: int = None, inject=None) -> dict:
    """Run the MX6 GEMM probe's cases on one GPU.

    Returns {"cases": {mx6_gemm_case_name: summarize_mx6_gemm_probe(...)}, "ok",
    "bad_cus"} where `ok` is the AND and `bad_cus` the union ((xcc, se, sh, cu)
    dicts, sorted). `inject=(block, round)` flips
    one accumulator bit in wave 0 of that workgroup in that round (register
    arithmetic only) to exercise detection on healthy hardware.
    """
    return _tiled_gemm_report(device, cases, M, N, K, rounds, inject, "mx6_gemm_pipe",
                              mx6_gemm_operands, summarize_mx6_gemm_probe, mx6_gemm_case_name)
