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

from .gemm_probe import GEMM_TILE, summarize_gemm_probe
from .mfma_tiles import _lossless
from .mx_gemm_probe import MX_GEMM_MAX_K, mx_gemm_pack, mx_gemm_unpack
from .mx_scale import MX_SCALE_SPREAD, mx_encode, mx_scaled_product
from .records import place_dicts, place_keys

# format name: (bits per code, the instruction's format code (mx_scale.py))
_MX6_FORMATS = {"mxfp8": (8, 0), "mxfp6": (6, 2), "mxbf6": (6, 3), "mxfp4": (4, 4)}
# (a_fmt, b_fmt, b_layout): what the kernel is instantiated for
MX6_GEMM_CASES = (("mxfp6", "mxfp6", "nk"), ("mxfp6", "mxfp6", "kn"),
                  ("mxbf6", "mxbf6", "nk"), ("mxbf6", "mxbf6", "kn"),
                  ("mxfp8", "mxfp6", "nk"), ("mxfp8", "mxfp4", "nk"))
MX6_GEMM_BK = 128                       # elements of K per step, in every case
MX6_GEMM_PERIOD = 4 * MX6_GEMM_BK       # as mx_gemm_period: a stale stage holds step k-2
# default shape and rounds (BENCHMARKS.md "MX6 GEMM probe"): 1024 workgroups,
# four per CU of an MI355X; 99 rounds put every case's timed launch at 27 to
# 31 ms, inside what the GEMM probe's cases take; an odd number keeps the xor
# checksum non-zero
_DEFAULT_MNK = (4096, 4096, 8192)
_DEFAULT_ROUNDS = 99


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
    """Integers in {-2..2} as codes of the format, one per byte."""
    import torch

    table = mx_encode(_MX6_FORMATS[fmt][1], torch.arange(-2, 3).double())
    return table[ints.long() + 2]


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


def _mx6_gemm_units(a_fmt: str, b_fmt: str, seed: int = 0):
    """_mx_gemm_units with a format per side: one period a [128,P], b [P,128]
    in {-2..2}, scales sa [128,P/32], sb [P/32,128] in 127 +- MX_SCALE_SPREAD
    and the unit tile; rows of a redrawn until no element of it is zero."""
    import torch

    P = MX6_GEMM_PERIOD
    ca, cb = _MX6_FORMATS[a_fmt][1], _MX6_FORMATS[b_fmt][1]
    g = torch.Generator().manual_seed(seed)
    k = torch.arange(P, dtype=torch.int64).unsqueeze(1)
    n = torch.arange(GEMM_TILE, dtype=torch.int64).unsqueeze(0)
    b = (3 * k + n + seed) % 5 - 2
    lo, hi = 127 - MX_SCALE_SPREAD, 127 + MX_SCALE_SPREAD + 1
    sa = torch.randint(lo, hi, (GEMM_TILE, P // 32), generator=g, dtype=torch.uint8)
    sb = torch.randint(lo, hi, (P // 32, GEMM_TILE), generator=g, dtype=torch.uint8)
    a = torch.randint(-2, 3, (GEMM_TILE, P), generator=g, dtype=torch.int64)
    b_codes = _encode(b, b_fmt)
    while True:
        unit = mx_scaled_product(ca, cb, _encode(a, a_fmt), b_codes, sa, sb)
        redraw = (unit == 0).any(dim=1)
        if not redraw.any():
            return a, b, sa, sb, unit
        a[redraw] = torch.randint(-2, 3, (int(redraw.sum()), P), generator=g, dtype=torch.int64)


def mx6_gemm_operands(a_fmt: str, b_fmt: str, b_layout: str, M: int, N: int, K: int,
                      seed: int = 0):
    """(A, B, scale_a, scale_b, expected [128,128] fp32) on the CPU, as the op
    takes them: period 128 in M and N and four K steps (512) in K, so every
    tile of C is (K/512) * the unit tile. Exact for the reason mx_gemm_operands
    gives, which does not depend on the format: integers of magnitude <= 2
    (exact codes in e4m3, e2m3, e3m2 and e2m1) under scales 2^-2..2^2, every
    partial sum an integer of at most K * 2^10 units of 2^-4: K <= 16384."""
    import torch

    _check_case(a_fmt, b_fmt, b_layout)
    P = MX6_GEMM_PERIOD
    if M % GEMM_TILE or N % GEMM_TILE or K % P or min(M, N, K) <= 0:
        raise ValueError(f"M, N must be multiples of 128 and K of {P}; got {M}, {N}, {K}")
    if K > MX_GEMM_MAX_K:
        raise ValueError(f"K {K} breaks fp32 exactness (need K * 2^10 <= 2^24)")
    a, b, sa, sb, unit = _mx6_gemm_units(a_fmt, b_fmt, seed)
    expected = (K // P) * unit
    assert float(expected.abs().max()) * 16 <= K << 10 <= 1 << 24
    assert _lossless(expected.float(), expected) and not torch.equal(unit, unit.t())
    A, B, scale_a, scale_b = mx6_gemm_layout(a_fmt, b_fmt, b_layout, a, b, sa, sb)
    tiles_b = (K // P, N // GEMM_TILE) if b_layout == "kn" else (N // GEMM_TILE, K // P)
    return (A.repeat(M // GEMM_TILE, K // P), B.repeat(*tiles_b),
            scale_a.repeat(M // GEMM_TILE, K // P), scale_b.repeat(*tiles_b),
            expected.float().contiguous())


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
    s = summarize_gemm_probe(records, ms, "fp8", b_layout, M, N, K, rounds, expected_cus)
    grid = (M // GEMM_TILE) * (N // GEMM_TILE)
    loaded = float(grid) * (K // MX6_GEMM_BK) * mx6_gemm_step_bytes(a_fmt, b_fmt, b_layout) * rounds
    s["operand_gbps"] = loaded / (ms * 1e-3) / 1e9 if ms > 0 else 0.0
    return s


def mx6_gemm_probe_report(device: int = 0, cases=MX6_GEMM_CASES, M: int = None, N: int = None,
                          K: int = None, rounds: int = None, inject=None) -> dict:
    """Run the MX6 GEMM probe's cases on one GPU.

    Returns {"cases": {mx6_gemm_case_name: summarize_mx6_gemm_probe(...)}, "ok",
    "bad_cus"} where `ok` is the AND and `bad_cus` the union ((xcc, se, sh, cu)
    dicts, sorted). `inject=(block, round)` flips
    one accumulator bit in wave 0 of that workgroup in that round (register
    arithmetic only) to exercise detection on healthy hardware.
    """
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
        operands = mx6_gemm_operands(*case, M, N, K)
        records, _, ms = ops.mx6_gemm_pipe(*(t.cuda(device) for t in operands), *case, rounds,
                                           False, inject_block, inject_round)
        s = summarize_mx6_gemm_probe(records.cpu().numpy(), ms, *case, M, N, K, rounds,
                                     expected_cus)
        out["cases"][mx6_gemm_case_name(*case)] = s
        bad |= place_keys(s["bad_cus"], 4)
    out["ok"] = bool(all(s["ok"] for s in out["cases"].values()))
    out["bad_cus"] = place_dicts(bad)
    return out
