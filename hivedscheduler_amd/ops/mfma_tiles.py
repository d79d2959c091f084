"""Single-tile MFMA checks (ops.mfma_check, mfma_check_fp8, mfma_check_mx):
operands whose product fp32 holds exactly, and the bitwise verdict on the
tiles the kernels return. Pure torch on the CPU; see the kernel comments in
hived_ops.hip.

Why no tolerance is needed: bf16 inputs that are multiples of 2^-8 below 1
give products that are multiples of 2^-16 and sums below 32: 21 bits, which
fp32 holds, with every partial sum on the way, in any summation order. e2m1
values give multiples of 1/4 below 36 * 128. For e4m3 the same argument
(multiples of 2^-18, sums below 64, 24 bits) holds for an fp32 accumulator
but not for the MI355X: its fp8 MFMA drops low-order bits of small products
next to large ones (measured, BENCHMARKS.md), so randn-like e4m3 operands are
not bitwise reproducible from a float64 reference. The e4m3 operands here
are therefore built by exponent field: row m of A has every code in exponent
field m, column n of B in field n, so all products of one output element are
integers (at most 15 * 15) times one power of two, and their sum is exact on
any accumulator of 15 bits or more.
"""
from __future__ import annotations

TILE_FORMATS = ("bf16", "fp8", "mx8", "mx4")
TILE_K = {"bf16": 32, "fp8": 32, "mx8": 128, "mx4": 128}
# the seed gpu_health_report uses for each format
TILE_PROBE_SEEDS = {"bf16": 0, "fp8": 1, "mx8": 2, "mx4": 3}
_FP4_E2M1_VALUES = [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0,
                    -0.0, -0.5, -1.0, -1.5, -2.0, -3.0, -4.0, -6.0]
# bits below the leading bit of a lane group's largest product that the fp8
# pipes keep (measured on an MI355X; see e4m3_within_group_window)
E4M3_GROUP_WINDOW_BITS = 13
# the two NaN codes of OCP e4m3fn; every other code is finite (no infinities)
E4M3_NAN_CODES = (0x7F, 0xFF)


def e4m3_values():
    """float64 value of each of the 256 OCP e4m3fn codes (NaN for 0x7F, 0xFF):
    sign, 4 exponent bits (bias 7), 3 mantissa bits; exponent field 0 is
    subnormal, m * 2^-9."""
    import torch

    code = torch.arange(256, dtype=torch.int64)
    exp, man = (code >> 3) & 15, (code & 7).double()
    mag = torch.where(exp == 0, man * 2.0 ** -9, (8.0 + man) * torch.pow(2.0, (exp - 10).double()))
    val = torch.where(code >> 7 == 1, -mag, mag)
    val[list(E4M3_NAN_CODES)] = float("nan")
    return val


def decode_tile_operand(fmt: str, X):
    """The float64 values of an operand encoded for `fmt`: a bf16 tensor, raw
    e4m3 bytes (fp8, mx8) or e2m1 codes 0..15 one per byte (mx4)."""
    import torch

    if fmt == "bf16":
        assert X.dtype == torch.bfloat16, X.dtype
        return X.double()
    assert X.dtype == torch.uint8, X.dtype
    if fmt in ("fp8", "mx8"):
        return e4m3_values()[X.long()]
    assert fmt == "mx4", fmt
    assert int(X.max()) < 16
    return torch.tensor(_FP4_E2M1_VALUES, dtype=torch.float64)[X.long()]


def encode_tile_operand(fmt: str, values):
    """Encode float64 `values` for `fmt`; asserts that nothing is lost. (mx4:
    zero becomes code 0, so code 8, -0, is never produced.)"""
    import torch

    values = values.double()
    if fmt == "bf16":
        X = values.to(torch.bfloat16)
    elif fmt in ("fp8", "mx8"):
        X = values.float().to(torch.float8_e4m3fn).view(torch.uint8)
    else:
        lut = torch.tensor(_FP4_E2M1_VALUES[:8] + _FP4_E2M1_VALUES[9:], dtype=torch.float64)
        idx = (values.unsqueeze(-1) == lut).double().argmax(-1)
        X = torch.where(idx >= 8, idx + 1, idx).to(torch.uint8)
    assert torch.equal(decode_tile_operand(fmt, X), values), f"{fmt} cannot hold these values"
    return X.contiguous()


def tile_product(fmt: str, A, B):
    """float64 product of two encoded operands."""
    return decode_tile_operand(fmt, A) @ decode_tile_operand(fmt, B)


def _lossless(x32, x64) -> bool:
    """True if the fp32 tensor holds the finite float64 one without loss."""
    import torch

    return bool(torch.isfinite(x64).all()) and torch.equal(x32.double(), x64)


def exact_tile(fmt: str, A, B):
    """The [16,16] fp32 tile a healthy GPU must return for encoded operands
    whose product fp32 holds exactly: the float64 product, cast. Asserts that
    the cast loses nothing."""
    prod = tile_product(fmt, A, B)
    expected = prod.float()
    assert _lossless(expected, prod), f"{fmt} product is not exact in fp32"
    return expected.contiguous()


def _draw(fmt: str, K: int, g):
    """One [16,K] draw: A as it is, B transposed."""
    import torch

    if fmt == "bf16":  # signed multiples of 2^-8, |i| <= 255
        i = torch.randint(-255, 256, (16, K), generator=g, dtype=torch.int64)
        return (i.double() / 256).to(torch.bfloat16)
    if fmt in ("fp8", "mx8"):  # row m: exponent field m, random sign and mantissa
        sign = torch.randint(0, 2, (16, K), generator=g, dtype=torch.int64)
        man = torch.randint(0, 8, (16, K), generator=g, dtype=torch.int64)
        code = (sign << 7) | (torch.arange(16).unsqueeze(1) << 3) | man
        nan = (code & 0x7F) == 0x7F   # 0x7F, 0xFF: lowered by one
        return (code - nan.long()).to(torch.uint8)
    return torch.randint(0, 16, (16, K), generator=g, dtype=torch.uint8)


def _e4m3_fields(X):
    return (X.long() >> 3) & 15


def e4m3_within_group_window(fmt: str, A, B):
    """[16,16] bool: True where the MI355X returns the exact product of e4m3
    operands (fmt fp8 or mx8) that an fp32 accumulator would hold exactly.

    Measured (BENCHMARKS.md): the products of one 16-lane group's share of K
    (K/4 consecutive slots) are aligned to the largest of them and bits more
    than E4M3_GROUP_WINDOW_BITS below its leading bit are dropped; across the
    four groups the sum is as wide as fp32. An element is inside the window
    if, in every group, the lowest set bit of every product is at most that
    far below the leading bit of the group's largest product. This is a
    sufficient condition: an element outside it may still come out exact.
    """
    import torch

    assert fmt in ("fp8", "mx8"), fmt
    a, b = decode_tile_operand(fmt, A), decode_tile_operand(fmt, B)
    K = TILE_K[fmt]
    # every product is an integer multiple of 2^-18 below 2^36
    p = (a.unsqueeze(2) * b.unsqueeze(0) * 2.0 ** 18).long().abs().view(16, 4, K // 4, 16)
    zero = p == 0
    top = torch.frexp(p.double())[1] - 1                       # leading bit
    low = torch.frexp((p & -p).double())[1] - 1                # lowest set bit
    top = torch.where(zero, torch.full_like(top, -1), top).amax(dim=2)
    low = torch.where(zero, torch.full_like(low, 64), low).amin(dim=2)
    return ((top - low <= E4M3_GROUP_WINDOW_BITS) | zero.all(dim=2)).all(dim=1)


def tile_operand_invariants(fmt: str, A, B) -> dict:
    """What mfma_tile_operands guarantees, as {name: bool}. Each one makes a
    class of fault visible in the product: a zeroed element (no zero in A @ B),
    a dropped K slot (no all-zero column of A or row of B), two swapped K slots
    in either operand (columns of A and rows of B pairwise different, by
    value), a transposed C (expected != expected.T), and exactness in fp32
    (for e4m3 also on the narrower window of the fp8 pipes)."""
    import torch

    a, b = decode_tile_operand(fmt, A), decode_tile_operand(fmt, B)
    prod = a @ b
    K = TILE_K[fmt]
    off = ~torch.eye(K, dtype=torch.bool)
    inv = {
        "finite": bool(torch.isfinite(a).all() and torch.isfinite(b).all()),
        "no_zero_product": bool((prod != 0).all()),
        "no_zero_slot": bool((a != 0).any(dim=0).all() and (b != 0).any(dim=1).all()),
        "a_columns_differ": bool(((a.T.unsqueeze(1) != a.T.unsqueeze(0)).any(-1) | ~off).all()),
        "b_rows_differ": bool(((b.unsqueeze(1) != b.unsqueeze(0)).any(-1) | ~off).all()),
        "asymmetric": not torch.equal(prod, prod.T),
        "exact_in_fp32": _lossless(prod.float(), prod),
    }
    if fmt == "bf16":
        inv["in_range"] = bool(torch.equal(a * 256, (a * 256).round()) and a.abs().max() < 1
                               and torch.equal(b * 256, (b * 256).round()) and b.abs().max() < 1)
    elif fmt in ("fp8", "mx8"):
        field = torch.arange(16)
        inv["in_range"] = bool((_e4m3_fields(A) == field.unsqueeze(1)).all()
                               and (_e4m3_fields(B) == field.unsqueeze(0)).all())
        inv["within_group_window"] = bool(e4m3_within_group_window(fmt, A, B).all())
    else:
        inv["in_range"] = bool(len(torch.unique(torch.cat([A.flatten(), B.flatten()]))) == 16)
    return inv


def mfma_tile_operands(fmt: str, seed: int = 0):
    """Operands for one single-tile check, on the CPU, encoded as the kernels
    take them, and the tile a healthy GPU must return.

    Returns (A [16,K], B [K,16], expected [16,16] fp32): bf16 tensors for
    bf16, raw e4m3 bytes for fp8 and mx8, e2m1 codes one per byte for mx4.
    bf16 draws signed multiples of 2^-8 below 1, mx4 all 16 codes; fp8 and mx8
    put exponent field m (0 = subnormal .. 15) in row m of A and column m of
    B with random signs and mantissas. `expected` is the float64 product cast
    to fp32, which is asserted lossless. Rows of A are redrawn until no
    element of A @ B is zero (as in _burn_integers), and the whole draw is
    repeated until every entry of tile_operand_invariants holds.
    """
    import torch

    K = TILE_K[fmt]
    g = torch.Generator().manual_seed(int(seed))
    for _ in range(64):
        A, B = _draw(fmt, K, g), _draw(fmt, K, g).T.contiguous()
        for _ in range(64):
            redraw = (tile_product(fmt, A, B) == 0).any(dim=1)
            if not redraw.any():
                break
            A[redraw] = _draw(fmt, K, g)[redraw]
        if all(tile_operand_invariants(fmt, A, B).values()):
            return A.contiguous(), B.contiguous(), exact_tile(fmt, A, B)
    raise AssertionError(f"no {fmt} operands with seed {seed} satisfy the invariants")


def judge_mfma_tiles(tiles, expected):
    """The verdict on the [waves,16,16] fp32 tiles of one single-tile check.

    Returns (max_err, spread, ok): the largest |tile - expected| over every
    wave, the largest difference between any wave's tile and wave 0's, and
    ok = every element of every wave's tile equals `expected`. The comparison
    is by value (-0 == 0; a NaN equals nothing), with no tolerance.
    """
    expected = expected.to(tiles.device).unsqueeze(0)
    max_err = (tiles - expected).abs().max().item()
    spread = (tiles - tiles[0].unsqueeze(0)).abs().max().item()
    return max_err, spread, bool((tiles == expected).all().item())


def run_mfma_tile(ops, fmt: str, A, B, blocks: int):
    """Call the single-tile kernel of `fmt` on operands already on the device,
    with the positional arguments it takes."""
    if fmt == "bf16":
        return ops.mfma_check(A, B, blocks, 1)
    if fmt == "fp8":
        return ops.mfma_check_fp8(A, B, blocks)
    return ops.mfma_check_mx(A, B, blocks, 0 if fmt == "mx8" else 4)


def mfma_tile_probe(ops, device: int, fmt: str, blocks: int = 2048):
    """One single-tile check as gpu_health_report runs it: the probe operands
    of `fmt` on every CU (8192 waves >> 256 CUs). Returns judge_mfma_tiles'
    (max_err, spread, ok)."""
    A, B, expected = mfma_tile_operands(fmt, TILE_PROBE_SEEDS[fmt])
    tiles = run_mfma_tile(ops, fmt, A.cuda(device), B.cuda(device), blocks)
    return judge_mfma_tiles(tiles, expected)
