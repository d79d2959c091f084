"""CPU tests for the single-tile MFMA checks' host side (ops.mfma_tiles): the
operands' invariants and encodings, and that the bitwise verdict rejects every
fault a tolerance used to let through: dropped, swapped and scaled K slots,
a flipped low-order bit, a transposed C. No GPU: faults are applied to the
expected tile, or to what a fake extension returns."""
import itertools

import pytest

torch = pytest.importorskip("torch")

import hivedscheduler_amd.ops as ops  # noqa: E402
from hivedscheduler_amd.ops import (TILE_FORMATS, TILE_K, TILE_PROBE_SEEDS,  # noqa: E402
                                    decode_tile_operand, e4m3_values, encode_tile_operand,
                                    exact_tile, judge_mfma_tiles, mfma_tile_operands,
                                    tile_operand_invariants)
from test_hbm_march_report import FakeOps  # noqa: E402

SEEDS = (0, 1, 2, 3, 7)
WAVES = 8
_cache = {}


def operands(fmt, seed):
    """(A, B, expected, a64, b64), computed once per (fmt, seed) and shared."""
    if (fmt, seed) not in _cache:
        A, B, expected = mfma_tile_operands(fmt, seed)
        _cache[fmt, seed] = (A, B, expected, decode_tile_operand(fmt, A),
                             decode_tile_operand(fmt, B))
    return _cache[fmt, seed]


def flip_bit(x, bit):
    return (x.contiguous().view(torch.int32) ^ (1 << bit)).view(torch.float32)


def smallest_product_removed(a, b, expected):
    """expected with the smallest nonzero |a*b| taken out of the one element
    it belongs to."""
    prods = a.unsqueeze(2) * b.unsqueeze(0)            # [m, k, n]
    mag = prods.abs()
    mag[mag == 0] = float("inf")
    m, k, n = [int(i) for i in torch.unravel_index(mag.argmin(), mag.shape)]
    out = expected.double().clone()
    out[m, n] -= prods[m, k, n]
    return out.float()


# name -> f(a64, b64, expected fp32) -> the tile every wave returns
UNIFORM_FAULTS = {
    "k_slot_dropped": lambda a, b, e: (e.double() - a[:, 5:6] @ b[5:6, :]).float(),
    "k_quarter_dropped": lambda a, b, e: (
        e.double() - a[:, a.shape[1] // 4:a.shape[1] // 2] @ b[a.shape[1] // 4:a.shape[1] // 2, :]
    ).float(),
    "k_slots_swapped_in_a": lambda a, b, e: (
        a[:, [1, 0] + list(range(2, a.shape[1]))] @ b).float(),
    "halved": lambda a, b, e: e / 2,
    "bit14_flipped": lambda a, b, e: flip_bit(e, 14),
    "transposed": lambda a, b, e: e.T.contiguous(),
    "smallest_product_removed": smallest_product_removed,
    "lowest_bit_flipped_everywhere": lambda a, b, e: flip_bit(e, 0),
}


def waves_of(tile):
    return tile.unsqueeze(0).repeat(WAVES, 1, 1)


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("fmt", TILE_FORMATS)
def test_operand_invariants(fmt, seed):
    A, B, expected, a, b = operands(fmt, seed)
    K = TILE_K[fmt]
    assert A.shape == (16, K) and B.shape == (K, 16)
    assert A.dtype == B.dtype == (torch.bfloat16 if fmt == "bf16" else torch.uint8)
    assert A.is_contiguous() and B.is_contiguous()
    assert expected.shape == (16, 16) and expected.dtype == torch.float32
    inv = tile_operand_invariants(fmt, A, B)
    assert all(inv.values()), inv
    # spelled out, independently of the helper
    prod = a @ b
    assert torch.equal(expected.double(), prod) and (prod != 0).all()
    assert not torch.equal(expected, expected.T)
    for k1, k2 in itertools.combinations(range(K), 2):
        assert not torch.equal(a[:, k1], a[:, k2]) and not torch.equal(b[k1], b[k2])
    # deterministic
    A2, B2, e2 = mfma_tile_operands(fmt, seed)
    assert torch.equal(A2.view(torch.int16 if fmt == "bf16" else torch.uint8),
                       A.view(torch.int16 if fmt == "bf16" else torch.uint8))
    assert torch.equal(B2.float() if fmt == "bf16" else B2, B.float() if fmt == "bf16" else B)
    assert torch.equal(e2, expected)


@pytest.mark.parametrize("fmt", TILE_FORMATS)
def test_product_is_exact_in_fp32_in_any_order(fmt):
    """The reason no tolerance is needed: fp32 accumulation of the probe
    operands gives the float64 product whatever the order of the K slots."""
    _, _, expected, a, b = operands(fmt, TILE_PROBE_SEEDS[fmt])
    g = torch.Generator().manual_seed(5)
    a32, b32 = a.float(), b.float()
    for _ in range(20):
        acc = torch.zeros(16, 16)
        for k in torch.randperm(a.shape[1], generator=g).tolist():
            acc = acc + a32[:, k:k + 1] * b32[k:k + 1, :]   # one rounding per step
        assert torch.equal(acc, expected)


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("fmt", TILE_FORMATS)
def test_clean_tiles_pass(fmt, seed):
    expected = operands(fmt, seed)[2]
    assert judge_mfma_tiles(waves_of(expected), expected) == (0.0, 0.0, True)
    # by value: -0 equals 0
    z = torch.zeros(16, 16)
    assert judge_mfma_tiles(waves_of(-z), z) == (0.0, 0.0, True)


@pytest.mark.parametrize("fault", sorted(UNIFORM_FAULTS))
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("fmt", TILE_FORMATS)
def test_uniform_fault_is_rejected(fmt, seed, fault):
    """Every wave returns the same wrong tile: the spread stays 0, so only
    the comparison with the expected tile can see it."""
    _, _, expected, a, b = operands(fmt, seed)
    bad = UNIFORM_FAULTS[fault](a, b, expected)
    assert bad.dtype == torch.float32 and bad.shape == (16, 16)
    err, spread, ok = judge_mfma_tiles(waves_of(bad), expected)
    assert ok is False and err > 0.0 and spread == 0.0


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("fmt", TILE_FORMATS)
def test_one_bit_in_one_wave_is_rejected(fmt, seed):
    expected = operands(fmt, seed)[2]
    for wave in (0, 3, WAVES - 1):
        tiles = waves_of(expected)
        tiles[wave, 9, 4] = flip_bit(tiles[wave, 9, 4], 0)
        err, spread, ok = judge_mfma_tiles(tiles, expected)
        assert ok is False and err > 0.0 and spread > 0.0


def test_nan_and_inf_are_rejected():
    expected = operands("fp8", 1)[2]
    for poison in (float("nan"), float("inf")):
        tiles = waves_of(expected)
        tiles[2, 0, 0] = poison
        assert judge_mfma_tiles(tiles, expected)[2] is False


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("fmt", TILE_FORMATS)
def test_every_slot_swap_changes_expected(fmt, seed):
    """All K(K-1)/2 swaps of two K slots, in A alone and in B alone."""
    _, _, expected, a, b = operands(fmt, seed)
    K = TILE_K[fmt]
    prod = expected.double()
    for k1, k2 in itertools.combinations(range(K), 2):
        # swapping slots k1, k2 of A adds (a[:,k1]-a[:,k2]) x (b[k2]-b[k1]);
        # the same term comes from swapping them in B
        delta = torch.outer(a[:, k1] - a[:, k2], b[k2] - b[k1])
        assert (delta != 0).any(), (k1, k2)
        assert not torch.equal((prod + delta).float(), expected), (k1, k2)
    # the outer-product shortcut is the swap: spot-check against a real one
    perm = list(range(K))
    perm[2], perm[K - 1] = perm[K - 1], perm[2]
    delta = torch.outer(a[:, 2] - a[:, K - 1], b[K - 1] - b[2])
    assert torch.equal(a[:, perm] @ b, prod + delta)
    assert torch.equal(a @ b[perm, :], prod + delta)


# ---------------------------------------------------------------------------
# the two relative bounds of the GPU tests (inexact inputs) still see a
# dropped K slot
# ---------------------------------------------------------------------------
def dropped_slot_escapes(a, b, c):
    """K slots whose loss the bound c * 2^-24 * (|a| @ |b|) would not notice."""
    bound = c * 2.0 ** -24 * (a.abs() @ b.abs())
    return [k for k in range(a.shape[1])
            if not (torch.outer(a[:, k], b[k]).abs() > bound).any()]


def test_bf16_randn_bound_rejects_a_dropped_k_slot():
    from test_gpu import BF16_RANDN_C, BF16_RANDN_MEASURED_RATIO, bf16_randn_operands

    # the next power of two above four times the measured ratio
    assert BF16_RANDN_C / 2 <= 4 * BF16_RANDN_MEASURED_RATIO < BF16_RANDN_C
    assert BF16_RANDN_C & (BF16_RANDN_C - 1) == 0
    A, B = bf16_randn_operands()
    assert dropped_slot_escapes(A.double(), B.double(), BF16_RANDN_C) == []


def test_e4m3_randn_bound_rejects_a_dropped_k_slot():
    from test_gpu_mfma_tiles import (E4M3_RANDN_C, E4M3_RANDN_MEASURED_RATIO, E4M3_RANDN_SEEDS,
                                     randn_e4m3_operands)

    assert E4M3_RANDN_C / 2 <= 4 * E4M3_RANDN_MEASURED_RATIO < E4M3_RANDN_C
    assert E4M3_RANDN_C & (E4M3_RANDN_C - 1) == 0
    for fmt in ("fp8", "mx8"):
        for seed in E4M3_RANDN_SEEDS:
            A, B = randn_e4m3_operands(fmt, seed)
            a, b = decode_tile_operand(fmt, A), decode_tile_operand(fmt, B)
            assert dropped_slot_escapes(a, b, E4M3_RANDN_C) == []


def test_e4m3_group_window():
    """The window predicate on hand-made cases: 2^p + 2^-18 in one lane group
    is inside up to p = -5, in two lane groups always."""
    from hivedscheduler_amd.ops import E4M3_GROUP_WINDOW_BITS, e4m3_within_group_window

    assert E4M3_GROUP_WINDOW_BITS == 13
    for fmt, group in (("fp8", 8), ("mx8", 32)):
        K = TILE_K[fmt]
        for slot, same_group in ((1, True), (group - 1, True), (group, False), (K - 1, False)):
            a = torch.zeros(16, K, dtype=torch.float64)
            b = torch.zeros(K, 16, dtype=torch.float64)
            a[:, 0] = 2.0 ** (torch.arange(16, dtype=torch.float64) - 9)   # 2^-9 .. 2^6
            b[0, :] = 1.0
            a[:, slot] = b[slot, :] = 2.0 ** -9
            inside = e4m3_within_group_window(fmt, encode_tile_operand(fmt, a),
                                              encode_tile_operand(fmt, b))
            want = torch.ones(16, dtype=torch.bool)
            if same_group:
                want[5:] = False          # rows with 2^-4 and above
            assert torch.equal(inside, want.unsqueeze(1).expand(16, 16)), (fmt, slot)
    # the probe operands are inside by construction
    for fmt in ("fp8", "mx8"):
        A, B, _ = mfma_tile_operands(fmt, TILE_PROBE_SEEDS[fmt])
        assert e4m3_within_group_window(fmt, A, B).all()


# ---------------------------------------------------------------------------
# encodings
# ---------------------------------------------------------------------------
def test_e4m3_table_matches_torch_and_round_trips():
    table = e4m3_values()
    codes = torch.arange(256, dtype=torch.uint8)
    via_torch = codes.view(torch.float8_e4m3fn).double()
    finite = torch.isfinite(table)
    assert finite.sum() == 254 and not finite[0x7F] and not finite[0xFF]
    assert torch.equal(torch.isnan(via_torch), ~finite)
    assert torch.equal(table[finite], via_torch[finite])
    assert table[finite].abs().max() == 448.0 and table[1] == 2.0 ** -9
    # every finite value is a multiple of 2^-9
    assert torch.equal(table[finite] * 512, (table[finite] * 512).round())
    # value -> code -> value, and code -> value -> code (but -0 -> 0 is +0's code)
    back = encode_tile_operand("fp8", table[finite])
    assert torch.equal(decode_tile_operand("fp8", back), table[finite])
    keep = finite & (codes != 0x80)
    assert torch.equal(encode_tile_operand("mx8", table[keep]), codes[keep])


def test_e2m1_and_bf16_round_trip():
    codes = torch.arange(16, dtype=torch.uint8)
    vals = decode_tile_operand("mx4", codes)
    assert vals.tolist() == [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0,
                             -0.0, -0.5, -1.0, -1.5, -2.0, -3.0, -4.0, -6.0]
    keep = codes != 8
    assert torch.equal(encode_tile_operand("mx4", vals[keep]), codes[keep])
    i = torch.arange(-255, 256, dtype=torch.float64)
    for scale in (1.0, 256.0):
        x = encode_tile_operand("bf16", i / scale)
        assert x.dtype == torch.bfloat16 and torch.equal(x.double(), i / scale)
    # what the formats cannot hold is refused, not rounded
    for fmt, v in (("bf16", 257.0), ("fp8", 17.0), ("mx8", 2.0 ** -10), ("mx4", 5.0)):
        with pytest.raises(AssertionError):
            encode_tile_operand(fmt, torch.tensor([v], dtype=torch.float64))


def test_exact_tile_refuses_an_inexact_product():
    a = encode_tile_operand("bf16", torch.full((16, 32), 1 + 2.0 ** -7, dtype=torch.float64))
    b = encode_tile_operand("bf16", torch.full((32, 16), 2.0 ** -30, dtype=torch.float64))
    b[0] = 1.0
    with pytest.raises(AssertionError):
        exact_tile("bf16", a, b)


# ---------------------------------------------------------------------------
# the report
# ---------------------------------------------------------------------------
class FaultyOps(FakeOps):
    """FakeOps whose single-tile kernel `broken` returns tiles put through
    `mutate` ([waves,16,16] -> the same)."""

    def __init__(self, broken, mutate):
        self.broken, self.mutate = broken, mutate

    def _answer(self, name, tiles):
        return self.mutate(tiles.clone()) if name == self.broken else tiles

    def mfma_check(self, A, B, blocks, repeats):
        return self._answer("bf16", super().mfma_check(A, B, blocks, repeats))

    def mfma_check_fp8(self, A, B, blocks):
        return self._answer("fp8", super().mfma_check_fp8(A, B, blocks))

    def mfma_check_mx(self, A, B, blocks, fmt):
        name = "mx8" if fmt == 0 else "mx4"
        if fmt == 0:   # the parent routes this through mfma_check_fp8
            tiles = FakeOps.mfma_check_fp8(self, A, B, blocks)
        else:
            tiles = super().mfma_check_mx(A, B, blocks, fmt)
        return self._answer(name, tiles)


def one_wave_one_bit(tiles):
    tiles[1, 3, 5] = flip_bit(tiles[1, 3, 5], 0)
    return tiles


REPORT_FAULTS = {
    "halved": lambda t: t / 2,
    "bit14_flipped": lambda t: flip_bit(t, 14),
    "lowest_bit_flipped_everywhere": lambda t: flip_bit(t, 0),
    "lowest_bit_flipped_in_one_wave": one_wave_one_bit,
    "transposed": lambda t: t.transpose(1, 2).contiguous(),
    "one_element_zeroed": lambda t: t * (torch.arange(256).view(1, 16, 16) != 77),
}
REPORT_KEYS = {"bf16": "mfma", "fp8": "mfma_fp8", "mx8": "mfma_mx8", "mx4": "mfma_fp4"}


@pytest.fixture()
def cpu_report(monkeypatch):
    """gpu_health_report over a fake extension, everything on the CPU."""
    monkeypatch.setattr(torch.cuda, "set_device", lambda d: None)
    monkeypatch.setattr(torch.Tensor, "cuda", lambda self, *a, **k: self)

    def report(fake):
        monkeypatch.setattr(ops, "get_ops", lambda: fake)
        return ops.gpu_health_report(0, quick=True)

    return report


def test_report_healthy_is_exact(cpu_report):
    rep = cpu_report(FakeOps())
    for key in REPORT_KEYS.values():
        assert rep[f"{key}_max_err_vs_fp32"] == 0.0 and rep[f"{key}_cross_cu_spread"] == 0.0
        assert rep[f"{key}_ok"] is True
    assert rep["mfma_ok"] is True and rep["mfma_lowprec_ok"] is True and rep["healthy"] is True


@pytest.mark.parametrize("fault", sorted(REPORT_FAULTS))
@pytest.mark.parametrize("fmt", TILE_FORMATS)
def test_report_flips_on_a_faulty_kernel(cpu_report, fmt, fault):
    rep = cpu_report(FaultyOps(fmt, REPORT_FAULTS[fault]))
    key = REPORT_KEYS[fmt]
    assert rep[f"{key}_ok"] is False and rep[f"{key}_max_err_vs_fp32"] > 0.0
    assert rep["mfma_ok" if fmt == "bf16" else "mfma_lowprec_ok"] is False
    assert rep["healthy"] is False
    # the other formats' verdicts are untouched
    for other, okey in REPORT_KEYS.items():
        if other != fmt:
            assert rep[f"{okey}_ok"] is True and rep[f"{okey}_max_err_vs_fp32"] == 0.0
    assert rep["mfma_ok" if fmt != "bf16" else "mfma_lowprec_ok"] is True


def test_report_uses_the_probe_operands(cpu_report):
    """The kernels get the mfma_tile_operands inputs, encoded and positional."""
    seen = {}

    class Recording(FakeOps):
        def mfma_check(self, A, B, blocks, repeats):
            seen["bf16"] = (A, B, blocks, repeats)
            return super().mfma_check(A, B, blocks, repeats)

        def mfma_check_fp8(self, A, B, blocks):
            seen.setdefault("fp8", (A, B, blocks))
            return super().mfma_check_fp8(A, B, blocks)

        def mfma_check_mx(self, A, B, blocks, fmt):
            seen["mx8" if fmt == 0 else "mx4"] = (A, B, blocks, fmt)
            return super().mfma_check_mx(A, B, blocks, fmt)

    cpu_report(Recording())
    for fmt in TILE_FORMATS:
        A, B, _ = mfma_tile_operands(fmt, TILE_PROBE_SEEDS[fmt])
        got = seen[fmt]
        assert got[0].dtype == A.dtype and got[2] == 2048
        assert torch.equal(got[0].double() if fmt == "bf16" else got[0],
                           A.double() if fmt == "bf16" else A)
        assert torch.equal(got[1].double() if fmt == "bf16" else got[1],
                           B.double() if fmt == "bf16" else B)
    assert seen["bf16"][3] == 1 and seen["mx8"][3] == 0 and seen["mx4"][3] == 4
