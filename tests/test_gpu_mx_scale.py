"""GPU tests for the MX scale probe (ops.mx_scale_tile, ops.mx_scale_burn):
every wave's tile bitwise against the float64 reference of ops/mx_scale.py,
for exact scaled tiles in every instantiated format pair and both shapes, the
sweeps that pin the scale lanes, the byte select, each format's decoder, the
6-bit and 4-bit packing and the full width of the scale byte, the burn with
and without an injected bit, the refusals and the health-report wiring. That
each case is exact on the reference alone is tests/test_mx_scale_report.py."""
import pytest

torch = pytest.importorskip("torch")

from hivedscheduler_amd.ops import (MX_BURN_FORMATS, MX_FULL_WIDTH_DELTAS, MX_SCALE_PAIRS,  # noqa: E402
                                    MX_SHAPES, decode_hw_word, get_ops, gpu_health_report,
                                    mx_decode_sweep_case, mx_full_width_case, mx_k_slot_case,
                                    mx_scale_burn_operands, mx_scale_operands, mx_slot_sweep_case,
                                    summarize_mx_scale_burn)

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")]

BLOCKS = 8  # 32 waves
SHAPES = (0, 1)


def assert_exact(fmt_a, fmt_b, shape, A, B, sa, sb, expected, sel=(0, 0), blocks=BLOCKS):
    """Every wave's tile equals the float64 `expected`, which fp32 holds."""
    tiles = get_ops().mx_scale_tile(A.cuda(), B.cuda(), sa.cuda(), sb.cuda(), fmt_a, fmt_b, shape,
                                    sel[0], sel[1], blocks).cpu()
    M = MX_SHAPES[shape][0]
    assert tiles.shape == (blocks * 4, M, M) and tiles.dtype == torch.float32
    bad = (tiles.double() != expected.double().unsqueeze(0)).nonzero()
    if len(bad):
        w, m, n = bad[0].tolist()
        print("first wrong element", (w, m, n), "got", tiles[w, m, n].item(), "want",
              expected[m, n].item(), "wrong in wave 0:", int((tiles[0].double() != expected).sum()))
    assert len(bad) == 0


@pytest.mark.parametrize("seed", (0, 1))
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("fmt_a,fmt_b", MX_SCALE_PAIRS)
def test_exact_tiles(fmt_a, fmt_b, shape, seed):
    A, B, sa, sb, expected = mx_scale_operands(fmt_a, fmt_b, shape, seed)
    sel = ((fmt_a + seed) % 4, (fmt_b + shape + 2 * seed) % 4)
    assert_exact(fmt_a, fmt_b, shape, A, B, sa, sb, expected[sel], sel)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("side", ("a", "b"))
def test_scale_slot_sweep(side, shape):
    A, B, sa, sb, expected = mx_slot_sweep_case(shape, side)
    rows = expected if side == "a" else expected.T
    assert len(torch.unique(rows[:, 0])) == MX_SHAPES[shape][0]   # pairwise different
    assert_exact(0, 0, shape, A, B, sa, sb, expected)


@pytest.mark.parametrize("sel_a", range(4))
@pytest.mark.parametrize("sel_b", range(4))
def test_byte_select(sel_a, sel_b):
    A, B, sa, sb, expected = mx_scale_operands(2, 1, 1, seed=3)
    assert_exact(2, 1, 1, A, B, sa, sb, expected[sel_a, sel_b], (sel_a, sel_b))


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("side", ("a", "b"))
@pytest.mark.parametrize("fmt", range(5))
def test_decode_sweep(fmt, side, shape):
    A, B, sa, sb, expected = mx_decode_sweep_case(fmt, side, shape)
    assert_exact(fmt, fmt, shape, A, B, sa, sb, expected)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("fmt", (2, 4))
def test_k_slot_sweep(fmt, shape):
    for k in range(MX_SHAPES[shape][1]):
        A, B, sa, sb, expected = mx_k_slot_case(fmt, shape, k)
        assert_exact(fmt, fmt, shape, A, B, sa, sb, expected, blocks=1)


@pytest.mark.parametrize("shape", SHAPES)
def test_full_width_scale_bytes(shape):
    A, B, sa, sb, expected = mx_full_width_case(shape)
    print("deltas", MX_FULL_WIDTH_DELTAS[:MX_SHAPES[shape][1] // 32])
    assert_exact(0, 0, shape, A, B, sa, sb, expected)


def burn(fmt, shape, inject=(-1, -1), chain=8, rounds=4):
    A, B, sa, sb, unit = mx_scale_burn_operands(fmt, shape)
    records, ms = get_ops().mx_scale_burn(A.cuda(), B.cuda(), sa.cuda(), sb.cuda(),
                                          (unit * (chain // 4)).cuda(), fmt, shape, BLOCKS, chain,
                                          rounds, *inject)
    assert records.shape == (BLOCKS * 4, 4) and ms > 0
    return records.cpu().numpy(), summarize_mx_scale_burn(records.cpu().numpy(), ms, shape, chain,
                                                          rounds, expected_cus=1)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("fmt", MX_BURN_FORMATS)
def test_burn_is_clean_and_names_an_injected_wave(fmt, shape):
    rec, s = burn(fmt, shape)
    print(fmt, shape, "mismatched", rec[:, 1].tolist(), "checksum", hex(int(rec[0, 3]) & 0xFFFFFFFF))
    assert (rec[:, 1] == 0).all() and (rec[:, 2] == -1).all() and len(set(rec[:, 3])) == 1
    assert s["ok"] is True and s["bad_cus"] == []
    rec, s = burn(fmt, shape, inject=(5, 2))
    assert rec[5, 1] == 1 and rec[5, 2] == 2 and (rec[[w for w in range(32) if w != 5], 1] == 0).all()
    xcc, se, sh, cu = decode_hw_word(rec[5, 0])
    assert s["ok"] is False and s["mismatched_waves"] == 1 and s["checksum_spread"] is True
    assert s["bad_cus"] == [{"xcc": xcc, "se": se, "sh": sh, "cu": cu, "waves": 1,
                             "mismatched_elements": 1, "first_bad_round": 2}]


def test_refusals():
    ops = get_ops()
    A, B, sa, sb, _ = (t.cuda() for t in mx_scale_operands(2, 2, 0, 0))
    good = dict(A=A, B=B, scale_a=sa, scale_b=sb, fmt_a=2, fmt_b=2, shape=0, sel_a=0, sel_b=0,
                blocks=1)
    ops.mx_scale_tile(**good)
    nan_scale, wide = sa.clone(), A.clone()
    nan_scale[3, 1, 2], wide[0, 0] = 255, 64
    for change in (dict(scale_a=nan_scale), dict(A=wide), dict(shape=1), dict(shape=2),
                   dict(A=A.cpu()), dict(B=B.int()), dict(scale_b=sb[:, :, :2]),
                   dict(fmt_a=1), dict(fmt_b=5), dict(sel_a=4), dict(sel_b=-1), dict(blocks=0)):
        with pytest.raises(RuntimeError):
            ops.mx_scale_tile(**{**good, **change})
    A, B, sa, sb, unit = (t.cuda() for t in mx_scale_burn_operands(0, 1))
    good = [A, B, sa, sb, unit * 2, 0, 1, BLOCKS, 8, 4, -1, -1]
    for at, value in ((5, 1), (6, 0), (8, 6), (8, 512), (9, 0), (10, 32), (11, 4),
                      (2, sa + 3), (4, unit[:2])):
        with pytest.raises(RuntimeError):
            ops.mx_scale_burn(*(good[:at] + [value] + good[at + 1:]))


def test_health_report_carries_the_probe_only_when_asked():
    off = gpu_health_report(0)
    on = gpu_health_report(0, mx_scale_probe=True)
    assert "mx_scale_probe" not in off and set(on) - set(off) == {"mx_scale_probe"}
    probe = on["mx_scale_probe"]
    print({name: (round(c["elapsed_ms"], 2), round(c["tflops"])) for name, c in
           probe["burn"]["cases"].items()})
    assert len(probe["tiles"]["cases"]) == 18 and len(probe["burn"]["cases"]) == 6
    assert probe["ok"] is True and probe["bad_cus"] == [] and on["healthy"] is True
