"""Host-only tests of the GEMM probe's report and operands: summarize_gemm_probe
on hand-made records, the invariants of gemm_probe_operands, and the transpose
mirror on blocks small enough to state by hand."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from hivedscheduler_amd.ops import gemm_probe as gp  # noqa: E402

CASES = gp.GEMM_PROBE_CASES
SHAPE = dict(fmt="bf16", b_layout="kn", M=256, N=256, K=512, rounds=3, expected_cus=2)


def records(grid=4, cus=2):
    rec = np.zeros((grid, 4, 8), dtype=np.int32)
    rec[:, :, 0] = ((np.arange(grid) % cus) << 8)[:, None]  # CU id in HW_ID[11:8]
    rec[:, :, 2:4] = -1
    rec[:, :, 4] = np.array([11, 22, 33, 44])  # one checksum per wave position
    return rec


def test_clean_records_are_ok_and_rates_follow_the_shape():
    s = gp.summarize_gemm_probe(records().reshape(-1, 8), 2.0, **SHAPE)
    assert s["ok"] and s["waves"] == 16 and s["cus_seen"] == 2 and s["bad_cus"] == []
    assert s["tflops"] == pytest.approx(2.0 * 256 * 256 * 512 * 3 / 2e-3 / 1e12)
    # 4 workgroups x 8 steps x 32 KiB x 3 rounds
    assert s["operand_gbps"] == pytest.approx(4 * 8 * 32768 * 3 / 2e-3 / 1e9)


def test_one_bad_wave_is_attributed_to_its_cu():
    rec = records()
    rec[3, 0, 1:4] = (1, 2, 0)
    rec[3, 0, 4] ^= 1
    s = gp.summarize_gemm_probe(rec.reshape(-1, 8), 2.0, **SHAPE)
    assert not s["ok"] and s["mismatched_waves"] == 1 and s["checksum_spread"]
    assert s["bad_cus"] == [{"xcc": 0, "se": 0, "sh": 0, "cu": 1, "waves": 1,
                             "mismatched_elements": 1, "first_bad_round": 2,
                             "first_bad_index": 0}]


def test_checksum_spread_and_missing_cu_are_not_ok():
    rec = records()
    rec[1, 2, 4] = 5
    s = gp.summarize_gemm_probe(rec.reshape(-1, 8), 2.0, **SHAPE)
    assert not s["ok"] and s["checksum_spread"] and s["mismatched_waves"] == 0
    s = gp.summarize_gemm_probe(records().reshape(-1, 8), 2.0, **{**SHAPE, "expected_cus": 3})
    assert not s["ok"] and s["cus_seen"] == 2 and not s["checksum_spread"]


@pytest.mark.parametrize("fmt,b_layout", CASES)
def test_operand_invariants(fmt, b_layout):
    P, BK = gp.gemm_probe_period(fmt), gp.gemm_probe_bk(fmt)
    assert P == 4 * BK and BK * {"bf16": 2, "fp8": 1}[fmt] == 128
    M, N, K = 256, 384, 2 * P
    A, B, expected = gp.gemm_probe_operands(fmt, b_layout, M, N, K)
    dec = (lambda t: t.float()) if fmt == "bf16" else \
        (lambda t: t.view(torch.float8_e4m3fn).float())
    a, b = dec(A).double(), dec(B).double()
    b = b if b_layout == "kn" else b.t()
    assert a.shape == (M, K) and b.shape == (K, N) and a.abs().max() <= 2 and b.abs().max() <= 2
    # the period: 128 in M and N, P in K
    assert torch.equal(a[:128], a[128:]) and torch.equal(a[:, :P], a[:, P:])
    assert torch.equal(b[:, :128], b[:, 256:]) and torch.equal(b[:P], b[P:])
    unit = a[:128, :P] @ b[:P, :128]
    assert (unit != 0).all()
    assert torch.equal(expected.double(), (K // P) * unit)
    assert torch.equal((a @ b)[128:, 256:], expected.double())
    # the four K steps of a period differ pairwise, in A and in B, and B is asymmetric
    steps = [(a[:128, s * BK:(s + 1) * BK], b[s * BK:(s + 1) * BK, :128]) for s in range(4)]
    for s in range(4):
        for t in range(s + 1, 4):
            assert not torch.equal(steps[s][0], steps[t][0])
            assert not torch.equal(steps[s][1], steps[t][1])
    assert not torch.equal(b[:128, :128], b[:128, :128].t())
    with pytest.raises(ValueError):
        gp.gemm_probe_operands(fmt, b_layout, M, N, P + BK)


def test_wave_checksums_cancel_over_even_rounds():
    expected = gp.gemm_probe_operands("fp8", "nk", 128, 128, 512)[2].numpy()
    odd = gp.gemm_probe_wave_checksums(expected, 3)
    assert odd[0] == np.bitwise_xor.reduce(expected[:64, :64].view(np.uint32).ravel())
    assert len(set(odd.tolist())) == 4 and not gp.gemm_probe_wave_checksums(expected, 2).any()


@pytest.mark.parametrize("width", gp.LDS_TR_WIDTHS)
def test_transpose_mirror_on_an_index_image(width):
    """Element e of row r of group g holds a value that names (g, r, e): lane i
    of the group must receive element i of every row, row 0 lowest."""
    rows = {16: 4, 8: 8, 4: 16, 6: 16}[width]
    span = gp.lds_tr_span(width)[0]
    row_bytes = 16 * width // 8
    image = np.zeros(4 * rows * 64, dtype=np.uint8)  # rows 64 bytes apart
    value = lambda g, r, e: (g * 7 + r * 5 + e * 3 + 1) % (1 << width)  # noqa: E731
    for g in range(4):
        for r in range(rows):
            packed = sum(value(g, r, e) << (width * e) for e in range(16))
            at = (g * rows + r) * 64
            image[at:at + row_bytes] = np.frombuffer(packed.to_bytes(row_bytes, "little"), np.uint8)
    addrs = gp.lds_tr_tile_addrs(width, 64)
    assert (addrs % gp.lds_tr_span(width)[1] == 0).all()
    got = gp.lds_tr_expected(width, image.view(np.int32), addrs).view(np.uint32)
    for lane in range(64):
        word = sum(int(w) << (32 * k) for k, w in enumerate(got[lane]))
        assert word < (1 << (8 * span))
        assert [(word >> (width * r)) & ((1 << width) - 1) for r in range(rows)] == \
            [value(lane // 16, r, lane % 16) for r in range(rows)]
