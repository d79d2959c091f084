"""Host-only tests of the MX GEMM probe's report and operands:
summarize_mx_gemm_probe on hand-made records, the invariants of
mx_gemm_operands, and the fp4 packing."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from hivedscheduler_amd.ops import mx_gemm_probe as mg  # noqa: E402

SHAPE = dict(fmt="mxfp4", b_layout="kn", M=256, N=256, K=1024, rounds=3, expected_cus=2)


def records(grid=4, cus=2):
    rec = np.zeros((grid, 4, 8), dtype=np.int32)
    rec[:, :, 0] = ((np.arange(grid) % cus) << 8)[:, None]  # CU id in HW_ID[11:8]
    rec[:, :, 2:4] = -1
    rec[:, :, 4] = np.array([11, 22, 33, 44])  # one checksum per wave position
    return rec


def test_summary_clean_bad_wave_and_missing_cu():
    s = mg.summarize_mx_gemm_probe(records().reshape(-1, 8), 2.0, **SHAPE)
    assert s["ok"] and s["waves"] == 16 and s["cus_seen"] == 2 and s["bad_cus"] == []
    assert s["tflops"] == pytest.approx(2.0 * 256 * 256 * 1024 * 3 / 2e-3 / 1e12)
    # 4 workgroups x 4 steps x (32 KiB of operands + 256 rows x 8 scale bytes) x 3 rounds
    assert s["operand_gbps"] == pytest.approx(4 * 4 * (32768 + 2048) * 3 / 2e-3 / 1e9)
    rec = records()
    rec[3, 0, 1:4] = (1, 2, 0)
    rec[3, 0, 4] ^= 1
    s = mg.summarize_mx_gemm_probe(rec.reshape(-1, 8), 2.0, **SHAPE)
    assert not s["ok"] and s["mismatched_waves"] == 1 and s["checksum_spread"]
    assert s["bad_cus"] == [{"xcc": 0, "se": 0, "sh": 0, "cu": 1, "waves": 1,
                             "mismatched_elements": 1, "first_bad_round": 2,
                             "first_bad_index": 0}]
    s = mg.summarize_mx_gemm_probe(records().reshape(-1, 8), 2.0, **{**SHAPE, "expected_cus": 3})
    assert not s["ok"] and s["cus_seen"] == 2 and not s["checksum_spread"]


@pytest.mark.parametrize("fmt,b_layout", mg.MX_GEMM_CASES)
def test_operand_invariants(fmt, b_layout):
    P, BK = mg.mx_gemm_period(fmt), mg.mx_gemm_bk(fmt)
    assert P == 4 * BK and BK == {"mxfp8": 128, "mxfp4": 256}[fmt]
    M, N, K = 256, 384, 2 * P
    A, B, sa, sb, expected = mg.mx_gemm_operands(fmt, b_layout, M, N, K)
    pack = 1 if fmt == "mxfp8" else 2
    assert A.shape == (M, K // pack) and sa.shape == (M, K // 32)
    assert B.shape == ((K, N // pack) if b_layout == "kn" else (N, K // pack))
    assert sb.shape == ((K // 32, N) if b_layout == "kn" else (N, K // 32))
    assert all(t.dtype == torch.uint8 and t.is_contiguous() for t in (A, B, sa, sb))
    # the period: 128 in M and N, P in K, in operands and scales
    a, b = mg.mx_gemm_unpack(A, fmt), mg.mx_gemm_unpack(B, fmt)
    b, sbk = (b, sb) if b_layout == "kn" else (b.t(), sb.t())
    assert a.shape == (M, K) and b.shape == (K, N)
    assert torch.equal(a[:128], a[128:]) and torch.equal(a[:, :P], a[:, P:])
    assert torch.equal(b[:P], b[P:]) and torch.equal(b[:, :128], b[:, 256:])
    assert torch.equal(sa[:128], sa[128:]) and torch.equal(sa[:, :P // 32], sa[:, P // 32:])
    assert torch.equal(sbk[:P // 32], sbk[P // 32:]) and torch.equal(sbk[:, :128], sbk[:, 256:])
    # scales in range, varying per row and per block on both sides
    for s in (sa[:128, :P // 32], sbk[:P // 32, :128].t()):
        assert int(s.min()) >= 125 and int(s.max()) <= 129
        assert (s != s[:1]).any(dim=0).all() and (s != s[:, :1]).any(dim=1).all()
    # the unit tile: no zero, asymmetric, exact in fp32, and what every tile of C is
    want = mg.mx_gemm_reference(fmt, b_layout, A, B, sa, sb)
    unit = want[:128, :128]
    assert (unit != 0).all() and not torch.equal(unit, unit.t())
    assert torch.equal(expected.double(), unit) and torch.equal(want[128:, 256:], unit)
    assert torch.equal(want.float().double(), want)
    # the four K steps of a period differ pairwise in A
    steps = [A[:128, s * 128:(s + 1) * 128] for s in range(4)]
    assert all(not torch.equal(steps[s], steps[t]) for s in range(4) for t in range(s))
    with pytest.raises(ValueError):
        mg.mx_gemm_operands(fmt, b_layout, M, N, P + BK)
    with pytest.raises(ValueError):
        mg.mx_gemm_operands(fmt, b_layout, 128, 128, mg.MX_GEMM_MAX_K + P)
    mg.mx_gemm_operands(fmt, b_layout, 128, 128, mg.MX_GEMM_MAX_K)


@pytest.mark.parametrize("axis", [0, 1])
def test_fp4_pack_round_trip(axis):
    codes = (torch.arange(6 * 8).view(6, 8) * 7 % 16).to(torch.uint8)
    packed = mg.mx_gemm_pack(codes, "mxfp4", axis)
    assert packed.shape == ((3, 8) if axis == 0 else (6, 4))
    pair = codes[0:2, 0] if axis == 0 else codes[0, 0:2]
    assert int(packed[0, 0]) == int(pair[0]) | int(pair[1]) << 4  # even element low
    assert torch.equal(mg.mx_gemm_unpack(packed, "mxfp4", axis), codes)
    assert torch.equal(mg.mx_gemm_pack(codes, "mxfp8", axis), codes)
