"""GPU tests for the MX6 GEMM probe (ops.mx6_gemm_pipe): the 6-bit and
mixed-width block-scaled GEMM against a float64 host product at the smallest
shapes at which the pipeline can go wrong, full-width scale bytes, the
in-register compare (clean, dead-wrong and injected), argument checks, the
default report and the health-report wiring. Everything is bitwise: no
tolerance."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")]

from hivedscheduler_amd import ops  # noqa: E402
from hivedscheduler_amd.ops import mx6_gemm_probe as m6  # noqa: E402

CASES = m6.MX6_GEMM_CASES
IDS = [m6.mx6_gemm_case_name(*c) for c in CASES]
BK = m6.MX6_GEMM_BK
# per-clock issue rate of the scaled MFMA at the 4-bit rate, FLOP/clk/SIMD:
# fp6 runs at it and the mixed cases below it
PEAK_FLOP_PER_CLK_SIMD = 4096


def run_gemm(case, a, b, sa, sb):
    """C of integer operands a [M,K], b [K,N] under scale bytes sa, sb, and its reference."""
    operands = m6.mx6_gemm_layout(*case, a, b, sa, sb)
    want = m6.mx6_gemm_reference(*case, *operands)
    records, C, ms = ops.get_ops().mx6_gemm_pipe(*(t.cuda() for t in operands),
                                                 torch.zeros(128, 128).cuda(), *case, 1, True)
    assert records.shape == (a.shape[0] // 128 * (b.shape[1] // 128) * 4, 8) and ms > 0
    return C.cpu().double(), want


def random_ints(M, N, K, seed):
    """Random, non-periodic integer operands in {-2..2}; B's first tile asymmetric."""
    g = torch.Generator().manual_seed(seed)
    a = torch.randint(-2, 3, (M, K), generator=g, dtype=torch.int64)
    b = torch.randint(-2, 3, (K, N), generator=g, dtype=torch.int64)
    assert not torch.equal(b[:128, :128], b[:128, :128].t())
    return a, b, g


@pytest.mark.parametrize("case", CASES, ids=IDS)
@pytest.mark.parametrize("shape", [(128, 128, 1), (128, 128, 3), (256, 384, 2)])
def test_gemm_against_float64(case, shape):
    M, N, K = shape[0], shape[1], shape[2] * BK
    a, b, g = random_ints(M, N, K, seed=K + N)
    sa = torch.randint(125, 130, (M, K // 32), generator=g, dtype=torch.uint8)
    sb = torch.randint(125, 130, (K // 32, N), generator=g, dtype=torch.uint8)
    C, want = run_gemm(case, a, b, sa, sb)
    assert torch.equal(C, want)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_full_width_scale_bytes(case):
    """127 + d on A, 127 - d on B, d by block index: every bit of the scale byte
    is 0 in one block and 1 in another, and C is the unscaled product."""
    M = N = 128
    K = 3 * BK
    a, b, _ = random_ints(M, N, K, seed=7)
    d = torch.tensor(ops.MX_FULL_WIDTH_DELTAS)[torch.arange(K // 32) % 4]
    sa = (127 + d).to(torch.uint8).expand(M, -1)
    sb = (127 - d).to(torch.uint8).unsqueeze(1).expand(-1, N)
    C, want = run_gemm(case, a, b, sa, sb)
    assert torch.equal(want, a.double() @ b.double()) and torch.equal(C, want)


@pytest.fixture(scope="module", params=CASES, ids=IDS)
def verify_case(request):
    M = N = 256
    K = 2 * m6.MX6_GEMM_PERIOD
    *operands, expected = m6.mx6_gemm_operands(*request.param, M, N, K)
    return request.param, (M, N, K), [t.cuda() for t in operands], expected


def run_verify(vc, expected, rounds=3, inject=(-1, -1)):
    case, _, operands, _ = vc
    records, C, ms = ops.get_ops().mx6_gemm_pipe(*operands, expected.cuda(), *case, rounds, False,
                                                 *inject)
    assert C.numel() == 0 and ms > 0
    return records.cpu().numpy().reshape(-1, 4, 8)


def test_verify_clean(verify_case):
    expected = verify_case[3]
    rec = run_verify(verify_case, expected)
    assert (rec[:, :, 1] == 0).all() and (rec[:, :, 2:4] == -1).all() and (rec[:, :, 5:] == 0).all()
    assert (rec[:, :, 4].view(np.uint32) == ops.gemm_probe_wave_checksums(expected.numpy(), 3)).all()


def test_verify_compare_is_live(verify_case):
    rec = run_verify(verify_case, verify_case[3] * 2)
    assert (rec[:, :, 1] == 3 * 64 * 64).all() and (rec[:, :, 2:4] == 0).all()


def test_verify_injection_is_attributed(verify_case):
    case, (M, N, K), _, expected = verify_case
    rec = run_verify(verify_case, expected, inject=(2, 1))
    want = ops.gemm_probe_wave_checksums(expected.numpy(), 3)
    assert rec[:, :, 1].sum() == 1 and tuple(rec[2, 0, 1:4]) == (1, 1, 0)
    assert int(rec[2, 0, 4]) & 0xFFFFFFFF == int(want[0]) ^ 1
    s = m6.summarize_mx6_gemm_probe(rec.reshape(-1, 8), 1.0, *case, M, N, K, 3, 1)
    assert not s["ok"] and s["mismatched_waves"] == 1 and s["checksum_spread"]
    assert [tuple(e[k] for k in ("xcc", "se", "sh", "cu")) for e in s["bad_cus"]] == \
        [ops.decode_hw_word(rec[2, 0, 0])]


def test_argument_checks():
    o = ops.get_ops()
    f6, f86, f84 = ("mxfp6", "mxfp6", "kn"), ("mxfp8", "mxfp6", "nk"), ("mxfp8", "mxfp4", "nk")
    A, B, sa, sb, exp = (t.cuda() for t in m6.mx6_gemm_operands(*f6, 128, 128, 512))
    A8, B6, sa8, sb6, _ = (t.cuda() for t in m6.mx6_gemm_operands(*f86, 128, 128, 512))
    B4 = m6.mx6_gemm_operands(*f84, 128, 128, 512)[1].cuda()
    big = (1 << 22) + 128
    refusals = [
        (A[:64], B, sa[:64], sb, exp, *f6),                          # M not a multiple of 128
        (A, B[:, :48], sa, sb[:, :64], exp, *f6),                    # N not a multiple of 128
        (A[:, :48], B[:64], sa[:, :2], sb[:2], exp, *f6),            # K = 64
        (A[:, :144], B[:192], sa[:, :6], sb[:6], exp, *f6),          # K = 192, off the step
        (A[:, :382], B, sa, sb, exp, *f6),                           # A's bytes hold no whole codes
        (A8, B6[:, :383], sa8, sb6, exp, *f86),                      # 6-bit B not 3K/4 bytes wide
        (A8, B6[:, :256], sa8, sb6, exp, *f86),                      # B's packed K differs
        (A8, B6, sa8, sb6, exp, *f84),                               # 4-bit B not K/2 bytes wide
        (A[:, :1].expand(128, big * 3 // 4), B[:1].expand(big, 96),
         sa[:, :1].expand(128, big // 32), sb[:1].expand(big // 32, 128), exp, *f6),  # K past 2^22
        (A, B, sa[:, :8], sb, exp, *f6),                             # scale_a not [M, K/32]
        (A, B, sa, sb.t(), exp, *f6),                                # scale_b in the other layout
        (A8, B6, sa8, sb6.t(), exp, *f86),                           # likewise for nk
        (A.float(), B, sa, sb, exp, *f6),                            # operand not uint8
        (A, B, sa.int(), sb, exp, *f6),                              # scale not uint8
        (A, B, sa, sb, exp.double(), *f6),                           # expected not fp32
        (A, B, sa, sb, exp[:64], *f6),                               # expected not [128,128]
        (A.cpu(), B, sa, sb, exp, *f6),                              # wrong device
        (A, B, sa, sb.cpu(), exp, *f6),                              # a scale on the wrong device
        (A, B, sa, sb, exp, "mxfp6", "mxbf6", "kn"),                 # unsupported pair
        (A, B4, sa, sb6, exp, "mxfp6", "mxfp4", "nk"),               # 6-bit A against 4-bit B
        (A8, B, sa8, sb, exp, "mxfp8", "mxfp6", "kn"),               # mixed kn
        (A8, A8, sa8, sa8, exp, "mxfp8", "mxfp8", "nk"),             # mx_gemm_pipe's case
        (A, B, sa, sb, exp, "mxfp6", "e2m3", "kn"),                  # unknown format
        (A, B, sa, sb, exp, "mxfp6", "mxfp6", "tn"),                 # unknown b_layout
    ]
    for args in refusals:
        with pytest.raises(RuntimeError):
            o.mx6_gemm_pipe(*args, 1, False)
    for inject in ((1, 0), (-2, 0), (0, 1), (0, -2)):                # injection index out of range
        with pytest.raises(RuntimeError, match="inject"):
            o.mx6_gemm_pipe(A, B, sa, sb, exp, *f6, 1, False, *inject)
    with pytest.raises(RuntimeError, match="rounds"):
        o.mx6_gemm_pipe(A, B, sa, sb, exp, *f6, 0, False)
    with pytest.raises(RuntimeError, match="2\\^33"):
        o.mx6_gemm_pipe(A, B, sa, sb, exp, *f6, 1 << 26, False)


def test_default_report():
    info = ops.get_ops().device_info(0)
    cus = info["multiProcessorCount"]
    peak = PEAK_FLOP_PER_CLK_SIMD * 4 * cus * info["clockRate_kHz"] * 1e-9
    rep = ops.mx6_gemm_probe_report(0)
    assert list(rep["cases"]) == IDS
    for name, s in rep["cases"].items():
        print(f"{name}: {s['tflops']:.1f} TFLOP/s, operands {s['operand_gbps']:.0f} GB/s in "
              f"{s['elapsed_ms']:.2f} ms (per-clock peak {peak:.1f}), cus_seen {s['cus_seen']}")
        assert s["ok"] is True and s["cus_seen"] >= cus, s
        assert 0 < s["tflops"] <= 1.25 * peak, (name, s["tflops"], peak)
    assert rep["ok"] is True and rep["bad_cus"] == []


def test_health_report_wiring():
    rep = ops.gpu_health_report(0, mx6_gemm_probe=True)
    assert rep["mx6_gemm_probe"]["ok"] is True and rep["healthy"] is True
    assert "mx6_gemm_probe" not in ops.gpu_health_report(0)
