"""GPU tests for the MX GEMM probe (ops.mx_gemm_pipe): the block-scaled GEMM
against a float64 host product at the smallest shapes at which the pipeline can
go wrong, full-width scale bytes through its scale path, the in-register
compare (clean, dead-wrong and injected), argument checks, the default report
and the health-report wiring. Everything is bitwise: no tolerance."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")]

from hivedscheduler_amd import ops  # noqa: E402
from hivedscheduler_amd.ops import mx_gemm_probe as mg  # noqa: E402

CASES = mg.MX_GEMM_CASES
# per-clock issue rate of the scaled MFMA, FLOP/clk/SIMD, as in test_gpu_burn.py (mx8, mx4)
PEAK_FLOP_PER_CLK_SIMD = {"mxfp8": 2048, "mxfp4": 4096}


def run_gemm(fmt, b_layout, a, b, sa, sb):
    """C of integer operands a [M,K], b [K,N] under scale bytes sa, sb, and its reference."""
    operands = mg.mx_gemm_layout(fmt, b_layout, a, b, sa, sb)
    want = mg.mx_gemm_reference(fmt, b_layout, *operands)
    records, C, ms = ops.get_ops().mx_gemm_pipe(*(t.cuda() for t in operands),
                                                torch.zeros(128, 128).cuda(), fmt, b_layout, 1, True)
    assert records.shape == (a.shape[0] // 128 * (b.shape[1] // 128) * 4, 8) and ms > 0
    return C.cpu().double(), want


def random_ints(M, N, K, seed):
    """Random, non-periodic integer operands in {-2..2}; B's first tile asymmetric."""
    g = torch.Generator().manual_seed(seed)
    a = torch.randint(-2, 3, (M, K), generator=g, dtype=torch.int64)
    b = torch.randint(-2, 3, (K, N), generator=g, dtype=torch.int64)
    assert not torch.equal(b[:128, :128], b[:128, :128].t())
    return a, b, g


@pytest.mark.parametrize("fmt,b_layout", CASES)
@pytest.mark.parametrize("shape", [(128, 128, 1), (128, 128, 3), (256, 384, 2)])
def test_gemm_against_float64(fmt, b_layout, shape):
    M, N, K = shape[0], shape[1], shape[2] * mg.mx_gemm_bk(fmt)
    a, b, g = random_ints(M, N, K, seed=K + N)
    sa = torch.randint(125, 130, (M, K // 32), generator=g, dtype=torch.uint8)
    sb = torch.randint(125, 130, (K // 32, N), generator=g, dtype=torch.uint8)
    C, want = run_gemm(fmt, b_layout, a, b, sa, sb)
    assert torch.equal(C, want)


@pytest.mark.parametrize("fmt,b_layout", CASES)
def test_full_width_scale_bytes(fmt, b_layout):
    """127 + d on A, 127 - d on B, d by block index: every bit of the scale byte
    is 0 in one block and 1 in another, and C is the unscaled product."""
    M = N = 128
    K = 3 * mg.mx_gemm_bk(fmt)
    a, b, _ = random_ints(M, N, K, seed=7)
    d = torch.tensor(ops.MX_FULL_WIDTH_DELTAS)[torch.arange(K // 32) % 4]
    sa = (127 + d).to(torch.uint8).expand(M, -1)
    sb = (127 - d).to(torch.uint8).unsqueeze(1).expand(-1, N)
    C, want = run_gemm(fmt, b_layout, a, b, sa, sb)
    assert torch.equal(want, a.double() @ b.double()) and torch.equal(C, want)


@pytest.fixture(scope="module", params=CASES, ids=lambda c: "_".join(c))
def verify_case(request):
    fmt, b_layout = request.param
    M = N = 256
    K = 2 * mg.mx_gemm_period(fmt)
    *operands, expected = mg.mx_gemm_operands(fmt, b_layout, M, N, K)
    return fmt, b_layout, (M, N, K), [t.cuda() for t in operands], expected


def run_verify(case, expected, rounds=3, inject=(-1, -1)):
    fmt, b_layout, _, operands, _ = case
    records, C, ms = ops.get_ops().mx_gemm_pipe(*operands, expected.cuda(), fmt, b_layout, rounds,
                                                False, *inject)
    assert C.numel() == 0 and ms > 0
    return records.cpu().numpy().reshape(-1, 4, 8)


def test_verify_clean(verify_case):
    expected = verify_case[4]
    rec = run_verify(verify_case, expected)
    assert (rec[:, :, 1] == 0).all() and (rec[:, :, 2:4] == -1).all() and (rec[:, :, 5:] == 0).all()
    assert (rec[:, :, 4].view(np.uint32) == ops.gemm_probe_wave_checksums(expected.numpy(), 3)).all()


def test_verify_compare_is_live(verify_case):
    rec = run_verify(verify_case, verify_case[4] * 2)
    assert (rec[:, :, 1] == 3 * 64 * 64).all() and (rec[:, :, 2:4] == 0).all()


def test_verify_injection_is_attributed(verify_case):
    fmt, b_layout, (M, N, K), _, expected = verify_case
    rec = run_verify(verify_case, expected, inject=(2, 1))
    want = ops.gemm_probe_wave_checksums(expected.numpy(), 3)
    assert rec[:, :, 1].sum() == 1 and tuple(rec[2, 0, 1:4]) == (1, 1, 0)
    assert int(rec[2, 0, 4]) & 0xFFFFFFFF == int(want[0]) ^ 1
    s = mg.summarize_mx_gemm_probe(rec.reshape(-1, 8), 1.0, fmt, b_layout, M, N, K, 3, 1)
    assert not s["ok"] and s["mismatched_waves"] == 1 and s["checksum_spread"]
    assert [tuple(e[k] for k in ("xcc", "se", "sh", "cu")) for e in s["bad_cus"]] == \
        [ops.decode_hw_word(rec[2, 0, 0])]


def test_argument_checks():
    o = ops.get_ops()
    A, B, sa, sb, exp = (t.cuda() for t in mg.mx_gemm_operands("mxfp8", "kn", 128, 128, 512))
    A4, B4, sa4, sb4, _ = (t.cuda() for t in mg.mx_gemm_operands("mxfp4", "nk", 128, 128, 1024))
    big = (1 << 22) + 128
    refusals = [
        (A[:64], B, sa[:64], sb, exp, "mxfp8", "kn"),                # M not a multiple of 128
        (A, B[:, :64], sa, sb[:, :64], exp, "mxfp8", "kn"),          # N not a multiple of 128
        (A[:, :448], B[:448], sa[:, :14], sb[:14], exp, "mxfp8", "kn"),    # K off the step
        (A4[:, :192], B4[:, :192], sa4[:, :12], sb4[:, :12], exp, "mxfp4", "nk"),  # K off (fp4)
        (A[:, :1].expand(128, big), B[:1].expand(big, 128), sa[:, :1].expand(128, big // 32),
         sb[:1].expand(big // 32, 128), exp, "mxfp8", "kn"),         # K beyond the 32-bit offsets
        (A, B[:256], sa, sb, exp, "mxfp8", "kn"),                    # B's K differs from A's
        (A4, B4[:, :256], sa4, sb4, exp, "mxfp4", "nk"),             # B's packed K differs
        (A, B, sa[:, :8], sb, exp, "mxfp8", "kn"),                   # scale_a not [M, K/32]
        (A, B, sa, sb.t(), exp, "mxfp8", "kn"),                      # scale_b in the other layout
        (A4, B4, sa4, sb4.t(), exp, "mxfp4", "nk"),                  # likewise for nk
        (A.float(), B, sa, sb, exp, "mxfp8", "kn"),                  # operand not uint8
        (A, B, sa.int(), sb, exp, "mxfp8", "kn"),                    # scale not uint8
        (A, B, sa, sb, exp.double(), "mxfp8", "kn"),                 # expected not fp32
        (A, B, sa, sb, exp[:64], "mxfp8", "kn"),                     # expected not [128,128]
        (A.cpu(), B, sa, sb, exp, "mxfp8", "kn"),                    # wrong device
        (A, B, sa, sb.cpu(), exp, "mxfp8", "kn"),                    # a scale on the wrong device
        (A, B, sa, sb, exp, "mxfp6", "kn"),                          # unknown fmt
        (A, B, sa, sb, exp, "mxfp8", "tn"),                          # unknown b_layout
    ]
    for args in refusals:
        with pytest.raises(RuntimeError):
            o.mx_gemm_pipe(*args, 1, False)
    for inject in ((1, 0), (-2, 0), (0, 1), (0, -2)):                # injection index out of range
        with pytest.raises(RuntimeError, match="inject"):
            o.mx_gemm_pipe(A, B, sa, sb, exp, "mxfp8", "kn", 1, False, *inject)
    with pytest.raises(RuntimeError, match="rounds"):
        o.mx_gemm_pipe(A, B, sa, sb, exp, "mxfp8", "kn", 0, False)
    with pytest.raises(RuntimeError, match="2\\^33"):
        o.mx_gemm_pipe(A, B, sa, sb, exp, "mxfp8", "kn", 1 << 26, False)


def test_default_report():
    info = ops.get_ops().device_info(0)
    cus = info["multiProcessorCount"]
    rep = ops.mx_gemm_probe_report(0)
    assert set(rep["cases"]) == {f"{f}_{b}" for f, b in CASES}
    for name, s in rep["cases"].items():
        peak = PEAK_FLOP_PER_CLK_SIMD[name.split("_")[0]] * 4 * cus * info["clockRate_kHz"] * 1e-9
        print(f"{name}: {s['tflops']:.1f} TFLOP/s, operands {s['operand_gbps']:.0f} GB/s in "
              f"{s['elapsed_ms']:.2f} ms (per-clock peak {peak:.1f}), cus_seen {s['cus_seen']}")
        assert s["ok"] is True and s["cus_seen"] >= cus, s
        assert 0 < s["tflops"] <= 1.25 * peak, (name, s["tflops"], peak)
    assert rep["ok"] is True and rep["bad_cus"] == []


def test_health_report_wiring():
    rep = ops.gpu_health_report(0, mx_gemm_probe=True)
    assert rep["mx_gemm_probe"]["ok"] is True and rep["healthy"] is True
    assert "mx_gemm_probe" not in ops.gpu_health_report(0)
