"""GPU tests for the GEMM probe (ops.lds_tr_read, ops.gemm_pipe): the transpose
reads against the host mirror, the GEMM against a float64 host product at the
smallest shapes at which the pipeline can go wrong, the in-register compare
(clean, dead-wrong and injected), argument checks, the default report and the
health-report wiring. Everything is bitwise: no tolerance."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")]

from hivedscheduler_amd import ops  # noqa: E402
from hivedscheduler_amd.ops import gemm_probe as gp  # noqa: E402

CASES = gp.GEMM_PROBE_CASES
# per-clock MFMA issue rate, FLOP/clk/SIMD, as in test_gpu_burn.py
PEAK_FLOP_PER_CLK_SIMD = 1024


def tr_addr_sets(width):
    """The GEMM's tile addressing, and another row stride with a non-zero base."""
    return (gp.lds_tr_tile_addrs(width, 256 if width == 16 else 128,
                                 group_rows=8 if width == 16 else 16),
            gp.lds_tr_tile_addrs(width, 80, base=1040))


@pytest.mark.parametrize("width", gp.LDS_TR_WIDTHS)
def test_transpose_map(width):
    o = ops.get_ops()
    for complement in (False, True):
        image = gp.lds_tr_image(4096, seed=3, complement=complement)
        for addrs in tr_addr_sets(width):
            got = o.lds_tr_read(width, torch.from_numpy(image).cuda(), torch.from_numpy(addrs))
            assert np.array_equal(got.cpu().numpy(), gp.lds_tr_expected(width, image, addrs))
    image = torch.from_numpy(gp.lds_tr_image(256)).cuda()
    span, align = gp.lds_tr_span(width)
    for lane, bad in ((5, 4), (63, 1024 - span + align), (0, -align), (17, 1 << 20)):
        addrs = torch.zeros(64, dtype=torch.int32)
        addrs[lane] = bad
        with pytest.raises(RuntimeError, match="aligned|outside"):
            o.lds_tr_read(width, image, addrs)


def random_case(fmt, b_layout, M, N, K, seed):
    """Random, non-periodic integer operands in {-2..2}; B's content asymmetric."""
    g = torch.Generator().manual_seed(seed)
    a = torch.randint(-2, 3, (M, K), generator=g, dtype=torch.int64)
    b = torch.randint(-2, 3, (K, N), generator=g, dtype=torch.int64)
    assert not torch.equal(b[:128, :128], b[:128, :128].t())
    B = gp.gemm_probe_encode(b if b_layout == "kn" else b.t(), fmt)
    return gp.gemm_probe_encode(a, fmt), B, a.double() @ b.double()


@pytest.mark.parametrize("fmt,b_layout", CASES)
@pytest.mark.parametrize("shape", [(128, 128, 1), (128, 128, 3), (256, 384, 2)])
def test_gemm_against_float64(fmt, b_layout, shape):
    M, N, K = shape[0], shape[1], shape[2] * gp.gemm_probe_bk(fmt)
    A, B, want = random_case(fmt, b_layout, M, N, K, seed=K + N)
    expected = torch.zeros(128, 128)
    records, C, ms = ops.get_ops().gemm_pipe(A.cuda(), B.cuda(), expected.cuda(), fmt, b_layout,
                                             1, True)
    assert records.shape == (M // 128 * (N // 128) * 4, 8) and ms > 0
    assert torch.equal(C.cpu().double(), want)


@pytest.fixture(scope="module", params=CASES, ids=lambda c: "_".join(c))
def verify_case(request):
    fmt, b_layout = request.param
    M = N = 256
    K = 2 * gp.gemm_probe_period(fmt)
    A, B, expected = gp.gemm_probe_operands(fmt, b_layout, M, N, K)
    return fmt, b_layout, (M, N, K), A.cuda(), B.cuda(), expected


def run_verify(case, expected, rounds=3, inject=(-1, -1)):
    fmt, b_layout, _, A, B, _ = case
    records, C, ms = ops.get_ops().gemm_pipe(A, B, expected.cuda(), fmt, b_layout, rounds, False,
                                             *inject)
    assert C.numel() == 0 and ms > 0
    return records.cpu().numpy().reshape(-1, 4, 8)


def test_verify_clean(verify_case):
    expected = verify_case[5]
    rec = run_verify(verify_case, expected)
    assert (rec[:, :, 1] == 0).all() and (rec[:, :, 2:4] == -1).all() and (rec[:, :, 5:] == 0).all()
    assert (rec[:, :, 4].view(np.uint32) == gp.gemm_probe_wave_checksums(expected.numpy(), 3)).all()


def test_verify_compare_is_live(verify_case):
    rec = run_verify(verify_case, verify_case[5] * 2)
    assert (rec[:, :, 1] == 3 * 64 * 64).all() and (rec[:, :, 2:4] == 0).all()


def test_verify_injection_is_attributed(verify_case):
    fmt, b_layout, (M, N, K), _, _, expected = verify_case
    rec = run_verify(verify_case, expected, inject=(2, 1))
    want = gp.gemm_probe_wave_checksums(expected.numpy(), 3)
    assert rec[:, :, 1].sum() == 1 and tuple(rec[2, 0, 1:4]) == (1, 1, 0)
    assert int(rec[2, 0, 4]) & 0xFFFFFFFF == int(want[0]) ^ 1
    clean = np.ones((4, 4), dtype=bool)
    clean[2, 0] = False
    assert (rec[:, :, 4].view(np.uint32)[clean] == np.broadcast_to(want, (4, 4))[clean]).all()
    s = gp.summarize_gemm_probe(rec.reshape(-1, 8), 1.0, fmt, b_layout, M, N, K, 3, 1)
    assert not s["ok"] and s["mismatched_waves"] == 1 and s["checksum_spread"]
    assert [tuple(e[k] for k in ("xcc", "se", "sh", "cu")) for e in s["bad_cus"]] == \
        [ops.decode_hw_word(rec[2, 0, 0])]


def test_argument_checks():
    o = ops.get_ops()
    A, B, expected = (t.cuda() for t in gp.gemm_probe_operands("bf16", "kn", 128, 128, 256))
    A8, B8, _ = (t.cuda() for t in gp.gemm_probe_operands("fp8", "nk", 128, 128, 512))
    big_k = (1 << 22) + 64
    refusals = [
        (A[:64], B, expected, "bf16", "kn"),                    # M not a multiple of 128
        (A, B[:, :64], expected, "bf16", "kn"),                 # N not a multiple of 128
        (A[:, :96], B[:96], expected, "bf16", "kn"),            # K not a multiple of BK
        (A8[:, :448], B8[:, :448], expected, "fp8", "nk"),      # K not a multiple of BK (fp8)
        (A[:, :1].expand(128, big_k), B[:1].expand(big_k, 128), expected, "bf16", "kn"),  # 4K > 2^24
        (A8, B8, expected, "bf16", "nk"),                       # wrong dtype for the format
        (A, B, expected.double(), "bf16", "kn"),                # expected not fp32
        (A, B, expected[:64], "bf16", "kn"),                    # expected not [128,128]
        (A.cpu(), B, expected, "bf16", "kn"),                   # wrong device
        (A, B[:128], expected, "bf16", "kn"),                   # B's K differs from A's
        (A, B, expected, "fp16", "kn"),                         # unknown fmt
        (A, B, expected, "bf16", "tn"),                         # unknown b_layout
    ]
    for args in refusals:
        with pytest.raises(RuntimeError):
            o.gemm_pipe(*args, 1, False)
    for inject in ((1, 0), (-2, 0), (0, 1), (0, -2)):           # injection index out of range
        with pytest.raises(RuntimeError, match="inject"):
            o.gemm_pipe(A, B, expected, "bf16", "kn", 1, False, *inject)
    with pytest.raises(RuntimeError, match="rounds"):
        o.gemm_pipe(A, B, expected, "bf16", "kn", 0, False)
    with pytest.raises(RuntimeError, match="2\\^33"):
        o.gemm_pipe(A, B, expected, "bf16", "kn", 1 << 26, False)


def test_default_report():
    info = ops.get_ops().device_info(0)
    cus = info["multiProcessorCount"]
    peak = PEAK_FLOP_PER_CLK_SIMD * 4 * cus * info["clockRate_kHz"] * 1e3 / 1e12
    rep = ops.gemm_probe_report(0)
    assert set(rep["cases"]) == {f"{f}_{b}" for f, b in CASES}
    assert rep["tr_map"] == {str(w): True for w in gp.LDS_TR_WIDTHS}
    for name, s in rep["cases"].items():
        print(f"{name}: {s['tflops']:.1f} TFLOP/s, operands {s['operand_gbps']:.0f} GB/s in "
              f"{s['elapsed_ms']:.2f} ms (per-clock peak {peak:.1f}), cus_seen {s['cus_seen']}")
        assert s["ok"] is True and s["cus_seen"] >= cus, s
        assert 0 < s["tflops"] <= 1.25 * peak, (name, s["tflops"], peak)
    assert rep["ok"] is True and rep["bad_cus"] == []


def test_health_report_wiring():
    rep = ops.gpu_health_report(0, gemm_probe=True)
    assert rep["gemm_probe"]["ok"] is True and rep["healthy"] is True
    assert "gemm_probe" not in ops.gpu_health_report(0)
