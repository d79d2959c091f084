"""Host-only tests of the MX6 GEMM probe: the 6-bit packing, the invariants of
mx6_gemm_operands, summarize_mx6_gemm_probe on hand-made records and the
agent's record fields from a stubbed report."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from hivedscheduler_amd.ops import mx6_gemm_probe as m6  # noqa: E402

CASES = m6.MX6_GEMM_CASES
IDS = [m6.mx6_gemm_case_name(*c) for c in CASES]
BITS = {"mxfp8": 8, "mxfp6": 6, "mxbf6": 6, "mxfp4": 4}


def test_case_names():
    assert IDS == ["mxfp6_nk", "mxfp6_kn", "mxbf6_nk", "mxbf6_kn", "mxfp8xfp6_nk", "mxfp8xfp4_nk"]


@pytest.mark.parametrize("axis", [0, 1])
def test_pack6_round_trip_and_bit_stream(axis):
    codes = (torch.arange(8 * 12).view(8, 12) * 11 % 64).to(torch.uint8)
    packed = m6.mx6_pack6(codes, axis)
    assert packed.shape == ((6, 12) if axis == 0 else (8, 9)) and packed.dtype == torch.uint8
    assert torch.equal(m6.mx6_unpack6(packed, axis), codes)
    # 0b000001, 0b100000, 0b111111, 0b010101 -> bits [6j, 6j+6) of 24, low byte first
    four = torch.tensor([1, 32, 63, 21], dtype=torch.uint8)
    stream = 1 | 32 << 6 | 63 << 12 | 21 << 18
    want = [stream & 255, stream >> 8 & 255, stream >> 16]
    assert want == [0x01, 0xF8, 0x57]
    assert m6.mx6_pack6(four.view(1, 4) if axis else four.view(4, 1), axis).flatten().tolist() == want


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_operand_invariants(case):
    a_fmt, b_fmt, b_layout = case
    P, M, N, K = m6.MX6_GEMM_PERIOD, 256, 256, 1024
    assert P == 4 * m6.MX6_GEMM_BK == 512
    A, B, sa, sb, expected = m6.mx6_gemm_operands(*case, M, N, K)
    assert A.shape == (M, K * BITS[a_fmt] // 8) and sa.shape == (M, K // 32)
    assert B.shape == ((K, N * 3 // 4) if b_layout == "kn" else (N, K * BITS[b_fmt] // 8))
    assert sb.shape == ((K // 32, N) if b_layout == "kn" else (N, K // 32))
    assert all(t.dtype == torch.uint8 and t.is_contiguous() for t in (A, B, sa, sb))
    for s in (sa, sb):
        assert int(s.min()) >= 125 and int(s.max()) <= 129
    # the reference of the tiled operands: the unit tile (K/P times) in every tile of C
    want = m6.mx6_gemm_reference(*case, A, B, sa, sb)
    unit = want[:128, :128]
    assert (unit != 0).all() and not torch.equal(unit, unit.t())
    assert torch.equal(want.float().double(), want)            # lossless in fp32
    assert torch.equal(expected.double(), unit)
    assert torch.equal(m6.mx6_gemm_operands(*case, 128, 128, P)[4] * (K // P), expected)
    assert all(torch.equal(want[i:i + 128, j:j + 128], unit) for i in (0, 128) for j in (0, 128))
    # the four K steps of a period differ pairwise in A
    w = A.shape[1] // (K // 128)
    steps = [A[:128, s * w:(s + 1) * w] for s in range(4)]
    assert all(not torch.equal(steps[s], steps[t]) for s in range(4) for t in range(s))
    with pytest.raises(ValueError):
        m6.mx6_gemm_operands(*case, M, N, P + 128)
    with pytest.raises(ValueError):
        m6.mx6_gemm_operands(*case, 128, 128, m6.MX_GEMM_MAX_K + P)
    with pytest.raises(ValueError):
        m6.mx6_gemm_operands("mxfp8", b_fmt, "kn", M, N, K)


def records(grid=4, cus=2):
    rec = np.zeros((grid, 4, 8), dtype=np.int32)
    rec[:, :, 0] = ((np.arange(grid) % cus) << 8)[:, None]  # CU id in HW_ID[11:8]
    rec[:, :, 2:4] = -1
    rec[:, :, 4] = np.array([11, 22, 33, 44])  # one checksum per wave position
    return rec


@pytest.mark.parametrize("case,step_bytes", [
    (("mxfp6", "mxfp6", "nk"), 128 * (96 + 96) + 1024),
    (("mxfp6", "mxfp6", "kn"), 128 * (96 + 128) + 1024),     # dword loads fetch the padding too
    (("mxfp8", "mxfp6", "nk"), 128 * (128 + 96) + 1024),
    (("mxfp8", "mxfp4", "nk"), 128 * (128 + 64) + 1024)])
def test_summary_clean_and_bad_wave(case, step_bytes):
    shape = dict(M=256, N=256, K=1024, rounds=3, expected_cus=2)
    s = m6.summarize_mx6_gemm_probe(records().reshape(-1, 8), 2.0, *case, **shape)
    assert s["ok"] and s["waves"] == 16 and s["cus_seen"] == 2 and s["bad_cus"] == []
    assert s["tflops"] == pytest.approx(2.0 * 256 * 256 * 1024 * 3 / 2e-3 / 1e12)
    # 4 workgroups x 8 steps x the step's bytes x 3 rounds
    assert s["operand_gbps"] == pytest.approx(4 * 8 * step_bytes * 3 / 2e-3 / 1e9)
    rec = records()
    rec[3, 0, 1:4] = (1, 2, 0)
    rec[3, 0, 4] ^= 1
    s = m6.summarize_mx6_gemm_probe(rec.reshape(-1, 8), 2.0, *case, **shape)
    assert not s["ok"] and s["mismatched_waves"] == 1 and s["checksum_spread"]
    assert s["bad_cus"] == [{"xcc": 0, "se": 0, "sh": 0, "cu": 1, "waves": 1,
                             "mismatched_elements": 1, "first_bad_round": 2,
                             "first_bad_index": 0}]


@pytest.mark.parametrize("ok", [True, False])
def test_agent_record_fields(monkeypatch, ok):
    from hivedscheduler_amd import ops
    from hivedscheduler_amd.agent import health

    bad = [] if ok else [{"xcc": 1, "se": 0, "sh": 0, "cu": 3}]
    probe = {"cases": {"mxfp6_nk": {"tflops": 1234.56}}, "ok": ok, "bad_cus": bad}
    seen = {}

    def report(device, **flags):
        seen.update(flags)
        return {"healthy": True, "hbm_gbps": 5000.0, "mfma_ok": True, "cu_coverage": 256,
                "lds_errors": 0, "mx6_gemm_probe": probe}

    monkeypatch.setattr(ops, "gpu_health_report", report)
    monkeypatch.setattr(health, "_rocm_smi_gpu_state", lambda: {0: True})
    gpu = health.collect_node_health(deep=True, mx6_gemm_probe=True)["gpus"]["0"]
    assert seen.get("mx6_gemm_probe") is True
    assert gpu["mx6_gemm_probe_ok"] is ok and gpu["mx6_gemm_tflops"] == {"mxfp6_nk": 1234.6}
    assert gpu["mx6_gemm_bad_cus"] == bad and gpu["healthy"] is ok
