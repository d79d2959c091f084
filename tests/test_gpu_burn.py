"""GPU tests for the sustained MFMA burn-in (ops.mfma_burn): exact results
under chained issue, round reset, a live compare, per-CU attribution of an
injected one-bit fault, the exactness bound, and CU coverage / TFLOP/s
plausibility at the default shape. Everything is bitwise: no tolerance."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

needs_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")

FMTS = ("bf16", "fp8", "mx8", "mx4")
K = {"bf16": 32, "fp8": 32, "mx8": 128, "mx4": 128}
# per-clock MFMA issue rate of each instruction form, FLOP/clk/SIMD
# (16x16x32 bf16/fp8: 16384 flop per 16 cycles; BENCHMARKS.md)
PEAK_FLOP_PER_CLK_SIMD = {"bf16": 1024, "fp8": 1024, "mx8": 2048, "mx4": 4096}
BLOCKS = 8  # 32 waves
WAVES = BLOCKS * 4

_operands = {}


def operands(fmt):
    """(A, B, expected_unit) on the GPU, computed once per format and shared."""
    if fmt not in _operands:
        from hivedscheduler_amd.ops import burn_operands

        A, B, unit = burn_operands(fmt, seed=7)
        if A.dtype != torch.bfloat16:
            A, B = A.view(torch.uint8), B.view(torch.uint8)
        _operands[fmt] = (A.cuda(), B.cuda(), unit.cuda())
    return _operands[fmt]


def burn(fmt, chain, rounds, expected_chain=None, **kw):
    from hivedscheduler_amd.ops import get_ops

    A, B, unit = operands(fmt)
    exp = unit * float(chain if expected_chain is None else expected_chain)
    records, ms = get_ops().mfma_burn(A, B, exp, fmt, BLOCKS, chain, rounds, **kw)
    assert records.shape == (WAVES, 4) and records.dtype == torch.int32
    assert ms > 0
    return records.cpu().numpy(), ms


def host_checksum(fmt, chain, rounds):
    """xor of the bits of chain*(A_i@B) over all elements and rounds."""
    bits = (operands(fmt)[2].cpu() * float(chain)).numpy().view(np.uint32).ravel()
    x = np.bitwise_xor.reduce(bits) if rounds % 2 else np.uint32(0)
    return int(np.uint32(x).astype(np.int32))


def assert_clean(rec, fmt, chain, rounds):
    assert (rec[:, 1] == 0).all(), f"mismatches: {rec[rec[:, 1] != 0]}"
    assert (rec[:, 2] == -1).all()
    assert (rec[:, 3] == rec[0, 3]).all(), "checksums differ between waves"
    assert int(rec[0, 3]) == host_checksum(fmt, chain, rounds)


@needs_gpu
@pytest.mark.parametrize("fmt", FMTS)
def test_burn_clean_chain_and_rounds(fmt):
    """chain=3, rounds=2 separates "the chain accumulates" from "a round
    resets": forgetting the reset gives 6x, resetting inside the chain 1x.
    rounds=3 makes the xor checksum non-trivial (an even count cancels)."""
    rec, _ = burn(fmt, chain=3, rounds=2)
    assert_clean(rec, fmt, 3, 2)
    rec, _ = burn(fmt, chain=3, rounds=3)
    assert_clean(rec, fmt, 3, 3)
    assert int(rec[0, 3]) != 0


@needs_gpu
@pytest.mark.parametrize("fmt", FMTS)
def test_burn_edge_single_mfma(fmt):
    rec, _ = burn(fmt, chain=1, rounds=1)
    assert_clean(rec, fmt, 1, 1)


@needs_gpu
@pytest.mark.parametrize("fmt", FMTS)
def test_burn_compare_is_live(fmt):
    """Run chain=3 against the expected tiles of chain=4: no expected element
    is zero, so every element of every accumulator differs in every round."""
    rounds = 2
    rec, _ = burn(fmt, chain=3, rounds=rounds, expected_chain=4)
    assert (rec[:, 1] == 16 * 16 * 4 * rounds).all(), rec[:, 1]
    assert (rec[:, 2] == 0).all()


@needs_gpu
@pytest.mark.parametrize("fmt", FMTS)
def test_burn_injection_is_attributed(fmt):
    from hivedscheduler_amd.ops import decode_hw_word, summarize_burn

    rec, ms = burn(fmt, chain=3, rounds=3, inject_wave=5, inject_round=1)
    assert rec[5, 1] == 1 and rec[5, 2] == 1, rec[5]
    others = np.delete(rec, 5, axis=0)
    assert (others[:, 1] == 0).all() and (others[:, 2] == -1).all()
    assert (others[:, 3] == host_checksum(fmt, 3, 3)).all()
    # one flipped low mantissa bit in one round
    assert int(rec[5, 3]) ^ host_checksum(fmt, 3, 3) == 1
    s = summarize_burn(rec, ms, fmt, 3, 3, expected_cus=1)
    xcc, se, sh, cu = decode_hw_word(rec[5, 0])
    assert s["bad_cus"] == [{"xcc": xcc, "se": se, "sh": sh, "cu": cu, "waves": 1,
                             "mismatched_elements": 1, "first_bad_round": 1}]
    assert s["mismatched_waves"] == 1 and s["checksum_spread"] is True
    assert s["ok"] is False


@needs_gpu
@pytest.mark.parametrize("fmt", FMTS)
def test_burn_exactness_bound(fmt):
    """The largest chain the wrapper admits still runs exact, and one more is
    refused."""
    from hivedscheduler_amd.ops import burn_chain_limit, get_ops

    limit = burn_chain_limit(fmt)
    assert limit * 4 * K[fmt] == 2 ** 24
    rec, _ = burn(fmt, chain=limit, rounds=1)
    assert_clean(rec, fmt, limit, 1)
    A, B, unit = operands(fmt)
    with pytest.raises(RuntimeError, match="exactness"):
        get_ops().mfma_burn(A, B, unit, fmt, BLOCKS, limit + 1, 1)


@needs_gpu
def test_burn_argument_checks():
    from hivedscheduler_amd.ops import get_ops

    ops = get_ops()
    A, B, unit = operands("bf16")
    for bad in (dict(blocks=0), dict(chain=0), dict(rounds=0),
                dict(inject_wave=WAVES), dict(inject_round=2)):
        args = dict(blocks=BLOCKS, chain=2, rounds=2)
        args.update(bad)
        with pytest.raises(RuntimeError):
            ops.mfma_burn(A, B, unit, "bf16", **args)
    with pytest.raises(RuntimeError):
        ops.mfma_burn(A, B, unit, "fp6", BLOCKS, 1, 1)
    with pytest.raises(RuntimeError):  # bf16 operands under a byte format
        ops.mfma_burn(A, B, unit, "fp8", BLOCKS, 1, 1)
    with pytest.raises(RuntimeError):  # K=32 operands under a K=128 format
        ops.mfma_burn(*operands("fp8"), "mx8", BLOCKS, 1, 1)
    with pytest.raises(RuntimeError):
        ops.mfma_burn(A, B, unit.cpu(), "bf16", BLOCKS, 1, 1)


@needs_gpu
def test_burn_default_shape_coverage_and_plausibility():
    """Default grid, chain and rounds: every CU runs the burn, the result is
    clean, and the TFLOP/s figure does not exceed what the per-clock MFMA
    rate allows (a cap that catches flop-count or timing errors, which are
    off by 2x or more; not a performance target, so no lower bound)."""
    from hivedscheduler_amd.ops import get_ops, mfma_burn_report

    info = get_ops().device_info(0)
    cus = info["multiProcessorCount"]
    rep = mfma_burn_report(0)
    assert rep["chain"] == 1024 and rep["rounds"] == 64 and rep["blocks"] == 2048
    assert set(rep["formats"]) == set(FMTS)
    for fmt, s in rep["formats"].items():
        peak = PEAK_FLOP_PER_CLK_SIMD[fmt] * 4 * cus * info["clockRate_kHz"] * 1e3 / 1e12
        print(f"{fmt}: {s['tflops']:.1f} TFLOP/s in {s['elapsed_ms']:.2f} ms "
              f"(per-clock peak {peak:.1f}), cus_seen {s['cus_seen']}")
        assert s["waves"] == 2048 * 4
        assert s["cus_seen"] >= cus, s
        assert s["ok"] is True, s
        assert 0 < s["tflops"] <= 1.25 * peak, (fmt, s["tflops"], peak)
    assert rep["ok"] is True and rep["bad_cus"] == []


@needs_gpu
def test_burn_report_injection_names_one_cu():
    from hivedscheduler_amd.ops import mfma_burn_report

    rep = mfma_burn_report(0, fmts=("bf16", "mx4"), blocks=BLOCKS, chain=2, rounds=2,
                           inject=(3, 0))
    assert rep["ok"] is False
    # wave 3 may land on a different CU in each format's launch
    named = set()
    for s in rep["formats"].values():
        assert s["ok"] is False and len(s["bad_cus"]) == 1
        assert s["bad_cus"][0]["mismatched_elements"] == 1
        named.add(tuple(s["bad_cus"][0][k] for k in ("xcc", "se", "sh", "cu")))
    assert [tuple(c[k] for k in ("xcc", "se", "sh", "cu")) for c in rep["bad_cus"]] \
        == sorted(named)


@needs_gpu
def test_health_report_burn_wiring():
    from hivedscheduler_amd.ops import gpu_health_report

    rep = gpu_health_report(0, quick=True, burn=True)
    assert rep["mfma_burn"]["ok"] is True and rep["healthy"] is True
    assert "mfma_burn" not in gpu_health_report(0, quick=True)
