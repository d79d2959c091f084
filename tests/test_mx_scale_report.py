"""CPU tests for the MX scale probe's host side (ops/mx_scale.py): the decode
tables, that the reference alone shows every case of tests/test_gpu_mx_scale.py
to be exact, the burn summariser and the flag plumbing."""
import inspect

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from hivedscheduler_amd import ops  # noqa: E402
from hivedscheduler_amd.ops import (MX_BURN_FORMATS, MX_SCALE_PAIRS, MX_SHAPES,  # noqa: E402
                                    mx_decode, mx_exactness, mx_scale_invariants)

SHAPES = (0, 1)


def test_decode_tables():
    byte = torch.arange(256, dtype=torch.uint8)
    for fmt, dtype in ((0, torch.float8_e4m3fn), (1, torch.float8_e5m2)):
        want, got = byte.view(dtype).double(), mx_decode(fmt, byte)
        finite = torch.isfinite(want)
        assert torch.equal(got[finite], want[finite]) and torch.isnan(got[~finite]).all()
        assert int(finite.sum()) == (254 if fmt == 0 else 248)
    # the small formats, written out: (exponent bits, mantissa bits, bias)
    for fmt, (e, m, bias) in ((2, (2, 3, 1)), (3, (3, 2, 3)), (4, (2, 1, 1))):
        for code in range(1 << (1 + e + m)):
            exp, man = (code >> m) & ((1 << e) - 1), code & ((1 << m) - 1)
            mag = man / 2 ** m * 2.0 ** (1 - bias) if exp == 0 else (1 + man / 2 ** m) * 2.0 ** (exp - bias)
            assert mx_decode(fmt, torch.tensor([code])).item() == (-mag if code >> (e + m) else mag)
    assert mx_decode(2, torch.tensor([31])).item() == 7.5      # the formats' largest values
    assert mx_decode(3, torch.tensor([31])).item() == 28.0
    assert mx_decode(4, torch.arange(8)).tolist() == [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0]
    assert ops.e8m0_value(torch.tensor([0, 127, 254])).tolist() == [2.0 ** -127, 1.0, 2.0 ** 127]
    assert torch.isnan(ops.e8m0_value(torch.tensor([255]))).all()


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("fmt_a,fmt_b", MX_SCALE_PAIRS)
def test_tile_operands_hold_their_invariants(fmt_a, fmt_b, shape):
    """Seeds 0 and 1 of every pair, and seed 3 of the byte-select case."""
    for s in (0, 1, 3) if (fmt_a, fmt_b, shape) == (2, 1, 1) else (0, 1):
        A, B, sa, sb, expected = ops.mx_scale_operands(fmt_a, fmt_b, shape, s)
        inv = mx_scale_invariants(fmt_a, fmt_b, A, B, sa, sb)
        assert all(inv.values()), inv
        want = ops.mx_scaled_product(fmt_a, fmt_b, A, B, sa[..., 1], sb[..., 2])
        assert torch.equal(expected[1, 2].double(), want)
        assert not torch.equal(expected[1, 2], expected[2, 1])   # the select matters


def sweep_cases(shape):
    for side in ("a", "b"):
        yield (0, ops.mx_slot_sweep_case(shape, side))
        for fmt in range(5):
            yield (fmt, ops.mx_decode_sweep_case(fmt, side, shape))
    for fmt in (2, 4):
        for k in range(MX_SHAPES[shape][1]):
            yield (fmt, ops.mx_k_slot_case(fmt, shape, k))
    yield (0, ops.mx_full_width_case(shape))


@pytest.mark.parametrize("shape", SHAPES)
def test_sweep_cases_are_exact_on_the_reference(shape):
    for fmt, (A, B, sa, sb, expected) in sweep_cases(shape):
        exact = mx_exactness(fmt, fmt, A, B, sa[..., 0], sb[..., 0])
        assert all(exact.values()), (fmt, exact)
        assert all(torch.equal(sa[..., 0], sa[..., p]) for p in range(1, 4))
    M, K = MX_SHAPES[shape]
    # the decode sweep carries every finite code, the K-slot sweep distinct rows
    for fmt, finite in ((0, 254), (1, 248), (2, 64), (3, 64), (4, 16)):
        A = ops.mx_decode_sweep_case(fmt, "a", shape)[0]
        assert len(torch.unique(A)) == finite   # code 0 also stands in for the NaN codes
    B = mx_decode(4, ops.mx_k_slot_case(4, shape, 0)[1])
    assert len(torch.unique(B, dim=0)) == K
    # full width: the net scale is one and every bit of the byte takes both values
    A, B, sa, sb, expected = ops.mx_full_width_case(0)
    unit = torch.full_like(sa[..., 0], 127)
    assert torch.equal(expected, ops.mx_scaled_product(0, 0, A, B, unit, unit.T))
    seen = sa[0, :, 0].long()
    assert int(np.bitwise_or.reduce(seen.numpy())) == 0xFF
    assert int(np.bitwise_and.reduce(seen.numpy())) == 0


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("fmt", MX_BURN_FORMATS)
def test_burn_operands_are_exact_up_to_the_chain_limit(fmt, shape):
    M, K = MX_SHAPES[shape]
    A, B, sa, sb, unit = ops.mx_scale_burn_operands(fmt, shape)
    limit = ops.mx_scale_chain_limit(shape)
    assert limit == {0: 128, 1: 256}[shape] and 4 * K * limit * 2 ** 8 <= 2 ** 24
    a, b = mx_decode(fmt, A), mx_decode(fmt, B)
    assert a.abs().max() == 2 and b.abs().max() == 2 and torch.equal(a, a.round())
    assert ((sa.long() - 127).abs() <= 2).all() and ((sb.long() - 127).abs() <= 2).all()
    total = torch.zeros(4 * M, M, dtype=torch.float64)
    for sel in range(4):
        SA, SB = sa[..., sel], sb[..., sel]
        assert all(mx_exactness(fmt, fmt, A, B, SA, SB).values())
        total += ops.mx_scaled_product(fmt, fmt, A, B, SA, SB)
        # sum of magnitudes over a whole chain, in units of 2^-4
        mag = ops.mx_scaled_product(fmt, fmt, ops.mx_encode(fmt, a.abs()), ops.mx_encode(fmt, b.abs()),
                                    SA, SB)
        assert (mag * 16 * limit <= 2 ** 24).all() and torch.equal(mag * 16, (mag * 16).round())
    assert torch.equal(unit.double().view(4 * M, M), total) and (total != 0).all()


def test_summarize_names_the_cu_of_a_bad_record():
    word = (3 << 16) | (2 << 13) | (1 << 12) | (5 << 8)
    rec = np.array([[word, 0, -1, 7], [word, 3, 2, 6], [word + 256, 0, -1, 7]], dtype=np.int32)
    s = ops.summarize_mx_scale_burn(rec, 2.0, 1, 8, 4, expected_cus=2)
    assert s["ok"] is False and s["mismatched_waves"] == 1 and s["checksum_spread"] is True
    assert s["bad_cus"] == [{"xcc": 3, "se": 2, "sh": 1, "cu": 5, "waves": 1,
                             "mismatched_elements": 3, "first_bad_round": 2}]
    assert s["cus_seen"] == 2 and s["tflops"] == 2.0 * 32 * 32 * 64 * 4 * 8 * 4 * 3 / 2e-3 / 1e12
    rec[1, 1:] = (0, -1, 7)
    assert ops.summarize_mx_scale_burn(rec, 2.0, 1, 8, 4, expected_cus=2)["ok"] is True
    assert ops.summarize_mx_scale_burn(rec, 2.0, 1, 8, 4, expected_cus=3)["ok"] is False


def test_flag_plumbing(monkeypatch):
    from hivedscheduler_amd.agent import health

    assert inspect.signature(ops.gpu_health_report).parameters["mx_scale_probe"].default is False
    assert inspect.signature(health.collect_node_health).parameters[
        "mx_scale_probe"].default is False
    bad_cu = {"xcc": 1, "se": 0, "sh": 0, "cu": 4}
    probe = {"tiles": {"ok": True, "cases": {}}, "ok": False, "bad_cus": [dict(bad_cu, waves=1)],
             "burn": {"ok": False, "cases": {"32x32x64/e2m3": {"tflops": 1234.56}}}}
    calls = []

    def fake_report(device=0, **kwargs):
        calls.append(kwargs)
        rep = {"hbm_gbps": 5000.0, "mfma_ok": True, "cu_coverage": 256, "lds_errors": 0,
               "healthy": True}
        if kwargs.get("mx_scale_probe"):
            rep.update(mx_scale_probe=probe, healthy=False)
        return rep

    monkeypatch.setattr(ops, "gpu_health_report", fake_report)
    monkeypatch.setattr(health, "_rocm_smi_gpu_state", lambda: {0: True})
    g = health.collect_node_health(deep=True)["gpus"]["0"]
    assert g["healthy"] is True and "mx_scale_probe" not in calls[-1]
    assert not any(k.startswith("mx_scale") for k in g)
    g = health.collect_node_health(deep=True, mx_scale_probe=True)["gpus"]["0"]
    assert g["healthy"] is False and g["mx_scale_probe_ok"] is False
    assert g["mx_scale_tiles_ok"] is True and g["mx_scale_burn_ok"] is False
    assert g["mx_scale_tflops"] == {"32x32x64/e2m3": 1234.6} and g["mx_scale_bad_cus"] == [bad_cu]
    # the agent's cadence and the command line
    monkeypatch.setattr(health.NodeHealthAgent, "post_report", lambda self, r: True)
    monkeypatch.setattr(health.NodeHealthAgent, "run_placement_probes", lambda self: [])
    monkeypatch.setattr(health, "p2p_link_matrix", lambda: {"matrix": {}, "links": []})
    assert health.NodeHealthAgent("http://x").mx_scale_probe_every == 0
    agent = health.NodeHealthAgent("http://x", node_name="n", deep_every=1, probe_pairs=False,
                                   p2p_matrix_every=10 ** 9, mx_scale_probe_every=2)
    got = [agent.run_once()["gpus"]["0"] for _ in range(4)]
    assert ["mx_scale_probe_ok" in g for g in got] == [True, False, True, False]
    from hivedscheduler_amd.agent import __main__ as cli

    seen = {}
    monkeypatch.setattr(health, "collect_node_health", lambda **kw: seen.update(kw) or {"gpus": {}})
    monkeypatch.setattr("sys.argv", ["agent", "--local", "--mx-scale-probe", "--no-probe-pairs"])
    cli.main()
    assert seen["mx_scale_probe"] is True and seen["atomic_probe"] is False
    monkeypatch.setattr(health, "NodeHealthAgent",
                        lambda url, **kw: seen.update(kw) or type("A", (), {"run_once": lambda s: {}})())
    monkeypatch.setattr("sys.argv", ["agent", "--scheduler", "http://x", "--once",
                                     "--mx-scale-probe-every", "6"])
    cli.main()
    assert seen["mx_scale_probe_every"] == 6 and seen["atomic_probe_every"] == 0
