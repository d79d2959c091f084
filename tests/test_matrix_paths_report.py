"""CPU tests for the matrix-path probe's host side (ops.matrix_paths): the
operands' invariants and exactness, the reference against a plain float64 /
int64 product, the chain limit, the burn summary and the agent's fields."""
import inspect

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from hivedscheduler_amd import ops  # noqa: E402

PATHS = ops.MATRIX_PATHS
WORD_A, WORD_B = (1 << 16) | (2 << 13) | (3 << 8), (2 << 16) | (1 << 13) | (5 << 8)


def dense(path, A, B, index):
    """A and B as float64 (int64 for i8), written without the module's helpers."""
    def values(X):
        if X.dtype == torch.int8:
            return X.to(torch.int64)
        if X.dtype == torch.uint8:
            return None
        return X.to(torch.float64)

    a, b = values(A), values(B)
    if a is None or b is None:   # raw fp8 bytes: e4m3 / e5m2 per operand, by the path's name
        fa, fb = {"fp8": "ee", "bf8": "55", "fp8bf8": "e5", "bf8fp8": "5e"}[path.split("_")[0]]
        view = {"e": torch.float8_e4m3fn, "5": torch.float8_e5m2}
        a, b = A.view(view[fa]).to(torch.float64), B.view(view[fb]).to(torch.float64)
    if index is not None:
        full = torch.zeros(a.shape[0], 2 * a.shape[1], dtype=a.dtype)
        for r in range(a.shape[0]):
            for c in range(a.shape[1]):
                full[r, 4 * (c // 2) + int(index[r, c])] = a[r, c]
        a = full
    return a, b


@pytest.mark.parametrize("seed", (0, 1))
@pytest.mark.parametrize("path", PATHS)
def test_operands(path, seed):
    A, B, expected, *index = ops.matrix_operands(path, seed)
    index = index[0] if index else None
    inv = ops.matrix_operand_invariants(path, A, B, index)
    assert all(inv.values()), inv
    assert ("all_index_pairs" in inv) == (path in ops.MATRIX_SPARSE_PATHS)
    a, b = dense(path, A, B, index)
    M, K, sparse = ops.matrix_path_shape(path)
    assert a.shape == (M, K) and b.shape == (K, M) and expected.shape == (M, M)
    want = a @ b
    assert expected.dtype == (torch.int32 if want.dtype == torch.int64 else
                              torch.float64 if A.dtype == torch.float64 else torch.float32)
    assert torch.equal(expected.to(want.dtype), want)


@pytest.mark.parametrize("path", ops.MATRIX_BURN_PATHS)
def test_burn_operands_and_chain_limit(path):
    A, B, unit, *index = ops.matrix_burn_operands(path)
    a, b = dense(path, A, B, index[0] if index else None)
    M, K, _ = ops.matrix_path_shape(path)
    assert int(a.abs().max()) <= 2 and int(b.abs().max()) <= 2 and (unit != 0).all()
    assert torch.equal(unit.to(a.dtype).view(4 * M, M), a @ b)
    limit = ops.matrix_chain_limit(path)
    bound = {torch.float64: 1 << 53, torch.float32: 1 << 24, torch.int32: 1 << 31}[unit.dtype]
    assert limit == min(bound // (4 * K), 1 << 22) and 4 * K * limit <= bound
    with pytest.raises(AssertionError):
        ops.matrix_burn_report(0, paths=(path,), chain=limit + 1)   # raised before any GPU use


def test_summarize_matrix_burn():
    path, chain, rounds = "sp_f16_16x16x64", 8, 4
    rec = np.zeros((8, 4), dtype=np.int64)
    rec[:, 0], rec[:, 2], rec[:, 3] = [WORD_A] * 4 + [WORD_B] * 4, -1, 0x1234
    s = ops.summarize_matrix_burn(rec, 2.0, path, chain, rounds, expected_cus=2)
    assert s["ok"] and s["bad_cus"] == [] and s["cus_seen"] == 2 and s["waves"] == 8
    # dense-equivalent FLOPs: 2*M*M*K with K = 64
    assert s["tflops"] == pytest.approx(2 * 16 * 16 * 64 * 4 * chain * rounds * 8 / 2e-3 / 1e12)
    assert not ops.summarize_matrix_burn(rec, 2.0, path, chain, rounds, expected_cus=3)["ok"]
    bad = rec.copy()
    bad[5, 1:] = (3, 2, 0x1235)
    s = ops.summarize_matrix_burn(bad, 2.0, path, chain, rounds, expected_cus=2)
    assert not s["ok"] and s["mismatched_waves"] == 1 and s["checksum_spread"]
    assert s["bad_cus"] == [{"xcc": 2, "se": 1, "sh": 0, "cu": 5, "waves": 1,
                             "mismatched_elements": 3, "first_bad_round": 2}]


def test_flag_plumbing(monkeypatch):
    from hivedscheduler_amd.agent import __main__ as cli
    from hivedscheduler_amd.agent import health

    assert inspect.signature(ops.gpu_health_report).parameters["matrix_probe"].default is False
    bad_cu = {"xcc": 1, "se": 0, "sh": 0, "cu": 4}
    probe = {"tiles": {"ok": True}, "burn": {"paths": {"f64_16x16x4": {"tflops": 61.23}}},
             "ok": False, "bad_cus": [dict(bad_cu, waves=1)]}

    def fake_report(device=0, **kwargs):
        rep = {"hbm_gbps": 5000.0, "mfma_ok": True, "cu_coverage": 256, "lds_errors": 0,
               "healthy": True}
        if kwargs.get("matrix_probe"):
            rep.update(matrix_probe=probe, healthy=False)
        return rep

    monkeypatch.setattr(ops, "gpu_health_report", fake_report)
    monkeypatch.setattr(health, "_rocm_smi_gpu_state", lambda: {0: True})
    g = health.collect_node_health(deep=True)["gpus"]["0"]
    assert g["healthy"] is True and not any(k.startswith("matrix") for k in g)
    g = health.collect_node_health(deep=True, matrix_probe=True)["gpus"]["0"]
    assert g["healthy"] is False and g["matrix_probe_ok"] is False
    assert g["matrix_tflops"] == {"f64_16x16x4": 61.2} and g["matrix_bad_cus"] == [bad_cu]
    monkeypatch.setattr(health.NodeHealthAgent, "post_report", lambda self, r: True)
    monkeypatch.setattr(health.NodeHealthAgent, "run_placement_probes", lambda self: [])
    monkeypatch.setattr(health, "p2p_link_matrix", lambda: {"matrix": {}, "links": []})
    assert health.NodeHealthAgent("http://x").matrix_probe_every == 0
    agent = health.NodeHealthAgent("http://x", node_name="n", deep_every=1, probe_pairs=False,
                                   p2p_matrix_every=10 ** 9, matrix_probe_every=2)
    got = [agent.run_once()["gpus"]["0"] for _ in range(4)]
    assert ["matrix_probe_ok" in g for g in got] == [True, False, True, False]
    seen = {}
    monkeypatch.setattr(health, "collect_node_health", lambda **kw: seen.update(kw) or {"gpus": {}})
    monkeypatch.setattr("sys.argv", ["agent", "--local", "--matrix-probe", "--no-probe-pairs"])
    cli.main()
    assert seen["matrix_probe"] is True and seen["mempath_probe"] is False
    monkeypatch.setattr(health, "NodeHealthAgent",
                        lambda url, **kw: seen.update(kw) or type("A", (), {"run_once": lambda s: {}})())
    monkeypatch.setattr("sys.argv", ["agent", "--scheduler", "http://x", "--once",
                                     "--matrix-probe-every", "6"])
    cli.main()
    assert seen["matrix_probe_every"] == 6 and seen["mempath_probe_every"] == 0
