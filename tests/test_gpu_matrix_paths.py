"""GPU tests for the matrix-path probe (ops.matrix_tile, ops.matrix_burn): every
path's tile, the one-hot K-slot and sparse index cases, clean and injected
burns, argument checks and the health-report wiring. Everything is bitwise:
no tolerance."""
import pytest

torch = pytest.importorskip("torch")

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")]

from hivedscheduler_amd import ops  # noqa: E402

BLOCKS = 8
DENSE = tuple(p for p in ops.MATRIX_PATHS if p not in ops.MATRIX_SPARSE_PATHS)
PATH_ABIDS = [(p, a) for p in ops.MATRIX_PATHS for a in ops.MATRIX_ABIDS[p]]


def run_tile(path, A, B, index=None, abid=0):
    tiles = ops.get_ops().matrix_tile(path, A.cuda(), B.cuda(), BLOCKS,
                                      None if index is None else index.cuda(), abid)
    M = ops.matrix_path_shape(path)[0]
    assert tiles.shape == (BLOCKS * 4, M, M)
    return tiles.cpu()


@pytest.mark.parametrize("path,abid", PATH_ABIDS)
def test_tile(path, abid):
    A, B, expected, *index = ops.matrix_operands(path)
    tiles = run_tile(path, A, B, index[0] if index else None, abid)
    assert tiles.dtype == expected.dtype
    assert torch.equal(tiles, expected.expand_as(tiles))


@pytest.mark.parametrize("path", DENSE)
def test_k_slot(path):
    """First, last and one slot per lane group: the same slot in A and B gives
    the single product, the next slot in B gives zero."""
    M, K, _ = ops.matrix_path_shape(path)
    groups = 64 // M
    for k in sorted({0, K - 1, *(K // groups * g for g in range(groups))}):
        A, B, expected = ops.matrix_k_slot_case(path, k)
        assert (expected != 0).all()
        assert torch.equal(run_tile(path, A, B), expected.expand(BLOCKS * 4, M, M)), k
        A, B, expected = ops.matrix_k_slot_case(path, k, (k + 1) % K)
        assert not expected.any() and not run_tile(path, A, B).any(), k


@pytest.mark.parametrize("pair", ops.MATRIX_INDEX_PAIRS)
@pytest.mark.parametrize("path", ops.MATRIX_SPARSE_PATHS)
def test_sparse_index(path, pair):
    A, B, expected, index = ops.matrix_index_case(path, pair)
    tiles = run_tile(path, A, B, index)
    assert torch.equal(tiles, expected.expand_as(tiles))


def run_burn(path, chain=8, rounds=4, inject=(-1, -1), blocks=BLOCKS, edit=None):
    A, B, unit, *index = ops.matrix_burn_operands(path)
    args = {"A": A, "B": B, "expected": unit * chain, "index": index[0] if index else None}
    args = {k: None if v is None else v.cuda() for k, v in args.items()}
    if edit:
        edit(args)
    records, ms = ops.get_ops().matrix_burn(path, args["A"], args["B"], args["expected"], blocks,
                                            chain, rounds, *inject, args["index"], 0)
    return records.cpu().numpy(), ms


@pytest.mark.parametrize("path", ops.MATRIX_BURN_PATHS)
def test_burn_clean_and_injected(path):
    rec, ms = run_burn(path)
    assert rec.shape == (BLOCKS * 4, 4) and ms > 0
    assert (rec[:, 1] == 0).all() and (rec[:, 2] == -1).all() and len(set(rec[:, 3])) == 1
    wave, rnd = 13, 2
    rec, ms = run_burn(path, inject=(wave, rnd))
    assert rec[:, 1].sum() == 1 and tuple(rec[wave, 1:3]) == (1, rnd)
    s = ops.summarize_matrix_burn(rec, ms, path, 8, 4, expected_cus=1)
    assert not s["ok"] and [(c["waves"], c["first_bad_round"]) for c in s["bad_cus"]] == [(1, rnd)]
    assert tuple(s["bad_cus"][0][k] for k in ("xcc", "se", "sh", "cu")) == \
        ops.decode_hw_word(rec[wave, 0])


@pytest.mark.parametrize("path", ops.MATRIX_BURN_PATHS)
def test_chain_above_limit_raises(path):
    with pytest.raises(RuntimeError, match="breaks exactness"):
        run_burn(path, chain=ops.matrix_chain_limit(path) + 1, rounds=1)


def _set(key, fn):
    return lambda args: args.__setitem__(key, fn(args[key]))


BAD_BURN_ARGS = [
    ("f64_16x16x4", dict(edit=_set("A", lambda t: t.float()))),
    ("f16_16x16x32", dict(edit=_set("B", lambda t: t[:-1]))),
    ("i8_16x16x64", dict(edit=_set("expected", lambda t: t.float()))),
    ("bf8_16x16x32", dict(edit=_set("A", lambda t: t.cpu()))),
    ("f32_32x32x2", dict(blocks=0)),
    ("f32_32x32x2", dict(rounds=0)),
    ("f32_32x32x2", dict(inject=(BLOCKS * 4, 0))),
    ("f32_32x32x2", dict(inject=(0, 4))),
    ("f16_32x32x16", {}),                                                # no burn kernel
    ("f16_16x16x32", dict(edit=_set("index", lambda t: torch.zeros(64, 32, dtype=torch.uint8).cuda()))),
    ("sp_f16_16x16x64", dict(edit=_set("index", lambda t: None))),
    ("sp_f16_16x16x64", dict(edit=_set("index", lambda t: t.flip(1)))),  # pairs decreasing
    ("sp_f16_16x16x64", dict(edit=_set("index", lambda t: t + 4))),
    ("no_such_path", {}),
]


@pytest.mark.parametrize("path,kwargs", BAD_BURN_ARGS)
def test_bad_arguments(path, kwargs):
    with pytest.raises(RuntimeError):
        if path in ops.MATRIX_BURN_PATHS:
            run_burn(path, **kwargs)
        else:
            A, B, _ = ops.matrix_burn_operands("f16_16x16x32")
            ops.get_ops().matrix_burn(path, A.cuda(), B.cuda(), torch.zeros(4, 16, 16).cuda(),
                                      BLOCKS, 8, 4, -1, -1, None, 0)


def test_bad_tile_arguments():
    A, B, _ = ops.matrix_operands("f16_16x16x32")
    tile = ops.get_ops().matrix_tile
    for call in (lambda: tile("f16_16x16x32", A.cuda(), B.cuda(), BLOCKS, None, 1),   # dense abid
                 lambda: tile("f16_16x16x32", A.cuda(), B.cuda(), 0, None, 0),
                 lambda: tile("f16_16x16x32", A.cuda().T, B.cuda(), BLOCKS, None, 0),
                 lambda: tile("sp_f16_16x16x64", A.cuda(), B.cuda(), BLOCKS, None, 2)):
        with pytest.raises(RuntimeError):
            call()


def test_health_report():
    base = ops.gpu_health_report(0, quick=True)
    rep = ops.gpu_health_report(0, quick=True, matrix_probe=True)
    assert set(rep) - set(base) == {"matrix_probe"} and rep["healthy"]
    probe = rep["matrix_probe"]
    assert probe["ok"] and probe["bad_cus"] == [] and probe["tiles"]["ok"]
    assert set(probe["tiles"]["paths"]) == {
        p if p not in ops.MATRIX_SPARSE_PATHS else f"{p}/abid{a}" for p, a in PATH_ABIDS}
    assert set(probe["burn"]["paths"]) == set(ops.MATRIX_BURN_PATHS)
    for path, s in probe["burn"]["paths"].items():
        print(f"{path}: chain {s['chain']} rounds {s['rounds']} {s['elapsed_ms']:.2f} ms "
              f"{s['tflops']:.1f} TFLOP/s")
        assert s["ok"] and s["cus_seen"] == rep["info"]["multiProcessorCount"]
