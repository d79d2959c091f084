"""Matrix-path probe (ops.matrix_tile, ops.matrix_burn): the f64, f32, f16,
i8, e5m2 and 32x32 MFMA shapes and the 2:4 structured-sparse smfmac forms.
Here: the path table, operands whose product the accumulator holds exactly,
the float64 / int64 reference, the one-hot cases that pin the fragment maps,
and the reports. See the kernel comment in hived_ops.hip.

A path is named by its instruction. In memory A is [M,K] and B is [K,M] in
the path's element type: float64, float32, float16, bfloat16, int8, or uint8
holding raw e4m3 / e5m2 bytes. A sparse path takes A compressed, [M,K/2]
values plus `index` [M,K/2] uint8: the position 0..3 of each value in its
group of four along K, two values per group, positions increasing.

Why no tolerance is needed, per element type:
  f16, bf16  signed multiples of 2^-8 below 1: products are multiples of 2^-16
             and a sum of 64 stays below 64, 22 bits, in any order
  f32        11-bit signed integers times one power of two per row of A and
             per column of B (2^-20 .. 2^20): all products of an output
             element share one power of two, are below 2^20 in its units, and
             the K <= 4 of them sum below 2^22
  f64        24-bit signed integers times one power of two per row or column
             (2^-200 .. 2^200): products below 2^46, four of them below 2^48
  e4m3       one exponent field per row of A and column of B (mfma_tiles): the
             products of an output element are integers <= 15 * 15 times one
             power of two, inside any window the fp8 pipes keep
  e5m2       the same with field m mod 31 (never field 31: inf and NaN);
             products are integers <= 7 * 7 times one power of two
  i8         the whole range with -128; |sum| <= 128 * 2^14 = 2^21
"""
from __future__ import annotations

from .mfma_tiles import _lossless, e4m3_values
from .mx_scale import mx_decode
from .records import (BadUnits, checksum_outliers, decode_hw_word, place_dicts, place_keys,
                      units_seen)

# path: (M, K, element of A, element of B, sparse)
_PATHS = {
    "f64_16x16x4": (16, 4, "f64", "f64", False),
    "f32_16x16x4": (16, 4, "f32", "f32", False),
    "f32_32x32x2": (32, 2, "f32", "f32", False),
    "f16_16x16x32": (16, 32, "f16", "f16", False),
    "f16_32x32x16": (32, 16, "f16", "f16", False),
    "bf16_32x32x16": (32, 16, "bf16", "bf16", False),
    "i8_16x16x64": (16, 64, "i8", "i8", False),
    "i8_32x32x32": (32, 32, "i8", "i8", False),
    "fp8_32x32x16": (32, 16, "e4m3", "e4m3", False),
    "bf8_16x16x32": (16, 32, "e5m2", "e5m2", False),
    "fp8bf8_16x16x32": (16, 32, "e4m3", "e5m2", False),
    "bf8fp8_16x16x32": (16, 32, "e5m2", "e4m3", False),
    "sp_f16_16x16x64": (16, 64, "f16", "f16", True),
    "sp_f16_32x32x32": (32, 32, "f16", "f16", True),
    "sp_bf16_16x16x64": (16, 64, "bf16", "bf16", True),
    "sp_i8_16x16x128": (16, 128, "i8", "i8", True),
}
MATRIX_PATHS = tuple(_PATHS)
MATRIX_SPARSE_PATHS = tuple(p for p in _PATHS if _PATHS[p][4])
MATRIX_BURN_PATHS = ("f64_16x16x4", "f32_32x32x2", "f16_16x16x32", "i8_16x16x64",
                     "bf8_16x16x32", "sp_f16_16x16x64")
# the index part selects that read another part of the index register: the
# 16-bit paths use 16 of its bits, i8 all 32 (BENCHMARKS.md "Matrix-path probe")
MATRIX_ABIDS = {p: ((0, 1) if _PATHS[p][2] != "i8" else (0,)) if _PATHS[p][4] else (0,)
                for p in _PATHS}
# the six ways two values sit in a group of four
MATRIX_INDEX_PAIRS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))
MATRIX_PROBE_SEED = 0
_MAT_NACC = 4
# per burn path, so that the timed launch at 2048 blocks takes tens of
# milliseconds (BENCHMARKS.md "Matrix-path probe")
_MAT_BURN_DEFAULTS = {
    "f64_16x16x4": (256, 64), "f32_32x32x2": (256, 32), "f16_16x16x32": (1024, 64),
    "i8_16x16x64": (1024, 64), "bf8_16x16x32": (1024, 64), "sp_f16_16x16x64": (1024, 64),
}


def matrix_path_shape(path: str) -> tuple:
    """(M, K, sparse) of a path; K is the dense K."""
    M, K, _, _, sparse = _PATHS[path]
    return M, K, sparse


def _torch_dtype(elem: str):
    import torch

    return {"f64": torch.float64, "f32": torch.float32, "f16": torch.float16,
            "bf16": torch.bfloat16, "i8": torch.int8, "e4m3": torch.uint8,
            "e5m2": torch.uint8}[elem]


def _acc_dtype(path: str):
    import torch

    elem = _PATHS[path][2]
    return torch.float64 if elem == "f64" else torch.int32 if elem == "i8" else torch.float32


def matrix_decode(elem: str, X):
    """The values of an operand: float64, or int64 for i8."""
    assert X.dtype == _torch_dtype(elem), (elem, X.dtype)
    if elem == "i8":
        return X.long()
    if elem == "e4m3":
        return e4m3_values()[X.long()]
    if elem == "e5m2":
        return mx_decode(1, X)
    return X.double()


def _encode(elem: str, values):
    """Encode float64 (i8: int64) `values`; asserts that nothing is lost."""
    import torch

    if elem == "e4m3":
        X = values.float().to(torch.float8_e4m3fn).view(torch.uint8)
    elif elem == "e5m2":
        X = values.float().to(torch.float8_e5m2).view(torch.uint8)
    else:
        X = values.to(_torch_dtype(elem))
    assert torch.equal(matrix_decode(elem, X), values), f"{elem} cannot hold these values"
    return X.contiguous()


def matrix_expand(values, index):
    """The dense [rows,K] operand of compressed `values` [rows,K/2] (decoded)
    and their positions `index`."""
    import torch

    rows, half = values.shape
    dense = torch.zeros(rows, 2 * half, dtype=values.dtype)
    col = 4 * (torch.arange(half) // 2).unsqueeze(0) + index.long()
    dense.scatter_(1, col, values)
    return dense


def matrix_product(path: str, A, B, index=None):
    """The reference: the float64 (i8: int64) product of the decoded operands,
    A expanded by `index` on a sparse path."""
    _, _, ea, eb, sparse = _PATHS[path]
    a, b = matrix_decode(ea, A), matrix_decode(eb, B)
    assert (index is not None) == sparse, path
    return (matrix_expand(a, index) if sparse else a) @ b


def matrix_exact(path: str, prod):
    """`prod` in the accumulator's type; asserts that the cast loses nothing."""
    import torch

    out = prod.to(_acc_dtype(path))
    if prod.dtype == torch.int64:
        assert torch.equal(out.long(), prod), f"{path}: the product does not fit int32"
    else:
        assert _lossless(out, prod), f"{path}: the product is not exact in the accumulator"
    return out.contiguous()


def _draw(elem: str, rows: int, cols: int, g, nonzero: bool = False):
    """[rows,cols] of `elem`, one row per row of A (B is drawn transposed)."""
    import torch

    def integers(bound):  # uniform in [-bound, bound], without 0 if nonzero
        i = torch.randint(-bound, bound + 1, (rows, cols), generator=g, dtype=torch.int64)
        return torch.where(i == 0, torch.full_like(i, bound), i) if nonzero else i

    r = torch.arange(rows).unsqueeze(1)
    if elem in ("f16", "bf16"):
        return _encode(elem, integers(255).double() / 256)
    if elem == "f32":    # the exponents walk 2^-20 .. 2^20 over the rows
        return _encode(elem, torch.ldexp(integers(1023).double(), (40 * r) // (rows - 1) - 20))
    if elem == "f64":
        return _encode(elem, torch.ldexp(integers((1 << 23) - 1).double(),
                                         (400 * r) // (rows - 1) - 200))
    if elem == "i8":
        i = torch.randint(-128, 128, (rows, cols), generator=g, dtype=torch.int64)
        return _encode(elem, torch.where(i == 0, torch.full_like(i, -128), i) if nonzero else i)
    ebits, mbits, fields = (4, 3, 16) if elem == "e4m3" else (5, 2, 31)
    sign = torch.randint(0, 2, (rows, cols), generator=g, dtype=torch.int64)
    man = torch.randint(0, 1 << mbits, (rows, cols), generator=g, dtype=torch.int64)
    code = (sign << (ebits + mbits)) | ((r % fields) << mbits) | man
    if elem == "e4m3":   # 0x7F, 0xFF are NaN: lowered by one, as in mfma_tiles
        code = code - ((code & 0x7F) == 0x7F).long()
    return code.to(torch.uint8)


def _draw_index(rows: int, half: int, g):
    """[rows,half] uint8 positions: one of the six pairs per group of four."""
    import torch

    pairs = torch.tensor(MATRIX_INDEX_PAIRS, dtype=torch.uint8)
    pick = torch.randint(0, 6, (rows, half // 2), generator=g)
    return pairs[pick].reshape(rows, half).contiguous()


def matrix_operand_invariants(path: str, A, B, index=None) -> dict:
    """What matrix_operands guarantees, as {name: bool}; each makes a class of
    fault visible in the product, as in tile_operand_invariants: no zero in
    A @ B, no all-zero column of A or row of B, columns of A and rows of B
    pairwise different by value, expected != expected.T, the product exact in
    the accumulator, and the range the element type is meant to cover (both
    extremes of i8, every exponent field of e4m3 / e5m2 that the rows reach,
    the power-of-two span of f32 and f64). Sparse paths add: all six position
    pairs occur and no compressed value is zero."""
    import torch

    M, K, ea, eb, sparse = _PATHS[path]
    av, b = matrix_decode(ea, A), matrix_decode(eb, B)
    a = matrix_expand(av, index) if sparse else av
    prod = a @ b
    off = ~torch.eye(K, dtype=torch.bool)
    try:
        matrix_exact(path, prod)
        exact = True
    except AssertionError:
        exact = False
    inv = {
        "finite": bool(torch.isfinite(a.double()).all() and torch.isfinite(b.double()).all()),
        "no_zero_product": bool((prod != 0).all()),
        "no_zero_slot": bool((a != 0).any(dim=0).all() and (b != 0).any(dim=1).all()),
        "a_columns_differ": bool(((a.T.unsqueeze(1) != a.T.unsqueeze(0)).any(-1) | ~off).all()),
        "b_rows_differ": bool(((b.unsqueeze(1) != b.unsqueeze(0)).any(-1) | ~off).all()),
        "asymmetric": not torch.equal(prod, prod.T),
        "exact": exact,
    }
    for elem, X, v in ((ea, A, av), (eb, B.T, b.T)):
        if elem == "i8":
            ok = int(v.min()) == -128 and int(v.max()) == 127
        elif elem in ("e4m3", "e5m2"):
            mbits, mask, fields = (3, 15, 16) if elem == "e4m3" else (2, 31, 31)
            rows = torch.arange(X.shape[0]).unsqueeze(1)
            ok = bool((((X.long() >> mbits) & mask) == rows % fields).all())
        elif elem in ("f32", "f64"):
            span, bits = (20, 10) if elem == "f32" else (200, 23)
            top = v.abs().amax(dim=1)
            ok = bool(top.min() < 2.0 ** (bits - span) and top.max() >= 2.0 ** span)
        else:
            ok = bool(torch.equal(v * 256, (v * 256).round()) and v.abs().max() < 1)
        inv["in_range"] = inv.get("in_range", True) and ok
    if sparse:
        pairs = {tuple(p) for p in index.view(-1, 2).tolist()}
        inv["all_index_pairs"] = pairs == set(MATRIX_INDEX_PAIRS)
        inv["no_zero_value"] = bool((av != 0).all())
    return inv


def matrix_operands(path: str, seed: int = MATRIX_PROBE_SEED):
    """Operands for one matrix_tile check, on the CPU, as the kernel takes
    them, and the tile a healthy GPU must return: (A, B, expected), or
    (A, B, expected, index) on a sparse path, `expected` [M,M] in the
    accumulator's type. Rows of A are redrawn until no element of the product
    is zero and the whole draw is repeated until every entry of
    matrix_operand_invariants holds."""
    import torch

    M, K, ea, eb, sparse = _PATHS[path]
    ka = K // 2 if sparse else K
    g = torch.Generator().manual_seed(int(seed))
    for _ in range(64):
        A, B = _draw(ea, M, ka, g, nonzero=sparse), _draw(eb, M, K, g).T.contiguous()
        index = _draw_index(M, ka, g) if sparse else None
        for _ in range(64):
            redraw = (matrix_product(path, A, B, index) == 0).any(dim=1)
            if not redraw.any():
                break
            A[redraw] = _draw(ea, M, ka, g, nonzero=sparse)[redraw]
        if all(matrix_operand_invariants(path, A, B, index).values()):
            expected = matrix_exact(path, matrix_product(path, A, B, index))
            return (A, B, expected, index) if sparse else (A, B, expected)
    raise AssertionError(f"no {path} operands with seed {seed} satisfy the invariants")


# --------------------------------------------------------------------------
# one-hot cases: each pins one thing about how the fragments are laid out
# --------------------------------------------------------------------------
def matrix_k_slot_case(path: str, k: int, k_b: int = None):
    """A dense path's slot case: A's only non-zero column is k (1 + m % 3 in
    row m), B's only non-zero row is k_b (default k; 1 + n % 4 in column n).
    The tile is the single product (1 + m % 3)(1 + n % 4), asymmetric, when
    the two name the same slot and zero otherwise: load_a and load_b put slot
    k in the same place. Returns (A, B, expected)."""
    import torch

    M, K, ea, eb, sparse = _PATHS[path]
    assert not sparse, path
    k_b = k if k_b is None else k_b
    wide = torch.int64 if ea == "i8" else torch.float64
    a, b = torch.zeros(M, K, dtype=wide), torch.zeros(K, M, dtype=wide)
    a[:, k] = (1 + torch.arange(M) % 3).to(wide)
    b[k_b] = (1 + torch.arange(M) % 4).to(wide)
    A, B = _encode(ea, a), _encode(eb, b)
    return A, B, matrix_exact(path, matrix_product(path, A, B))


def matrix_index_case(path: str, pair: tuple):
    """A sparse path's index case: in row m, group (m + 3 * pair number) mod
    K/4 holds the values (1, 2) at the positions `pair`, and every other
    compressed value is 0 at positions (0, 1). Row k of B is
    (7k + 3n) mod 11 - 5, different for any two rows of a group, so row m of
    the tile is B[4q + pair[0]] + 2 B[4q + pair[1]]: exactly those two rows.
    Over the rows the group walks every lane group and register pair.
    Returns (A, B, expected, index)."""
    import torch

    M, K, ea, eb, sparse = _PATHS[path]
    assert sparse, path
    wide = torch.int64 if ea == "i8" else torch.float64
    q = (torch.arange(M) + 3 * MATRIX_INDEX_PAIRS.index(tuple(pair))) % (K // 4)
    a = torch.zeros(M, K // 2, dtype=wide)
    index = torch.tensor([0, 1], dtype=torch.uint8).repeat(M, K // 4)
    rows = torch.arange(M)
    for j in (0, 1):
        a[rows, 2 * q + j] = 1 + j
        index[rows, 2 * q + j] = pair[j]
    kk, n = torch.arange(K).unsqueeze(1), torch.arange(M).unsqueeze(0)
    A, B = _encode(ea, a), _encode(eb, ((7 * kk + 3 * n) % 11 - 5).to(wide))
    return A, B, matrix_exact(path, matrix_product(path, A, B, index)), index.contiguous()


# --------------------------------------------------------------------------
# burn
# --------------------------------------------------------------------------
def matrix_chain_limit(path: str) -> int:
    """Largest `chain` for which the burn stays exact: operands are integers
    of magnitude <= 2, so a partial sum is an integer <= 4*K*chain (K the dense
    K), which must stay within 2^24 (f32 accumulator), 2^53 (f64) or 2^31
    (i32); and at most the 2^22 MFMAs per accumulator of a bounded run."""
    elem = _PATHS[path][2]
    bound = 1 << (53 if elem == "f64" else 31 if elem == "i8" else 24)
    return min(bound // (4 * _PATHS[path][1]), 1 << 22)


def matrix_burn_operands(path: str, seed: int = 0):
    """Integer operands in {-2..2} as in _burn_integers: (A [4M,K], B [K,M],
    unit [4,M,M]) with unit[n] the exact product A[nM:(n+1)M] @ B in the
    accumulator's type, the expected tile for chain = 1; a sparse path returns
    (A [4M,K/2] without zeros, B, unit, index). B is a fixed asymmetric
    pattern and rows of A are redrawn until no element of `unit` is zero."""
    import torch

    M, K, ea, eb, sparse = _PATHS[path]
    ka = K // 2 if sparse else K
    wide = torch.int64 if ea == "i8" else torch.float64
    g = torch.Generator().manual_seed(int(seed))
    k, n = torch.arange(K).unsqueeze(1), torch.arange(M).unsqueeze(0)
    b = ((3 * k + n + seed) % 5 - 2).to(wide)
    index = _draw_index(_MAT_NACC * M, ka, g) if sparse else None

    def draw():
        i = torch.randint(-2, 3, (_MAT_NACC * M, ka), generator=g, dtype=torch.int64)
        return (torch.where(i == 0, torch.full_like(i, 2), i) if sparse else i).to(wide)

    a = draw()
    while True:
        unit = (matrix_expand(a, index) if sparse else a) @ b
        redraw = (unit == 0).any(dim=1)
        if not redraw.any():
            break
        a[redraw] = draw()[redraw]
    assert not torch.equal(unit[:M], unit[:M].T)
    unit = matrix_exact(path, unit).view(_MAT_NACC, M, M).contiguous()
    A, B = _encode(ea, a), _encode(eb, b)
    return (A, B, unit, index) if sparse else (A, B, unit)


def judge_matrix_tiles(tiles, expected) -> bool:
    """Every element of every wave's tile equals `expected`, by value (-0 ==
    0; a NaN equals nothing), with no tolerance, as judge_mfma_tiles."""
    return bool((tiles == expected.to(tiles.device).unsqueeze(0)).all().item())


def summarize_matrix_burn(records, elapsed_ms: float, path: str, chain: int, rounds: int,
                          expected_cus: int) -> dict:
    """Turn the per-wave records of one ops.matrix_burn launch into a verdict,
    with the fields of summarize_burn. `tflops` counts 2*M*M*K per MFMA with
    the path's dense K: a sparse path reports dense-equivalent FLOP/s, twice
    the multiplies it performs. Pure numpy; needs no GPU."""
    import numpy as np

    rec = np.asarray(records).reshape(-1, 4).astype(np.int64)
    waves = int(rec.shape[0])
    M, K, _ = matrix_path_shape(path)
    flop = 2.0 * M * M * K * _MAT_NACC * chain * rounds * waves
    cus_seen = units_seen(rec[:, 0], decode_hw_word)
    bad = BadUnits()
    for word, mism, first, _ in rec[rec[:, 1] != 0]:
        bad.add(decode_hw_word(word), {"waves": 1, "mismatched_elements": mism}, (int(first),))
    mismatched_waves = int((rec[:, 1] != 0).sum())
    checksum_spread = bool(checksum_outliers(rec[:, 3]).any())
    return {
        "tflops": flop / (elapsed_ms * 1e-3) / 1e12 if elapsed_ms > 0 else 0.0,
        "elapsed_ms": float(elapsed_ms),
        "waves": waves,
        "cus_seen": cus_seen,
        "mismatched_waves": mismatched_waves,
        "bad_cus": bad.entries(("first_bad_round",)),
        "checksum_spread": checksum_spread,
        "ok": bool(mismatched_waves == 0 and not checksum_spread and cus_seen >= expected_cus),
    }


def _on(device: int, *tensors):
    return [None if t is None else t.cuda(device) for t in tensors]


def matrix_tile_report(device: int = 0, paths=MATRIX_PATHS, blocks: int = 2048) -> dict:
    """Every path (a sparse path once per meaningful abid, "<path>/abid<n>")
    over a full grid on matrix_operands(path, MATRIX_PROBE_SEED), judged
    bitwise. Returns {"paths": {name: {"ok", "spread"}}, "ok"}; `spread` says
    whether any wave's tile differs from wave 0's."""
    from . import _ops_on

    ops = _ops_on(device)
    out: dict = {"blocks": blocks, "paths": {}}
    for path in paths:
        A, B, expected, *index = matrix_operands(path)
        A, B, index = _on(device, A, B, index[0] if index else None)
        for abid in MATRIX_ABIDS[path]:
            tiles = ops.matrix_tile(path, A, B, blocks, index, abid)
            name = f"{path}/abid{abid}" if index is not None else path
            out["paths"][name] = {"ok": judge_matrix_tiles(tiles, expected),
                                  "spread": bool((tiles != tiles[:1]).any().item())}
    out["ok"] = all(p["ok"] for p in out["paths"].values())
    return out


def matrix_burn_report(device: int = 0, paths=MATRIX_BURN_PATHS, blocks: int = 2048,
                       chain: int = None, rounds: int = None, inject=None, abid: int = 0) -> dict:
    """Run the burn for each burn path on one GPU. Returns {"paths": {path:
    summarize_matrix_burn(...) + chain, rounds}, "ok", "bad_cus"}: `ok` the
    AND and `bad_cus` the union over paths. chain and rounds default per path.
    `inject=(wave, round)` flips one accumulator bit in that wave at that
    round (register-only) to exercise detection."""
    from . import _ops_on

    plan = {path: (_MAT_BURN_DEFAULTS[path][0] if chain is None else int(chain),
                   _MAT_BURN_DEFAULTS[path][1] if rounds is None else int(rounds))
            for path in paths}
    for path, (c, _) in plan.items():
        assert 1 <= c <= matrix_chain_limit(path), f"{path}: chain {c} breaks exactness"
    ops = _ops_on(device)
    inject_wave, inject_round = (-1, -1) if inject is None else inject
    expected_cus = ops.device_info(device)["multiProcessorCount"]
    out: dict = {"blocks": blocks, "paths": {}}
    bad = set()
    for path, (c, r) in plan.items():
        A, B, unit, *index = matrix_burn_operands(path, seed=0)
        A, B, want, index = _on(device, A, B, unit * c, index[0] if index else None)
        records, ms = ops.matrix_burn(path, A, B, want, blocks, c, r, inject_wave, inject_round,
                                      index, abid if index is not None else 0)
        s = summarize_matrix_burn(records.cpu().numpy(), ms, path, c, r, expected_cus)
        s.update(chain=c, rounds=r)
        out["paths"][path] = s
        bad |= place_keys(s["bad_cus"], 4)
    out["ok"] = all(s["ok"] for s in out["paths"].values())
    out["bad_cus"] = place_dicts(bad)
    return out


def matrix_probe_report(device: int = 0) -> dict:
    """The matrix-path probe on one GPU: {"tiles": matrix_tile_report, "burn":
    matrix_burn_report, "ok", "bad_cus"} (the burn names CUs; a wrong tile
    fails the GPU without naming one, as for the single-tile checks)."""
    tiles = matrix_tile_report(device)
    burn = matrix_burn_report(device)
    return {"tiles": tiles, "burn": burn, "ok": bool(tiles["ok"] and burn["ok"]),
            "bad_cus": burn["bad_cus"]}
