"""Atomic probe: the exact atomic burn (ops.atomic_burn) on cells a lane owns,
attributed per CU, and contended atomics on cells every workgroup shares
(ops.atomic_contend), attributed per cell and per CU. See the kernel comments
in hived_ops.hip.

What it proves: the results and returned values of the global and LDS atomic
instructions listed there, both cmpswap arms, exact float adds in four
formats, and that no update is lost or duplicated when every CU of every XCD
contends. What it does not prove: which unit executed a global atomic (a wrong
result is attributed to the issuing CU and to the cell's byte offset),
system-scope or cross-GPU atomics, or float atomics on values that round.
"""
from __future__ import annotations

from .records import (_M32, _M64, BadUnits, _fmix32, _mix64, _u64_fields, checksum_outliers,
                      decode_hw_word, place_dicts, place_keys, units_seen)

ATOMIC_SECTIONS = ("g32", "g64", "gfp", "lds")
_ATOMIC_SECTION_ID = {s: i for i, s in enumerate(ATOMIC_SECTIONS)}
# cells per lane, in the order of `expected`
ATOMIC_CELLS = {"g32": 4, "g64": 4, "gfp": 5, "lds": 10}
# operation indices within a step; the last stands for the final compare
ATOMIC_STEP_OPS = {"g32": 28, "g64": 28, "gfp": 12, "lds": 44}
ATOMIC_INT_OPS = ("add", "sub", "xor", "smin", "smax", "umin", "umax", "and", "or", "swap",
                  "inc", "dec", "cmpswap_ok", "cmpswap_fail")
ATOMIC_FP_OPS = ("add_f32", "add_f64", "min_f64", "max_f64", "pk_add_f16", "pk_add_bf16")
ATOMIC_LDS_MAX_CHAIN = 64  # the ticket's owner table (u16 x 256 x chain) lives in LDS
# per section, so that each timed launch takes tens of milliseconds at the
# default grid (BENCHMARKS.md "Atomic probe")
_ATOMIC_DEFAULT_CHAIN = {"g32": 8, "g64": 8, "gfp": 16, "lds": 32}
# odd: every round ends in the same cells, so the xor checksum over an even
# number of rounds cancels to zero
_ATOMIC_DEFAULT_ROUNDS = 33
_ATOMIC_DEFAULT_BLOCKS = 2048

CONTEND_SECTIONS = ("ticket", "reduce", "cas")
CONTEND_CELL_BYTES = 4096
REDUCE_OPS = ("add_u32", "add_u64", "xor", "or", "and", "umin", "umax", "smin", "smax",
              "add_f32", "add_f64", "pk_add_bf16", "pk_add_f16")
# slot k of a cell is int64 word 16*k (128 bytes apart); the bits that count
_REDUCE_MASK = {op: (_M64 if op in ("add_u64", "add_f64") else _M32) for op in REDUCE_OPS}
REDUCE_OR_CONTRIBUTIONS = 24    # per cell: the rest contribute the identity
REDUCE_PK_CONTRIBUTIONS = 128   # per cell: |sum| <= 128 (bf16), <= 2048 (f16)
_CONTEND_BLOCKS_PER_CU = 8
# (per_lane, cells) per section at the default grid (BENCHMARKS.md "Atomic probe")
_CONTEND_DEFAULT_SHAPE = {"ticket": (4, 64), "reduce": (1, 64), "cas": (1, 4096)}

_K1, _K2 = 0x9E3779B1, 0x85EBCA6B


# --------------------------------------------------------------------------
# host mirror of the burn: the 64 lanes of a wave at once, integers only
# --------------------------------------------------------------------------
def _seed_words(section: str, seed: int, cell: int):
    """valu_seed_state(seed, section id, cell*64 + lane) of the kernel for the
    64 lanes: (low words, high words) as np.uint32."""
    import numpy as np

    idx = np.arange(64, dtype=np.uint32) + np.uint32(cell * 64)
    start = idx * np.uint32(_K2) + np.uint32(
        (int(seed) + _ATOMIC_SECTION_ID[section] * 0x9E3779B9) & _M32)
    lo = _fmix32(start)
    return lo, _fmix32(lo ^ np.uint32(0xC2B2AE35))


def _seed_u64(section: str, seed: int, cell: int):
    import numpy as np

    lo, hi = _seed_words(section, seed, cell)
    return (hi.astype(np.uint64) << np.uint64(32)) | lo.astype(np.uint64)


def _operand(m, c: int, i: int):
    """atomic_operand of the kernel: fmix32 (u32 mirrors) or splitmix64 (u64)
    of the mirror xor a word of the step and the operation."""
    import numpy as np

    k = (int(c) * _K1 + int(i) * _K2) & _M32
    if m.dtype == np.uint32:
        return _fmix32(m ^ np.uint32(k))
    return _mix64(m ^ np.uint64(k))


def _int_step(m: list, c: int, outcomes: set = None) -> None:
    """One step of the integer sequence on the four cells m[0..3] (np.uint32
    or np.uint64 [64] each), in place. `outcomes` collects which arm of inc,
    dec and cmpswap occurred."""
    import numpy as np

    signed = np.int32 if m[0].dtype == np.uint32 else np.int64
    one, zero = m[0].dtype.type(1), m[0].dtype.type(0)

    def note(name, wrapped):
        if outcomes is not None:
            if wrapped.any():
                outcomes.add((name, "wrap"))
            if (~wrapped).any():
                outcomes.add((name, "step"))

    def inc(v, x):
        note("inc", v >= x)
        return np.where(v >= x, zero, v + one)

    def dec(v, x):
        wrapped = (v == zero) | (v > x)
        note("dec", wrapped)
        return np.where(wrapped, x, v - one)

    sequence = (
        (0, lambda v, x: v + x), (0, lambda v, x: v - x), (0, lambda v, x: v ^ x),
        (1, lambda v, x: np.where(x.view(signed) < v.view(signed), x, v)),
        (1, lambda v, x: np.where(x.view(signed) > v.view(signed), x, v)),
        (1, np.minimum), (1, np.maximum),
        (2, lambda v, x: v & x), (2, lambda v, x: v | x), (2, lambda v, x: x),
        (3, inc), (3, dec),
        (3, lambda v, x: x),   # cmpswap with the true value: succeeds
        (3, lambda v, x: v),   # cmpswap with a wrong value: fails
    )
    for k, (j, apply) in enumerate(sequence):
        for form in (0, 1):  # returning, then non-returning
            m[j] = apply(m[j], _operand(m[j], c, 2 * k + form))
    if outcomes is not None:
        outcomes |= {("cmpswap", "ok"), ("cmpswap", "fail")}


def _f16_bits(v):
    import numpy as np

    return v.astype(np.float16).view(np.uint16).astype(np.uint32)


def _bf16_bits(v):
    import numpy as np

    return v.astype(np.float32).view(np.uint32) >> np.uint32(16)


def _pack(bits0, bits1):
    import numpy as np

    return bits0 | (bits1 << np.uint32(16))


class _FpCells:
    """The float cells of the 64 lanes as integer mirrors (np.int64): f32 add,
    f64 add, f64 min/max, packed f16 halves, packed bf16 halves. `exact` turns
    False when a value leaves the range in which its format holds every
    integer: |x| < 2^24 (f32), < 2^53 (f64), <= 2048 (f16), <= 256 (bf16)."""

    def __init__(self, section: str, seed: int, first_cell: int):
        import numpy as np

        i64 = np.int64
        lo = [_seed_words(section, seed, first_cell + j)[0] for j in range(5)]
        wide = [_seed_u64(section, seed, first_cell + j) for j in (1, 2)]
        self.f = (lo[0] & np.uint32(0xFFFFF)).astype(i64) - 0x80000
        self.d = (wide[0] & np.uint64((1 << 50) - 1)).astype(i64) - (1 << 49)
        self.mm = (wide[1] & np.uint64((1 << 50) - 1)).astype(i64) - (1 << 49)
        self.h = [(lo[3] & np.uint32(511)).astype(i64) - 256,
                  ((lo[3] >> np.uint32(16)) & np.uint32(511)).astype(i64) - 256]
        self.b = [(lo[4] & np.uint32(63)).astype(i64) - 32,
                  ((lo[4] >> np.uint32(16)) & np.uint32(63)).astype(i64) - 32]
        self.exact = True
        self._check()

    def _check(self) -> None:
        import numpy as np

        ok = (np.abs(self.f).max() < (1 << 24) and np.abs(self.d).max() < (1 << 53)
              and np.abs(self.mm).max() < (1 << 53)
              and max(np.abs(h).max() for h in self.h) <= 2048
              and max(np.abs(b).max() for b in self.b) <= 256)
        self.exact = bool(self.exact and ok)

    def step(self, c: int) -> None:
        import numpy as np

        i64, u32, u64 = np.int64, np.uint32, np.uint64
        for form in (0, 1):
            h = _operand(self.f.astype(u32), c, form)
            self.f = self.f + ((h % u32(2047)).astype(i64) - 1023)
            self._check()
        for form in (0, 1):
            h = _operand(self.d.view(u64), c, 2 + form)
            self.d = self.d + ((h & u64((1 << 41) - 1)).astype(i64) - (1 << 40))
            self._check()
        for form in range(4):
            h = _operand(self.mm.view(u64), c, 4 + form)
            x = (h & u64((1 << 52) - 1)).astype(i64) - (1 << 51)
            self.mm = np.minimum(self.mm, x) if form < 2 else np.maximum(self.mm, x)
        for form in (0, 1):
            h = _operand(_pack(_f16_bits(self.h[0]), _f16_bits(self.h[1])), c, 8 + form)
            self.h[0] = self.h[0] + (((h & u32(0xFFFF)) % u32(31)).astype(i64) - 15)
            self.h[1] = self.h[1] + (((h >> u32(16)) % u32(31)).astype(i64) - 15)
            self._check()
        for form in (0, 1):
            h = _operand(_pack(_bf16_bits(self.b[0]), _bf16_bits(self.b[1])), c, 10 + form)
            self.b[0] = self.b[0] + (((h & u32(0xFFFF)) % u32(7)).astype(i64) - 3)
            self.b[1] = self.b[1] + (((h >> u32(16)) % u32(7)).astype(i64) - 3)
            self._check()

    def bits(self) -> list:
        """The five cells' raw bits as np.uint64 [64] each, in `expected` order."""
        import numpy as np

        u64 = np.uint64
        return [self.f.astype(np.float32).view(np.uint32).astype(u64),
                self.d.astype(np.float64).view(u64), self.mm.astype(np.float64).view(u64),
                _pack(_f16_bits(self.h[0]), _f16_bits(self.h[1])).astype(u64),
                _pack(_bf16_bits(self.b[0]), _bf16_bits(self.b[1])).astype(u64)]


def _burn_mirror(section: str, seed: int, chain: int, stop_when_inexact: bool = False):
    """(cells as a list of np.uint64 [64], exact, outcomes) after `chain` steps."""
    import numpy as np

    if section not in ATOMIC_SECTIONS:
        raise ValueError(f"section must be one of {ATOMIC_SECTIONS}; got {section!r}")
    ints = wide = fp = None
    if section in ("g32", "lds"):
        ints = [_seed_words(section, seed, j)[0] for j in range(4)]
    if section == "g64":
        ints = [_seed_u64(section, seed, j) for j in range(4)]
    if section == "lds":
        wide = _seed_u64(section, seed, 4)
    if section in ("gfp", "lds"):
        fp = _FpCells(section, seed, 5 if section == "lds" else 0)
    outcomes: set = set()
    for c in range(int(chain)):
        if ints is not None:
            _int_step(ints, c, outcomes)
        if wide is not None:
            for form in (0, 1):
                wide = wide + _operand(wide, c, form)
            for form in (2, 3):
                wide = wide ^ _operand(wide, c, form)
        if fp is not None:
            fp.step(c)
            if stop_when_inexact and not fp.exact:
                break
    cells = [] if ints is None else [v.astype(np.uint64) for v in ints]
    if wide is not None:
        cells.append(wide)
    if fp is not None:
        cells += fp.bits()
    return cells, (fp.exact if fp is not None else True), outcomes


def atomic_burn_expected(section: str, seed: int, chain: int):
    """The raw bits (np.uint64 [cells*64], cell j of lane l at j*64 + l) every
    wave's cells must hold after `chain` steps of ops.atomic_burn: the host
    mirror of the kernel, on integers only."""
    import numpy as np

    return np.concatenate(_burn_mirror(section, seed, chain)[0])


def atomic_burn_outcomes(section: str, seed: int, chain: int) -> set:
    """Which arms the integer cells of a section went through in `chain` steps:
    ("inc" | "dec", "wrap" | "step") and ("cmpswap", "ok" | "fail")."""
    return _burn_mirror(section, seed, chain)[2]


def atomic_fp_exact(seed: int, chain: int) -> bool:
    """Does every float cell of sections gfp and lds stay, through `chain`
    steps from `seed`, in the range in which its format holds every integer?
    Only then are the float adds exact and the bitwise compare meaningful."""
    return all(_burn_mirror(s, seed, chain, stop_when_inexact=True)[1] for s in ("gfp", "lds"))


def atomic_burn_checksum(section: str, seed: int, chain: int, rounds: int) -> int:
    """The 64-bit xor checksum (record fields [4] low, [5] high) of a healthy
    wave: the xor of the final cells over the lanes for odd `rounds` (u32 cells
    alternate between the low and the high word), 0 for even."""
    import numpy as np

    if int(rounds) % 2 == 0:
        return 0
    cells = _burn_mirror(section, seed, chain)[0]
    total = 0
    if section != "gfp":
        shift = 32 if section in ("g32", "lds") else 0
        for j, cell in enumerate(cells[:4]):
            total ^= int(np.bitwise_xor.reduce(cell)) << (shift * (j & 1))
    if section == "lds":
        total ^= int(np.bitwise_xor.reduce(cells[4]))
    if section in ("gfp", "lds"):
        f, d, mm, h, b = (int(np.bitwise_xor.reduce(cell)) for cell in cells[-5:])
        total ^= d ^ mm ^ (f << 32) ^ h ^ (b << 32)
    return total & _M64


# --------------------------------------------------------------------------
# host mirror of the contended sections
# --------------------------------------------------------------------------
def contend_lanes_on_cell(lanes: int, cells: int):
    """How many of the `lanes` lanes (lane gid works on cell gid % cells) work
    on each cell: np.int64 [cells]."""
    import numpy as np

    return lanes // cells + (np.arange(cells, dtype=np.int64) < lanes % cells)


def atomic_cas_cap(lanes: int, per_lane: int, cells: int):
    """The retry cap of the cmpswap section per cell, derived: exactly N =
    lanes on the cell * per_lane cmpswaps succeed in a launch and every failure
    is caused by one of them, so no healthy lane fails N times."""
    return contend_lanes_on_cell(lanes, cells) * int(per_lane)


def atomic_reduce_contributions(seed: int, lanes: int, per_lane: int, cells: int) -> dict:
    """What every (lane, j) contributes in the reduce section, flattened in
    (lane, j) order: {"cell": np.int64, op: values}. Integer ops hold the
    np.uint32 / np.uint64 operands, the float ops the integers added (np.int64;
    [n, 2] halves for the packed ops)."""
    import numpy as np

    u32, i64 = np.uint32, np.int64
    gid = np.repeat(np.arange(lanes, dtype=i64), per_lane)
    j = np.tile(np.arange(per_lane, dtype=i64), lanes)
    n = (gid // cells) * per_lane + j
    h = _fmix32(gid.astype(u32) * u32(_K1) + j.astype(u32) * u32(_K2) + u32(int(seed) & _M32))
    hk = [_fmix32(h + u32((k * 0x632BE5AB) & _M32)) for k in range(13)]
    few, pk = n < REDUCE_OR_CONTRIBUTIONS, n < REDUCE_PK_CONTRIBUTIONS
    bit = lambda x: u32(1) << (x & u32(31))  # noqa: E731
    sign = lambda x, b: np.where((x & u32(b)) != 0, 1, -1).astype(i64)  # noqa: E731
    half = lambda x: (x % u32(33)).astype(i64) - 16  # noqa: E731
    return {
        "cell": gid % cells,
        "add_u32": hk[0],
        "add_u64": (hk[1].astype(np.uint64) << np.uint64(32)) | h.astype(np.uint64),
        "xor": hk[2],
        "or": np.where(few, bit(hk[3]), u32(0)),
        "and": np.where(few, ~bit(hk[4]), u32(_M32)),
        "umin": hk[5], "umax": hk[6], "smin": hk[7], "smax": hk[8],
        "add_f32": (hk[9] % u32(257)).astype(i64) - 128,
        "add_f64": hk[10].view(np.int32).astype(i64),
        "pk_add_bf16": np.where(pk[:, None], np.stack([sign(hk[11], 1), sign(hk[11], 2)], 1), 0),
        "pk_add_f16": np.where(pk[:, None], np.stack([half(hk[12] & u32(0xFFFF)),
                                                      half(hk[12] >> u32(16))], 1), 0),
    }


_REDUCE_INIT = {"and": _M32, "umin": _M32, "smin": 0x7FFFFFFF, "smax": 0x80000000}


def atomic_reduce_expected(seed: int, lanes: int, per_lane: int, cells: int) -> dict:
    """{op: np.uint64 [cells]}: the raw bits every cell's slot must hold after
    the reduce section, whatever the arrival order. Exact integer arithmetic;
    the float results are converted at the end (every partial sum is an integer
    the format holds: tests/test_atomic_probe_report.py folds them in native
    width in several orders)."""
    import numpy as np

    u64, i64 = np.uint64, np.int64
    con = atomic_reduce_contributions(seed, lanes, per_lane, cells)
    cell = con["cell"]

    def fold(ufunc, values, init, dtype):
        acc = np.full(cells, init, dtype=dtype)
        ufunc.at(acc, cell, values.astype(dtype))
        return acc

    out = {
        "add_u32": fold(np.add, con["add_u32"], 0, u64) & u64(_M32),
        "add_u64": fold(np.add, con["add_u64"], 0, u64),
        "xor": fold(np.bitwise_xor, con["xor"], 0, u64),
        "or": fold(np.bitwise_or, con["or"], 0, u64),
        "and": fold(np.bitwise_and, con["and"], _M32, u64),
        "umin": fold(np.minimum, con["umin"], _M32, u64),
        "umax": fold(np.maximum, con["umax"], 0, u64),
    }
    for op, ufunc, init in (("smin", np.minimum, 0x7FFFFFFF), ("smax", np.maximum, -0x80000000)):
        out[op] = (fold(ufunc, con[op].view(np.int32), init, i64) & _M32).astype(u64)
    out["add_f32"] = fold(np.add, con["add_f32"], 0, i64).astype(np.float32).view(
        np.uint32).astype(u64)
    out["add_f64"] = fold(np.add, con["add_f64"], 0, i64).astype(np.float64).view(u64)
    for op, bits in (("pk_add_bf16", _bf16_bits), ("pk_add_f16", _f16_bits)):
        halves = [bits(fold(np.add, con[op][:, k], 0, i64)) for k in (0, 1)]
        out[op] = _pack(*halves).astype(u64)
    return out


def _cas_values(seed: int, index):
    """mix64((seed << 32) | index) on np.uint64, as the kernel's."""
    import numpy as np

    return _mix64(np.uint64((int(seed) & _M32) << 32) ^ index.astype(np.uint64))


def atomic_cas_expected(seed: int, lanes: int, per_lane: int, cells: int):
    """np.uint64 [cells]: the seeded cell plus per_lane times the value of
    every lane on it, mod 2^64."""
    import numpy as np

    gid = np.arange(lanes, dtype=np.int64)
    acc = _cas_values(seed, np.arange(cells, dtype=np.int64))
    np.add.at(acc, gid % cells, _cas_values(seed, gid) * np.uint64(per_lane))
    return acc


# --------------------------------------------------------------------------
# summarisers
# --------------------------------------------------------------------------
def summarize_atomic_burn(records, elapsed_ms: float, section: str, chain: int, rounds: int,
                          expected_cus: int) -> dict:
    """Turn the per-wave records of one ops.atomic_burn launch into a verdict.

    records: [waves, 8] int32 rows {hw word, mismatched lane-steps (the final
    compare counts as one more step), first bad round (-1), lowest bad lane in
    it (-1), xor checksum low / high word, that lane's first bad operation
    index (-1; ATOMIC_STEP_OPS[section] stands for the final compare), ticket
    faults (lds only)}. A wave is bad when it mismatched, when its checksum is
    not the majority's or when its workgroup's ticket was wrong; it is
    attributed to the CU of its hw word. Pure numpy; needs no GPU.
    """
    import numpy as np

    rec = np.asarray(records).reshape(-1, 8).astype(np.int64)
    cus_seen = units_seen(rec[:, 0], decode_hw_word)
    odd = checksum_outliers(_u64_fields(rec, 4))
    bad = BadUnits()
    for row in rec[(rec[:, 1] != 0) | odd | (rec[:, 7] != 0)]:
        bad.add(decode_hw_word(row[0]),
                {"waves": 1, "mismatched_lane_steps": row[1], "ticket_faults": row[7]},
                (int(row[2]), int(row[3]), int(row[6])) if row[1] != 0 else None)
    mismatched_waves = int((rec[:, 1] != 0).sum())
    checksum_spread = bool(odd.any())
    ticket_faults = int(rec[:, 7].sum())
    steps = int(chain) * int(rounds)
    return {
        "section": section,
        "chain": int(chain),
        "rounds": int(rounds),
        "elapsed_ms": float(elapsed_ms),
        "us_per_step": float(elapsed_ms) * 1000.0 / steps if steps else 0.0,
        "waves": int(rec.shape[0]),
        "cus_seen": cus_seen,
        "mismatched_waves": mismatched_waves,
        "checksum_spread": checksum_spread,
        "ticket_faults": ticket_faults,
        "bad_cus": bad.entries(("first_bad_round", "first_bad_lane", "first_bad_op")),
        "ok": bool(mismatched_waves == 0 and not checksum_spread and ticket_faults == 0
                   and cus_seen >= expected_cus),
    }


def summarize_atomic_contend(section: str, shared, owner, records, elapsed_ms: float, seed: int,
                             blocks: int, per_lane: int, cells: int,
                             expected_xccs: int) -> dict:
    """Judge one ops.atomic_contend launch from the buffers copied back.

    shared: [cells, 512] int64, owner: [cells, width] int32 (ticket), records:
    [blocks*4, 8] int32 rows {hw word, non-increasing tickets, out-of-range
    tickets, lanes that gave up, failed cmpswaps, ...}. `bad_cells` lists
    {cell, byte_offset, section, op, got, want}: per cell a wrong counter (op
    "counter"), unmarked owner entries (op "owner": got is their number, with
    `first_hole`) or a wrong reduced or summed value (op: its name);
    out-of-range tickets, which no cell shows, are listed with cell -1. `bad_cus`
    names the CUs of waves whose own tickets did not increase, that drew an
    out-of-range ticket or that gave up. `ok` also needs waves on
    `expected_xccs` XCDs. Rates are reported, never judged. Pure numpy.
    """
    import numpy as np

    if section not in CONTEND_SECTIONS:
        raise ValueError(f"section must be one of {CONTEND_SECTIONS}; got {section!r}")
    shared = np.asarray(shared).reshape(cells, -1).astype(np.int64)
    rec = np.asarray(records).reshape(-1, 8).astype(np.int64)
    lanes = int(blocks) * 256
    on_cell = contend_lanes_on_cell(lanes, cells) * int(per_lane)
    operations = lanes * int(per_lane)
    bad_cells = []

    def cell_fault(cell, op, got, want, **more):
        bad_cells.append({"cell": int(cell), "byte_offset": int(cell) * CONTEND_CELL_BYTES
                          if cell >= 0 else -1, "section": section, "op": op,
                          "got": int(got), "want": int(want), **more})

    out = {"section": section, "blocks": int(blocks), "per_lane": int(per_lane),
           "cells": int(cells), "operations": operations, "elapsed_ms": float(elapsed_ms)}
    us = float(elapsed_ms) * 1000.0
    if section == "ticket":
        own = np.asarray(owner).reshape(cells, -1)
        counters = shared[:, 0] & _M32
        lost = 0
        for c in range(cells):
            if counters[c] != on_cell[c]:
                cell_fault(c, "counter", counters[c], on_cell[c])
            holes = np.flatnonzero(own[c, :on_cell[c]] == 0)
            if len(holes):
                lost += len(holes)
                cell_fault(c, "owner", len(holes), 0, first_hole=int(holes[0]))
        out_of_range = int(rec[:, 2].sum())
        if out_of_range:
            cell_fault(-1, "out_of_range", out_of_range, 0)
        out.update(lost=int(lost), out_of_range=out_of_range,
                   counter_error=[int(v) for v in counters - on_cell],
                   tickets_per_us=operations / us if us else 0.0)
    elif section == "reduce":
        want = atomic_reduce_expected(seed, lanes, per_lane, cells)
        values = {}
        for k, op in enumerate(REDUCE_OPS):
            got = shared[:, 16 * k].view(np.uint64) & np.uint64(_REDUCE_MASK[op])
            values[op] = {"got": [int(v) for v in got], "want": [int(v) for v in want[op]]}
            for c in np.flatnonzero(got != want[op]):
                cell_fault(c, op, got[c], want[op][c])
        # bytes the thirteen operations add per contribution: 9 x 4 + 2 x 8 + 2 x 4
        out.update(values=values, added_gbytes_per_s=operations * 60 / (us * 1e3) if us else 0.0)
    else:
        want = atomic_cas_expected(seed, lanes, per_lane, cells)
        got = shared[:, 0].view(np.uint64)
        for c in np.flatnonzero(got != want):
            cell_fault(c, "cmpswap_add", got[c], want[c])
        retries = int(rec[:, 4].sum())
        out.update(gave_up=int(rec[:, 3].sum()), retries=retries,
                   retries_per_success=retries / operations)
    bad = BadUnits()
    for row in rec[(rec[:, 1] != 0) | (rec[:, 2] != 0) | (rec[:, 3] != 0)]:
        bad.add(decode_hw_word(row[0]), {"waves": 1, "not_increasing": row[1],
                                         "out_of_range": row[2], "gave_up": row[3]})
    xccs_seen = len({int(w) >> 16 for w in np.unique(rec[:, 0])})
    out.update(
        bad_cells=bad_cells,
        bad_cus=bad.entries(()),
        xccs_seen=xccs_seen,
        cus_seen=units_seen(rec[:, 0], decode_hw_word),
        ok=bool(not bad_cells and not bad._units and xccs_seen >= expected_xccs),
    )
    return out


# --------------------------------------------------------------------------
# reports (these launch kernels)
# --------------------------------------------------------------------------
def atomic_burn_report(device: int = 0, sections=ATOMIC_SECTIONS,
                       blocks: int = _ATOMIC_DEFAULT_BLOCKS, chain: int = None,
                       rounds: int = None, seed: int = 1, inject=None) -> dict:
    """Run the atomic burn for each section on one GPU.

    Returns {"sections": {section: summarize_atomic_burn(...)}, "ok",
    "bad_cus"} where `ok` is the AND and `bad_cus` the union ((xcc, se, sh, cu)
    dicts, sorted) over sections. `chain` defaults per section. A `chain` for
    which atomic_fp_exact(seed, chain) is False is refused for the float
    sections: their compare is bitwise only while every sum is exact.
    `inject=(wave, round, lane, bit)` has that lane issue one extra atomic xor
    of that bit on its own first cell before that round's chain: it touches
    nothing the lane does not own and exercises the detection path on healthy
    hardware.
    """
    import torch

    from . import _ops_on

    rounds = _ATOMIC_DEFAULT_ROUNDS if rounds is None else int(rounds)
    ops = _ops_on(device)
    inject_args = (-1, -1, -1, -1) if inject is None else tuple(int(v) for v in inject)
    expected_cus = ops.device_info(device)["multiProcessorCount"]
    out: dict = {"blocks": blocks, "rounds": rounds, "sections": {}}
    bad = set()
    for section in sections:
        steps = _ATOMIC_DEFAULT_CHAIN[section] if chain is None else int(chain)
        if section in ("gfp", "lds") and not atomic_fp_exact(seed, steps):
            raise ValueError(f"chain {steps} from seed {seed} leaves the range in which the "
                             f"float atomics of section {section} are exact")
        want = atomic_burn_expected(section, seed, steps)
        expected = torch.from_numpy(want.view("int64").copy()).cuda(device)
        records, ms = ops.atomic_burn(expected, section, seed, blocks, steps, rounds, *inject_args)
        s = summarize_atomic_burn(records.cpu().numpy(), ms, section, steps, rounds, expected_cus)
        out["sections"][section] = s
        bad |= place_keys(s["bad_cus"], 4)
    out["ok"] = all(s["ok"] for s in out["sections"].values())
    out["bad_cus"] = place_dicts(bad)
    return out


def atomic_contend_report(device: int = 0, sections=CONTEND_SECTIONS, blocks: int = None,
                          per_lane: int = None, cells: int = None, seed: int = 1,
                          expected_xccs: int = None) -> dict:
    """Run the contended sections on one GPU and judge them on the host.

    Returns {"sections": {section: summarize_atomic_contend(...)}, "ok",
    "bad_cus", "bad_cells", "xccs_seen"}. The default grid is eight workgroups
    per CU, so every CU of every XCD takes part; per_lane and cells default per
    section. `expected_xccs` defaults to the number of XCDs a coverage launch
    finds on the device.
    """
    from . import _ops_on

    ops = _ops_on(device)
    cus = ops.device_info(device)["multiProcessorCount"]
    blocks = _CONTEND_BLOCKS_PER_CU * cus if blocks is None else int(blocks)
    if expected_xccs is None:
        expected_xccs = len({int(w) >> 16 for w in ops.cu_coverage(4096).cpu().numpy()})
    out: dict = {"blocks": blocks, "expected_xccs": int(expected_xccs), "sections": {}}
    bad, bad_cells = set(), []
    for section in sections:
        lane_default, cell_default = _CONTEND_DEFAULT_SHAPE[section]
        n = lane_default if per_lane is None else int(per_lane)
        c = cell_default if cells is None else int(cells)
        got = ops.atomic_contend(section, seed, blocks, n, c)
        s = summarize_atomic_contend(section, got["shared"].cpu().numpy(),
                                     got["owner"].cpu().numpy(), got["records"].cpu().numpy(),
                                     got["ms"], seed, blocks, n, c, expected_xccs)
        s.pop("values", None)  # per op and cell: kept by the summariser, too long for a report
        s.pop("counter_error", None)
        out["sections"][section] = s
        bad |= place_keys(s["bad_cus"], 4)
        bad_cells += s["bad_cells"]
    out["ok"] = all(s["ok"] for s in out["sections"].values())
    out["bad_cus"] = place_dicts(bad)
    out["bad_cells"] = bad_cells
    out["xccs_seen"] = min(s["xccs_seen"] for s in out["sections"].values())
    return out


def atomic_probe_report(device: int = 0) -> dict:
    """Both parts at their default shapes: {"burn": atomic_burn_report,
    "contend": atomic_contend_report, "ok", "bad_cus", "bad_cells"}, `ok` the
    AND, `bad_cus` the union and `bad_cells` the contended part's."""
    parts = {"burn": atomic_burn_report(device), "contend": atomic_contend_report(device)}
    bad = set().union(*(place_keys(p["bad_cus"], 4) for p in parts.values()))
    return {**parts, "ok": all(p["ok"] for p in parts.values()), "bad_cus": place_dicts(bad),
            "bad_cells": parts["contend"]["bad_cells"]}
