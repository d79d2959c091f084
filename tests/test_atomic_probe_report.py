"""CPU tests for the atomic probe: the host mirrors of ops.atomic_burn against
an independently written scalar step per section, the exactness proof of the
float sections, the order independence of the contended reduce section shown
in native-width arithmetic, the derived cmpswap cap, the summarisers on
synthetic records and buffers, and the wiring through the agent, the CLI and
the inspect view with stubbed ops. Needs no GPU."""
import struct

import numpy as np
import pytest

from hivedscheduler_amd import ops
from hivedscheduler_amd.ops import (ATOMIC_CELLS, ATOMIC_SECTIONS, ATOMIC_STEP_OPS,
                                    CONTEND_SECTIONS, REDUCE_OPS, atomic_burn_checksum,
                                    atomic_burn_expected, atomic_burn_outcomes, atomic_cas_cap,
                                    atomic_cas_expected, atomic_fp_exact,
                                    atomic_reduce_contributions, atomic_reduce_expected,
                                    contend_lanes_on_cell, summarize_atomic_burn,
                                    summarize_atomic_contend)
from hivedscheduler_amd.ops import atomic_probe

M32, M64 = 0xFFFFFFFF, (1 << 64) - 1
SEED = 5


# --------------------------------------------------------------------------
# an independent model: one lane at a time, on Python ints
# --------------------------------------------------------------------------
def fmix32(h):
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & M32
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & M32
    return h ^ (h >> 16)


def mix64(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def seed_state(seed, section, cell, lane):
    sid = ATOMIC_SECTIONS.index(section)
    lo = fmix32((seed + sid * 0x9E3779B9 + (cell * 64 + lane) * 0x85EBCA6B) & M32)
    return (fmix32(lo ^ 0xC2B2AE35) << 32) | lo


def signed(x, bits):
    return x - (1 << bits) if x >> (bits - 1) else x


def operand(m, c, i, bits):
    k = (c * 0x9E3779B1 + i * 0x85EBCA6B) & M32
    return fmix32(m ^ k) if bits == 32 else mix64(m ^ k)


def model_int_lane(section, seed, lane, chain, bits, seen=None):
    """The four integer cells of one lane after `chain` steps; every atomic is
    applied to a `memory` of its own, the way the instruction set describes it,
    and the returned old value is checked against the running mirror."""
    mask = (1 << bits) - 1
    memory = [seed_state(seed, section, j, lane) & mask for j in range(4)]

    def rmw(j, fn, x):
        old = memory[j]
        memory[j] = fn(old, x) & mask
        return old

    def cmpswap(j, compare, new):
        old = memory[j]
        if old == compare:
            memory[j] = new
        return old

    table = [
        (0, lambda o, x: o + x), (0, lambda o, x: o - x), (0, lambda o, x: o ^ x),
        (1, lambda o, x: o if signed(o, bits) <= signed(x, bits) else x),
        (1, lambda o, x: o if signed(o, bits) >= signed(x, bits) else x),
        (1, min), (1, max),
        (2, lambda o, x: o & x), (2, lambda o, x: o | x), (2, lambda o, x: x),
        (3, lambda o, x: 0 if o >= x else o + 1),
        (3, lambda o, x: x if (o == 0 or o > x) else o - 1),
    ]
    for c in range(chain):
        for k, (j, fn) in enumerate(table):
            for form in (0, 1):
                x = operand(memory[j], c, 2 * k + form, bits)
                old = rmw(j, fn, x)
                if seen is not None and k == 10:
                    seen.add(("inc", "wrap" if old >= x else "step"))
                if seen is not None and k == 11:
                    seen.add(("dec", "wrap" if (old == 0 or old > x) else "step"))
        for i in (24, 25):  # compare with what is there: swaps
            before = memory[3]
            x = operand(before, c, i, bits)
            assert cmpswap(3, before, x) == before and memory[3] == x
        for i in (26, 27):  # compare with something else: leaves it
            before = memory[3]
            x = operand(before, c, i, bits)
            assert cmpswap(3, before ^ (x | 1), x) == before and memory[3] == before
    return memory


def f32_bits(v):
    return struct.unpack("<I", struct.pack("<f", float(v)))[0]


def f64_bits(v):
    return struct.unpack("<Q", struct.pack("<d", float(v)))[0]


def f16_bits(v):
    return struct.unpack("<H", struct.pack("<e", float(v)))[0]


def bf16_bits(v):
    return f32_bits(v) >> 16


def model_fp_lane(section, seed, lane, chain, first_cell):
    """The five float cells of one lane as raw bits after `chain` steps."""
    s = [seed_state(seed, section, first_cell + j, lane) for j in range(5)]
    f = (s[0] & 0xFFFFF) - 0x80000
    d = (s[1] & ((1 << 50) - 1)) - (1 << 49)
    mm = (s[2] & ((1 << 50) - 1)) - (1 << 49)
    h = [(s[3] & 511) - 256, ((s[3] >> 16) & 511) - 256]
    b = [(s[4] & 63) - 32, ((s[4] >> 16) & 63) - 32]
    for c in range(chain):
        for form in (0, 1):
            f += operand(f & M32, c, form, 32) % 2047 - 1023
        for form in (0, 1):
            d += (operand(d & M64, c, 2 + form, 64) & ((1 << 41) - 1)) - (1 << 40)
        for form in range(4):
            x = (operand(mm & M64, c, 4 + form, 64) & ((1 << 52) - 1)) - (1 << 51)
            mm = min(mm, x) if form < 2 else max(mm, x)
        for form in (0, 1):
            x = operand(f16_bits(h[0]) | (f16_bits(h[1]) << 16), c, 8 + form, 32)
            h = [h[0] + (x & 0xFFFF) % 31 - 15, h[1] + (x >> 16) % 31 - 15]
        for form in (0, 1):
            x = operand(bf16_bits(b[0]) | (bf16_bits(b[1]) << 16), c, 10 + form, 32)
            b = [b[0] + (x & 0xFFFF) % 7 - 3, b[1] + (x >> 16) % 7 - 3]
    return [f32_bits(f), f64_bits(d), f64_bits(mm), f16_bits(h[0]) | (f16_bits(h[1]) << 16),
            bf16_bits(b[0]) | (bf16_bits(b[1]) << 16)]


def model_lane(section, seed, lane, chain):
    if section == "g32":
        return model_int_lane(section, seed, lane, chain, 32)
    if section == "g64":
        return model_int_lane(section, seed, lane, chain, 64)
    if section == "gfp":
        return model_fp_lane(section, seed, lane, chain, 0)
    wide = seed_state(seed, section, 4, lane)
    for c in range(chain):
        for form in (0, 1):
            wide = (wide + operand(wide, c, form, 64)) & M64
        for form in (2, 3):
            wide ^= operand(wide, c, form, 64)
    return (model_int_lane(section, seed, lane, chain, 32) + [wide]
            + model_fp_lane(section, seed, lane, chain, 5))


# --------------------------------------------------------------------------
# constants and the burn's mirror
# --------------------------------------------------------------------------
def test_constants():
    assert ATOMIC_SECTIONS == ("g32", "g64", "gfp", "lds")
    assert ATOMIC_CELLS == {"g32": 4, "g64": 4, "gfp": 5, "lds": 10}
    # two forms of 14 integer, 2 wide and 6 float operations
    assert ATOMIC_STEP_OPS == {"g32": 28, "g64": 28, "gfp": 12, "lds": 28 + 4 + 12}
    assert len(ops.ATOMIC_INT_OPS) == 14 and len(ops.ATOMIC_FP_OPS) == 6
    assert CONTEND_SECTIONS == ("ticket", "reduce", "cas")
    assert len(REDUCE_OPS) == 13 and ops.CONTEND_CELL_BYTES == 4096
    assert ops.ATOMIC_LDS_MAX_CHAIN * 256 * 2 == 32 * 1024  # the owner table, u16
    assert set(atomic_probe._ATOMIC_DEFAULT_CHAIN) == set(ATOMIC_SECTIONS)
    assert atomic_probe._ATOMIC_DEFAULT_CHAIN["lds"] <= ops.ATOMIC_LDS_MAX_CHAIN
    assert atomic_probe._ATOMIC_DEFAULT_ROUNDS % 2 == 1
    assert set(atomic_probe._CONTEND_DEFAULT_SHAPE) == set(CONTEND_SECTIONS)


@pytest.mark.parametrize("section", ATOMIC_SECTIONS)
def test_expected_matches_the_independent_model(section):
    for chain in (1, 3):
        want = atomic_burn_expected(section, SEED, chain)
        assert want.dtype == np.uint64 and want.shape == (ATOMIC_CELLS[section] * 64,)
        for lane in (0, 1, 17, 63):
            model = model_lane(section, SEED, lane, chain)
            got = [int(want[j * 64 + lane]) for j in range(ATOMIC_CELLS[section])]
            assert got == model, (chain, lane)
    with pytest.raises(ValueError):
        atomic_burn_expected("g16", SEED, 1)


@pytest.mark.parametrize("section", ("g32", "g64", "lds"))
def test_both_arms_of_inc_dec_and_cmpswap_occur_within_the_default_chain(section):
    chain = atomic_probe._ATOMIC_DEFAULT_CHAIN[section]
    want = {("inc", "wrap"), ("inc", "step"), ("dec", "wrap"), ("dec", "step"),
            ("cmpswap", "ok"), ("cmpswap", "fail")}
    assert atomic_burn_outcomes(section, 1, chain) == want
    # and by the independent model, over the lanes of a wave
    seen = set()
    bits = 64 if section == "g64" else 32
    for lane in range(64):
        model_int_lane(section, 1, lane, chain, bits, seen)
    assert seen == want - {("cmpswap", "ok"), ("cmpswap", "fail")}


@pytest.mark.parametrize("section", ATOMIC_SECTIONS)
def test_compare_is_live_and_the_checksum_cancels_over_even_rounds(section):
    three, four = atomic_burn_expected(section, SEED, 3), atomic_burn_expected(section, SEED, 4)
    cells = ATOMIC_CELLS[section]
    # every lane differs in at least one cell
    assert (three.reshape(cells, 64) != four.reshape(cells, 64)).any(axis=0).all()
    assert (atomic_burn_expected(section, SEED + 1, 3) != three).any()
    assert atomic_burn_checksum(section, SEED, 3, 2) == 0
    odd = atomic_burn_checksum(section, SEED, 3, 3)
    assert odd != 0 and odd == atomic_burn_checksum(section, SEED, 3, 1)
    assert odd != atomic_burn_checksum(section, SEED, 4, 3)


def test_fp_exact_proves_the_bound():
    for section in ("gfp", "lds"):
        assert atomic_fp_exact(1, atomic_probe._ATOMIC_DEFAULT_CHAIN[section]) is True
    assert atomic_fp_exact(SEED, 3) is True
    # a bf16 half walks +-3 twice a step from within +-32: far out of +-256 by then
    assert atomic_fp_exact(1, 100000) is False
    # the mirror checks the values themselves: an out-of-range start is caught
    cells = atomic_probe._FpCells("gfp", 1, 0)
    assert cells.exact is True
    cells.b[0][7] = 257
    cells._check()
    assert cells.exact is False
    cells = atomic_probe._FpCells("gfp", 1, 0)
    cells.f[0] = 1 << 24
    cells.step(0)
    assert cells.exact is False


def test_report_refuses_an_inexact_chain(monkeypatch):
    class Ops:
        def device_info(self, device):
            return {"multiProcessorCount": 4}

        def atomic_burn(self, *args):
            raise AssertionError("must not launch")

    monkeypatch.setattr(ops, "_ops_on", lambda device: Ops())
    monkeypatch.setattr(atomic_probe, "atomic_fp_exact", lambda seed, chain: False)
    with pytest.raises(ValueError, match="exact"):
        ops.atomic_burn_report(0, sections=("gfp",), chain=3)


# --------------------------------------------------------------------------
# contended sections: mirrors
# --------------------------------------------------------------------------
LANES, PER_LANE, CELLS = 1024, 4, 3


def fold_native(op, values, init):
    """Apply contributions one after the other in the cell's own arithmetic."""
    if op in ("add_f32",):
        acc = np.float32(init)
        for v in values:
            acc = np.float32(acc + np.float32(v))
        return int(np.float32(acc).view(np.uint32))
    if op == "add_f64":
        acc = np.float64(init)
        for v in values:
            acc = acc + np.float64(v)
        return int(np.float64(acc).view(np.uint64))
    if op in ("pk_add_bf16", "pk_add_f16"):
        halves = []
        for k in (0, 1):
            acc = np.float32(0)
            for v in values[:, k]:
                total = np.float32(acc + np.float32(v))
                if op == "pk_add_f16":
                    acc = np.float32(np.float16(total))
                else:  # round to nearest even on the upper 16 bits
                    bits = int(total.view(np.uint32))
                    bits = (bits + 0x7FFF + ((bits >> 16) & 1)) & 0xFFFF0000
                    acc = np.uint32(bits).view(np.float32)
            halves.append(f16_bits(acc) if op == "pk_add_f16" else bf16_bits(acc))
        return halves[0] | (halves[1] << 16)
    acc = init
    for v in (int(v) for v in values):
        if op == "add_u32":
            acc = (acc + v) & M32
        elif op == "add_u64":
            acc = (acc + v) & M64
        elif op == "xor":
            acc ^= v
        elif op == "or":
            acc |= v
        elif op == "and":
            acc &= v
        elif op == "umin":
            acc = min(acc, v)
        elif op == "umax":
            acc = max(acc, v)
        elif op == "smin":
            acc = min(signed(acc, 32), signed(v, 32)) & M32
        elif op == "smax":
            acc = max(signed(acc, 32), signed(v, 32)) & M32
    return acc


def test_reduce_expected_is_invariant_under_the_arrival_order():
    con = atomic_reduce_contributions(SEED, LANES, PER_LANE, CELLS)
    want = atomic_reduce_expected(SEED, LANES, PER_LANE, CELLS)
    assert set(want) == set(REDUCE_OPS)
    init = {"and": M32, "umin": M32, "smin": 0x7FFFFFFF, "smax": 0x80000000}
    rng = np.random.default_rng(7)
    orders = [np.arange(LANES * PER_LANE), np.arange(LANES * PER_LANE)[::-1]]
    orders += [rng.permutation(LANES * PER_LANE) for _ in range(3)]
    for order in orders:
        cell = con["cell"][order]
        for op in REDUCE_OPS:
            values = con[op][order]
            for c in range(CELLS):
                got = fold_native(op, values[cell == c], init.get(op, 0))
                assert got == int(want[op][c]), (op, c)
    # the identity contributions really are most of the packed and or/and ones
    assert (con["pk_add_bf16"] != 0).any(axis=1).sum() == 128 * CELLS
    assert set(np.unique(con["pk_add_bf16"])) == {-1, 0, 1}
    assert np.abs(con["pk_add_f16"]).max() <= 16 and np.abs(con["add_f32"]).max() <= 128
    assert (con["or"] != 0).sum() == 24 * CELLS and (con["and"] != M32).sum() == 24 * CELLS
    # the seed matters
    other = atomic_reduce_expected(SEED + 1, LANES, PER_LANE, CELLS)
    assert all((other[op] != want[op]).any() for op in REDUCE_OPS)


def test_float_bounds_hold_at_the_largest_shape_a_launch_accepts():
    """2^16 contributions on a cell (the kernel's bound): |f32 sum| < 2^24."""
    assert (1 << 16) * 128 < (1 << 24)
    assert (1 << 16) * (1 << 31) < (1 << 53)
    assert 128 * 1 <= 256 and 128 * 16 <= 2048


def test_cas_cap_and_expected():
    assert list(contend_lanes_on_cell(1024, 3)) == [342, 341, 341]
    assert list(atomic_cas_cap(1024, 4, 3)) == [1368, 1364, 1364]
    assert list(atomic_cas_cap(4096, 4, 1)) == [16384]
    # every success on a cell is somebody's: the caps sum to all operations
    assert int(atomic_cas_cap(LANES, PER_LANE, CELLS).sum()) == LANES * PER_LANE
    want = atomic_cas_expected(SEED, LANES, PER_LANE, CELLS)
    for c in range(CELLS):
        total = mix64(((SEED << 32) ^ c) & M64)
        for gid in range(c, LANES, CELLS):
            total = (total + PER_LANE * mix64((SEED << 32) | gid)) & M64
        assert int(want[c]) == total


# --------------------------------------------------------------------------
# summarisers on synthetic records
# --------------------------------------------------------------------------
CUS = [(0, 0, 0, 1), (5, 2, 0, 15), (0, 3, 1, 7), (7, 7, 1, 0)]


def hw_word(xcc, se, sh, cu, simd=0):
    return (xcc << 16) | (se << 13) | (sh << 12) | (cu << 8) | (simd << 4)


def as_i32(x):
    return x - (1 << 32) if x & 0x80000000 else x


def clean_burn_records(section="g32", rounds=3, cus=CUS):
    checksum = atomic_burn_checksum(section, SEED, 3, rounds)
    rec = np.zeros((len(cus) * 4, 8), dtype=np.int32)
    for b, cu in enumerate(cus):
        for w in range(4):
            rec[4 * b + w] = (hw_word(*cu, w), 0, -1, -1, as_i32(checksum & M32),
                              as_i32(checksum >> 32), -1, 0)
    return rec


def burn_summary(rec, section="g32", expected_cus=4, **kw):
    return summarize_atomic_burn(rec, kw.get("elapsed_ms", 6.0), section, 3, 3, expected_cus)


def test_summarize_burn_clean():
    s = burn_summary(clean_burn_records(), elapsed_ms=4.5)
    assert s["waves"] == 16 and s["cus_seen"] == 4 and s["mismatched_waves"] == 0
    assert s["checksum_spread"] is False and s["bad_cus"] == [] and s["ok"] is True
    assert s["ticket_faults"] == 0 and s["elapsed_ms"] == 4.5 and s["us_per_step"] == 500.0
    assert (s["section"], s["chain"], s["rounds"]) == ("g32", 3, 3)


def test_summarize_burn_names_one_cu_and_keeps_the_earliest_round():
    rec = clean_burn_records(cus=CUS + [CUS[1]])
    rec[5, 1:4], rec[5, 6] = (4, 2, 9), 6      # CUS[1]
    rec[18, 1:4], rec[18, 6] = (8, 1, 40), 28  # CUS[1] again, an earlier round
    s = burn_summary(rec)
    assert s["mismatched_waves"] == 2 and s["ok"] is False
    assert s["bad_cus"] == [{"xcc": 5, "se": 2, "sh": 0, "cu": 15, "waves": 2,
                             "mismatched_lane_steps": 12, "ticket_faults": 0,
                             "first_bad_round": 1, "first_bad_lane": 40, "first_bad_op": 28}]


def test_summarize_burn_checksum_outlier_is_named():
    rec = clean_burn_records("g64")
    rec[13, 5] ^= 0x100
    s = burn_summary(rec, "g64")
    assert s["mismatched_waves"] == 0 and s["checksum_spread"] is True and s["ok"] is False
    assert s["bad_cus"] == [{"xcc": 7, "se": 7, "sh": 1, "cu": 0, "waves": 1,
                             "mismatched_lane_steps": 0, "ticket_faults": 0,
                             "first_bad_round": -1, "first_bad_lane": -1, "first_bad_op": -1}]


def test_summarize_burn_ticket_fault_and_short_coverage_are_not_ok():
    rec = clean_burn_records("lds")
    rec[8:12, 7] = 2  # the four waves of one workgroup report its ticket
    s = burn_summary(rec, "lds")
    assert s["ticket_faults"] == 8 and s["ok"] is False
    assert [(c["xcc"], c["cu"], c["ticket_faults"]) for c in s["bad_cus"]] == [(0, 7, 8)]
    s = burn_summary(clean_burn_records(), expected_cus=5)
    assert s["cus_seen"] == 4 and s["mismatched_waves"] == 0 and s["ok"] is False


BLOCKS = 4  # 1024 lanes, 16 waves


def contend_records(xccs=(0, 1, 2, 3)):
    rec = np.zeros((BLOCKS * 4, 8), dtype=np.int32)
    for w in range(BLOCKS * 4):
        rec[w, 0] = hw_word(xccs[w % len(xccs)], w % 3, 0, w % 5, w % 4)
    return rec


def clean_contend(section):
    shared = np.zeros((CELLS, 512), dtype=np.int64)
    owner = np.zeros((CELLS, 0), dtype=np.int32)
    if section == "ticket":
        draws = contend_lanes_on_cell(LANES, CELLS) * PER_LANE
        owner = np.zeros((CELLS, int(draws.max())), dtype=np.int32)
        for c in range(CELLS):
            shared[c, 0] = draws[c]
            owner[c, :draws[c]] = 1 + np.arange(draws[c])
    elif section == "reduce":
        for k, op in enumerate(REDUCE_OPS):
            shared[:, 16 * k] = atomic_reduce_expected(SEED, LANES, PER_LANE, CELLS)[op].view(
                np.int64)
    else:
        shared[:, 0] = atomic_cas_expected(SEED, LANES, PER_LANE, CELLS).view(np.int64)
    return shared, owner, contend_records()


def contend_summary(section, shared, owner, rec, expected_xccs=4, ms=2.0):
    return summarize_atomic_contend(section, shared, owner, rec, ms, SEED, BLOCKS, PER_LANE, CELLS,
                                    expected_xccs)


@pytest.mark.parametrize("section", CONTEND_SECTIONS)
def test_summarize_contend_clean_and_short_xcd_coverage(section):
    s = contend_summary(section, *clean_contend(section))
    assert s["ok"] is True and s["bad_cells"] == [] and s["bad_cus"] == []
    assert s["xccs_seen"] == 4 and s["operations"] == LANES * PER_LANE
    if section == "ticket":
        assert s["lost"] == 0 and s["out_of_range"] == 0 and s["counter_error"] == [0, 0, 0]
        assert s["tickets_per_us"] == pytest.approx(4096 / 2000.0)
    if section == "cas":
        assert s["gave_up"] == 0 and s["retries"] == 0
    s = contend_summary(section, *clean_contend(section), expected_xccs=8)
    assert s["bad_cells"] == [] and s["ok"] is False
    with pytest.raises(ValueError):
        contend_summary("queue", *clean_contend(section))


def test_summarize_ticket_hole_out_of_range_and_wrong_counter():
    shared, owner, rec = clean_contend("ticket")
    owner[1, 77] = 0
    owner[1, 900] = 0
    s = contend_summary("ticket", shared, owner, rec)
    assert s["ok"] is False and s["lost"] == 2
    assert s["bad_cells"] == [{"cell": 1, "byte_offset": 4096, "section": "ticket", "op": "owner",
                               "got": 2, "want": 0, "first_hole": 77}]
    shared, owner, rec = clean_contend("ticket")
    shared[2, 0] += 1
    rec[6, 2] = 1  # the wave that drew the ticket past the end
    s = contend_summary("ticket", shared, owner, rec)
    assert s["ok"] is False and s["out_of_range"] == 1 and s["counter_error"] == [0, 0, 1]
    assert s["bad_cells"] == [
        {"cell": 2, "byte_offset": 8192, "section": "ticket", "op": "counter", "got": 1365,
         "want": 1364},
        {"cell": -1, "byte_offset": -1, "section": "ticket", "op": "out_of_range", "got": 1,
         "want": 0}]
    assert [(c["xcc"], c["out_of_range"]) for c in s["bad_cus"]] == [(2, 1)]
    # a lane whose own tickets did not increase names its CU
    shared, owner, rec = clean_contend("ticket")
    rec[9, 1] = 3
    s = contend_summary("ticket", shared, owner, rec)
    assert s["ok"] is False and s["bad_cells"] == []
    assert s["bad_cus"] == [{"xcc": 1, "se": 0, "sh": 0, "cu": 4, "waves": 1,
                             "not_increasing": 3, "out_of_range": 0, "gave_up": 0}]


def test_summarize_reduce_and_cas_faults():
    shared, owner, rec = clean_contend("reduce")
    k = REDUCE_OPS.index("add_f32")
    want = int(shared[2, 16 * k])
    shared[2, 16 * k] ^= 1 << 13
    s = contend_summary("reduce", shared, owner, rec)
    assert s["ok"] is False
    assert s["bad_cells"] == [{"cell": 2, "byte_offset": 8192, "section": "reduce",
                               "op": "add_f32", "got": want ^ (1 << 13), "want": want}]
    assert s["values"]["add_f32"]["want"][2] == want
    shared, owner, rec = clean_contend("cas")
    rec[3, 3:5] = (2, 2728)
    s = contend_summary("cas", shared, owner, rec)
    assert s["ok"] is False and s["gave_up"] == 2 and s["bad_cells"] == []
    assert [c["gave_up"] for c in s["bad_cus"]] == [2]
    shared, owner, rec = clean_contend("cas")
    rec[:, 4] = 100  # retries are reported and not judged
    shared[0, 0] += 1
    s = contend_summary("cas", shared, owner, rec)
    assert s["retries"] == 1600 and s["retries_per_success"] == pytest.approx(1600 / 4096)
    assert [(c["cell"], c["op"]) for c in s["bad_cells"]] == [(0, "cmpswap_add")]
    assert s["ok"] is False


# --------------------------------------------------------------------------
# wiring: agent, CLI, inspect view
# --------------------------------------------------------------------------
BAD_CU = {"xcc": 5, "se": 2, "sh": 0, "cu": 15}
BAD_CELL = {"cell": 2, "byte_offset": 8192, "section": "reduce", "op": "add_f32", "got": 1,
            "want": 2}


def canned_report(bad_cus=(), bad_cells=(), burn_ok=None, contend_ok=None):
    burn_ok = (not bad_cus) if burn_ok is None else burn_ok
    contend_ok = (not bad_cells) if contend_ok is None else contend_ok
    ok = bool(burn_ok and contend_ok)
    return {
        "hbm_gbps": 5000.0, "mfma_ok": True, "cu_coverage": 256, "lds_errors": 0,
        "healthy": ok,
        "atomic_probe": {
            "burn": {"ok": burn_ok, "bad_cus": list(bad_cus), "sections": {}},
            "contend": {"ok": contend_ok, "bad_cus": [], "bad_cells": list(bad_cells),
                        "sections": {}},
            "ok": ok,
            "bad_cus": list(bad_cus),
            "bad_cells": list(bad_cells),
        },
    }


@pytest.fixture()
def agent_health(monkeypatch):
    """collect_node_health over one fake GPU: returns the agent module and a
    dict holding the canned `report` to serve and the `calls` it received."""
    from hivedscheduler_amd.agent import health

    state = {"report": None, "calls": []}

    def fake_report(device=0, **kwargs):
        state["calls"].append(kwargs)
        rep = dict(state["report"])
        if not kwargs.get("atomic_probe"):
            rep.pop("atomic_probe")
            rep["healthy"] = True
        return rep

    monkeypatch.setattr(ops, "gpu_health_report", fake_report)
    monkeypatch.setattr(health, "_rocm_smi_gpu_state", lambda: {0: True})
    return health, state


def test_agent_probe_verdicts(agent_health):
    health, state = agent_health
    state["report"] = canned_report()
    g = health.collect_node_health(deep=True, atomic_probe=True)["gpus"]["0"]
    assert g["healthy"] is True and g["atomic_probe_ok"] is True
    assert g["atomic_burn_ok"] is True and g["atomic_contend_ok"] is True
    assert g["atomic_bad_cus"] == [] and g["atomic_bad_cells"] == []
    assert state["calls"][-1]["atomic_probe"] is True
    assert "scalar_probe" not in state["calls"][-1] and "burn" not in state["calls"][-1]
    assert "bad_cus" not in g and "lds_bad_cus" not in g and "bad_simds" not in g
    # a named CU fails the GPU and is reported with the four keys only
    state["report"] = canned_report(bad_cus=[dict(BAD_CU, waves=1)])
    g = health.collect_node_health(deep=True, atomic_probe=True)["gpus"]["0"]
    assert g["healthy"] is False and g["atomic_probe_ok"] is False
    assert g["atomic_burn_ok"] is False and g["atomic_contend_ok"] is True
    assert g["atomic_bad_cus"] == [BAD_CU] and g["atomic_bad_cells"] == []
    # a bad cell too, with cell, section and op
    state["report"] = canned_report(bad_cells=[dict(BAD_CELL)])
    g = health.collect_node_health(deep=True, atomic_probe=True)["gpus"]["0"]
    assert g["healthy"] is False and g["atomic_contend_ok"] is False
    assert g["atomic_bad_cells"] == [{"cell": 2, "section": "reduce", "op": "add_f32"}]
    # a part that failed without naming anything (coverage, checksum)
    for part in ("burn", "contend"):
        state["report"] = canned_report(**{f"{part}_ok": False})
        g = health.collect_node_health(deep=True, atomic_probe=True)["gpus"]["0"]
        assert g["healthy"] is False and g["atomic_probe_ok"] is False
        assert g["atomic_burn_ok"] is (part != "burn")
        assert g["atomic_contend_ok"] is (part != "contend")


def test_agent_without_probe_is_unchanged(agent_health):
    health, state = agent_health
    state["report"] = canned_report(bad_cus=[dict(BAD_CU)])
    g = health.collect_node_health(deep=True)["gpus"]["0"]
    assert g == {"healthy": True, "hbm_gbps": 5000.0, "mfma_ok": True, "cu_coverage": 256,
                 "lds_errors": 0}
    assert "atomic_probe" not in state["calls"][-1]
    n = len(state["calls"])
    g = health.collect_node_health(deep=False, atomic_probe=True)["gpus"]["0"]
    assert g == {"healthy": True} and len(state["calls"]) == n


def test_agent_probe_cadence(agent_health, monkeypatch):
    health, state = agent_health
    state["report"] = canned_report(bad_cus=[dict(BAD_CU)])
    monkeypatch.setattr(health.NodeHealthAgent, "post_report", lambda self, r: True)
    monkeypatch.setattr(health.NodeHealthAgent, "run_placement_probes", lambda self: [])
    monkeypatch.setattr(health, "p2p_link_matrix", lambda: {"matrix": {}, "links": []})
    never = health.NodeHealthAgent("http://x", node_name="n", deep_every=1, probe_pairs=False,
                                   p2p_matrix_every=10 ** 9)
    assert never.atomic_probe_every == 0
    assert all("atomic_probe_ok" not in never.run_once()["gpus"]["0"] for _ in range(3))
    assert all("atomic_probe" not in c for c in state["calls"])
    agent = health.NodeHealthAgent("http://x", node_name="n", deep_every=1, probe_pairs=False,
                                   p2p_matrix_every=10 ** 9, atomic_probe_every=2)
    got = [agent.run_once()["gpus"]["0"] for _ in range(4)]
    assert ["atomic_bad_cus" in g for g in got] == [True, False, True, False]
    assert [g["healthy"] for g in got] == [False, True, False, True]
    # only on deep sweeps: every 2nd round is a probe round, every 4th deep
    agent = health.NodeHealthAgent("http://x", node_name="n", deep_every=4, probe_pairs=False,
                                   p2p_matrix_every=10 ** 9, atomic_probe_every=2)
    got = [agent.run_once()["gpus"]["0"] for _ in range(6)]
    assert ["atomic_bad_cus" in g for g in got] == [True, False, False, False, True, False]


def test_cli_has_the_probe_flags(monkeypatch, capsys):
    import json
    import sys

    from hivedscheduler_amd.agent import __main__ as cli
    from hivedscheduler_amd.agent import health

    seen = {}

    def fake_collect(**kwargs):
        seen.update(kwargs)
        return {"gpus": {}}

    monkeypatch.setattr(health, "collect_node_health", fake_collect)
    monkeypatch.setattr(sys, "argv", ["agent", "--local", "--atomic-probe", "--no-probe-pairs"])
    cli.main()
    assert seen["atomic_probe"] is True and seen["scalar_probe"] is False
    assert json.loads(capsys.readouterr().out) == {"gpus": {}}
    monkeypatch.setattr(sys, "argv", ["agent", "--local", "--no-probe-pairs"])
    cli.main()
    assert seen["atomic_probe"] is False

    made = {}

    class FakeAgent:
        def __init__(self, url, **kwargs):
            made.update(kwargs)

        def run_once(self):
            return {}

    monkeypatch.setattr(health, "NodeHealthAgent", FakeAgent)
    monkeypatch.setattr(sys, "argv", ["agent", "--scheduler", "http://x", "--once",
                                      "--atomic-probe-every", "6"])
    cli.main()
    assert made["atomic_probe_every"] == 6 and made["scalar_probe_every"] == 0
    monkeypatch.setattr(sys, "argv", ["agent", "--scheduler", "http://x", "--once"])
    cli.main()
    assert made["atomic_probe_every"] == 0


def test_health_report_signature_has_the_option_off_by_default():
    import inspect

    sig = inspect.signature(ops.gpu_health_report)
    assert sig.parameters["atomic_probe"].default is False
    sig = inspect.signature(ops.atomic_burn_report)
    assert sig.parameters["blocks"].default == 2048 and sig.parameters["inject"].default is None
    from hivedscheduler_amd.agent import health

    assert inspect.signature(health.collect_node_health).parameters[
        "atomic_probe"].default is False


def test_probe_report_joins_the_parts(monkeypatch):
    burn = {"ok": True, "bad_cus": [dict(BAD_CU)], "sections": {}}
    contend = {"ok": False, "bad_cus": [{"xcc": 0, "se": 1, "sh": 0, "cu": 3}],
               "bad_cells": [dict(BAD_CELL)], "sections": {}}
    monkeypatch.setattr(atomic_probe, "atomic_burn_report", lambda device: burn)
    monkeypatch.setattr(atomic_probe, "atomic_contend_report", lambda device: contend)
    rep = ops.atomic_probe_report(0)
    assert rep["burn"] is burn and rep["contend"] is contend and rep["ok"] is False
    assert rep["bad_cus"] == [{"xcc": 0, "se": 1, "sh": 0, "cu": 3}, BAD_CU]
    assert rep["bad_cells"] == [BAD_CELL]


def test_atomic_keys_reach_the_inspect_view():
    from hivedscheduler_amd.scheduler import HivedScheduler
    from hivedscheduler_amd.sim import mi355x_cluster_config

    sched = HivedScheduler(mi355x_cluster_config(num_nodes=1))
    node = sched.algorithm.all_nodes()[0]
    sched.on_node_add({"metadata": {"name": node, "uid": "n1"}, "spec": {},
                       "status": {"conditions": [{"type": "Ready", "status": "True"}]}})
    bad_cells = [{"cell": 2, "section": "reduce", "op": "add_f32"}]
    report = {"gpus": {"3": {"healthy": False, "atomic_probe_ok": False, "atomic_burn_ok": False,
                             "atomic_contend_ok": False, "atomic_bad_cus": [dict(BAD_CU)],
                             "atomic_bad_cells": bad_cells}}}
    assert sched.on_health_report(node, report)["applied"] == {"3": False}
    gpu = sched.get_health_reports()[node]["gpus"]["3"]
    assert gpu["atomic_bad_cus"] == [BAD_CU] and gpu["atomic_bad_cells"] == bad_cells
    assert gpu["atomic_probe_ok"] is False and gpu["atomic_burn_ok"] is False
    assert gpu["atomic_contend_ok"] is False
