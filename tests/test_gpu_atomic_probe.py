"""GPU tests for the atomic probe: the exact atomic burn (ops.atomic_burn)
against its host mirror per section, a live compare, one injected atomic xor
per section and its per-CU attribution, the LDS ticket; the contended ticket,
reduce and cmpswap sections (ops.atomic_contend) judged on the host from the
copied-back buffers, tampered copies, argument checks, the default shapes and
the health-report wiring. Everything is bitwise: no tolerance."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

needs_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")

BLOCKS = 8  # 32 waves
WAVES = BLOCKS * 4
SEED = 5
M32 = 0xFFFFFFFF
SECTIONS = ("g32", "g64", "gfp", "lds")
NO_INJECT = (-1, -1, -1, -1)


@functools.lru_cache(maxsize=None)
def expected_on_gpu(section, chain):
    from hivedscheduler_amd.ops import atomic_burn_expected

    want = atomic_burn_expected(section, SEED, chain)
    return torch.from_numpy(want.view("int64").copy()).cuda()


@functools.lru_cache(maxsize=None)
def burn(section, chain, rounds, expected_chain=None, inject=NO_INJECT):
    """Records [32, 8] as int64 of one launch, compared against the mirror of
    `expected_chain` steps (default: `chain`); each distinct launch runs once
    and is shared."""
    from hivedscheduler_amd.ops import get_ops

    want = expected_on_gpu(section, chain if expected_chain is None else expected_chain)
    records, ms = get_ops().atomic_burn(want, section, SEED, BLOCKS, chain, rounds, *inject)
    assert records.shape == (WAVES, 8) and records.dtype == torch.int32
    assert ms > 0
    rec = records.cpu().numpy().astype(np.int64)
    rec.setflags(write=False)
    return rec


def checksums(rec):
    return [((int(r[5]) & M32) << 32) | (int(r[4]) & M32) for r in rec]


def assert_clean_burn(rec, rows=None):
    rows = range(len(rec)) if rows is None else rows
    for w in rows:
        assert tuple(rec[w, 1:4]) == (0, -1, -1), (w, rec[w])
        assert tuple(rec[w, 6:8]) == (-1, 0), (w, rec[w])


@needs_gpu
@pytest.mark.parametrize("section", SECTIONS)
def test_burn_matches_the_host_mirror(section):
    from hivedscheduler_amd.ops import atomic_burn_checksum

    for chain, rounds in ((3, 2), (3, 3), (1, 1)):
        rec = burn(section, chain, rounds)
        want = atomic_burn_checksum(section, SEED, chain, rounds)
        print(section, chain, rounds, "checksum", hex(checksums(rec)[0]), "mirror", hex(want))
        assert_clean_burn(rec)
        assert checksums(rec) == [want] * WAVES, (chain, rounds, hex(want))
    assert atomic_burn_checksum(section, SEED, 3, 3) != 0
    assert atomic_burn_checksum(section, SEED, 3, 2) == 0


@needs_gpu
@pytest.mark.parametrize("section", SECTIONS)
def test_burn_compare_is_live(section):
    """Three steps judged against the mirror of four: every returned value is
    right and every lane's final cells are wrong, in every round on every
    wave."""
    from hivedscheduler_amd.ops import ATOMIC_STEP_OPS

    rounds = 2
    rec = burn(section, 3, rounds, expected_chain=4)
    assert (rec[:, 1] == 64 * rounds).all(), rec[:, 1]
    assert (rec[:, 2] == 0).all() and (rec[:, 3] == 0).all()
    assert (rec[:, 6] == ATOMIC_STEP_OPS[section]).all(), rec[:, 6]


@needs_gpu
@pytest.mark.parametrize("section,lane,bit", [("g32", 6, 9), ("g64", 3, 40), ("gfp", 17, 22),
                                              ("lds", 33, 0)])
def test_burn_injection_names_one_cu(section, lane, bit):
    """One extra atomic xor on the lane's first cell before round 1: its
    operations are bijective in the cell (add, sub, xor; for gfp exact adds
    onto a value off by a power of two), so the first returned value of each
    of the three steps and the final compare see it: four lane-steps."""
    from hivedscheduler_amd.ops import (atomic_burn_checksum, decode_hw_word,
                                        summarize_atomic_burn)

    wave, rnd, chain, rounds = 5, 1, 3, 3  # odd rounds: the checksum does not cancel
    rec = burn(section, chain, rounds, inject=(wave, rnd, lane, bit))
    assert tuple(rec[wave, 1:4]) == (chain + 1, rnd, lane), rec[wave]
    assert rec[wave, 6] == 0 and rec[wave, 7] == 0
    assert_clean_burn(rec, [w for w in range(WAVES) if w != wave])
    want = atomic_burn_checksum(section, SEED, chain, rounds)
    got = checksums(rec)
    assert got[wave] != want
    assert all(got[w] == want for w in range(WAVES) if w != wave)
    s = summarize_atomic_burn(rec, 1.0, section, chain, rounds, expected_cus=1)
    assert s["ok"] is False and s["mismatched_waves"] == 1 and s["checksum_spread"] is True
    xcc, se, sh, cu = decode_hw_word(rec[wave, 0])
    assert s["bad_cus"] == [{"xcc": xcc, "se": se, "sh": sh, "cu": cu, "waves": 1,
                             "mismatched_lane_steps": chain + 1, "ticket_faults": 0,
                             "first_bad_round": rnd, "first_bad_lane": lane,
                             "first_bad_op": 0}]


@needs_gpu
def test_lds_ticket():
    """Chain 2: 256 lanes draw two tickets each from one LDS word. Field [7]
    counts unmarked owner entries, out-of-range tickets and a word that is not
    256 * chain = 512: zero says all three."""
    rec = burn("lds", 2, 1)
    assert_clean_burn(rec)
    assert (rec[:, 7] == 0).all()


# --------------------------------------------------------------------------
# contended sections
# --------------------------------------------------------------------------
SHAPES = [(16, 4, 2), (16, 4, 1), (1, 4, 2)]  # (blocks, per_lane, cells)


@functools.lru_cache(maxsize=None)
def contend(section, blocks, per_lane, cells):
    """The copied-back buffers of one launch: (shared, owner, records, ms)."""
    from hivedscheduler_amd.ops import get_ops

    out = get_ops().atomic_contend(section, SEED, blocks, per_lane, cells)
    assert out["shared"].shape == (cells, 512) and out["shared"].dtype == torch.int64
    assert out["records"].shape == (blocks * 4, 8) and out["ms"] > 0
    arrays = tuple(out[k].cpu().numpy() for k in ("shared", "owner", "records"))
    for a in arrays:
        a.setflags(write=False)
    return arrays + (out["ms"],)


def judge(section, blocks, per_lane, cells, buffers=None, expected_xccs=None):
    from hivedscheduler_amd.ops import summarize_atomic_contend

    shared, owner, records, ms = contend(section, blocks, per_lane, cells)
    if buffers is not None:
        shared, owner = buffers
    if expected_xccs is None:
        expected_xccs = 2 if blocks >= 16 else 1
    return summarize_atomic_contend(section, shared, owner, records, ms, SEED, blocks, per_lane,
                                    cells, expected_xccs)


@needs_gpu
@pytest.mark.parametrize("blocks,per_lane,cells", SHAPES)
def test_ticket_returns_every_value_once(blocks, per_lane, cells):
    s = judge("ticket", blocks, per_lane, cells)
    print("ticket", (blocks, per_lane, cells), "xccs_seen", s["xccs_seen"], "ms", s["elapsed_ms"],
          "tickets_per_us", round(s["tickets_per_us"], 1))
    assert s["lost"] == 0 and s["out_of_range"] == 0 and s["counter_error"] == [0] * cells
    assert s["bad_cells"] == [] and s["bad_cus"] == [] and s["ok"] is True
    shared, owner, _, _ = contend("ticket", blocks, per_lane, cells)
    draws = blocks * 256 * per_lane // cells
    assert owner.shape == (cells, draws)
    for c in range(cells):
        assert int(shared[c, 0]) == draws
        # every ticket has an owner, a lane of this cell, each per_lane times
        lanes, counts = np.unique(owner[c] - 1, return_counts=True)
        assert (lanes % cells == c).all() and (counts == per_lane).all()
        assert len(lanes) == blocks * 256 // cells
    if blocks >= 16:
        assert s["xccs_seen"] >= 2  # the contention crossed an XCD boundary


@needs_gpu
@pytest.mark.parametrize("blocks,per_lane,cells", SHAPES)
def test_reduce_equals_the_mirror(blocks, per_lane, cells):
    from hivedscheduler_amd.ops import REDUCE_OPS

    s = judge("reduce", blocks, per_lane, cells)
    print("reduce", (blocks, per_lane, cells), "xccs_seen", s["xccs_seen"], "ms", s["elapsed_ms"])
    for op in REDUCE_OPS:
        assert s["values"][op]["got"] == s["values"][op]["want"], op
    assert s["bad_cells"] == [] and s["ok"] is True
    if blocks >= 16:
        assert s["xccs_seen"] >= 2


@needs_gpu
@pytest.mark.parametrize("blocks,per_lane,cells", SHAPES)
def test_cas_is_exact_and_nobody_gives_up(blocks, per_lane, cells):
    s = judge("cas", blocks, per_lane, cells)
    print("cas", (blocks, per_lane, cells), "xccs_seen", s["xccs_seen"], "ms", s["elapsed_ms"],
          "retries_per_success", round(s["retries_per_success"], 2))
    assert s["gave_up"] == 0 and s["bad_cells"] == [] and s["bad_cus"] == [] and s["ok"] is True
    if blocks >= 16:
        assert s["xccs_seen"] >= 2


@needs_gpu
def test_summariser_catches_a_tampered_copy():
    """The copied-back arrays are changed on the host; the GPU is not asked to
    misbehave."""
    from hivedscheduler_amd.ops import REDUCE_OPS

    blocks, per_lane, cells = SHAPES[0]
    shared, owner, _, _ = contend("ticket", blocks, per_lane, cells)
    owner = owner.copy()
    owner[1, 4321] = 0
    s = judge("ticket", blocks, per_lane, cells, (shared, owner))
    assert s["ok"] is False and s["lost"] == 1
    assert s["bad_cells"] == [{"cell": 1, "byte_offset": 4096, "section": "ticket",
                               "op": "owner", "got": 1, "want": 0, "first_hole": 4321}]
    shared, owner, _, _ = contend("reduce", blocks, per_lane, cells)
    shared = shared.copy()
    k = REDUCE_OPS.index("pk_add_bf16")
    want = int(shared[0, 16 * k])
    shared[0, 16 * k] ^= 0x80
    s = judge("reduce", blocks, per_lane, cells, (shared, owner))
    assert s["ok"] is False
    assert s["bad_cells"] == [{"cell": 0, "byte_offset": 0, "section": "reduce",
                               "op": "pk_add_bf16", "got": want ^ 0x80, "want": want}]
    # what went in is fine
    assert judge("reduce", blocks, per_lane, cells)["ok"] is True
    # and short XCD coverage alone is not ok
    assert judge("reduce", blocks, per_lane, cells, expected_xccs=64)["ok"] is False


# --------------------------------------------------------------------------
# argument checks, default shapes, wiring
# --------------------------------------------------------------------------
@needs_gpu
def test_burn_argument_checks():
    from hivedscheduler_amd.ops import get_ops

    ops = get_ops()
    want = expected_on_gpu("g32", 3)

    def bad(*args, expected=want, section="g32"):
        with pytest.raises(RuntimeError):
            ops.atomic_burn(expected, section, SEED, *args)

    bad(BLOCKS, 3, 2, *NO_INJECT, section="g16")
    bad(0, 3, 2, *NO_INJECT)
    bad((1 << 14) + 1, 3, 2, *NO_INJECT)
    bad(BLOCKS, 0, 2, *NO_INJECT)
    bad(BLOCKS, 3, 0, *NO_INJECT)
    bad(BLOCKS, 65, 64, *NO_INJECT)           # chain * rounds > 2^12
    bad(BLOCKS, (1 << 12) + 1, 1, *NO_INJECT)
    bad(1 << 14, 3, 128, *NO_INJECT)          # blocks * chain * rounds > 2^22
    bad(BLOCKS, 3, 2, WAVES, 0, 0, 0)         # wave out of range
    bad(BLOCKS, 3, 2, 5, 2, 0, 0)             # round out of range
    bad(BLOCKS, 3, 2, 5, 1, 64, 0)            # lane out of range
    bad(BLOCKS, 3, 2, 5, 1, 0, 32)            # bit out of range for u32 cells
    bad(BLOCKS, 3, 2, 5, -1, 0, 0)            # an injection without a round
    bad(BLOCKS, 3, 2, *NO_INJECT, expected=want.cpu())
    bad(BLOCKS, 3, 2, *NO_INJECT, expected=want.to(torch.int32))
    bad(BLOCKS, 3, 2, *NO_INJECT, expected=want[:-1])
    bad(BLOCKS, 3, 2, *NO_INJECT, expected=want, section="gfp")  # 5 cells, not 4
    bad(BLOCKS, 65, 1, *NO_INJECT, expected=expected_on_gpu("lds", 3), section="lds")


@needs_gpu
def test_contend_argument_checks():
    from hivedscheduler_amd.ops import get_ops

    ops = get_ops()

    def bad(section, blocks, per_lane, cells):
        with pytest.raises(RuntimeError):
            ops.atomic_contend(section, SEED, blocks, per_lane, cells)

    bad("queue", 16, 4, 2)
    bad("ticket", 0, 4, 2)
    bad("ticket", (1 << 13) + 1, 1, 4096)
    bad("ticket", 16, 0, 2)
    bad("ticket", 16, 65, 2)
    bad("ticket", 16, 4, 0)
    bad("ticket", 16, 4, 4097)
    bad("ticket", 1, 4, 257)           # more cells than lanes
    bad("reduce", 1024, 1, 1)          # 2^18 operations on one cell
    bad("cas", 16, 8, 1)               # 2^15 cmpswap adds on one cell
    bad("ticket", 1 << 13, 8, 4096)    # 2^24 operations
    bad("cas", 1 << 13, 2, 4096)       # 2^22 cmpswap adds


@needs_gpu
def test_default_shapes_cover_the_device():
    from hivedscheduler_amd.ops import atomic_probe_report, get_ops

    rep = atomic_probe_report(0)
    cus = get_ops().device_info(0)["multiProcessorCount"]
    for name, s in rep["burn"]["sections"].items():
        print("burn", name, "chain", s["chain"], "rounds", s["rounds"], "ms",
              round(s["elapsed_ms"], 2), "us/step", round(s["us_per_step"], 2))
        assert s["ok"] is True and s["cus_seen"] == cus, (name, s)
    for name, s in rep["contend"]["sections"].items():
        print("contend", name, {k: v for k, v in s.items()
                                if k not in ("bad_cells", "bad_cus")})
        assert s["ok"] is True and s["cus_seen"] == cus, (name, s)
        assert s["xccs_seen"] == rep["contend"]["expected_xccs"]
    assert rep["contend"]["expected_xccs"] >= 1
    assert rep["contend"]["blocks"] == 8 * cus
    assert rep["ok"] is True and rep["bad_cus"] == [] and rep["bad_cells"] == []


@needs_gpu
def test_health_report_carries_the_probe_only_when_asked(monkeypatch):
    from hivedscheduler_amd import ops

    calls = []
    real = ops.atomic_probe_report

    def counting(device):
        calls.append(device)
        return real(device)

    monkeypatch.setattr(ops, "atomic_probe_report", counting)
    off = ops.gpu_health_report(0)
    assert "atomic_probe" not in off and calls == []
    on = ops.gpu_health_report(0, atomic_probe=True)
    assert calls == [0] and set(on) - set(off) == {"atomic_probe"}
    assert on["atomic_probe"]["ok"] is True and on["healthy"] is True
