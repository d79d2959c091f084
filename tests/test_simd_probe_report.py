"""SIMD probe, host side (no GPU): the VALU burn's mirrors against steps
written out independently on Python ints and fractions, the register march's
pattern and read sum, record summarising and per-SIMD attribution, agent
verdicts and cadence, and the path of `bad_simds` through the scheduler to the
inspect view."""
from fractions import Fraction

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from hivedscheduler_amd import ops
from hivedscheduler_amd.ops import (
    VALU_EXACT_SECTIONS,
    VALU_SECTIONS,
    VGPR_MARCH_FIRST_REG,
    VGPR_MARCH_INJECT_AGPR,
    VGPR_MARCH_INJECT_VGPR,
    VGPR_MARCH_REGS,
    decode_hw_simd,
    summarize_valu_burn,
    summarize_vgpr_march,
    valu_burn_checksum,
    valu_burn_expected,
    valu_fma_exact,
    vgpr_march_pattern,
    vgpr_march_wave_sum,
)

M32 = 0xFFFFFFFF
M64 = (1 << 64) - 1
K = 0x9E3779B1
SEEDS = (1, 5, 0xDEADBEEF)  # the seeds the tests (CPU and GPU) use
SEED, ROUNDS = 5, 2


def fmix32(h):
    """murmur3 finaliser on Python ints, written out independently."""
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & M32
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & M32
    return h ^ (h >> 16)


def rotl(x, k):
    return ((x << k) | (x >> (32 - k))) & M32


def as_i32(v):
    return int(np.uint32(v & M32).astype(np.int32))


# --------------------------------------------------------------------------
# register march: pattern and read sum
# --------------------------------------------------------------------------
def test_march_constants():
    assert (VGPR_MARCH_FIRST_REG, VGPR_MARCH_REGS) == (32, 480)
    assert VGPR_MARCH_FIRST_REG <= VGPR_MARCH_INJECT_VGPR < 256
    assert 256 <= VGPR_MARCH_INJECT_AGPR < 512


def test_march_pattern_matches_hand_computed_entries():
    p = vgpr_march_pattern(1, 0)
    assert p.dtype == np.uint32 and p.shape == (512, 64)
    rs = fmix32(1)  # seed 1, round 0
    assert rs == 0x514E28B7
    assert int(p[0, 0]) == rs
    assert int(p[0, 1]) == 0x9E3779B1 ^ rs
    # R = 256 (a0), lane 0: 256*64*K = K << 14 mod 2^32
    assert int(p[256, 0]) == ((K << 14) & M32) ^ rs == 0xDE6C4000 ^ rs
    # round 1 of seed 0 starts from the golden-ratio increment
    assert int(vgpr_march_pattern(0, 1)[0, 0]) == fmix32(0x9E3779B9)
    for seed, rnd, reg, lane in ((1, 0, 511, 63), (7, 3, 77, 17), (0xFFFFFFFF, 2, 397, 40)):
        want = (((reg * 64 + lane) * K) & M32) ^ fmix32((seed + rnd * 0x9E3779B9) & M32)
        assert int(vgpr_march_pattern(seed, rnd)[reg, lane]) == want


def test_march_pattern_is_unique_and_complement_is_its_inverse():
    for seed in SEEDS:
        for rnd in range(2):
            p = vgpr_march_pattern(seed, rnd)
            assert len(np.unique(p)) == 512 * 64
            assert np.array_equal(~p, p ^ np.uint32(M32))
            assert len(np.unique(~p)) == 512 * 64
    assert not np.array_equal(vgpr_march_pattern(SEED, 0), vgpr_march_pattern(SEED, 1))
    assert not np.array_equal(vgpr_march_pattern(SEED, 0), vgpr_march_pattern(SEED + 1, 0))


def test_march_wave_sum_against_direct_sum():
    for seed, rounds in ((1, 1), (5, 2), (0xDEADBEEF, 3)):
        direct = 0
        for r in range(rounds):
            p = vgpr_march_pattern(seed, r)
            direct += sum(int(v) for v in p[32:].reshape(-1))
        assert vgpr_march_wave_sum(seed, rounds) == direct % 2 ** 32
    assert vgpr_march_wave_sum(5, 1) != vgpr_march_wave_sum(5, 2)


# --------------------------------------------------------------------------
# VALU burn: one step of each exact section, written out independently
# --------------------------------------------------------------------------
def seed_states(section, seed):
    sid = VALU_SECTIONS.index(section)
    out = []
    for lane in range(64):
        lo = fmix32((seed + sid * 0x9E3779B9 + lane * 0x85EBCA6B) & M32)
        hi = fmix32(lo ^ 0xC2B2AE35)
        out.append((hi << 32) | lo if section == "f64" else lo)
    return out


def step_int(s):
    lo = (s * K) & M32                      # v_mul_lo_u32
    hi = (s * 0x85EBCA6B) >> 32             # v_mul_hi_u32
    m = (lo * (hi | 1) + ((hi << 32) | s)) & M64  # v_mad_u64_u32
    t = (((m & M32) ^ (m >> 32)) + lo) & M32
    return ((rotl(t, 13) ^ ((hi >> 7) & 0x7FF)) + bin(lo).count("1")) & M32


def exact_fma(a, b, c, mantissa_bits):
    """a*b + c on Fractions; asserts that the result is an integer an fp
    format with that many significand bits holds exactly."""
    r = Fraction(a) * Fraction(b) + Fraction(c)
    assert r.denominator == 1 and int(r) <= 1 << mantissa_bits
    return int(r)


def step_f32(s):
    k = ((s >> 5) & 15) - 8
    scale = Fraction(2) ** k
    # the scalar fma runs on a and c scaled by 2^k, k in [-8, 7], and its
    # result is scaled back: a significand of at most 25 bits times a power
    # of two throughout, so nothing is rounded
    r0 = ((s & 0xFFF) * scale * ((s >> 12) & 0xFFF) + (s >> 19) * scale) / scale
    assert r0.denominator == 1 and r0 <= 1 << 24
    r1 = exact_fma((s >> 3) & 0xFFF, (s >> 16) & 0xFFF, (s >> 7) & 0x1FFF, 24)
    r2 = exact_fma((s >> 9) & 0xFFF, (s >> 1) & 0xFFF, (s >> 13) & 0x1FFF, 24)
    mix = (int(r0) + (r1 << 5) + (r2 << 9)) & M32
    return ((s * K + 0x7F4A7C15) & M32) ^ mix


def step_f64(s):
    m26 = (1 << 26) - 1
    cc = exact_fma(s >> 38, 1 << 26, (s >> 7) & m26, 52)
    r = exact_fma(s & m26, (s >> 26) & m26, cc, 53)
    assert r < 1 << 53
    return ((s * 0x9E3779B97F4A7C15 + 0xBF58476D1CE4E5B9) & M64) ^ r ^ ((r << 11) & M64)


def step_xlane(x, c):
    lanes = range(64)
    q = [x[l ^ 1] for l in lanes]                                  # quad_perm:[1,0,3,2]
    x = [(rotl(x[l], 5) + q[l]) & M32 for l in lanes]
    r = [x[l] if l % 16 == 0 else x[l - 1] for l in lanes]         # row_shr:1
    x = [rotl(x[l], 7) ^ r[l] for l in lanes]
    m = [x[(l & ~15) | (15 - (l & 15))] for l in lanes]            # row_mirror
    x = [(x[l] + rotl(m[l], 13)) & M32 for l in lanes]
    y = [rotl(v, 3) for v in x]
    # v_permlane32_swap: lanes 32-63 of x swap with lanes 0-31 of y
    nx = x[:32] + y[:32]
    ny = x[32:] + y[32:]
    x = [(nx[l] + (ny[l] ^ 0x9E3779B9)) & M32 for l in lanes]
    b = [x[(l * 13 + 7) % 64] for l in lanes]                      # ds_bpermute
    x = [rotl(x[l], 9) ^ b[l] for l in lanes]
    return [(v + x[(c * 11 + 5) % 64]) & M32 for v in x]          # v_readlane


def independent_expected(section, seed, chain):
    s = seed_states(section, seed)
    for c in range(chain):
        if section == "xlane":
            s = step_xlane(s, c)
        else:
            s = [{"int": step_int, "f32": step_f32, "f64": step_f64}[section](v) for v in s]
    return s


@pytest.mark.parametrize("section", VALU_EXACT_SECTIONS)
def test_valu_expected_matches_independent_step(section):
    for seed in SEEDS:
        got = valu_burn_expected(section, seed, 1)
        assert got.dtype == np.uint64 and got.shape == (64,)
        assert [int(v) for v in got] == independent_expected(section, seed, 1)
    # and a few steps on, where the chain index of the xlane readlane moves
    assert [int(v) for v in valu_burn_expected(section, 1, 5)] == independent_expected(
        section, 1, 5)


@pytest.mark.parametrize("section", VALU_EXACT_SECTIONS)
def test_valu_expected_is_a_live_compare(section):
    """The 64 lanes differ, and a chain one step longer differs in every lane:
    a kernel that skipped a step, or a lane reading another's value, cannot
    pass."""
    for seed in SEEDS:
        e3 = valu_burn_expected(section, seed, 3)
        e4 = valu_burn_expected(section, seed, 4)
        assert len(set(int(v) for v in e3)) == 64
        assert (e3 != e4).all()
        if section != "f64":
            assert (e3 >> np.uint64(32) == 0).all()
    assert not np.array_equal(valu_burn_expected(section, 1, 3),
                              valu_burn_expected(section, 2, 3))


def test_valu_expected_rejects_trans():
    with pytest.raises(ValueError):
        valu_burn_expected("trans", 1, 1)


def test_valu_fma_bounds_fire_one_bit_too_wide():
    assert int(valu_fma_exact("f32", 4095, 4095, 8191)) == 1 << 24
    for a, b, c in ((4096, 1, 1), (1, 4096, 1), (1, 1, 8192)):
        with pytest.raises(AssertionError):
            valu_fma_exact("f32", a, b, c)
    top = (1 << 26) - 1
    assert int(valu_fma_exact("f64", top, top, (1 << 52) - 1)) == top * top + (1 << 52) - 1
    assert top * top + (1 << 52) - 1 < 1 << 53
    for a, b, c in ((1 << 26, 1, 1), (1, 1 << 26, 1), (1, 1, 1 << 52)):
        with pytest.raises(AssertionError):
            valu_fma_exact("f64", a, b, c)
    # arrays: one wide element is enough
    with pytest.raises(AssertionError):
        valu_fma_exact("f32", np.array([1, 4096], dtype=np.uint64), 1, 1)


def test_valu_checksum_cancels_over_even_rounds():
    for section in VALU_EXACT_SECTIONS:
        direct = 0
        for v in valu_burn_expected(section, SEED, 3):
            direct ^= int(v)
        assert valu_burn_checksum(section, SEED, 3, 1) == direct != 0
        assert valu_burn_checksum(section, SEED, 3, 3) == direct
        assert valu_burn_checksum(section, SEED, 3, 2) == 0


# --------------------------------------------------------------------------
# decode and summarisers on synthetic records
# --------------------------------------------------------------------------
def hw_word(xcc, se, sh, cu, simd, wave_id=0):
    return (xcc << 16) | (se << 13) | (sh << 12) | (cu << 8) | (simd << 4) | wave_id


def test_decode_hw_simd_hand_packed():
    assert decode_hw_simd(0) == (0, 0, 0, 0, 0)
    assert decode_hw_simd(0x00000030) == (0, 0, 0, 0, 3)
    assert decode_hw_simd(0x0005_4F2A) == (5, 2, 0, 15, 2)
    # 7<<16 | se 7 | sh 1 | cu 9 | simd 1 | wave 7; bits 6-7 are not SIMD_ID
    assert decode_hw_simd((7 << 16) | 0xF000 | 0x0900 | 0x00D7) == (7, 7, 1, 9, 1)
    assert decode_hw_simd(np.int32(hw_word(3, 1, 1, 4, 2, 5))) == (3, 1, 1, 4, 2)
    # the CU part is decode_hw_word's, which stays as it is
    assert decode_hw_simd(0x0005_4F2A)[:4] == ops.decode_hw_word(0x0005_4F2A)


# 4 distinct CUs, one block (4 waves, one per SIMD) each
CUS = [(0, 0, 0, 1), (0, 3, 1, 7), (5, 2, 0, 15), (7, 7, 1, 0)]
CHECK = 0x1234_5678_9ABC_DEF1


def clean_burn_records(cus=CUS, checksum=CHECK):
    rec = np.zeros((len(cus) * 4, 8), dtype=np.int32)
    for b, cu in enumerate(cus):
        for w in range(4):
            rec[4 * b + w] = (hw_word(*cu, w, wave_id=b % 8), 0, -1, -1,
                              as_i32(checksum), as_i32(checksum >> 32), 0, 0)
    return rec


def burn_summary(rec, section="int", expected_simds=16, elapsed_ms=1.0):
    return summarize_valu_burn(rec, elapsed_ms, section, 3, 3, expected_simds)


def test_summarize_burn_clean():
    s = burn_summary(clean_burn_records(), elapsed_ms=2.5)
    assert s["waves"] == 16 and s["simds_seen"] == 16
    assert s["mismatched_waves"] == 0 and s["checksum_spread"] is False
    assert s["bad_simds"] == [] and s["ok"] is True
    assert s["elapsed_ms"] == 2.5 and s["section"] == "int"


def test_summarize_burn_names_the_bad_simd_and_keeps_the_earliest():
    rec = clean_burn_records(cus=CUS + [CUS[2]])  # blocks 2 and 4 share a CU
    rec[10, 1:4] = (3, 2, 40)           # CUS[2] simd 2: round 2 lane 40
    rec[18, 1:4] = (1, 1, 63)           # same SIMD, another wave: earlier round
    rec[1, 1:4] = (2, 0, 17)            # CUS[0] simd 1
    s = burn_summary(rec)
    assert s["waves"] == 20 and s["simds_seen"] == 16 and s["mismatched_waves"] == 3
    assert s["bad_simds"] == [
        {"xcc": 0, "se": 0, "sh": 0, "cu": 1, "simd": 1, "waves": 1,
         "mismatched_lane_rounds": 2, "first_bad_round": 0, "first_bad_lane": 17},
        {"xcc": 5, "se": 2, "sh": 0, "cu": 15, "simd": 2, "waves": 2,
         "mismatched_lane_rounds": 4, "first_bad_round": 1, "first_bad_lane": 63},
    ]
    assert s["ok"] is False
    # same round in both waves: the lower lane is kept
    rec[18, 1:4] = (1, 2, 5)
    assert burn_summary(rec)["bad_simds"][1]["first_bad_lane"] == 5


def test_summarize_burn_checksum_spread_names_the_odd_simd():
    """All a consensus-only section can show: no mismatch count, one wave's
    checksum not the majority's."""
    rec = clean_burn_records()
    rec[13, 5] ^= 0x100  # high word of CUS[3] simd 1
    s = burn_summary(rec, section="trans")
    assert s["mismatched_waves"] == 0 and s["checksum_spread"] is True
    assert s["bad_simds"] == [{"xcc": 7, "se": 7, "sh": 1, "cu": 0, "simd": 1, "waves": 1,
                               "mismatched_lane_rounds": 0, "first_bad_round": -1,
                               "first_bad_lane": -1}]
    assert s["ok"] is False


def test_summarize_burn_short_coverage_is_not_ok():
    s = burn_summary(clean_burn_records(), expected_simds=17)
    assert s["simds_seen"] == 16 and s["mismatched_waves"] == 0
    assert s["checksum_spread"] is False and s["ok"] is False


def clean_march_records(seed=SEED, rounds=ROUNDS, cus=CUS):
    total = vgpr_march_wave_sum(seed, rounds)
    rec = np.zeros((len(cus) * 4, 8), dtype=np.int32)
    for b, cu in enumerate(cus):
        for w in range(4):
            # the dispatcher need not hand out SIMDs in wave order
            rec[4 * b + w] = (hw_word(*cu, (w + b) % 4, wave_id=0), 0, -1, -1, 0, 0,
                              as_i32(total), 480)
    return rec


def march_summary(rec, expected_simds=16, elapsed_ms=1.0):
    return summarize_vgpr_march(rec, elapsed_ms, ROUNDS, SEED, expected_simds)


def test_summarize_march_clean():
    s = march_summary(clean_march_records(), elapsed_ms=0.75)
    assert s["blocks"] == 4 and s["waves"] == 16 and s["simds_seen"] == 16
    assert s["mismatched_waves"] == 0 and s["split_blocks"] == 0
    assert s["checksum_ok"] is True and s["bad_simds"] == [] and s["ok"] is True
    assert s["elapsed_ms"] == 0.75


def test_summarize_march_names_the_bad_simd_ors_masks_keeps_earliest_pass():
    rec = clean_march_records(cus=CUS + [CUS[2]])
    # block 2 wave 1 -> simd (1+2)%4 = 3; block 4 wave 3 -> simd (3+4)%4 = 3
    rec[9, 1:6] = (2, 3, 300, as_i32(0x80000000), 0)
    rec[19, 1:6] = (1, 1, 397, 0, 1)
    rec[2, 1:6] = (1, 0, 77, 0x4, 0)  # block 0 wave 2 -> simd 2
    s = march_summary(rec)
    assert s["mismatched_waves"] == 3 and s["split_blocks"] == 0 and s["checksum_ok"] is True
    assert s["bad_simds"] == [
        {"xcc": 0, "se": 0, "sh": 0, "cu": 1, "simd": 2, "waves": 1, "mismatched_registers": 1,
         "first_bad_pass": 0, "first_bad_reg": 77, "dropped_mask": 0x4, "raised_mask": 0},
        {"xcc": 5, "se": 2, "sh": 0, "cu": 15, "simd": 3, "waves": 2, "mismatched_registers": 3,
         "first_bad_pass": 1, "first_bad_reg": 397, "dropped_mask": 0x80000000,
         "raised_mask": 1},
    ]
    assert s["ok"] is False


def test_summarize_march_wrong_sum_or_register_count_is_not_ok():
    rec = clean_march_records()
    rec[6, 6] ^= 1
    s = march_summary(rec)
    assert s["mismatched_waves"] == 0 and s["bad_simds"] == []
    assert s["checksum_ok"] is False and s["ok"] is False
    rec = clean_march_records()
    rec[3, 7] = 479  # a march that skipped a register
    assert march_summary(rec)["checksum_ok"] is False
    # the records of another seed or round count do not pass either
    clean = clean_march_records()
    assert summarize_vgpr_march(clean, 1.0, ROUNDS, SEED + 1, 16)["checksum_ok"] is False
    assert summarize_vgpr_march(clean, 1.0, ROUNDS + 1, SEED, 16)["checksum_ok"] is False


def test_summarize_march_mask_without_count_is_bad():
    """A complement-pass fault whose count was lost: the read sum does not
    cover it, so the set mask bit alone must fail the run and name the SIMD."""
    rec = clean_march_records()
    rec[14, 5] = 0x40  # block 3 wave 2 -> simd (2+3)%4 = 1
    s = march_summary(rec)
    assert s["checksum_ok"] is True and s["split_blocks"] == 0
    assert s["mismatched_waves"] == 1 and s["ok"] is False
    assert s["bad_simds"] == [
        {"xcc": 7, "se": 7, "sh": 1, "cu": 0, "simd": 1, "waves": 1, "mismatched_registers": 0,
         "first_bad_pass": -1, "first_bad_reg": -1, "dropped_mask": 0, "raised_mask": 0x40}]
    rec = clean_march_records()
    rec[0, 4] = as_i32(0x80000000)
    s = march_summary(rec)
    assert s["ok"] is False and s["bad_simds"][0]["dropped_mask"] == 0x80000000


def test_summarize_march_split_blocks():
    # two waves of a block on one SIMD: the "alone on its SIMD" premise broke
    rec = clean_march_records()
    rec[5, 0] = rec[4, 0]
    s = march_summary(rec)
    assert s["split_blocks"] == 1 and s["ok"] is False
    assert s["mismatched_waves"] == 0 and s["checksum_ok"] is True
    # one wave of a block names another CU
    rec = clean_march_records()
    rec[5, 0] = hw_word(*CUS[0], decode_hw_simd(rec[5, 0])[4])
    s = march_summary(rec)
    assert s["split_blocks"] == 1 and s["ok"] is False


def test_summarize_march_short_coverage_is_not_ok():
    s = march_summary(clean_march_records(), expected_simds=17)
    assert s["simds_seen"] == 16 and s["split_blocks"] == 0 and s["ok"] is False


# --------------------------------------------------------------------------
# wiring: agent, CLI, inspect view
# --------------------------------------------------------------------------
BAD_SIMD = {"xcc": 5, "se": 2, "sh": 0, "cu": 15, "simd": 3}
BAD_SIMD_DETAIL = dict(BAD_SIMD, waves=1, mismatched_registers=1, first_bad_pass=1,
                       first_bad_reg=397, dropped_mask=0, raised_mask=8)


def canned_report(bad=(), valu_ok=True, march_ok=None):
    march_ok = (not bad) if march_ok is None else march_ok
    return {
        "hbm_gbps": 5000.0, "mfma_ok": True, "cu_coverage": 256, "lds_errors": 0,
        "healthy": bool(valu_ok and march_ok),
        "simd_probe": {
            "valu": {"ok": valu_ok, "bad_simds": [], "sections": {}},
            "vgpr_march": {"ok": march_ok, "bad_simds": [BAD_SIMD_DETAIL] if bad else []},
            "ok": bool(valu_ok and march_ok),
            "bad_simds": list(bad),
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
        if not kwargs.get("simd_probe"):
            rep.pop("simd_probe")
            rep["healthy"] = True
        return rep

    monkeypatch.setattr(ops, "gpu_health_report", fake_report)
    monkeypatch.setattr(health, "_rocm_smi_gpu_state", lambda: {0: True})
    return health, state


def test_agent_probe_verdicts(agent_health):
    health, state = agent_health
    state["report"] = canned_report()
    g = health.collect_node_health(deep=True, simd_probe=True)["gpus"]["0"]
    assert g["healthy"] is True and g["simd_probe_ok"] is True
    assert g["valu_burn_ok"] is True and g["vgpr_march_ok"] is True and g["bad_simds"] == []
    assert state["calls"][-1]["simd_probe"] is True
    assert "burn" not in state["calls"][-1] and "lds_march" not in state["calls"][-1]
    assert "bad_cus" not in g and "lds_bad_cus" not in g
    # a named SIMD fails the GPU and is reported with the five keys only
    state["report"] = canned_report(bad=[dict(BAD_SIMD)])
    g = health.collect_node_health(deep=True, simd_probe=True)["gpus"]["0"]
    assert g["healthy"] is False and g["simd_probe_ok"] is False
    assert g["vgpr_march_ok"] is False and g["valu_burn_ok"] is True
    assert g["bad_simds"] == [BAD_SIMD]
    # a probe that failed without naming a SIMD (coverage, checksum) too
    state["report"] = canned_report(valu_ok=False)
    g = health.collect_node_health(deep=True, simd_probe=True)["gpus"]["0"]
    assert g["healthy"] is False and g["simd_probe_ok"] is False
    assert g["valu_burn_ok"] is False and g["vgpr_march_ok"] is True and g["bad_simds"] == []


def test_agent_without_probe_is_unchanged(agent_health):
    health, state = agent_health
    state["report"] = canned_report(bad=[dict(BAD_SIMD)])
    g = health.collect_node_health(deep=True)["gpus"]["0"]
    assert g == {"healthy": True, "hbm_gbps": 5000.0, "mfma_ok": True, "cu_coverage": 256,
                 "lds_errors": 0}
    assert "simd_probe" not in state["calls"][-1]
    # not deep: the kernels do not run at all
    n = len(state["calls"])
    g = health.collect_node_health(deep=False, simd_probe=True)["gpus"]["0"]
    assert g == {"healthy": True} and len(state["calls"]) == n


def test_agent_probe_cadence(agent_health, monkeypatch):
    health, state = agent_health
    state["report"] = canned_report(bad=[dict(BAD_SIMD)])
    monkeypatch.setattr(health.NodeHealthAgent, "post_report", lambda self, r: True)
    monkeypatch.setattr(health.NodeHealthAgent, "run_placement_probes", lambda self: [])
    monkeypatch.setattr(health, "p2p_link_matrix", lambda: {"matrix": {}, "links": []})
    never = health.NodeHealthAgent("http://x", node_name="n", deep_every=1, probe_pairs=False,
                                   p2p_matrix_every=10 ** 9)
    assert never.simd_probe_every == 0
    assert all("simd_probe_ok" not in never.run_once()["gpus"]["0"] for _ in range(3))
    assert all("simd_probe" not in c for c in state["calls"])
    agent = health.NodeHealthAgent("http://x", node_name="n", deep_every=1, probe_pairs=False,
                                   p2p_matrix_every=10 ** 9, simd_probe_every=2)
    got = [agent.run_once()["gpus"]["0"] for _ in range(4)]
    assert ["bad_simds" in g for g in got] == [True, False, True, False]
    assert [g["healthy"] for g in got] == [False, True, False, True]
    # only on deep sweeps: every 2nd round is a probe round, every 4th deep
    agent = health.NodeHealthAgent("http://x", node_name="n", deep_every=4, probe_pairs=False,
                                   p2p_matrix_every=10 ** 9, simd_probe_every=2)
    got = [agent.run_once()["gpus"]["0"] for _ in range(6)]
    assert ["bad_simds" in g for g in got] == [True, False, False, False, True, False]


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
    monkeypatch.setattr(sys, "argv", ["agent", "--local", "--simd-probe", "--no-probe-pairs"])
    cli.main()
    assert seen["simd_probe"] is True
    assert json.loads(capsys.readouterr().out) == {"gpus": {}}
    monkeypatch.setattr(sys, "argv", ["agent", "--local", "--no-probe-pairs"])
    cli.main()
    assert seen["simd_probe"] is False

    made = {}

    class FakeAgent:
        def __init__(self, url, **kwargs):
            made.update(kwargs)

        def run_once(self):
            return {}

    monkeypatch.setattr(health, "NodeHealthAgent", FakeAgent)
    monkeypatch.setattr(sys, "argv", ["agent", "--scheduler", "http://x", "--once",
                                      "--simd-probe-every", "6"])
    cli.main()
    assert made["simd_probe_every"] == 6
    monkeypatch.setattr(sys, "argv", ["agent", "--scheduler", "http://x", "--once"])
    cli.main()
    assert made["simd_probe_every"] == 0


def test_health_report_signature_has_the_option_off_by_default():
    import inspect

    sig = inspect.signature(ops.gpu_health_report)
    assert sig.parameters["simd_probe"].default is False
    sig = inspect.signature(ops.valu_burn_report)
    assert sig.parameters["blocks"].default == 2048 and sig.parameters["inject"].default is None
    with pytest.raises(ValueError):  # before anything touches a GPU
        ops.valu_burn_report(0, sections=("trans",), rounds=2)


def test_bad_simds_reach_the_inspect_view():
    from hivedscheduler_amd.scheduler import HivedScheduler
    from hivedscheduler_amd.sim import mi355x_cluster_config

    sched = HivedScheduler(mi355x_cluster_config(num_nodes=1))
    node = sched.algorithm.all_nodes()[0]
    sched.on_node_add({"metadata": {"name": node, "uid": "n1"}, "spec": {},
                       "status": {"conditions": [{"type": "Ready", "status": "True"}]}})
    bad_simds = [dict(BAD_SIMD)]
    report = {"gpus": {"3": {"healthy": False, "simd_probe_ok": False, "valu_burn_ok": True,
                             "vgpr_march_ok": False, "bad_simds": bad_simds}}}
    assert sched.on_health_report(node, report)["applied"] == {"3": False}

    def leaves(c):
        kids = c.get("cellChildren") or []
        return [c] if not kids else [l for k in kids for l in leaves(k)]

    status = sched.get_physical_cluster_status()
    unhealthy = [c for c in leaves(status[0]) if c.get("cellHealthiness") != "Healthy"]
    assert len(unhealthy) == 1, [c.get("cellAddress") for c in unhealthy]
    gpu = sched.get_health_reports()[node]["gpus"]["3"]
    assert gpu["bad_simds"] == bad_simds
    assert gpu["simd_probe_ok"] is False and gpu["vgpr_march_ok"] is False
    assert gpu["valu_burn_ok"] is True
