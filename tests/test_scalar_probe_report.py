"""Scalar probe, host side (no GPU): the SALU burn's mirrors against steps
written out independently on Python ints, both arms of the ctl section's
branches, the SGPR march's pattern and read sum, the scalar-load pattern,
record summarising and per-SIMD attribution, agent verdicts and cadence, and
the path of `scalar_bad_simds` through the scheduler to the inspect view."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from hivedscheduler_amd import ops
from hivedscheduler_amd.ops import (
    SALU_CHAINS,
    SALU_SECTIONS,
    SGPR_MARCH_FIRST_REG,
    SGPR_MARCH_INJECT_REG,
    SGPR_MARCH_REGS,
    salu_burn_checksum,
    salu_burn_expected,
    salu_ctl_arms,
    scalar_load_pattern,
    sgpr_march_pattern,
    sgpr_march_wave_sum,
    summarize_salu_burn,
    summarize_scalar_load,
    summarize_sgpr_march,
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


def as_i32(v):
    return int(np.uint32(v & M32).astype(np.int32))


def signed(x, bits=32):
    return x - (1 << bits) if x >> (bits - 1) else x


def bits_of(x, n):
    return [(x >> i) & 1 for i in range(n)]


def from_bits(b):
    return sum(v << i for i, v in enumerate(b))


def popcount(x):
    return sum(bits_of(x, 64))


def first_one_from_lsb(x, n):
    for i in range(n):
        if (x >> i) & 1:
            return i
    return M32  # -1


def first_one_from_msb(x, n):
    for i in range(n):
        if (x >> (n - 1 - i)) & 1:
            return i
    return M32  # -1


def field(x, offset, width, sign, n):
    """bits [offset, offset+width) of x, zero- or sign-extended to n bits."""
    v = (x >> offset) & ((1 << width) - 1)
    if sign and v >> (width - 1):
        v |= ((1 << n) - 1) & ~((1 << width) - 1)
    return v


# --------------------------------------------------------------------------
# SALU burn: one step of each section, written out independently
# --------------------------------------------------------------------------
def seed_state(section, seed, index):
    sid = SALU_SECTIONS.index(section)
    lo = fmix32((seed + sid * 0x9E3779B9 + index * 0x85EBCA6B) & M32)
    hi = fmix32(lo ^ 0xC2B2AE35)
    return (hi << 32) | lo if section == "s64" else lo


def step_s32(s):
    a = (s * K) % 2 ** 32                                    # s_mul_i32
    b = (s * 0x85EBCA6B) // 2 ** 32                          # s_mul_hi_u32
    c = ((signed(s) * signed(0xC2B2AE35)) // 2 ** 32) % 2 ** 32  # s_mul_hi_i32
    t = a + b                                                # s_add_u32
    a, carry = t % 2 ** 32, t // 2 ** 32
    t = b + c + carry                                        # s_addc_u32
    b = t % 2 ** 32
    borrow = 1 if a > c else 0                               # s_sub_u32
    c = (c - a) % 2 ** 32
    t = a - b - borrow                                       # s_subb_u32
    a, borrow = t % 2 ** 32, 1 if t < 0 else 0
    c = (c + s + borrow) % 2 ** 32                           # s_addc_u32
    d = (a << (b % 32)) % 2 ** 32                            # s_lshl_b32
    d ^= c >> (a % 32)                                       # s_lshr_b32
    d = (d + (signed(b) >> (c % 32))) % 2 ** 32              # s_ashr_i32
    d ^= field(a, 7, 11, False, 32)                          # s_bfe_u32
    d = (d + field(c, 5, 13, True, 32)) % 2 ** 32            # s_bfe_i32
    d = (2 * popcount(b) + d) % 2 ** 32                      # s_bcnt1, s_lshl1_add_u32
    d = (4 * first_one_from_lsb(c, 32) + d) % 2 ** 32        # s_ff1, s_lshl2_add_u32
    d = (8 * first_one_from_msb(a, 32) + d) % 2 ** 32        # s_flbit, s_lshl3_add_u32
    r = from_bits(bits_of(b, 32)[::-1])                      # s_brev_b32
    d = ((16 * r + d) % 2 ** 32) ^ r                         # s_lshl4_add_u32
    d = (d + abs(signed(a & 0xFFFF, 16) - signed(c & 0xFF, 8))) % 2 ** 32  # sext, s_absdiff_i32
    e = (min(signed(a), signed(b)) % 2 ** 32) ^ (max(signed(a), signed(c)) % 2 ** 32)
    e = (e + min(b, c)) % 2 ** 32
    e ^= max(a, d)
    d = (d + e) % 2 ** 32
    ll = ((b & 0xFFFF) << 16) | (a & 0xFFFF)                 # s_pack_ll: {S1.lo, S0.lo}
    lh = ((c >> 16) << 16) | (b & 0xFFFF)                    # s_pack_lh: {S1.hi, S0.lo}
    hh = ((a >> 16) << 16) | (c >> 16)                       # s_pack_hh: {S1.hi, S0.hi}
    d ^= ((ll ^ lh) + hh) % 2 ** 32
    e = bits_of(c, 32)
    e[a % 32] = 0                                            # s_bitset0_b32
    e[b % 32] = 1                                            # s_bitset1_b32
    d = (d + from_bits(e)) % 2 ** 32
    inv = lambda v: v ^ M32
    e = (a & inv(b)) ^ (b | inv(c))                          # s_andn2, s_orn2
    e = (e + inv(c & a)) % 2 ** 32                           # s_nand
    e ^= inv(a | d)                                          # s_nor
    e = (e + inv(b ^ d)) % 2 ** 32                           # s_xnor
    d ^= e
    return (d + 0x7F4A7C15) % 2 ** 32


def step_s64(s):
    inv = lambda v: v ^ M64
    A = ((s << 13) % 2 ** 64) ^ (s >> 7) ^ (signed(s, 64) >> 17) % 2 ** 64
    B = field(s, 9, 40, False, 64)                           # s_bfe_u64
    C = field(A, 17, 29, True, 64)                           # s_bfe_i64
    A = (A + B) % 2 ** 64                                    # s_add_u32 + s_addc_u32
    D = (A & C) ^ (B | C) ^ (A & inv(B)) ^ inv(s & C) ^ inv(A | s) ^ inv(B ^ s)
    D ^= from_bits(bits_of(inv(C), 64)[::-1])                # s_not_b64, s_brev_b64
    wqm = 0
    for q in range(16):                                      # s_wqm_b64
        if (B >> (4 * q)) & 0xF:
            wqm |= 0xF << (4 * q)
    D ^= wqm
    e = popcount(A)
    f = first_one_from_lsb(D, 64)
    g = first_one_from_msb(C, 64)
    h = e if (s & 1) == ((A >> 3) & 1) else f                # s_cmp_eq_u64
    g = g if (s & 1) != ((B >> 5) & 1) else e                # s_cmp_lg_u64
    e = ((e << 8) % 2 ** 32) ^ f
    lo = (D % 2 ** 32) + h
    hi = ((D >> 32) + g + (lo >> 32)) % 2 ** 32
    lo %= 2 ** 32
    hi ^= e
    lo += 0x7F4A7C15
    hi = (hi + 0x9E3779B9 + (lo >> 32)) % 2 ** 32
    return (hi << 32) | (lo % 2 ** 32)


def step_ctl(s, arms):
    a = (signed(s) * 0x6B43 + 0x7C15) % 2 ** 32              # s_mulk_i32, s_addk_i32
    b = (s >> 15) ^ a
    c, e, g, h = a % 4, b % 4, a >> 16, b >> 16
    sa, sb, ss = signed(a), signed(b), signed(s)
    f = (-12059) % 2 ** 32                                   # s_movk_i32 sign-extends
    n = a if c == e else b
    if c != 2:
        f = h
    R = ((a << 32) | b) if sa > sb else ((b << 32) | s)
    outcomes = [c == e, c != 2, sa > sb, sb >= ss, sa < ss, ss <= sb,
                e == 1, c != e, a > b, b >= s, s < a, h <= g,
                not (a >> (b % 32)) & 1, bool((b >> (a % 32)) & 1),
                c == 1, e != 2, sa > 0x1234, sb >= -4660, sa < -28672, sb <= 0x7000,
                e == 3, c != 0, g > 0x8000, h >= 0x4000, g < 0xC000, h <= 0x2000]
    assert len(outcomes) == 26
    d = 0x1B
    for o in outcomes:
        d = (2 * d + (1 if o else 0)) % 2 ** 32
    n ^= f
    if (s >> 7) & 1:
        arms.add((1, True))
        n = (n * K + d) % 2 ** 32
    else:
        arms.add((1, False))
        n = ((n - d) % 2 ** 32) ^ a
    if n < b:
        arms.add((2, True))
    else:
        arms.add((2, False))
        n = ((n ^ M32) + h) % 2 ** 32
    n ^= R % 2 ** 32
    return (n + (R >> 32)) % 2 ** 32


def step_mask(x, c):
    inside = [(v >> (c % 32)) & 1 for v in x]
    m = from_bits(inside)
    pc = sum(inside)
    ff = inside.index(1) + 1 if pc else 0
    y = []
    for v, i in zip(x, inside):
        if i:
            y.append((v * K + pc) % 2 ** 32)
        else:
            y.append(((v ^ (v >> 15)) * 0x85EBCA6B + ff) % 2 ** 32)
    feedback = y[0] ^ (m % 2 ** 32) ^ (m >> 32)
    return [(v + feedback) % 2 ** 32 for v in y]


def independent_expected(section, seed, chain, arms=None):
    arms = set() if arms is None else arms
    if section == "mask":
        x = [seed_state(section, seed, l) for l in range(64)]
        for c in range(chain):
            x = step_mask(x, c)
        return x
    out = []
    for k in range(SALU_CHAINS):
        s = seed_state(section, seed, k)
        for _ in range(chain):
            s = {"s32": step_s32, "s64": step_s64, "ctl": lambda v: step_ctl(v, arms)}[section](s)
        out.append(s)
    return out


def test_constants():
    assert SALU_SECTIONS == ("s32", "s64", "ctl", "mask") and SALU_CHAINS == 8
    assert (SGPR_MARCH_FIRST_REG, SGPR_MARCH_REGS, SGPR_MARCH_INJECT_REG) == (32, 70, 77)


@pytest.mark.parametrize("section", SALU_SECTIONS)
def test_salu_expected_matches_independent_step(section):
    units = 64 if section == "mask" else SALU_CHAINS
    for seed in SEEDS:
        for chain in (1, 3, 4):
            got = salu_burn_expected(section, seed, chain)
            assert got.dtype == np.uint64 and got.shape == (units,)
            assert [int(v) for v in got] == independent_expected(section, seed, chain), (seed, chain)
    assert [int(v) for v in salu_burn_expected(section, 1, 9)] == independent_expected(
        section, 1, 9)


@pytest.mark.parametrize("section", SALU_SECTIONS)
def test_salu_expected_is_a_live_compare(section):
    """The states differ, and a chain one step longer differs in every one: a
    kernel that skipped a step, or read another chain's value, cannot pass."""
    for seed in SEEDS:
        e3 = salu_burn_expected(section, seed, 3)
        e4 = salu_burn_expected(section, seed, 4)
        assert len(set(int(v) for v in e3)) == len(e3)
        assert (e3 != e4).all()
        if section != "s64":
            assert (e3 >> np.uint64(32) == 0).all()
    assert (salu_burn_expected("s64", SEED, 3) >> np.uint64(32) != 0).any()
    assert not np.array_equal(salu_burn_expected(section, 1, 3), salu_burn_expected(section, 2, 3))
    with pytest.raises(ValueError):
        salu_burn_expected("s16", 1, 1)


def test_ctl_takes_both_arms_of_both_branches():
    """Within the chain lengths the tests use, from the seeds they use."""
    both = {(1, True), (1, False), (2, True), (2, False)}
    for seed in SEEDS:
        for chain in (1, 3):
            assert salu_ctl_arms(seed, chain) == both, (seed, chain)
            arms = set()
            independent_expected("ctl", seed, chain, arms)
            assert arms == both, (seed, chain)


def test_salu_checksum_cancels_over_even_rounds():
    for section in SALU_SECTIONS:
        direct = 0
        for v in salu_burn_expected(section, SEED, 3):
            direct ^= int(v)
        assert salu_burn_checksum(section, SEED, 3, 1) == direct != 0
        assert salu_burn_checksum(section, SEED, 3, 3) == direct
        assert salu_burn_checksum(section, SEED, 3, 2) == 0


# --------------------------------------------------------------------------
# SGPR march: pattern and read sum; scalar-load pattern
# --------------------------------------------------------------------------
def test_march_pattern_matches_hand_computed_entries():
    p = sgpr_march_pattern(1, 0, 0)
    assert p.dtype == np.uint32 and p.shape == (102,)
    rs = fmix32(1)  # seed 1, round 0
    assert rs == 0x514E28B7
    assert int(p[0]) == rs
    assert int(p[1]) == 0x9E3779B1 ^ rs
    # wave 1, register 0: 128*K = K << 7 mod 2^32
    assert int(sgpr_march_pattern(1, 0, 1)[0]) == ((K << 7) & M32) ^ rs == 0x1BBCD880 ^ rs
    assert int(sgpr_march_pattern(0, 1, 0)[0]) == fmix32(0x9E3779B9)
    for seed, rnd, wave, reg in ((1, 0, 31, 101), (7, 3, 6, 77), (0xFFFFFFFF, 2, 2 ** 25 - 1, 32)):
        want = (((wave * 128 + reg) * K) & M32) ^ fmix32((seed + rnd * 0x9E3779B9) & M32)
        assert int(sgpr_march_pattern(seed, rnd, wave)[reg]) == want


def test_march_pattern_is_unique_and_complement_is_its_inverse():
    for seed in SEEDS:
        for rnd in range(2):
            p = np.stack([sgpr_march_pattern(seed, rnd, w) for w in range(64)])
            assert p.shape == (64, 102)
            assert len(np.unique(p)) == 102 * 64
            assert np.array_equal(~p, p ^ np.uint32(M32))
            assert np.array_equal(~(~p), p) and len(np.unique(~p)) == 102 * 64
    assert not np.array_equal(sgpr_march_pattern(SEED, 0, 0), sgpr_march_pattern(SEED, 1, 0))
    assert not np.array_equal(sgpr_march_pattern(SEED, 0, 0), sgpr_march_pattern(SEED + 1, 0, 0))


def test_march_wave_sum_against_direct_sum():
    for seed, rounds, wave in ((1, 1, 0), (5, 2, 6), (0xDEADBEEF, 3, 15)):
        direct = 0
        for r in range(rounds):
            direct += sum(int(v) for v in sgpr_march_pattern(seed, r, wave)[32:])
        assert sgpr_march_wave_sum(seed, rounds, wave) == direct % 2 ** 32
    assert sgpr_march_wave_sum(5, 1, 0) != sgpr_march_wave_sum(5, 2, 0)
    assert sgpr_march_wave_sum(5, 2, 0) != sgpr_march_wave_sum(5, 2, 1)


def test_scalar_load_pattern():
    for seed in SEEDS:
        p = scalar_load_pattern(seed, 64)
        assert p.shape == (2, 64) and p.dtype == np.uint32
        assert np.array_equal(p[1], ~p[0])
        assert [int(v) for v in p[0, :5]] == [fmix32((seed ^ (i * 0x85EBCA6B)) & M32)
                                             for i in range(5)]
        assert len(np.unique(p)) == 128
    assert np.array_equal(scalar_load_pattern(SEED, 4096)[:, :64], scalar_load_pattern(SEED, 64))


# --------------------------------------------------------------------------
# summarisers on synthetic records
# --------------------------------------------------------------------------
def hw_word(xcc, se, sh, cu, simd, wave_id=0):
    return (xcc << 16) | (se << 13) | (sh << 12) | (cu << 8) | (simd << 4) | wave_id


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


def burn_summary(rec, section="s32", expected_simds=16, elapsed_ms=1.0):
    return summarize_salu_burn(rec, elapsed_ms, section, 3, 3, expected_simds)


def test_summarize_burn_clean():
    s = burn_summary(clean_burn_records(), elapsed_ms=2.5)
    assert s["waves"] == 16 and s["simds_seen"] == 16
    assert s["mismatched_waves"] == 0 and s["checksum_spread"] is False
    assert s["bad_simds"] == [] and s["ok"] is True
    assert s["elapsed_ms"] == 2.5 and s["section"] == "s32"
    assert (s["chain"], s["rounds"]) == (3, 3)


def test_summarize_burn_names_the_bad_simd_and_keeps_the_earliest():
    rec = clean_burn_records(cus=CUS + [CUS[2]])  # blocks 2 and 4 share a CU
    rec[10, 1:4] = (3, 2, 6)            # CUS[2] simd 2: round 2 chain 6
    rec[18, 1:4] = (1, 1, 7)            # same SIMD, another wave: earlier round
    rec[1, 1:4] = (2, 0, 3)             # CUS[0] simd 1
    s = burn_summary(rec)
    assert s["waves"] == 20 and s["simds_seen"] == 16 and s["mismatched_waves"] == 3
    assert s["bad_simds"] == [
        {"xcc": 0, "se": 0, "sh": 0, "cu": 1, "simd": 1, "waves": 1,
         "mismatched_chain_rounds": 2, "first_bad_round": 0, "first_bad_chain": 3},
        {"xcc": 5, "se": 2, "sh": 0, "cu": 15, "simd": 2, "waves": 2,
         "mismatched_chain_rounds": 4, "first_bad_round": 1, "first_bad_chain": 7},
    ]
    assert s["ok"] is False
    # same round in both waves: the lower chain is kept
    rec[18, 1:4] = (1, 2, 5)
    assert burn_summary(rec)["bad_simds"][1]["first_bad_chain"] == 5


def test_summarize_burn_checksum_outlier_is_named():
    """A wave whose checksum is not the majority's is bad even with a zero
    count."""
    rec = clean_burn_records()
    rec[13, 5] ^= 0x100  # high word of CUS[3] simd 1
    s = burn_summary(rec, section="s64")
    assert s["mismatched_waves"] == 0 and s["checksum_spread"] is True
    assert s["bad_simds"] == [{"xcc": 7, "se": 7, "sh": 1, "cu": 0, "simd": 1, "waves": 1,
                               "mismatched_chain_rounds": 0, "first_bad_round": -1,
                               "first_bad_chain": -1}]
    assert s["ok"] is False


def test_summarize_burn_short_coverage_is_not_ok():
    s = burn_summary(clean_burn_records(), expected_simds=17)
    assert s["simds_seen"] == 16 and s["mismatched_waves"] == 0
    assert s["checksum_spread"] is False and s["ok"] is False


def clean_march_records(seed=SEED, rounds=ROUNDS, cus=CUS):
    rec = np.zeros((len(cus) * 4, 8), dtype=np.int32)
    for b, cu in enumerate(cus):
        for w in range(4):
            rec[4 * b + w] = (hw_word(*cu, (w + b) % 4), 0, -1, -1, 0, 0,
                              as_i32(sgpr_march_wave_sum(seed, rounds, 4 * b + w)), 70)
    return rec


def march_summary(rec, expected_simds=16, elapsed_ms=1.0):
    return summarize_sgpr_march(rec, elapsed_ms, ROUNDS, SEED, expected_simds)


def test_summarize_march_clean():
    s = march_summary(clean_march_records(), elapsed_ms=0.75)
    assert s["waves"] == 16 and s["simds_seen"] == 16 and s["mismatched_waves"] == 0
    assert s["checksum_ok"] is True and s["bad_simds"] == [] and s["ok"] is True
    assert s["elapsed_ms"] == 0.75


def test_summarize_march_names_the_bad_simd_ors_masks_keeps_earliest_pass():
    rec = clean_march_records(cus=CUS + [CUS[2]])
    # block 2 wave 1 -> simd (1+2)%4 = 3; block 4 wave 3 -> simd (3+4)%4 = 3
    rec[9, 1:6] = (2, 3, 90, as_i32(0x80000000), 0)
    rec[19, 1:6] = (1, 1, 101, 0, 1)
    rec[2, 1:6] = (1, 0, 77, 0x4, 0)  # block 0 wave 2 -> simd 2
    s = march_summary(rec)
    assert s["mismatched_waves"] == 3 and s["checksum_ok"] is True
    assert s["bad_simds"] == [
        {"xcc": 0, "se": 0, "sh": 0, "cu": 1, "simd": 2, "waves": 1, "mismatched_registers": 1,
         "first_bad_pass": 0, "first_bad_reg": 77, "dropped_mask": 0x4, "raised_mask": 0},
        {"xcc": 5, "se": 2, "sh": 0, "cu": 15, "simd": 3, "waves": 2, "mismatched_registers": 3,
         "first_bad_pass": 1, "first_bad_reg": 101, "dropped_mask": 0x80000000,
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
    rec[3, 7] = 69  # a march that skipped a register
    assert march_summary(rec)["checksum_ok"] is False
    # a wave holding another wave's data sums to that wave's sum
    rec = clean_march_records()
    rec[[4, 5], 6] = rec[[5, 4], 6]
    assert march_summary(rec)["checksum_ok"] is False
    # the records of another seed or round count do not pass either
    clean = clean_march_records()
    assert summarize_sgpr_march(clean, 1.0, ROUNDS, SEED + 1, 16)["checksum_ok"] is False
    assert summarize_sgpr_march(clean, 1.0, ROUNDS + 1, SEED, 16)["checksum_ok"] is False


def test_summarize_march_mask_without_count_is_bad():
    rec = clean_march_records()
    rec[14, 5] = 0x40  # block 3 wave 2 -> simd (2+3)%4 = 1
    s = march_summary(rec)
    assert s["checksum_ok"] is True and s["mismatched_waves"] == 1 and s["ok"] is False
    assert s["bad_simds"] == [
        {"xcc": 7, "se": 7, "sh": 1, "cu": 0, "simd": 1, "waves": 1, "mismatched_registers": 0,
         "first_bad_pass": -1, "first_bad_reg": -1, "dropped_mask": 0, "raised_mask": 0x40}]
    rec = clean_march_records()
    rec[0, 4] = as_i32(0x80000000)
    s = march_summary(rec)
    assert s["ok"] is False and s["bad_simds"][0]["dropped_mask"] == 0x80000000


def test_summarize_march_short_coverage_is_not_ok():
    s = march_summary(clean_march_records(), expected_simds=17)
    assert s["simds_seen"] == 16 and s["checksum_ok"] is True and s["ok"] is False


WORDS, LOAD_ROUNDS = 64, 5


def clean_load_records(cus=CUS):
    total = LOAD_ROUNDS * sum(int(v) for v in scalar_load_pattern(SEED, WORDS)[0])
    rec = np.zeros((len(cus) * 4, 8), dtype=np.int32)
    for b, cu in enumerate(cus):
        for w in range(4):
            rec[4 * b + w] = (hw_word(*cu, w), 0, -1, -1, 0, 0, as_i32(total), 2 * WORDS)
    return rec


def load_summary(rec, expected_simds=16, **kw):
    args = dict(rounds=LOAD_ROUNDS, seed=SEED, words=WORDS)
    args.update(kw)
    return summarize_scalar_load(rec, 1.0, expected_simds=expected_simds, **args)


def test_summarize_load():
    s = load_summary(clean_load_records())
    assert s["ok"] is True and s["waves"] == 16 and s["simds_seen"] == 16
    assert s["checksum_ok"] is True and s["bad_simds"] == []
    rec = clean_load_records()
    rec[5, 1:6] = (5, 0, 64 + 9, 0, 0x10)   # row 1 word 9 read a 1 for a 0, in all five rounds
    rec[7, 1:6] = (0, -1, -1, 0x2, 0)       # a mask without a count
    s = load_summary(rec)
    assert s["ok"] is False and s["mismatched_waves"] == 2 and s["checksum_ok"] is True
    assert s["bad_simds"] == [
        {"xcc": 0, "se": 3, "sh": 1, "cu": 7, "simd": 1, "waves": 1, "mismatched_words": 5,
         "first_bad_round": 0, "first_bad_word": 73, "dropped_mask": 0, "raised_mask": 0x10},
        {"xcc": 0, "se": 3, "sh": 1, "cu": 7, "simd": 3, "waves": 1, "mismatched_words": 0,
         "first_bad_round": -1, "first_bad_word": -1, "dropped_mask": 0x2, "raised_mask": 0}]
    rec = clean_load_records()
    rec[2, 6] += 1
    assert load_summary(rec)["checksum_ok"] is False
    rec = clean_load_records()
    rec[2, 7] = 2 * WORDS - 16
    assert load_summary(rec)["ok"] is False
    assert load_summary(clean_load_records(), expected_simds=17)["ok"] is False
    assert load_summary(clean_load_records(), rounds=LOAD_ROUNDS + 1)["checksum_ok"] is False


# --------------------------------------------------------------------------
# wiring: agent, CLI, inspect view
# --------------------------------------------------------------------------
BAD_SIMD = {"xcc": 5, "se": 2, "sh": 0, "cu": 15, "simd": 3}
BAD_SIMD_DETAIL = dict(BAD_SIMD, waves=1, mismatched_registers=1, first_bad_pass=1,
                       first_bad_reg=77, dropped_mask=0, raised_mask=8)


def canned_report(bad=(), salu_ok=True, march_ok=None, load_ok=True):
    march_ok = (not bad) if march_ok is None else march_ok
    ok = bool(salu_ok and march_ok and load_ok)
    return {
        "hbm_gbps": 5000.0, "mfma_ok": True, "cu_coverage": 256, "lds_errors": 0,
        "healthy": ok,
        "scalar_probe": {
            "salu": {"ok": salu_ok, "bad_simds": [], "sections": {}},
            "sgpr_march": {"ok": march_ok, "bad_simds": [BAD_SIMD_DETAIL] if bad else []},
            "scalar_load": {"ok": load_ok, "bad_simds": []},
            "ok": ok,
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
        if not kwargs.get("scalar_probe"):
            rep.pop("scalar_probe")
            rep["healthy"] = True
        return rep

    monkeypatch.setattr(ops, "gpu_health_report", fake_report)
    monkeypatch.setattr(health, "_rocm_smi_gpu_state", lambda: {0: True})
    return health, state


def test_agent_probe_verdicts(agent_health):
    health, state = agent_health
    state["report"] = canned_report()
    g = health.collect_node_health(deep=True, scalar_probe=True)["gpus"]["0"]
    assert g["healthy"] is True and g["scalar_probe_ok"] is True
    assert g["salu_burn_ok"] is True and g["sgpr_march_ok"] is True
    assert g["scalar_load_ok"] is True and g["scalar_bad_simds"] == []
    assert state["calls"][-1]["scalar_probe"] is True
    assert "simd_probe" not in state["calls"][-1] and "burn" not in state["calls"][-1]
    assert "bad_simds" not in g and "bad_cus" not in g
    # a named SIMD fails the GPU and is reported with the five keys only
    state["report"] = canned_report(bad=[dict(BAD_SIMD)])
    g = health.collect_node_health(deep=True, scalar_probe=True)["gpus"]["0"]
    assert g["healthy"] is False and g["scalar_probe_ok"] is False
    assert g["sgpr_march_ok"] is False and g["salu_burn_ok"] is True
    assert g["scalar_bad_simds"] == [BAD_SIMD]
    # a part that failed without naming a SIMD (coverage, checksum) too
    for part in ("salu", "load"):
        state["report"] = canned_report(**{f"{part}_ok": False})
        g = health.collect_node_health(deep=True, scalar_probe=True)["gpus"]["0"]
        assert g["healthy"] is False and g["scalar_probe_ok"] is False
        assert g["salu_burn_ok"] is (part != "salu") and g["scalar_load_ok"] is (part != "load")
        assert g["sgpr_march_ok"] is True and g["scalar_bad_simds"] == []


def test_agent_without_probe_is_unchanged(agent_health):
    health, state = agent_health
    state["report"] = canned_report(bad=[dict(BAD_SIMD)])
    g = health.collect_node_health(deep=True)["gpus"]["0"]
    assert g == {"healthy": True, "hbm_gbps": 5000.0, "mfma_ok": True, "cu_coverage": 256,
                 "lds_errors": 0}
    assert "scalar_probe" not in state["calls"][-1]
    # not deep: the kernels do not run at all
    n = len(state["calls"])
    g = health.collect_node_health(deep=False, scalar_probe=True)["gpus"]["0"]
    assert g == {"healthy": True} and len(state["calls"]) == n


def test_agent_probe_cadence(agent_health, monkeypatch):
    health, state = agent_health
    state["report"] = canned_report(bad=[dict(BAD_SIMD)])
    monkeypatch.setattr(health.NodeHealthAgent, "post_report", lambda self, r: True)
    monkeypatch.setattr(health.NodeHealthAgent, "run_placement_probes", lambda self: [])
    monkeypatch.setattr(health, "p2p_link_matrix", lambda: {"matrix": {}, "links": []})
    never = health.NodeHealthAgent("http://x", node_name="n", deep_every=1, probe_pairs=False,
                                   p2p_matrix_every=10 ** 9)
    assert never.scalar_probe_every == 0
    assert all("scalar_probe_ok" not in never.run_once()["gpus"]["0"] for _ in range(3))
    assert all("scalar_probe" not in c for c in state["calls"])
    agent = health.NodeHealthAgent("http://x", node_name="n", deep_every=1, probe_pairs=False,
                                   p2p_matrix_every=10 ** 9, scalar_probe_every=2)
    got = [agent.run_once()["gpus"]["0"] for _ in range(4)]
    assert ["scalar_bad_simds" in g for g in got] == [True, False, True, False]
    assert [g["healthy"] for g in got] == [False, True, False, True]
    # only on deep sweeps: every 2nd round is a probe round, every 4th deep
    agent = health.NodeHealthAgent("http://x", node_name="n", deep_every=4, probe_pairs=False,
                                   p2p_matrix_every=10 ** 9, scalar_probe_every=2)
    got = [agent.run_once()["gpus"]["0"] for _ in range(6)]
    assert ["scalar_bad_simds" in g for g in got] == [True, False, False, False, True, False]


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
    monkeypatch.setattr(sys, "argv", ["agent", "--local", "--scalar-probe", "--no-probe-pairs"])
    cli.main()
    assert seen["scalar_probe"] is True and seen["simd_probe"] is False
    assert json.loads(capsys.readouterr().out) == {"gpus": {}}
    monkeypatch.setattr(sys, "argv", ["agent", "--local", "--no-probe-pairs"])
    cli.main()
    assert seen["scalar_probe"] is False

    made = {}

    class FakeAgent:
        def __init__(self, url, **kwargs):
            made.update(kwargs)

        def run_once(self):
            return {}

    monkeypatch.setattr(health, "NodeHealthAgent", FakeAgent)
    monkeypatch.setattr(sys, "argv", ["agent", "--scheduler", "http://x", "--once",
                                      "--scalar-probe-every", "6"])
    cli.main()
    assert made["scalar_probe_every"] == 6
    monkeypatch.setattr(sys, "argv", ["agent", "--scheduler", "http://x", "--once"])
    cli.main()
    assert made["scalar_probe_every"] == 0


def test_health_report_signature_has_the_option_off_by_default():
    import inspect

    sig = inspect.signature(ops.gpu_health_report)
    assert sig.parameters["scalar_probe"].default is False
    sig = inspect.signature(ops.salu_burn_report)
    assert sig.parameters["blocks"].default == 2048 and sig.parameters["inject"].default is None
    # burn rounds are odd by default: the xor checksum cancels over an even count
    from hivedscheduler_amd.ops import scalar_probe

    assert scalar_probe._SALU_DEFAULT_ROUNDS % 2 == 1
    assert set(scalar_probe._SALU_DEFAULT_CHAIN) == set(SALU_SECTIONS)


def test_scalar_bad_simds_reach_the_inspect_view():
    from hivedscheduler_amd.scheduler import HivedScheduler
    from hivedscheduler_amd.sim import mi355x_cluster_config

    sched = HivedScheduler(mi355x_cluster_config(num_nodes=1))
    node = sched.algorithm.all_nodes()[0]
    sched.on_node_add({"metadata": {"name": node, "uid": "n1"}, "spec": {},
                       "status": {"conditions": [{"type": "Ready", "status": "True"}]}})
    bad_simds = [dict(BAD_SIMD)]
    report = {"gpus": {"3": {"healthy": False, "scalar_probe_ok": False, "salu_burn_ok": True,
                             "sgpr_march_ok": False, "scalar_load_ok": True,
                             "scalar_bad_simds": bad_simds}}}
    assert sched.on_health_report(node, report)["applied"] == {"3": False}
    gpu = sched.get_health_reports()[node]["gpus"]["3"]
    assert gpu["scalar_bad_simds"] == bad_simds
    assert gpu["scalar_probe_ok"] is False and gpu["sgpr_march_ok"] is False
    assert gpu["salu_burn_ok"] is True and gpu["scalar_load_ok"] is True
