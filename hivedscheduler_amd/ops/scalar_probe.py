"""Scalar probe: the exact SALU burn (ops.salu_burn), the SGPR march
(ops.sgpr_march) and the scalar-load check (ops.scalar_load_check), attributed
per SIMD. See the kernel comments in hived_ops.hip.

A CU has one scalar ALU shared by its four SIMDs and one SGPR file per SIMD,
so an ALU fault is expected to name all four SIMDs of a CU and a register
fault one. That expectation comes from the architecture description; it has
not been measured on a faulty part.
"""
from __future__ import annotations

from .records import (_M32, _M64, BadUnits, _fmix32, _u64_fields, checksum_outliers,
                      decode_hw_simd, place_dicts, place_keys, units_seen)

SALU_SECTIONS = ("s32", "s64", "ctl", "mask")
SALU_CHAINS = 8  # independent states per wave in s32, s64 and ctl; mask has one per lane
_SALU_SECTION_ID = {s: i for i, s in enumerate(SALU_SECTIONS)}
# per section, so that each timed launch takes tens of milliseconds at the
# default grid (BENCHMARKS.md "Scalar probe")
_SALU_DEFAULT_CHAIN = {"s32": 64, "s64": 64, "ctl": 64, "mask": 1024}
# odd: every round ends in the same state, so the xor checksum over an even
# number of rounds cancels to zero
_SALU_DEFAULT_ROUNDS = 33

SGPR_MARCH_FIRST_REG = 32  # s0..s31 stay the compiler's
SGPR_MARCH_REGS = 70       # s32..s101, marched per pass
SGPR_MARCH_INJECT_REG = 77
_SGPR_MARCH_BLOCKS_PER_CU = 8
# about a millisecond at eight workgroups per CU (BENCHMARKS.md "Scalar probe")
_SGPR_MARCH_DEFAULT_ROUNDS = 32

_SCALAR_LOAD_DEFAULT_WORDS = 1024
_SCALAR_LOAD_DEFAULT_ROUNDS = 5  # each of the five widths once
_SCALAR_LOAD_DEFAULT_BLOCKS = 2048

_K = 0x9E3779B1


# --------------------------------------------------------------------------
# SALU instructions on Python ints (u32 / u64 values in, u32 / u64 out)
# --------------------------------------------------------------------------
def _i32(x: int) -> int:
    return x - (1 << 32) if x & 0x80000000 else x


def _i64(x: int) -> int:
    return x - (1 << 64) if x & (1 << 63) else x


def _sext(x: int, bits: int) -> int:
    """The low `bits` of x, sign-extended, as a Python int."""
    x &= (1 << bits) - 1
    return x - (1 << bits) if x >> (bits - 1) else x


def _add(a: int, b: int, carry: int = 0):
    r = a + b + carry
    return r & _M32, r >> 32


def _sub(a: int, b: int, borrow: int = 0):
    r = a - b - borrow
    return r & _M32, int(r < 0)


def _brev(x: int, bits: int) -> int:
    return int(format(x, f"0{bits}b")[::-1], 2)


def _ff1(x: int) -> int:
    """Index of the lowest set bit, -1 (all ones) when there is none."""
    return (x & -x).bit_length() - 1 if x else _M32


def _flbit(x: int, bits: int) -> int:
    """Zeros above the highest set bit, -1 (all ones) when there is none."""
    return bits - x.bit_length() if x else _M32


def _wqm64(x: int) -> int:
    out = 0
    for q in range(16):
        if (x >> (4 * q)) & 0xF:
            out |= 0xF << (4 * q)
    return out


def _salu_seed(section: str, seed: int, index: int) -> int:
    """valu_seed_state(seed, section id, index) of the kernel: the low word
    for the u32 sections, both words for s64."""
    import numpy as np

    start = (int(seed) + _SALU_SECTION_ID[section] * 0x9E3779B9 + index * 0x85EBCA6B) & _M32
    lo = int(_fmix32(np.array([start], dtype=np.uint32))[0])
    hi = int(_fmix32(np.array([lo ^ 0xC2B2AE35], dtype=np.uint32))[0])
    return (hi << 32) | lo if section == "s64" else lo


def _step_s32(s: int) -> int:
    a = (s * _K) & _M32
    b = (s * 0x85EBCA6B) >> 32
    c = ((_i32(s) * _i32(0xC2B2AE35)) >> 32) & _M32
    a, cy = _add(a, b)
    b, cy = _add(b, c, cy)
    c, bw = _sub(c, a)
    a, bw = _sub(a, b, bw)
    c, _ = _add(c, s, bw)
    d = (a << (b & 31)) & _M32
    d ^= c >> (a & 31)
    d = (d + (_i32(b) >> (c & 31))) & _M32
    d ^= (a >> 7) & 0x7FF                                  # s_bfe_u32, offset 7 width 11
    d = (d + _sext(c >> 5, 13)) & _M32                     # s_bfe_i32, offset 5 width 13
    d = ((bin(b).count("1") << 1) + d) & _M32              # s_lshl1_add_u32
    d = ((_ff1(c) << 2) + d) & _M32
    d = ((_flbit(a, 32) << 3) + d) & _M32
    e = _brev(b, 32)
    d = (((e << 4) + d) & _M32) ^ e
    d = (d + abs(_sext(a, 16) - _sext(c, 8))) & _M32       # s_absdiff_i32
    e = (min(_i32(a), _i32(b)) & _M32) ^ (max(_i32(a), _i32(c)) & _M32)
    e = (e + min(b, c)) & _M32
    e ^= max(a, d)
    d = (d + e) & _M32
    e = ((b & 0xFFFF) << 16 | (a & 0xFFFF)) ^ ((c & 0xFFFF0000) | (b & 0xFFFF))  # pack ll, lh
    e = (e + ((a & 0xFFFF0000) | (c >> 16))) & _M32        # pack hh
    d ^= e
    e = (c & ~(1 << (a & 31))) | (1 << (b & 31))           # s_bitset0 then s_bitset1
    d = (d + (e & _M32)) & _M32
    e = (a & ~b & _M32) ^ ((b | ~c) & _M32)                # andn2, orn2
    e = (e + (~(c & a) & _M32)) & _M32                     # nand
    e ^= ~(a | d) & _M32                                   # nor
    e = (e + (~(b ^ d) & _M32)) & _M32                     # xnor
    d ^= e
    return (d + 0x7F4A7C15) & _M32


def _step_s64(s: int) -> int:
    A = ((s << 13) & _M64) ^ (s >> 7)
    A ^= (_i64(s) >> 17) & _M64
    B = (s >> 9) & ((1 << 40) - 1)                         # s_bfe_u64, offset 9 width 40
    C = _sext(A >> 17, 29) & _M64                          # s_bfe_i64, offset 17 width 29
    A = (A + B) & _M64                                     # s_add_u32 + s_addc_u32
    D = (A & C) ^ (B | C)
    D ^= A & ~B & _M64
    D ^= ~(s & C) & _M64
    D ^= ~(A | s) & _M64
    D ^= ~(B ^ s) & _M64
    D ^= _brev(~C & _M64, 64)
    D ^= _wqm64(B)
    e = bin(A).count("1")
    f = _ff1(D)
    g = _flbit(C, 64)
    bit = s & 1
    h = e if bit == ((A >> 3) & 1) else f                  # s_cmp_eq_u64, s_cselect_b32
    g = g if bit != ((B >> 5) & 1) else e                  # s_cmp_lg_u64, s_cselect_b32
    e = ((e << 8) & _M32) ^ f
    dlo, cy = _add(D & _M32, h)
    dhi, _ = _add(D >> 32, g, cy)
    dhi ^= e
    dlo, cy = _add(dlo, 0x7F4A7C15)
    dhi, _ = _add(dhi, 0x9E3779B9, cy)
    return (dhi << 32) | dlo


def _step_ctl(s: int):
    """(new state, first branch taken, second branch taken)."""
    a = (_i32(s) * 0x6B43) & _M32                          # s_mulk_i32
    a = (a + 0x7C15) & _M32                                # s_addk_i32
    b = (s >> 15) ^ a
    P, Q = (a << 32) | b, (b << 32) | s
    c, e, g, h = a & 3, b & 3, a >> 16, b >> 16
    d = 0x1B                                               # s_movk_i32
    f = -12059 & _M32                                      # s_movk_i32, sign-extended
    sa, sb, ss = _i32(a), _i32(b), _i32(s)
    outcomes = []
    outcomes.append(c == e)
    n = a if outcomes[-1] else b                           # s_cselect_b32
    outcomes.append(c != 2)
    if outcomes[-1]:
        f = h                                              # s_cmov_b32
    outcomes.append(sa > sb)
    R = P if outcomes[-1] else Q                           # s_cselect_b64
    outcomes += [sb >= ss, sa < ss, ss <= sb,
                 e == 1, c != e, a > b, b >= s, s < a, h <= g,
                 (a >> (b & 31)) & 1 == 0, (b >> (a & 31)) & 1 == 1,  # s_bitcmp0, s_bitcmp1
                 c == 1, e != 2, sa > 0x1234, sb >= -4660, sa < -28672, sb <= 0x7000,
                 e == 3, c != 0, g > 0x8000, h >= 0x4000, g < 0xC000, h <= 0x2000]
    for o in outcomes:
        d = (d + d + int(bool(o))) & _M32                  # s_addc_u32 d, d, d
    n ^= f
    arm1 = bool((s >> 7) & 1)
    if arm1:
        n = ((n * _K) + d) & _M32
    else:
        n = ((n - d) & _M32) ^ a
    arm2 = n < b
    if not arm2:
        n = ((~n & _M32) + h) & _M32
    n ^= R & _M32
    return (n + (R >> 32)) & _M32, arm1, arm2


def _step_mask(s, c: int):
    """One step of the mask section on the 64 lanes at once (np.uint32[64])."""
    import numpy as np

    u32 = np.uint32
    inside = ((s >> u32(c & 31)) & u32(1)).astype(bool)
    m = sum(1 << l for l in range(64) if inside[l])
    pc = bin(m).count("1")
    ff = (m & -m).bit_length()                             # 0 for an empty mask, else 1 + index
    s = np.where(inside, s * u32(_K) + u32(pc),
                 (s ^ (s >> u32(15))) * u32(0x85EBCA6B) + u32(ff))
    first = int(s[0])                                      # v_readfirstlane: all lanes active
    return s + u32(first ^ (m & _M32) ^ (m >> 32))


def salu_burn_expected(section: str, seed: int, chain: int):
    """The states (np.uint64) every wave of ops.salu_burn must hold after
    `chain` steps: SALU_CHAINS of them for "s32", "s64" and "ctl", 64 (one per
    lane) for "mask". The host mirror of the kernel, on integers only."""
    import numpy as np

    if section not in SALU_SECTIONS:
        raise ValueError(f"section must be one of {SALU_SECTIONS}; got {section!r}")
    if section == "mask":
        s = np.array([_salu_seed(section, seed, l) for l in range(64)], dtype=np.uint32)
        for c in range(int(chain)):
            s = _step_mask(s, c)
        return s.astype(np.uint64)
    out = []
    for k in range(SALU_CHAINS):
        s = _salu_seed(section, seed, k)
        for _ in range(int(chain)):
            s = {"s32": _step_s32, "s64": _step_s64,
                 "ctl": lambda v: _step_ctl(v)[0]}[section](s)
        out.append(s)
    return np.array(out, dtype=np.uint64)


def salu_ctl_arms(seed: int, chain: int) -> set:
    """The (branch, taken) pairs the eight "ctl" chains go through in `chain`
    steps from `seed`; all four of {(1, True), (1, False), (2, True),
    (2, False)} when both arms of both branches occur."""
    arms = set()
    for k in range(SALU_CHAINS):
        s = _salu_seed("ctl", seed, k)
        for _ in range(int(chain)):
            s, arm1, arm2 = _step_ctl(s)
            arms |= {(1, arm1), (2, arm2)}
    return arms


def salu_burn_checksum(section: str, seed: int, chain: int, rounds: int) -> int:
    """The 64-bit xor checksum (record fields [4] low, [5] high) of a healthy
    wave: the xor over the chains (lanes) for odd `rounds`, 0 for even."""
    import numpy as np

    if int(rounds) % 2 == 0:
        return 0
    return int(np.bitwise_xor.reduce(salu_burn_expected(section, seed, chain)))


def sgpr_march_pattern(seed: int, round: int, wave: int):
    """The np.uint32[102] pattern p(round, R, wave) register sR of global wave
    `wave` holds in the true polarity: ((wave*128 + R) * 0x9E3779B1 mod 2^32)
    ^ rs with rs = fmix32(seed + round*0x9E3779B9). The multiply by an odd
    constant is a bijection, so the values are distinct across registers and
    across the waves of a launch. The complement pass writes ~p. Entries below
    SGPR_MARCH_FIRST_REG are not marched."""
    import numpy as np

    start = np.array([(int(seed) + int(round) * 0x9E3779B9) & _M32], dtype=np.uint32)
    rs = _fmix32(start)[0]
    idx = (np.arange(102, dtype=np.uint64) + np.uint64(int(wave) * 128)).astype(np.uint32)
    return (idx * np.uint32(_K)) ^ rs


def sgpr_march_wave_sum(seed: int, rounds: int, wave: int) -> int:
    """Expected record field [6] of wave `wave`: the sum mod 2^32 of its 70
    marched registers of p over the pattern passes of all rounds."""
    import numpy as np

    total = sum(int(sgpr_march_pattern(seed, r, wave)[SGPR_MARCH_FIRST_REG:].sum(dtype=np.uint64))
                for r in range(int(rounds)))
    return total & _M32


def scalar_load_pattern(seed: int, words: int):
    """The np.uint32[2, words] buffer ops.scalar_load_check reads: row 0 word
    i is fmix32(seed ^ (i*0x85EBCA6B)), row 1 its complement."""
    import numpy as np

    i = np.arange(int(words), dtype=np.uint32)
    row = _fmix32(np.uint32(int(seed) & _M32) ^ (i * np.uint32(0x85EBCA6B)))
    return np.stack([row, ~row])


# --------------------------------------------------------------------------
# summarisers
# --------------------------------------------------------------------------
def summarize_salu_burn(records, elapsed_ms: float, section: str, chain: int, rounds: int,
                        expected_simds: int) -> dict:
    """Turn the per-wave records of one ops.salu_burn launch into a verdict.

    records: [waves, 8] int32 rows {hw word, mismatched chain-rounds
    (lane-rounds for "mask"), first bad round (-1), lowest bad chain or lane
    in it (-1), xor checksum low / high word, two reserved}. A wave is bad
    when it mismatched or when its checksum is not the majority's; it is
    attributed to the SIMD of its hw word. Pure numpy; needs no GPU.
    """
    import numpy as np

    rec = np.asarray(records).reshape(-1, 8).astype(np.int64)
    simds_seen = units_seen(rec[:, 0], decode_hw_simd)
    odd = checksum_outliers(_u64_fields(rec, 4))
    bad = BadUnits()
    for row in rec[(rec[:, 1] != 0) | odd]:
        bad.add(decode_hw_simd(row[0]), {"waves": 1, "mismatched_chain_rounds": row[1]},
                (int(row[2]), int(row[3])) if row[1] != 0 else None)
    mismatched_waves = int((rec[:, 1] != 0).sum())
    checksum_spread = bool(odd.any())
    return {
        "section": section,
        "chain": int(chain),
        "rounds": int(rounds),
        "elapsed_ms": float(elapsed_ms),
        "waves": int(rec.shape[0]),
        "simds_seen": simds_seen,
        "mismatched_waves": mismatched_waves,
        "checksum_spread": checksum_spread,
        "bad_simds": bad.entries(("first_bad_round", "first_bad_chain")),
        "ok": bool(mismatched_waves == 0 and not checksum_spread
                   and simds_seen >= expected_simds),
    }


def _summarize_masked(rec, want_sums, want_count: int, count_key: str, first_keys,
                      elapsed_ms: float, expected_simds: int) -> dict:
    """What the march's and the load check's records share: {hw word,
    mismatches, first bad pass or round (-1), lowest bad unit in it (-1),
    dropped mask, raised mask, read sum, units per pass}. A wave is bad when
    it counted a mismatch or, which would contradict a zero count, reports a
    dropped or raised bit."""
    simds_seen = units_seen(rec[:, 0], decode_hw_simd)
    checksum_ok = bool(((rec[:, 6] & _M32) == want_sums).all()
                       and (rec[:, 7] == want_count).all())
    flagged = (rec[:, 1] != 0) | (rec[:, 4] != 0) | (rec[:, 5] != 0)
    bad = BadUnits()
    for row in rec[flagged]:
        bad.add(decode_hw_simd(row[0]), {"waves": 1, count_key: row[1]},
                (int(row[2]), int(row[3])) if row[2] >= 0 else None,
                {"dropped_mask": int(row[4]) & _M32, "raised_mask": int(row[5]) & _M32})
    mismatched_waves = int(flagged.sum())
    return {
        "elapsed_ms": float(elapsed_ms),
        "waves": int(rec.shape[0]),
        "simds_seen": simds_seen,
        "mismatched_waves": mismatched_waves,
        "checksum_ok": checksum_ok,
        "bad_simds": bad.entries(first_keys),
        "ok": bool(mismatched_waves == 0 and checksum_ok and simds_seen >= expected_simds),
    }


def summarize_sgpr_march(records, elapsed_ms: float, rounds: int, seed: int,
                         expected_simds: int) -> dict:
    """Turn the per-wave records of one ops.sgpr_march launch into a verdict.

    records: [waves, 8] int32 rows {hw word, mismatched registers, first bad
    global pass (-1), lowest bad register in it (-1), dropped mask, raised
    mask, sum of the values read in the pattern passes, registers marched per
    pass}; row w is global wave w, whose pattern and read sum differ from
    every other wave's. `checksum_ok` requires every wave's read sum to be its
    mirror's and every wave to have marched SGPR_MARCH_REGS registers. Pure
    numpy; needs no GPU.
    """
    import numpy as np

    rec = np.asarray(records).reshape(-1, 8).astype(np.int64)
    want = np.array([sgpr_march_wave_sum(seed, rounds, w) for w in range(rec.shape[0])],
                    dtype=np.int64)
    return _summarize_masked(rec, want, SGPR_MARCH_REGS, "mismatched_registers",
                             ("first_bad_pass", "first_bad_reg"), elapsed_ms, expected_simds)


def summarize_scalar_load(records, elapsed_ms: float, rounds: int, seed: int, words: int,
                          expected_simds: int) -> dict:
    """Turn the per-wave records of one ops.scalar_load_check launch into a
    verdict.

    records: [waves, 8] int32 rows {hw word, mismatched words, first bad round
    (-1), lowest bad word in it as row*W + index (-1), dropped mask, raised
    mask, sum of the row-0 words read, words read per round}. `checksum_ok`
    requires every wave's sum to be `rounds` times the sum of row 0 of
    scalar_load_pattern(seed, words) and 2*words words per round. Pure numpy;
    needs no GPU.
    """
    import numpy as np

    rec = np.asarray(records).reshape(-1, 8).astype(np.int64)
    row0 = int(scalar_load_pattern(seed, words)[0].sum(dtype=np.uint64))
    want = (row0 * int(rounds)) & _M32
    return _summarize_masked(rec, want, 2 * int(words), "mismatched_words",
                             ("first_bad_round", "first_bad_word"), elapsed_ms, expected_simds)


# --------------------------------------------------------------------------
# reports (these launch kernels)
# --------------------------------------------------------------------------
def salu_burn_report(device: int = 0, sections=SALU_SECTIONS, blocks: int = 2048,
                     chain: int = None, rounds: int = None, seed: int = 1,
                     inject=None) -> dict:
    """Run the SALU burn for each section on one GPU.

    Returns {"sections": {section: summarize_salu_burn(...)}, "ok",
    "bad_simds"} where `ok` is the AND and `bad_simds` the union ((xcc, se,
    sh, cu, simd) dicts, sorted) over sections. Every section compares against
    the host mirror. `chain` defaults per section (the steps differ in
    length). `inject=(wave, round, chain, bit)` xors that bit into that chain
    (lane, for "mask") of that wave at that round: a harmless register-only
    fault that exercises the detection path on healthy hardware.
    """
    import torch

    from . import _ops_on

    rounds = _SALU_DEFAULT_ROUNDS if rounds is None else int(rounds)
    ops = _ops_on(device)
    inject_args = (-1, -1, -1, -1) if inject is None else tuple(int(v) for v in inject)
    expected_simds = 4 * ops.device_info(device)["multiProcessorCount"]
    out: dict = {"blocks": blocks, "rounds": rounds, "sections": {}}
    bad = set()
    for section in sections:
        steps = _SALU_DEFAULT_CHAIN[section] if chain is None else int(chain)
        want = salu_burn_expected(section, seed, steps)
        expected = torch.from_numpy(want.view("int64").copy()).cuda(device)
        records, ms = ops.salu_burn(expected, section, seed, blocks, steps, rounds, *inject_args)
        s = summarize_salu_burn(records.cpu().numpy(), ms, section, steps, rounds, expected_simds)
        out["sections"][section] = s
        bad |= place_keys(s["bad_simds"], 5)
    out["ok"] = all(s["ok"] for s in out["sections"].values())
    out["bad_simds"] = place_dicts(bad)
    return out


def sgpr_march_report(device: int = 0, blocks: int = None, rounds: int = None, seed: int = 1,
                      inject=None) -> dict:
    """Run the SGPR march on one GPU and summarise it.

    The SGPR file is 800 entries per SIMD and a wave gets its allocation, not
    the file: the march verifies the SGPR_MARCH_REGS registers each wave was
    given, in both polarities. The default grid is eight workgroups per CU,
    more than a CU holds at once, so that the waves resident on a SIMD
    together hold most of the file; which entries they hold is the hardware's
    choice and is not verified. `waves_per_simd` is the occupancy query's
    answer, reported and not judged (it over-reports for SGPR-heavy kernels).
    `inject=(wave, bit, pass)` flips that bit of s77 in that wave between the
    write and the read of that global pass (round*2 + polarity): registers
    only.
    """
    from . import _ops_on

    ops = _ops_on(device)
    cus = ops.device_info(device)["multiProcessorCount"]
    blocks = _SGPR_MARCH_BLOCKS_PER_CU * cus if blocks is None else int(blocks)
    rounds = _SGPR_MARCH_DEFAULT_ROUNDS if rounds is None else int(rounds)
    inject_args = (-1, 0, -1) if inject is None else tuple(int(v) for v in inject)
    records, ms, per_simd = ops.sgpr_march(blocks, rounds, seed, *inject_args)
    out = summarize_sgpr_march(records.cpu().numpy(), ms, rounds, seed, 4 * cus)
    out["blocks"] = blocks
    out["rounds"] = rounds
    out["registers_per_pass"] = SGPR_MARCH_REGS
    out["waves_per_simd"] = int(per_simd)
    return out


def scalar_load_report(device: int = 0, blocks: int = _SCALAR_LOAD_DEFAULT_BLOCKS,
                       words: int = _SCALAR_LOAD_DEFAULT_WORDS,
                       rounds: int = _SCALAR_LOAD_DEFAULT_ROUNDS, seed: int = 1) -> dict:
    """Run the scalar-load check on one GPU and summarise it.

    Every wave reads the [2, words] pattern (row 1 the complement) through the
    scalar data cache with s_load_dword, x2, x4, x8 and x16, one width per
    round. This verifies the data bits of the scalar load path in both
    polarities and that all five widths return the right words; it does not
    march the cells of the scalar cache, which a kernel cannot choose.
    """
    import torch

    from . import _ops_on

    ops = _ops_on(device)
    cus = ops.device_info(device)["multiProcessorCount"]
    pattern = torch.from_numpy(scalar_load_pattern(seed, words).view("int32").copy()).cuda(device)
    records, ms = ops.scalar_load_check(pattern, seed, blocks, rounds)
    out = summarize_scalar_load(records.cpu().numpy(), ms, rounds, seed, words, 4 * cus)
    out["blocks"] = int(blocks)
    out["rounds"] = int(rounds)
    out["words"] = int(words)
    return out


def scalar_probe_report(device: int = 0) -> dict:
    """The three parts at their default shapes: {"salu": salu_burn_report,
    "sgpr_march": sgpr_march_report, "scalar_load": scalar_load_report, "ok",
    "bad_simds"}, `ok` the AND and `bad_simds` the union of the three."""
    parts = {"salu": salu_burn_report(device), "sgpr_march": sgpr_march_report(device),
             "scalar_load": scalar_load_report(device)}
    bad = set().union(*(place_keys(p["bad_simds"], 5) for p in parts.values()))
    return {**parts, "ok": all(p["ok"] for p in parts.values()), "bad_simds": place_dicts(bad)}
