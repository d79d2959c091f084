"""SIMD probe: the exact VALU burn (ops.valu_burn) and the register-file march
(ops.vgpr_march), attributed per SIMD. See the kernel comments in
hived_ops.hip.
"""
from __future__ import annotations

from .records import (_M32, BadUnits, _fmix32, _rotl32, _u64_fields, checksum_outliers,
                      decode_hw_simd, place_dicts, place_keys, units_seen)

VALU_SECTIONS = ("int", "f32", "f64", "xlane", "trans")
# sections a host mirror reproduces bit for bit; "trans" is consensus only
VALU_EXACT_SECTIONS = ("int", "f32", "f64", "xlane")
_VALU_SECTION_ID = {s: i for i, s in enumerate(VALU_SECTIONS)}
_VALU_DEFAULT_CHAIN = 1024
# odd: every round ends in the same state, so the xor checksum over an even
# number of rounds cancels to zero and a consensus check compares nothing
_VALU_DEFAULT_ROUNDS = 33

VGPR_MARCH_FIRST_REG = 32   # v0..v31 stay the compiler's
VGPR_MARCH_REGS = 480       # v32..v255 and a0..a255, marched per pass
# register indices R (0..255 architectural, 256..511 accumulators) that
# inject target 0 and target 1 flip a bit of
VGPR_MARCH_INJECT_VGPR = 77
VGPR_MARCH_INJECT_AGPR = 256 + 141
_VGPR_MARCH_BLOCKS_PER_CU = 2
# default rounds per workgroup (BENCHMARKS.md "SIMD probe")
_VGPR_MARCH_DEFAULT_ROUNDS = 16


def valu_fma_exact(section: str, a, b, c):
    """a*b + c on integers, as the f32 / f64 section's fma computes it, after
    asserting the bound that makes the floating-point fma exact: a, b < 2^12,
    c < 2^13 and a result <= 2^24 for "f32"; a, b < 2^26, c < 2^52 and a
    result < 2^53 for "f64". Works on Python ints and numpy uint64 arrays."""
    import numpy as np

    ab_bits, c_bits = {"f32": (12, 13), "f64": (26, 52)}[section]
    a, b, c = (np.asarray(v, dtype=np.uint64) for v in (a, b, c))
    if (a >> np.uint64(ab_bits)).any() or (b >> np.uint64(ab_bits)).any() \
            or (c >> np.uint64(c_bits)).any():
        raise AssertionError(f"{section} fma operand too wide for an exact result")
    r = a * b + c
    limit = (1 << 24) + 1 if section == "f32" else 1 << 53
    if (r >= np.uint64(limit)).any():
        raise AssertionError(f"{section} fma result not exactly representable")
    return r


def _valu_seed_states(section: str, seed: int):
    """The 64 seeded states of a section as np.uint64 (the u32 sections use
    the low word only)."""
    import numpy as np

    lane = np.arange(64, dtype=np.uint32)
    start = np.uint32((int(seed) + _VALU_SECTION_ID[section] * 0x9E3779B9) & _M32)
    lo = _fmix32(start + lane * np.uint32(0x85EBCA6B))
    hi = _fmix32(lo ^ np.uint32(0xC2B2AE35))
    if section != "f64":
        return lo.astype(np.uint64)
    return (hi.astype(np.uint64) << np.uint64(32)) | lo.astype(np.uint64)


def _valu_step(section: str, s, c: int):
    """One step of the kernel's ValuStep<section> on the 64 lanes at once,
    integer arithmetic only. s: np.uint32[64], np.uint64[64] for "f64"."""
    import numpy as np

    u32, u64 = np.uint32, np.uint64
    if section == "int":
        lo = s * u32(0x9E3779B1)
        hi = ((s.astype(u64) * u64(0x85EBCA6B)) >> u64(32)).astype(u32)
        # v_mad_u64_u32: 32 x 32 -> 64 plus a 64-bit addend, wrapping at 2^64
        m = lo.astype(u64) * (hi | u32(1)).astype(u64) \
            + ((hi.astype(u64) << u64(32)) | s.astype(u64))
        t = (m.astype(u32) ^ (m >> u64(32)).astype(u32)) + lo
        bfe = (hi >> u32(7)) & u32(0x7FF)
        pop = np.array([bin(int(v)).count("1") for v in lo], dtype=u32)
        return (_rotl32(t, 13) ^ bfe) + pop
    if section == "f32":
        w = s.astype(u64)

        def f(shift, bits):
            return (w >> u64(shift)) & u64((1 << bits) - 1)

        # the 2^k scaling around the scalar fma is exact and leaves no trace
        r0 = valu_fma_exact("f32", f(0, 12), f(12, 12), f(19, 13))
        r1 = valu_fma_exact("f32", f(3, 12), f(16, 12), f(7, 13))
        r2 = valu_fma_exact("f32", f(9, 12), f(1, 12), f(13, 13))
        mix = (r0 + (r1 << u64(5)) + (r2 << u64(9))).astype(u32)
        return (s * u32(0x9E3779B1) + u32(0x7F4A7C15)) ^ mix
    if section == "f64":
        m26 = u64(0x3FFFFFF)
        # ch*2^26 + cl with ch, cl < 2^26: a power-of-two product and a sum
        # below 2^52, exact
        cc = ((s >> u64(38)) << u64(26)) + ((s >> u64(7)) & m26)
        r = valu_fma_exact("f64", s & m26, (s >> u64(26)) & m26, cc)
        return (s * u64(0x9E3779B97F4A7C15) + u64(0xBF58476D1CE4E5B9)) ^ r ^ (r << u64(11))
    if section == "xlane":
        l = np.arange(64)
        x = _rotl32(s, 5) + s[l ^ 1]                          # quad_perm:[1,0,3,2]
        x = _rotl32(x, 7) ^ x[np.where(l % 16 == 0, l, l - 1)]  # row_shr:1
        x = x + _rotl32(x[l ^ 15], 13)                        # row_mirror
        y = _rotl32(x, 3)
        # v_permlane32_swap: x's lanes 32-63 swap with y's lanes 0-31
        nx = np.where(l < 32, x, y[(l - 32) % 64])
        ny = np.where(l < 32, x[(l + 32) % 64], y)
        x = nx + (ny ^ u32(0x9E3779B9))
        x = _rotl32(x, 9) ^ x[(l * 13 + 7) & 63]              # ds_bpermute
        return x + x[(int(c) * 11 + 5) & 63]                  # v_readlane
    raise ValueError(f"section {section!r} has no host mirror")


def valu_burn_expected(section: str, seed: int, chain: int):
    """The 64 states (np.uint64, one per lane) every wave of ops.valu_burn
    must hold after `chain` steps: the host mirror of the kernel, on integers
    only. The f32 and f64 sections assert at every step the bound that makes
    their fma exact (valu_fma_exact). "trans" has no mirror: its low bits are
    hardware-defined."""
    import numpy as np

    if section not in VALU_EXACT_SECTIONS:
        raise ValueError(f"section {section!r} has no host mirror")
    s = _valu_seed_states(section, seed)
    if section != "f64":
        s = s.astype(np.uint32)
    for c in range(int(chain)):
        s = _valu_step(section, s, c)
    return s.astype(np.uint64)


def valu_burn_checksum(section: str, seed: int, chain: int, rounds: int) -> int:
    """The 64-bit xor checksum (record fields [4] low, [5] high) of a healthy
    wave: every round ends in the same state, so it is the xor over the lanes
    for odd `rounds` and 0 for even."""
    import numpy as np

    if int(rounds) % 2 == 0:
        return 0
    return int(np.bitwise_xor.reduce(valu_burn_expected(section, seed, chain)))


def vgpr_march_pattern(seed: int, round: int):
    """The np.uint32[512, 64] pattern p(round, R, lane) the march writes in
    the true polarity: ((R*64 + lane) * 0x9E3779B1 mod 2^32) ^ rs with
    rs = fmix32(seed + round*0x9E3779B9); rows 0..255 are the architectural
    registers, 256..511 the accumulators. The multiply by an odd constant and
    the xor are bijections on 32 bits, so all 32768 values are distinct. The
    complement pass writes ~p. Rows below VGPR_MARCH_FIRST_REG are not
    marched."""
    import numpy as np

    start = np.array([(int(seed) + int(round) * 0x9E3779B9) & _M32], dtype=np.uint32)
    rs = _fmix32(start)[0]
    idx = np.arange(512 * 64, dtype=np.uint32).reshape(512, 64)
    return (idx * np.uint32(0x9E3779B1)) ^ rs


def vgpr_march_wave_sum(seed: int, rounds: int) -> int:
    """Expected record field [6] of every wave: the sum mod 2^32 of the 480
    marched registers x 64 lanes of p over the pattern passes of all rounds."""
    import numpy as np

    total = sum(int(vgpr_march_pattern(seed, r)[VGPR_MARCH_FIRST_REG:].sum(dtype=np.uint64))
                for r in range(int(rounds)))
    return total & _M32


def summarize_valu_burn(records, elapsed_ms: float, section: str, chain: int, rounds: int,
                        expected_simds: int) -> dict:
    """Turn the per-wave records of one ops.valu_burn launch into a verdict.

    records: [waves, 8] int32 rows {hw word, mismatched lane-rounds, first bad
    round (-1), lowest bad lane in it (-1), xor checksum low / high word, two
    reserved}. A wave is bad when it mismatched or when its checksum is not
    the majority's (all a "trans" run can show); it is attributed to the SIMD
    of its hw word. Pure numpy; needs no GPU.
    """
    import numpy as np

    rec = np.asarray(records).reshape(-1, 8).astype(np.int64)
    waves = int(rec.shape[0])
    simds_seen = units_seen(rec[:, 0], decode_hw_simd)
    odd = checksum_outliers(_u64_fields(rec, 4))
    bad = BadUnits()
    for row in rec[(rec[:, 1] != 0) | odd]:
        bad.add(decode_hw_simd(row[0]), {"waves": 1, "mismatched_lane_rounds": row[1]},
                (int(row[2]), int(row[3])) if row[1] != 0 else None)
    bad_simds = bad.entries(("first_bad_round", "first_bad_lane"))
    mismatched_waves = int((rec[:, 1] != 0).sum())
    checksum_spread = bool(odd.any())
    return {
        "section": section,
        "chain": int(chain),
        "rounds": int(rounds),
        "elapsed_ms": float(elapsed_ms),
        "waves": waves,
        "simds_seen": simds_seen,
        "mismatched_waves": mismatched_waves,
        "checksum_spread": checksum_spread,
        "bad_simds": bad_simds,
        "ok": bool(mismatched_waves == 0 and not checksum_spread
                   and simds_seen >= expected_simds),
    }


def summarize_vgpr_march(records, elapsed_ms: float, rounds: int, seed: int,
                         expected_simds: int) -> dict:
    """Turn the per-wave records of one ops.vgpr_march launch into a verdict.

    records: [blocks*4, 8] int32 rows {hw word, mismatched (register, lane)
    pairs, first bad global pass (-1), lowest bad register in it (-1), dropped
    mask, raised mask, sum of the values read in the pattern passes, registers
    marched per pass}. A wave is bad when it counted a mismatch or, which
    would contradict a zero count, reports a dropped or raised bit; it is
    attributed to the SIMD of its hw word.
    At one wave per SIMD the four waves of a block share a CU and hold four
    different SIMD ids; a block that does not is counted in `split_blocks`
    and fails the run (it is also what confirms on hardware that SIMD_ID sits
    at HW_ID[5:4]). `checksum_ok` requires every wave's read sum to be the
    mirror's and every wave to have marched VGPR_MARCH_REGS registers. Pure
    numpy; needs no GPU.
    """
    import numpy as np

    rec = np.asarray(records).reshape(-1, 4, 8).astype(np.int64)
    blocks = int(rec.shape[0])
    want_sum = vgpr_march_wave_sum(seed, rounds)
    simds_seen = units_seen(rec[:, :, 0], decode_hw_simd)
    checksum_ok = bool(((rec[:, :, 6] & _M32) == want_sum).all()
                       and (rec[:, :, 7] == VGPR_MARCH_REGS).all())
    split_blocks = 0
    bad = BadUnits()
    for blk in rec:
        places = [decode_hw_simd(w) for w in blk[:, 0]]
        if len({p[:4] for p in places}) != 1 or len({p[4] for p in places}) != 4:
            split_blocks += 1
        for place, row in zip(places, blk):
            # a set mask bit with a zero count contradicts itself: bad as well
            if row[1] == 0 and row[4] == 0 and row[5] == 0:
                continue
            bad.add(place, {"waves": 1, "mismatched_registers": row[1]},
                    (int(row[2]), int(row[3])) if row[2] >= 0 else None,
                    {"dropped_mask": int(row[4]) & _M32, "raised_mask": int(row[5]) & _M32})
    bad_simds = bad.entries(("first_bad_pass", "first_bad_reg"))
    mismatched_waves = int(((rec[:, :, 1] != 0) | (rec[:, :, 4] != 0)
                            | (rec[:, :, 5] != 0)).sum())
    return {
        "elapsed_ms": float(elapsed_ms),
        "blocks": blocks,
        "waves": 4 * blocks,
        "simds_seen": simds_seen,
        "mismatched_waves": mismatched_waves,
        "checksum_ok": checksum_ok,
        "split_blocks": split_blocks,
        "bad_simds": bad_simds,
        "ok": bool(mismatched_waves == 0 and checksum_ok and split_blocks == 0
                   and simds_seen >= expected_simds),
    }


def valu_burn_report(device: int = 0, sections=VALU_SECTIONS, blocks: int = 2048,
                     chain: int = None, rounds: int = None, seed: int = 1,
                     inject=None) -> dict:
    """Run the VALU burn for each section on one GPU.

    Returns {"sections": {section: summarize_valu_burn(...)}, "ok",
    "bad_simds"} where `ok` is the AND and `bad_simds` the union ((xcc, se,
    sh, cu, simd) dicts, sorted) over sections. The exact sections compare
    against the host mirror; "trans" is consensus between waves only: it can
    name a SIMD that disagrees, not a fault common to all of them, and it
    needs an odd `rounds` (the default is; the extension refuses an even one
    too) because the xor checksum of an even number of identical rounds is
    zero. `inject=(wave, round, lane,
    bit)` xors that bit into that lane's state in that wave at that round (a
    harmless register-only fault) to exercise the detection path on healthy
    hardware.
    """
    import torch

    chain = _VALU_DEFAULT_CHAIN if chain is None else int(chain)
    rounds = _VALU_DEFAULT_ROUNDS if rounds is None else int(rounds)
    if "trans" in sections and rounds % 2 == 0:
        raise ValueError("section 'trans' needs an odd number of rounds")
    from . import _ops_on

    ops = _ops_on(device)
    inject_args = (-1, -1, -1, -1) if inject is None else tuple(int(v) for v in inject)
    expected_simds = 4 * ops.device_info(device)["multiProcessorCount"]
    out: dict = {"blocks": blocks, "chain": chain, "rounds": rounds, "sections": {}}
    bad = set()
    for section in sections:
        if section in VALU_EXACT_SECTIONS:
            want = valu_burn_expected(section, seed, chain)
            expected = torch.from_numpy(want.view("int64").copy()).cuda(device)
        else:
            expected = torch.empty(0, dtype=torch.int64)
        records, ms = ops.valu_burn(expected, section, seed, blocks, chain, rounds, *inject_args)
        s = summarize_valu_burn(records.cpu().numpy(), ms, section, chain, rounds, expected_simds)
        out["sections"][section] = s
        bad |= place_keys(s["bad_simds"], 5)
    out["ok"] = all(s["ok"] for s in out["sections"].values())
    out["bad_simds"] = place_dicts(bad)
    return out


def vgpr_march_report(device: int = 0, blocks: int = None, rounds: int = None, seed: int = 1,
                      inject=None) -> dict:
    """Run the register-file march on one GPU and summarise it.

    The kernel allocates all 512 vector registers per lane, so one wave is
    resident per SIMD (the extension asserts it; `blocks_per_cu` is what the
    occupancy query said) and marches 480 of them: v0..v31 hold the kernel's
    own values and are exercised by the VALU burn instead. The default grid is
    two workgroups per CU and the default rounds keep the launch at about a
    millisecond, during which tenant waves wait for a SIMD. `inject=(wave,
    target, lane, bit, pass)` flips that bit of that lane of register
    VGPR_MARCH_INJECT_VGPR (target 0) or VGPR_MARCH_INJECT_AGPR (target 1) in
    that wave between the write and the read of that global pass (round*2 +
    polarity): registers only, to exercise detection and attribution on
    healthy hardware.
    """
    from . import _ops_on

    ops = _ops_on(device)
    cus = ops.device_info(device)["multiProcessorCount"]
    blocks = _VGPR_MARCH_BLOCKS_PER_CU * cus if blocks is None else int(blocks)
    rounds = _VGPR_MARCH_DEFAULT_ROUNDS if rounds is None else int(rounds)
    inject_args = (-1, 0, 0, 0, -1) if inject is None else tuple(int(v) for v in inject)
    records, ms, per_cu = ops.vgpr_march(blocks, rounds, seed, *inject_args)
    out = summarize_vgpr_march(records.cpu().numpy(), ms, rounds, seed, 4 * cus)
    out["rounds"] = rounds
    out["registers_per_pass"] = VGPR_MARCH_REGS
    out["blocks_per_cu"] = int(per_cu)
    return out


def simd_probe_report(device: int = 0) -> dict:
    """Both SIMD probes at their default shapes: {"valu": valu_burn_report,
    "vgpr_march": vgpr_march_report, "ok", "bad_simds"}, `ok` the AND and
    `bad_simds` the union of the two."""
    valu = valu_burn_report(device)
    march = vgpr_march_report(device)
    bad = place_keys(valu["bad_simds"], 5) | place_keys(march["bad_simds"], 5)
    return {"valu": valu, "vgpr_march": march, "ok": bool(valu["ok"] and march["ok"]),
            "bad_simds": place_dicts(bad)}
