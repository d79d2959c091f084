"""GPU tests for the scalar probe: the exact SALU burn (ops.salu_burn) against
its host mirror per section, a live compare, injected one-bit faults and their
per-SIMD attribution; the SGPR march (ops.sgpr_march) clean, its per-wave read
sum, and injected faults in both polarities; the scalar-load check
(ops.scalar_load_check) clean and with a flipped bit in either row of the
uploaded pattern; argument checks; the default shapes and the health-report
wiring. Everything is bitwise: no tolerance."""
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
SECTIONS = ("s32", "s64", "ctl", "mask")
NO_INJECT = (-1, -1, -1, -1)


def units(section):
    return 64 if section == "mask" else 8


@functools.lru_cache(maxsize=None)
def expected_on_gpu(section, chain):
    from hivedscheduler_amd.ops import salu_burn_expected

    want = salu_burn_expected(section, SEED, chain)
    return torch.from_numpy(want.view("int64").copy()).cuda()


@functools.lru_cache(maxsize=None)
def burn(section, chain, rounds, expected_chain=None, inject=NO_INJECT):
    """Records [32, 8] as int64 of one launch, compared against the mirror of
    `expected_chain` steps (default: `chain`); each distinct launch runs once
    and is shared."""
    from hivedscheduler_amd.ops import get_ops

    want = expected_on_gpu(section, chain if expected_chain is None else expected_chain)
    records, ms = get_ops().salu_burn(want, section, SEED, BLOCKS, chain, rounds, *inject)
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
        assert tuple(rec[w, 6:8]) == (0, 0)


@needs_gpu
@pytest.mark.parametrize("section", SECTIONS)
def test_burn_matches_the_host_mirror(section):
    from hivedscheduler_amd.ops import salu_burn_checksum

    for chain, rounds in ((3, 2), (3, 3), (1, 1)):
        rec = burn(section, chain, rounds)
        want = salu_burn_checksum(section, SEED, chain, rounds)
        print(section, chain, rounds, "checksum", hex(checksums(rec)[0]), "mirror", hex(want))
        assert_clean_burn(rec)
        assert checksums(rec) == [want] * WAVES, (chain, rounds, hex(want))
    assert salu_burn_checksum(section, SEED, 3, 3) != 0
    assert salu_burn_checksum(section, SEED, 3, 2) == 0


@needs_gpu
@pytest.mark.parametrize("section", SECTIONS)
def test_burn_compare_is_live(section):
    """Three steps judged against the mirror of four: every chain (lane)
    mismatches in every round on every wave."""
    rounds = 2
    rec = burn(section, 3, rounds, expected_chain=4)
    assert (rec[:, 1] == units(section) * rounds).all(), rec[:, 1]
    assert (rec[:, 2] == 0).all() and (rec[:, 3] == 0).all()


@needs_gpu
@pytest.mark.parametrize("section,unit,bit", [("s32", 6, 9), ("s64", 3, 40), ("ctl", 0, 31),
                                              ("mask", 17, 0)])
def test_burn_injection_names_one_simd(section, unit, bit):
    from hivedscheduler_amd.ops import decode_hw_simd, salu_burn_checksum, summarize_salu_burn

    wave, rnd, rounds = 5, 1, 3  # odd rounds: the checksum does not cancel
    rec = burn(section, 3, rounds, inject=(wave, rnd, unit, bit))
    assert tuple(rec[wave, 1:4]) == (1, rnd, unit), rec[wave]
    assert_clean_burn(rec, [w for w in range(WAVES) if w != wave])
    want = salu_burn_checksum(section, SEED, 3, rounds)
    got = checksums(rec)
    assert got[wave] == want ^ (1 << bit)
    assert all(got[w] == want for w in range(WAVES) if w != wave)
    s = summarize_salu_burn(rec, 1.0, section, 3, rounds, expected_simds=1)
    assert s["ok"] is False and s["mismatched_waves"] == 1 and s["checksum_spread"] is True
    xcc, se, sh, cu, simd = decode_hw_simd(rec[wave, 0])
    assert s["bad_simds"] == [{"xcc": xcc, "se": se, "sh": sh, "cu": cu, "simd": simd,
                               "waves": 1, "mismatched_chain_rounds": 1,
                               "first_bad_round": rnd, "first_bad_chain": unit}]


# --------------------------------------------------------------------------
# SGPR march
# --------------------------------------------------------------------------
MARCH_BLOCKS, MARCH_ROUNDS = 4, 2
MARCH_WAVES = MARCH_BLOCKS * 4
NO_MARCH_INJECT = (-1, 0, -1)


@functools.lru_cache(maxsize=None)
def march(inject=NO_MARCH_INJECT):
    """(records [16, 8] int64, waves per SIMD by the occupancy query) of one
    launch."""
    from hivedscheduler_amd.ops import get_ops

    records, ms, per_simd = get_ops().sgpr_march(MARCH_BLOCKS, MARCH_ROUNDS, SEED, *inject)
    assert records.shape == (MARCH_WAVES, 8) and records.dtype == torch.int32
    assert ms > 0
    rec = records.cpu().numpy().astype(np.int64)
    rec.setflags(write=False)
    return rec, per_simd


def assert_clean_march(rec, rows):
    from hivedscheduler_amd.ops import sgpr_march_wave_sum

    for w in rows:
        want = sgpr_march_wave_sum(SEED, MARCH_ROUNDS, w)
        assert tuple(rec[w, 1:6]) == (0, -1, -1, 0, 0), (w, rec[w])
        assert int(rec[w, 6]) & M32 == want, (w, hex(int(rec[w, 6]) & M32), hex(want))
        assert rec[w, 7] == 70


@needs_gpu
def test_march_clean_run():
    from hivedscheduler_amd.ops import summarize_sgpr_march

    rec, per_simd = march()
    print("sgpr_march occupancy query, waves per SIMD:", per_simd)
    assert per_simd >= 1  # reported, not judged: the query over-reports for this kernel
    assert_clean_march(rec, range(MARCH_WAVES))
    # every wave holds different data: the sums differ
    assert len({int(v) & M32 for v in rec[:, 6]}) == MARCH_WAVES
    s = summarize_sgpr_march(rec, 1.0, MARCH_ROUNDS, SEED, expected_simds=4)
    assert s["ok"] is True and s["checksum_ok"] is True
    assert s["bad_simds"] == [] and s["simds_seen"] >= 4


@needs_gpu
@pytest.mark.parametrize("pas", [0, 3])
def test_march_injection(pas):
    """One bit of s77 flipped between write and read of a pattern pass (0) and
    of a complement pass (3): in pass 0 a bit the register holds at 1, in pass
    3 one it holds at 0."""
    from hivedscheduler_amd.ops import (SGPR_MARCH_INJECT_REG, decode_hw_simd,
                                        sgpr_march_pattern, sgpr_march_wave_sum,
                                        summarize_sgpr_march)

    wave, reg = 6, SGPR_MARCH_INJECT_REG
    held = int(sgpr_march_pattern(SEED, pas // 2, wave)[reg]) ^ (M32 if pas & 1 else 0)
    want_one = pas == 0
    bit = next(b for b in range(32) if bool((held >> b) & 1) == want_one)
    rec, _ = march((wave, bit, pas))
    assert int(rec[:, 1].sum()) == 1
    assert tuple(rec[wave, 1:4]) == (1, pas, 77), rec[wave]
    dropped, raised = int(rec[wave, 4]) & M32, int(rec[wave, 5]) & M32
    assert (dropped, raised) == ((1 << bit, 0) if want_one else (0, 1 << bit))
    assert rec[wave, 7] == 70
    # pass 0 is summed, and the register read back without the bit it held;
    # pass 3 holds the complement, which the sum leaves out
    want_sum = sgpr_march_wave_sum(SEED, MARCH_ROUNDS, wave)
    assert int(rec[wave, 6]) & M32 == ((want_sum - (1 << bit)) & M32 if pas == 0 else want_sum)
    assert_clean_march(rec, [w for w in range(MARCH_WAVES) if w != wave])
    s = summarize_sgpr_march(rec, 1.0, MARCH_ROUNDS, SEED, expected_simds=4)
    assert s["ok"] is False and s["mismatched_waves"] == 1
    assert s["checksum_ok"] is (pas != 0)
    xcc, se, sh, cu, simd = decode_hw_simd(rec[wave, 0])
    assert s["bad_simds"] == [{"xcc": xcc, "se": se, "sh": sh, "cu": cu, "simd": simd,
                               "waves": 1, "mismatched_registers": 1, "first_bad_pass": pas,
                               "first_bad_reg": 77, "dropped_mask": dropped,
                               "raised_mask": raised}]


# --------------------------------------------------------------------------
# scalar-load check
# --------------------------------------------------------------------------
# 64 words: the smallest buffer in which the x16 load runs at more than one
# offset per row; five rounds use every width once
WORDS, LOAD_ROUNDS = 64, 5


@functools.lru_cache(maxsize=None)
def load_check(flip=None):
    """Records [32, 8] int64 of one launch; flip = (row, word, bit) flips
    that bit in the uploaded pattern."""
    from hivedscheduler_amd.ops import get_ops, scalar_load_pattern

    pattern = scalar_load_pattern(SEED, WORDS).copy()
    if flip is not None:
        row, word, bit = flip
        pattern[row, word] ^= np.uint32(1 << bit)
    dev = torch.from_numpy(pattern.view(np.int32)).cuda()
    records, ms = get_ops().scalar_load_check(dev, SEED, BLOCKS, LOAD_ROUNDS)
    assert records.shape == (WAVES, 8) and records.dtype == torch.int32
    assert ms > 0
    rec = records.cpu().numpy().astype(np.int64)
    rec.setflags(write=False)
    return rec


def row0_sum():
    from hivedscheduler_amd.ops import scalar_load_pattern

    return int(scalar_load_pattern(SEED, WORDS)[0].sum(dtype=np.uint64))


@needs_gpu
def test_load_clean_run():
    from hivedscheduler_amd.ops import summarize_scalar_load

    rec = load_check()
    want = (LOAD_ROUNDS * row0_sum()) & M32
    for w in range(WAVES):
        assert tuple(rec[w, 1:6]) == (0, -1, -1, 0, 0), (w, rec[w])
        assert int(rec[w, 6]) & M32 == want and rec[w, 7] == 2 * WORDS
    s = summarize_scalar_load(rec, 1.0, LOAD_ROUNDS, SEED, WORDS, expected_simds=4)
    assert s["ok"] is True and s["checksum_ok"] is True and s["bad_simds"] == []


@needs_gpu
@pytest.mark.parametrize("row,word,bit", [(0, 37, 12), (1, 50, 31)])
def test_load_finds_a_flipped_bit_in_every_wave(row, word, bit):
    """One bit flipped in the uploaded pattern: every wave finds it in every
    round (every width), at the right word, in the right direction."""
    from hivedscheduler_amd.ops import scalar_load_pattern, summarize_scalar_load

    held = int(scalar_load_pattern(SEED, WORDS)[row, word])
    was_one = bool((held >> bit) & 1)
    rec = load_check((row, word, bit))
    clean_sum = LOAD_ROUNDS * row0_sum()
    if row == 0:  # row 0 is summed as read
        clean_sum += LOAD_ROUNDS * (-(1 << bit) if was_one else (1 << bit))
    for w in range(WAVES):
        assert tuple(rec[w, 1:4]) == (LOAD_ROUNDS, 0, row * WORDS + word), (w, rec[w])
        dropped, raised = int(rec[w, 4]) & M32, int(rec[w, 5]) & M32
        assert (dropped, raised) == ((1 << bit, 0) if was_one else (0, 1 << bit))
        assert int(rec[w, 6]) & M32 == clean_sum & M32 and rec[w, 7] == 2 * WORDS
    s = summarize_scalar_load(rec, 1.0, LOAD_ROUNDS, SEED, WORDS, expected_simds=4)
    assert s["ok"] is False and s["mismatched_waves"] == WAVES
    assert s["checksum_ok"] is (row == 1)
    assert all(b["first_bad_word"] == row * WORDS + word and b["first_bad_round"] == 0
               for b in s["bad_simds"])


@needs_gpu
def test_argument_checks():
    from hivedscheduler_amd.ops import get_ops, scalar_load_pattern

    ops = get_ops()
    want = expected_on_gpu("s32", 3)
    for bad in (dict(section="s16"), dict(blocks=0), dict(blocks=2 ** 20 + 1), dict(chain=0),
                dict(rounds=0), dict(chain=2 ** 10, rounds=2 ** 9),
                dict(inject_wave=WAVES), dict(inject_wave=-2), dict(inject_round=2),
                dict(inject_round=-2), dict(inject_chain=8), dict(inject_chain=-2),
                dict(inject_bit=32), dict(inject_bit=-2), dict(inject_bit=-1),
                dict(expected=want[:7]), dict(expected=want.to(torch.int32)),
                dict(expected=want.cpu()), dict(expected=torch.empty(0, dtype=torch.int64)),
                dict(expected=expected_on_gpu("mask", 3))):
        args = dict(expected=want, section="s32", seed=SEED, blocks=BLOCKS, chain=3, rounds=2,
                    inject_wave=1, inject_round=0, inject_chain=5, inject_bit=0)
        args.update(bad)
        with pytest.raises(RuntimeError):
            ops.salu_burn(**args)
    # the s64 state has 64 bits, the others 32; mask has 64 lanes and wants 64 values
    with pytest.raises(RuntimeError):
        ops.salu_burn(expected_on_gpu("s64", 3), "s64", SEED, BLOCKS, 3, 2, 1, 0, 5, 64)
    with pytest.raises(RuntimeError):
        ops.salu_burn(expected_on_gpu("mask", 3), "mask", SEED, BLOCKS, 3, 2, 1, 0, 64, 0)
    with pytest.raises(RuntimeError):
        ops.salu_burn(want, "mask", SEED, BLOCKS, 3, 2)
    for bad in (dict(blocks=0), dict(blocks=2 ** 20 + 1), dict(rounds=0),
                dict(blocks=2 ** 20, rounds=2 ** 8), dict(rounds=2 ** 27 + 1),
                dict(inject_wave=MARCH_WAVES), dict(inject_wave=-2),
                dict(inject_bit=32), dict(inject_bit=-1),
                dict(inject_pass=MARCH_ROUNDS * 2), dict(inject_pass=-2)):
        args = dict(blocks=MARCH_BLOCKS, rounds=MARCH_ROUNDS, seed=SEED, inject_wave=1,
                    inject_bit=0, inject_pass=0)
        args.update(bad)
        with pytest.raises(RuntimeError):
            ops.sgpr_march(**args)

    def pattern(words):
        return torch.from_numpy(scalar_load_pattern(SEED, words).view(np.int32)).cuda()

    good = pattern(WORDS)
    wide = pattern(2 * WORDS)
    for bad in (dict(blocks=0), dict(blocks=2 ** 20 + 1), dict(rounds=0),
                dict(blocks=2 ** 20, rounds=2 ** 9), dict(rounds=2 ** 24 + 1),
                dict(pattern=pattern(8)), dict(pattern=pattern(72)), dict(pattern=pattern(4112)),
                dict(pattern=good.view(-1)), dict(pattern=good.view(4, WORDS // 2)),
                dict(pattern=good.to(torch.int64)), dict(pattern=good.float()),
                dict(pattern=good.cpu()), dict(pattern=wide[:, ::2]),
                dict(pattern=wide[:, :WORDS])):
        args = dict(pattern=good, seed=SEED, blocks=BLOCKS, rounds=LOAD_ROUNDS)
        args.update(bad)
        with pytest.raises(RuntimeError):
            ops.scalar_load_check(**args)


@needs_gpu
def test_default_shapes_cover_every_simd():
    from hivedscheduler_amd.ops import SALU_SECTIONS, get_ops, scalar_probe_report

    simds = 4 * get_ops().device_info(0)["multiProcessorCount"]
    rep = scalar_probe_report(0)
    m, l = rep["sgpr_march"], rep["scalar_load"]
    for section in SALU_SECTIONS:
        s = rep["salu"]["sections"][section]
        print(f"salu_burn {section}: {s['elapsed_ms']:.3f} ms, {s['waves']} waves x "
              f"{s['rounds']} rounds x {s['chain']} steps, simds_seen {s['simds_seen']}")
    print(f"sgpr_march: {m['elapsed_ms']:.3f} ms, {m['blocks']} blocks x {m['rounds']} rounds, "
          f"simds_seen {m['simds_seen']}, occupancy query {m['waves_per_simd']} waves/SIMD")
    print(f"scalar_load: {l['elapsed_ms']:.3f} ms, {l['blocks']} blocks x {l['rounds']} rounds x "
          f"{l['words']} words, simds_seen {l['simds_seen']}")
    assert rep["ok"] is True, rep
    assert rep["bad_simds"] == []
    assert set(rep["salu"]["sections"]) == set(SALU_SECTIONS)
    for section in SALU_SECTIONS:
        s = rep["salu"]["sections"][section]
        assert s["ok"] is True and s["simds_seen"] >= simds, (section, s)
        assert s["mismatched_waves"] == 0 and s["checksum_spread"] is False
        assert s["rounds"] % 2 == 1
    assert m["ok"] is True and m["simds_seen"] >= simds and m["registers_per_pass"] == 70
    assert m["checksum_ok"] is True and m["waves_per_simd"] >= 1
    assert l["ok"] is True and l["simds_seen"] >= simds and l["checksum_ok"] is True


@needs_gpu
def test_health_report_probe_wiring():
    from hivedscheduler_amd.ops import gpu_health_report

    plain = gpu_health_report(0, quick=True)
    rep = gpu_health_report(0, quick=True, scalar_probe=True)
    assert rep["scalar_probe"]["ok"] is True and rep["healthy"] is True
    assert "scalar_probe" not in plain
    assert set(rep) - set(plain) == {"scalar_probe"}
