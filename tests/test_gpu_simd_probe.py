"""GPU tests for the SIMD probe: the exact VALU burn (ops.valu_burn) against
its host mirror per section, a live compare, consensus of the transcendental
section, injected one-bit faults and their per-SIMD attribution; the register
march (ops.vgpr_march) clean, its read sum, occupancy and SIMD placement, and
injected faults in a VGPR and an AGPR in both polarities; argument checks; the
default shapes and the health-report wiring. Everything is bitwise: no
tolerance."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

needs_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")

BLOCKS = 8  # 32 waves
SEED = 5
M32 = 0xFFFFFFFF
EXACT = ("int", "f32", "f64", "xlane")
NO_INJECT = (-1, -1, -1, -1)


@functools.lru_cache(maxsize=None)
def expected_on_gpu(section, chain):
    from hivedscheduler_amd.ops import valu_burn_expected

    if section == "trans":
        return torch.empty(0, dtype=torch.int64)
    want = valu_burn_expected(section, SEED, chain)
    return torch.from_numpy(want.view("int64").copy()).cuda()


@functools.lru_cache(maxsize=None)
def burn(section, chain, rounds, expected_chain=None, inject=NO_INJECT):
    """Records [32, 8] as int64 of one launch, compared against the mirror of
    `expected_chain` steps (default: `chain`); each distinct launch runs once
    and is shared."""
    from hivedscheduler_amd.ops import get_ops

    want = expected_on_gpu(section, chain if expected_chain is None else expected_chain)
    records, ms = get_ops().valu_burn(want, section, SEED, BLOCKS, chain, rounds, *inject)
    assert records.shape == (BLOCKS * 4, 8) and records.dtype == torch.int32
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
@pytest.mark.parametrize("section", EXACT)
def test_burn_matches_the_host_mirror(section):
    from hivedscheduler_amd.ops import valu_burn_checksum

    for chain, rounds in ((3, 2), (3, 3), (1, 1)):
        rec = burn(section, chain, rounds)
        assert_clean_burn(rec)
        want = valu_burn_checksum(section, SEED, chain, rounds)
        assert checksums(rec) == [want] * (BLOCKS * 4), (chain, rounds, hex(want))
    # the xor over three equal rounds is the xor over the lanes: not zero
    assert valu_burn_checksum(section, SEED, 3, 3) != 0
    assert valu_burn_checksum(section, SEED, 3, 2) == 0


@needs_gpu
@pytest.mark.parametrize("section", EXACT)
def test_burn_compare_is_live(section):
    """Three steps judged against the mirror of four: all 64 lanes mismatch in
    every round on every wave."""
    rounds = 2
    rec = burn(section, 3, rounds, expected_chain=4)
    assert (rec[:, 1] == 64 * rounds).all(), rec[:, 1]
    assert (rec[:, 2] == 0).all() and (rec[:, 3] == 0).all()


@needs_gpu
def test_trans_is_a_consensus_between_waves():
    from hivedscheduler_amd.ops import decode_hw_simd, get_ops, summarize_valu_burn

    rec = burn("trans", 3, 3)
    assert_clean_burn(rec)
    sums = checksums(rec)
    assert len(set(sums)) == 1 and sums[0] != 0, [hex(s) for s in sums]
    # a second launch gives the same bits
    again, _ = get_ops().valu_burn(expected_on_gpu("trans", 3), "trans", SEED, BLOCKS, 3, 3)
    assert checksums(again.cpu().numpy().astype(np.int64)) == sums
    s = summarize_valu_burn(rec, 1.0, "trans", 3, 3, expected_simds=1)
    assert s["ok"] is True and s["checksum_spread"] is False and s["bad_simds"] == []
    # one injected bit: exactly that wave disagrees, and its SIMD is named
    wave, bit = 5, 3
    bad = burn("trans", 3, 3, inject=(wave, 1, 17, bit))
    assert_clean_burn(bad)  # nothing is compared in this section
    got = checksums(bad)
    assert [w for w in range(BLOCKS * 4) if got[w] != sums[0]] == [wave]
    assert got[wave] == sums[0] ^ (1 << bit)
    s = summarize_valu_burn(bad, 1.0, "trans", 3, 3, expected_simds=1)
    assert s["ok"] is False and s["checksum_spread"] is True and s["mismatched_waves"] == 0
    assert [(b["xcc"], b["se"], b["sh"], b["cu"], b["simd"]) for b in s["bad_simds"]] == [
        decode_hw_simd(bad[wave, 0])]


@needs_gpu
@pytest.mark.parametrize("section,bit", [("int", 9), ("f32", 31), ("f64", 40), ("xlane", 0)])
def test_burn_injection_names_one_simd(section, bit):
    from hivedscheduler_amd.ops import decode_hw_simd, summarize_valu_burn, valu_burn_checksum

    wave, rnd, lane, rounds = 5, 1, 17, 3  # odd rounds: the checksum does not cancel
    rec = burn(section, 3, rounds, inject=(wave, rnd, lane, bit))
    assert tuple(rec[wave, 1:4]) == (1, rnd, lane), rec[wave]
    assert_clean_burn(rec, [w for w in range(BLOCKS * 4) if w != wave])
    want = valu_burn_checksum(section, SEED, 3, rounds)
    got = checksums(rec)
    assert got[wave] == want ^ (1 << bit)
    assert all(got[w] == want for w in range(BLOCKS * 4) if w != wave)
    s = summarize_valu_burn(rec, 1.0, section, 3, rounds, expected_simds=1)
    assert s["ok"] is False and s["mismatched_waves"] == 1 and s["checksum_spread"] is True
    xcc, se, sh, cu, simd = decode_hw_simd(rec[wave, 0])
    assert s["bad_simds"] == [{"xcc": xcc, "se": se, "sh": sh, "cu": cu, "simd": simd,
                               "waves": 1, "mismatched_lane_rounds": 1,
                               "first_bad_round": rnd, "first_bad_lane": lane}]


# --------------------------------------------------------------------------
# register march
# --------------------------------------------------------------------------
MARCH_BLOCKS, MARCH_ROUNDS = 4, 2
NO_MARCH_INJECT = (-1, 0, 0, 0, -1)


@functools.lru_cache(maxsize=None)
def march(inject=NO_MARCH_INJECT):
    """(records [16, 8] int64, workgroups per CU) of one launch."""
    from hivedscheduler_amd.ops import get_ops

    records, ms, per_cu = get_ops().vgpr_march(MARCH_BLOCKS, MARCH_ROUNDS, SEED, *inject)
    assert records.shape == (MARCH_BLOCKS * 4, 8) and records.dtype == torch.int32
    assert ms > 0
    rec = records.cpu().numpy().astype(np.int64)
    rec.setflags(write=False)
    return rec, per_cu


def assert_clean_march(rec, rows):
    from hivedscheduler_amd.ops import vgpr_march_wave_sum

    want = vgpr_march_wave_sum(SEED, MARCH_ROUNDS)
    for w in rows:
        assert tuple(rec[w, 1:6]) == (0, -1, -1, 0, 0), (w, rec[w])
        assert int(rec[w, 6]) & M32 == want, (w, hex(int(rec[w, 6]) & M32), hex(want))
        assert rec[w, 7] == 480


@needs_gpu
def test_march_clean_run():
    from hivedscheduler_amd.ops import decode_hw_simd, summarize_vgpr_march

    rec, per_cu = march()
    assert per_cu == 1
    assert_clean_march(rec, range(MARCH_BLOCKS * 4))
    # one wave per SIMD: the four waves of a block share a CU and sit on four
    # different SIMDs, which also confirms SIMD_ID at HW_ID[5:4] on gfx950
    for blk in rec.reshape(MARCH_BLOCKS, 4, 8):
        places = [decode_hw_simd(w) for w in blk[:, 0]]
        assert len({p[:4] for p in places}) == 1, places
        assert {p[4] for p in places} == {0, 1, 2, 3}, places
    s = summarize_vgpr_march(rec, 1.0, MARCH_ROUNDS, SEED, expected_simds=4)
    assert s["ok"] is True and s["split_blocks"] == 0 and s["checksum_ok"] is True
    assert s["bad_simds"] == [] and s["simds_seen"] >= 4


@needs_gpu
@pytest.mark.parametrize("target", [0, 1])
@pytest.mark.parametrize("pas", [0, 3])
def test_march_injection(target, pas):
    """One bit flipped in the fixed VGPR (target 0) or AGPR (target 1) between
    write and read of a pattern pass (0) and of a complement pass (3): in pass
    0 a bit the register holds at 1, in pass 3 one it holds at 0."""
    from hivedscheduler_amd.ops import (VGPR_MARCH_INJECT_AGPR, VGPR_MARCH_INJECT_VGPR,
                                        decode_hw_simd, summarize_vgpr_march,
                                        vgpr_march_pattern, vgpr_march_wave_sum)

    wave, lane = 6, 21
    reg = (VGPR_MARCH_INJECT_VGPR, VGPR_MARCH_INJECT_AGPR)[target]
    held = int(vgpr_march_pattern(SEED, pas // 2)[reg, lane]) ^ (M32 if pas & 1 else 0)
    want_one = pas == 0
    bit = next(b for b in range(32) if bool((held >> b) & 1) == want_one)
    rec, _ = march((wave, target, lane, bit, pas))
    assert int(rec[:, 1].sum()) == 1
    assert tuple(rec[wave, 1:4]) == (1, pas, reg), rec[wave]
    dropped, raised = int(rec[wave, 4]) & M32, int(rec[wave, 5]) & M32
    assert (dropped, raised) == ((1 << bit, 0) if want_one else (0, 1 << bit))
    assert rec[wave, 7] == 480
    # pass 0 is summed, and the register read back without the bit it held;
    # pass 3 holds the complement, which the sum leaves out
    want_sum = vgpr_march_wave_sum(SEED, MARCH_ROUNDS)
    assert int(rec[wave, 6]) & M32 == ((want_sum - (1 << bit)) & M32 if pas == 0 else want_sum)
    assert_clean_march(rec, [w for w in range(MARCH_BLOCKS * 4) if w != wave])
    s = summarize_vgpr_march(rec, 1.0, MARCH_ROUNDS, SEED, expected_simds=4)
    assert s["ok"] is False and s["mismatched_waves"] == 1 and s["split_blocks"] == 0
    assert s["checksum_ok"] is (pas != 0)
    xcc, se, sh, cu, simd = decode_hw_simd(rec[wave, 0])
    assert s["bad_simds"] == [{"xcc": xcc, "se": se, "sh": sh, "cu": cu, "simd": simd,
                               "waves": 1, "mismatched_registers": 1, "first_bad_pass": pas,
                               "first_bad_reg": reg, "dropped_mask": dropped,
                               "raised_mask": raised}]


@needs_gpu
def test_argument_checks():
    from hivedscheduler_amd.ops import get_ops

    ops = get_ops()
    want = expected_on_gpu("int", 3)
    for bad in (dict(section="fp16"), dict(blocks=0), dict(blocks=2 ** 20 + 1), dict(chain=0),
                dict(rounds=0), dict(chain=2 ** 12, rounds=2 ** 11),
                dict(inject_wave=BLOCKS * 4), dict(inject_wave=-2), dict(inject_round=2),
                dict(inject_round=-2), dict(inject_lane=64), dict(inject_lane=-2),
                dict(inject_bit=32), dict(inject_bit=-2), dict(inject_bit=-1),
                dict(expected=want[:63]), dict(expected=want.to(torch.int32)),
                dict(expected=want.cpu()), dict(expected=torch.empty(0, dtype=torch.int64))):
        args = dict(expected=want, section="int", seed=SEED, blocks=BLOCKS, chain=3, rounds=2,
                    inject_wave=1, inject_round=0, inject_lane=5, inject_bit=0)
        args.update(bad)
        with pytest.raises(RuntimeError):
            ops.valu_burn(**args)
    # trans has only its checksum, which cancels over an even number of rounds
    with pytest.raises(RuntimeError):
        ops.valu_burn(expected_on_gpu("trans", 3), "trans", SEED, BLOCKS, 3, 2)
    # the f64 state has 64 bits, the others 32
    with pytest.raises(RuntimeError):
        ops.valu_burn(expected_on_gpu("f64", 3), "f64", SEED, BLOCKS, 3, 2, 1, 0, 5, 64)
    for bad in (dict(blocks=0), dict(blocks=2 ** 16 + 1), dict(rounds=0),
                dict(blocks=2 ** 16, rounds=2 ** 20),
                dict(inject_wave=MARCH_BLOCKS * 4), dict(inject_wave=-2),
                dict(inject_target=2), dict(inject_target=-1),
                dict(inject_lane=64), dict(inject_lane=-1),
                dict(inject_bit=32), dict(inject_bit=-1),
                dict(inject_pass=MARCH_ROUNDS * 2), dict(inject_pass=-2)):
        args = dict(blocks=MARCH_BLOCKS, rounds=MARCH_ROUNDS, seed=SEED, inject_wave=1,
                    inject_target=0, inject_lane=5, inject_bit=0, inject_pass=0)
        args.update(bad)
        with pytest.raises(RuntimeError):
            ops.vgpr_march(**args)


@needs_gpu
def test_default_shapes_cover_every_simd():
    from hivedscheduler_amd.ops import VALU_SECTIONS, get_ops, simd_probe_report

    simds = 4 * get_ops().device_info(0)["multiProcessorCount"]
    rep = simd_probe_report(0)
    m = rep["vgpr_march"]
    print(f"vgpr_march: {m['elapsed_ms']:.3f} ms, {m['blocks']} blocks x {m['rounds']} rounds, "
          f"simds_seen {m['simds_seen']}")
    for section in VALU_SECTIONS:
        s = rep["valu"]["sections"][section]
        print(f"valu_burn {section}: {s['elapsed_ms']:.3f} ms, {s['waves']} waves x "
              f"{s['rounds']} rounds x {s['chain']} steps, simds_seen {s['simds_seen']}")
    assert rep["ok"] is True, rep
    assert rep["bad_simds"] == []
    assert m["ok"] is True and m["simds_seen"] >= simds and m["split_blocks"] == 0
    assert m["blocks_per_cu"] == 1 and m["registers_per_pass"] == 480
    assert set(rep["valu"]["sections"]) == set(VALU_SECTIONS)
    for section in VALU_SECTIONS:
        s = rep["valu"]["sections"][section]
        assert s["ok"] is True and s["simds_seen"] >= simds, (section, s)
        assert s["mismatched_waves"] == 0 and s["checksum_spread"] is False


@needs_gpu
def test_health_report_probe_wiring():
    from hivedscheduler_amd.ops import gpu_health_report

    plain = gpu_health_report(0, quick=True)
    rep = gpu_health_report(0, quick=True, simd_probe=True)
    assert rep["simd_probe"]["ok"] is True and rep["healthy"] is True
    assert "simd_probe" not in plain
    assert set(rep) - set(plain) == {"simd_probe"}
