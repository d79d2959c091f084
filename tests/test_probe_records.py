"""The per-wave summarisers against frozen outputs, and the pieces they share
(hivedscheduler_amd/ops/records.py). CPU only.

tests/golden/probe_summaries.json holds what the summarisers returned for
exactly these hand-built records before they were rebuilt on the shared
module; equality covers keys, key order, values and value types.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from hivedscheduler_amd import ops

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "probe_summaries.json")
SEED, ROUNDS = 1, 1


def hw_word(xcc, se, sh, cu, simd=0):
    return (xcc << 16) | (se << 13) | (sh << 12) | (cu << 8) | (simd << 4)


def burn_records():
    """Two blocks of four waves, [8, 4]: two bad waves on one CU (the later
    wave failed earlier), one on another CU, the rest clean."""
    rec = np.zeros((8, 4), dtype=np.int32)
    rec[:, 0] = [hw_word(0, 1, 0, 3)] * 4 + [hw_word(5, 2, 1, 9)] * 2 + [hw_word(2, 0, 0, 1)] * 2
    rec[:, 2] = -1
    rec[:, 3] = 0x1234567
    rec[1] = [hw_word(0, 1, 0, 3), 5, 3, 0x1234566]
    rec[2] = [hw_word(0, 1, 0, 3), 2, 1, 0x1234565]
    rec[6] = [hw_word(2, 0, 0, 1), 1, 7, 0x1234567]
    return rec


def lds_records():
    """Two blocks, [8, 8]: block 0 clean with the mirror's checksum, block 1
    with two bad waves (masks and a first tuple each) and a wrong checksum."""
    rec = np.zeros((8, 8), dtype=np.int32)
    rec[:4, 0] = hw_word(1, 3, 1, 7)
    rec[4:, 0] = hw_word(6, 0, 0, 12)
    rec[:, 2:4] = -1
    want = ops.lds_march_block_checksum(SEED, ROUNDS)
    rec[0, 6] = np.uint32(want).astype(np.int32)
    rec[4, 6] = np.uint32(want).astype(np.int32)
    rec[5] = [hw_word(6, 0, 0, 12), 3, 2, 4097, 0x10, 0, 0, 0]
    rec[7] = [hw_word(6, 0, 0, 12), 1, 1, 40000, 0, np.int32(-2**31), 17, 0]
    return rec


def valu_records():
    """Two blocks, [8, 8]: a mismatching wave with a first tuple, a wave that
    only disagrees in its checksum, the rest clean."""
    rec = np.zeros((8, 8), dtype=np.int32)
    for w in range(8):
        rec[w, 0] = hw_word(w // 4, 2, 0, 5, w % 4)
    rec[:, 2:4] = -1
    rec[:, 4] = np.int32(-0x1234568)
    rec[:, 5] = 0x0BADCAFE
    rec[2, 1:4] = [4, 6, 33]
    rec[2, 4] = 99
    rec[5, 5] = 0x0BADCAFF
    return rec


def vgpr_records():
    """Two blocks, [8, 8]: a clean block, and a block with one bad wave (masks
    and a first tuple) and one wave that reports mask bits with a zero
    count."""
    rec = np.zeros((8, 8), dtype=np.int32)
    for w in range(8):
        rec[w, 0] = hw_word(3 + w // 4, 1, 1, 2, w % 4)
    rec[:, 2:4] = -1
    rec[:, 6] = np.uint32(ops.vgpr_march_wave_sum(SEED, ROUNDS)).astype(np.int32)
    rec[:, 7] = ops.VGPR_MARCH_REGS
    rec[5, 1:6] = [64, 1, ops.VGPR_MARCH_INJECT_AGPR, 0, 0x400]
    rec[6, 4] = 0x8
    return rec


def summaries():
    """name -> summariser output for the records above."""
    return {
        "burn": ops.summarize_burn(burn_records(), 2.0, "bf16", 16, 4, 3),
        "lds_march": ops.summarize_lds_march(lds_records(), 0.5, ROUNDS, SEED, 2),
        "valu_burn": ops.summarize_valu_burn(valu_records(), 0.25, "int", 8, 3, 8),
        "vgpr_march": ops.summarize_vgpr_march(vgpr_records(), 0.125, ROUNDS, SEED, 8),
    }


def ordered(value):
    """Dicts as lists of pairs, so that a comparison sees the key order."""
    if isinstance(value, dict):
        return [(k, ordered(v)) for k, v in value.items()]
    if isinstance(value, list):
        return [ordered(v) for v in value]
    return value


@pytest.mark.parametrize("name", ["burn", "lds_march", "valu_burn", "vgpr_march"])
def test_summary_matches_frozen_output(name):
    with open(GOLDEN) as f:
        want = json.load(f)[name]
    got = summaries()[name]
    assert got == want
    assert ordered(got) == ordered(want)
    # same value types too: JSON keeps bool, int and float apart
    assert json.loads(json.dumps(got)) == got
    assert [type(v) for _, v in ordered(got)] == [type(v) for _, v in ordered(want)]


def test_frozen_cases_are_the_intended_ones():
    """The fixture exercises what it is meant to: clean and bad waves, masks,
    a first tuple, and for the register march mask bits with a zero count."""
    s = summaries()
    assert [c["first_bad_round"] for c in s["burn"]["bad_cus"]] == [1, 7]
    assert s["burn"]["checksum_spread"] and not s["burn"]["ok"]
    (cu,) = s["lds_march"]["bad_cus"]
    assert (cu["first_bad_pass"], cu["first_bad_word"]) == (1, 40000)
    assert (cu["dropped_mask"], cu["raised_mask"]) == (0x10, 0x80000000)
    assert s["lds_march"]["mismatched_blocks"] == 1 and not s["lds_march"]["checksum_ok"]
    firsts = [(c["simd"], c["first_bad_round"], c["first_bad_lane"])
              for c in s["valu_burn"]["bad_simds"]]
    assert firsts == [(2, 6, 33), (1, -1, -1)]
    silent, loud = sorted(s["vgpr_march"]["bad_simds"], key=lambda c: c["mismatched_registers"])
    assert silent["mismatched_registers"] == 0 and silent["dropped_mask"] == 0x8
    assert (silent["first_bad_pass"], silent["first_bad_reg"]) == (-1, -1)
    assert loud["first_bad_reg"] == ops.VGPR_MARCH_INJECT_AGPR and loud["raised_mask"] == 0x400
    assert s["vgpr_march"]["mismatched_waves"] == 2 and s["vgpr_march"]["checksum_ok"]


def test_bad_units_accumulates_and_orders():
    from hivedscheduler_amd.ops.records import BadUnits, place_dicts, place_keys

    bad = BadUnits()
    bad.add((1, 0, 0, 2), {"waves": 1, "n": 3}, (4, 9), {"mask": 0x1})
    bad.add((0, 7, 1, 15), {"waves": 1, "n": 0}, None, {"mask": 0x2})
    bad.add((1, 0, 0, 2), {"waves": 1, "n": 2}, (4, 2), {"mask": 0x4})
    first, second = bad.entries(("p", "i"))
    assert list(first.items()) == [("xcc", 0), ("se", 7), ("sh", 1), ("cu", 15), ("waves", 1),
                                   ("n", 0), ("p", -1), ("i", -1), ("mask", 2)]
    assert second == {"xcc": 1, "se": 0, "sh": 0, "cu": 2, "waves": 2, "n": 5, "p": 4, "i": 2,
                      "mask": 5}
    assert place_dicts(place_keys([first, second, dict(second)], 4)) == [
        {"xcc": 0, "se": 7, "sh": 1, "cu": 15}, {"xcc": 1, "se": 0, "sh": 0, "cu": 2}]


def test_checksum_outliers_and_units_seen():
    from hivedscheduler_amd.ops.records import checksum_outliers, units_seen

    sums = np.array([7, 7, 9, 7], dtype=np.int64)
    assert checksum_outliers(sums).tolist() == [False, False, True, False]
    assert checksum_outliers(sums[:0]).tolist() == []
    words = np.array([hw_word(0, 1, 0, 3, 0), hw_word(0, 1, 0, 3, 2), hw_word(4, 1, 0, 3, 0)])
    assert units_seen(words, ops.decode_hw_word) == 2
    assert units_seen(words, ops.decode_hw_simd) == 3


def test_importing_ops_does_not_import_torch():
    code = ("import sys; import hivedscheduler_amd.ops as o; "
            "assert callable(o.summarize_burn) and callable(o.simd_probe_report); "
            "print(sorted(m for m in ('torch', 'numpy') if m in sys.modules))")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", code], cwd=root, capture_output=True, text=True,
                         check=True)
    assert out.stdout.strip() == "[]"
