"""GPU tests for the full-LDS march (ops.lds_march): a clean run with the host
checksum, an injected one-bit fault at both ends of the 160 KiB and just past
the 64 KiB that lds_check reaches, both polarities, the wide-read path, later
rounds, per-CU attribution, argument checks, and coverage and GB/s
plausibility at the default shape. Everything is bitwise: no tolerance."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

needs_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")

BLOCKS = 8  # 32 waves
SEED = 3
WORDS = 40960
M32 = 0xFFFFFFFF


@functools.lru_cache(maxsize=None)
def march(rounds=1, block=-1, word=-1, pas=-1, bit=0):
    """Records [BLOCKS, 4 waves, 8] as int64 of one launch; each distinct
    launch runs once and is shared."""
    from hivedscheduler_amd.ops import get_ops

    records, ms = get_ops().lds_march(BLOCKS, rounds, SEED, block, word, pas, bit)
    assert records.shape == (BLOCKS * 4, 8) and records.dtype == torch.int32
    assert ms > 0
    rec = records.cpu().numpy().astype(np.int64).reshape(BLOCKS, 4, 8)
    rec.setflags(write=False)
    return rec


def block_checksums(rec):
    return [int(b[:, 6].sum()) & M32 for b in rec]


def assert_single_fault(rec, block, word, pas, rounds):
    """Exactly one mismatched dword, in the injected block only, at the
    injected (pass, word); returns the (dropped, raised) masks of the block."""
    from hivedscheduler_amd.ops import lds_march_block_checksum

    assert int(rec[:, :, 1].sum()) == 1, rec[:, :, 1]
    assert int(rec[block, :, 1].sum()) == 1
    hit = rec[block][rec[block, :, 1] == 1][0]
    assert (int(hit[2]), int(hit[3])) == (pas, word), hit
    # every other wave of every block is clean
    clean = rec[:, :, 1] == 0
    assert (rec[:, :, 2][clean] == -1).all() and (rec[:, :, 3][clean] == -1).all()
    assert (rec[:, :, 4][clean] == 0).all() and (rec[:, :, 5][clean] == 0).all()
    assert rec[:, :, 7].max() == 0 and rec[:, :, 7].min() == 0
    want = lds_march_block_checksum(SEED, rounds)
    sums = block_checksums(rec)
    assert all(s == want for b, s in enumerate(sums) if b != block)
    return int(hit[4]) & M32, int(hit[5]) & M32


@needs_gpu
def test_march_clean_run():
    from hivedscheduler_amd.ops import decode_hw_word, lds_march_block_checksum

    for rounds in (1, 2):
        rec = march(rounds)
        assert (rec[:, :, 1] == 0).all(), f"mismatches: {rec[rec[:, :, 1] != 0]}"
        assert (rec[:, :, 2] == -1).all() and (rec[:, :, 3] == -1).all()
        assert (rec[:, :, 4] == 0).all() and (rec[:, :, 5] == 0).all()
        assert (rec[:, :, 7] == 0).all()
        assert block_checksums(rec) == [lds_march_block_checksum(SEED, rounds)] * BLOCKS
        for blk in rec:
            assert len({decode_hw_word(w) for w in blk[:, 0]}) == 1, blk[:, 0]
    assert lds_march_block_checksum(SEED, 1) != lds_march_block_checksum(SEED, 2)
    assert block_checksums(march(1)) != block_checksums(march(2))


@needs_gpu
@pytest.mark.parametrize("word", [0, 16384, WORDS - 1])
def test_march_covers_the_whole_lds(word):
    """Word 16384 is the first one past the 64 KiB slab of lds_check, word
    40959 the last of the 160 KiB."""
    block, pas, bit = 5, 1, 9
    rec = march(1, block, word, pas, bit)
    dropped, raised = assert_single_fault(rec, block, word, pas, rounds=1)
    assert dropped | raised == 1 << bit


@needs_gpu
def test_march_polarity():
    """The same cell flipped after the true write (phase 0) and after the
    complement write (phase 1): the bit that was written 1 reads back
    dropped, the one written 0 raised, never both."""
    from hivedscheduler_amd.ops import lds_march_pattern

    block, word, bit = 2, 23456, 17
    written_one = bool((int(lds_march_pattern(SEED, 0)[word]) >> bit) & 1)
    masks = [assert_single_fault(march(1, block, word, phase, bit), block, word, phase, 1)
             for phase in (0, 1)]
    flipped, zero = 1 << bit, 0
    for (dropped, raised), was_one in zip(masks, (written_one, not written_one)):
        assert (dropped, raised) == ((flipped, zero) if was_one else (zero, flipped))
    assert masks[0] != masks[1]


@needs_gpu
@pytest.mark.parametrize("phase", [2, 3])
def test_march_wide_read_path(phase):
    """ds_read_b128 passes: a fault in the last dword of a quad, and in the
    first dword of another, is found at the right word with only its bit."""
    from hivedscheduler_amd.ops import lds_march_pattern

    block, bit = 6, 30
    for word in (4 * 2501 + 3, 4 * 7000):
        rec = march(1, block, word, phase, bit)
        dropped, raised = assert_single_fault(rec, block, word, phase, rounds=1)
        written = int(lds_march_pattern(SEED, 0)[word]) ^ (M32 if phase == 3 else 0)
        if (written >> bit) & 1:
            assert (dropped, raised) == (1 << bit, 0)
        else:
            assert (dropped, raised) == (0, 1 << bit)


@needs_gpu
def test_march_later_round():
    """Round 1 uses another pattern than round 0 and reports global pass
    indices: an injection at pass 6 (round 1, phase 2) is found there."""
    block, word, pas, bit = 0, 31111, 6, 0
    rec = march(2, block, word, pas, bit)
    assert_single_fault(rec, block, word, pas, rounds=2)
    assert int(rec[block, :, 2].max()) >= 4


@needs_gpu
def test_march_report_injection_names_one_cu():
    from hivedscheduler_amd.ops import (decode_hw_word, get_ops, lds_march_report,
                                        summarize_lds_march)

    block, word, pas, bit = 3, 16385, 1, 4
    rep = lds_march_report(0, blocks=BLOCKS, rounds=1, seed=SEED, inject=(block, word, pas, bit))
    assert rep["ok"] is False and rep["mismatched_blocks"] == 1
    assert rep["split_blocks"] == 0 and rep["blocks"] == BLOCKS
    assert len(rep["bad_cus"]) == 1
    bad = rep["bad_cus"][0]
    assert bad["blocks"] == 1 and bad["mismatched_dwords"] == 1
    assert (bad["first_bad_pass"], bad["first_bad_word"]) == (pas, word)
    assert bad["dropped_mask"] | bad["raised_mask"] == 1 << bit
    assert bad["dropped_mask"] & bad["raised_mask"] == 0
    # pass 1 is a complement pass, which the checksum does not cover
    assert rep["checksum_ok"] is True
    # Placement can differ between launches, so compare within one launch: the
    # named CU is the one the injected block's own records carry.
    records, ms = get_ops().lds_march(BLOCKS, 1, SEED, block, word, pas, bit)
    rec = records.cpu().numpy()
    s = summarize_lds_march(rec, ms, 1, SEED, expected_cus=1)
    xcc, se, sh, cu = decode_hw_word(rec[4 * block, 0])
    assert [(c["xcc"], c["se"], c["sh"], c["cu"]) for c in s["bad_cus"]] == [(xcc, se, sh, cu)]
    # an injection in a true-polarity pass also shows in the checksum
    rep = lds_march_report(0, blocks=BLOCKS, rounds=1, seed=SEED, inject=(block, word, 0, bit))
    assert rep["checksum_ok"] is False and len(rep["bad_cus"]) == 1


@needs_gpu
def test_march_argument_checks():
    from hivedscheduler_amd.ops import get_ops

    ops = get_ops()
    rounds = 2
    for bad in (dict(blocks=0), dict(blocks=2 ** 16 + 1), dict(rounds=0),
                dict(blocks=2 ** 16, rounds=2 ** 20),
                dict(inject_block=BLOCKS), dict(inject_block=-2),
                dict(inject_word=WORDS), dict(inject_word=-2),
                dict(inject_bit=32), dict(inject_bit=-1),
                dict(inject_pass=rounds * 4), dict(inject_pass=-2)):
        args = dict(blocks=BLOCKS, rounds=rounds, seed=SEED, inject_block=1, inject_word=5,
                    inject_pass=0, inject_bit=0)
        args.update(bad)
        with pytest.raises(RuntimeError):
            ops.lds_march(**args)


@needs_gpu
def test_march_default_shape_coverage_and_plausibility():
    """Default grid and rounds: every CU runs the march, the result is clean,
    and the GB/s figure does not exceed the width of the LDS array (256 B per
    clock per CU, which bounds every pass from above; a cap that catches
    byte-count or timing errors, not a target, so no lower bound)."""
    from hivedscheduler_amd.ops import get_ops, lds_march_report

    info = get_ops().device_info(0)
    cus = info["multiProcessorCount"]
    rep = lds_march_report()
    peak = cus * 256 * info["clockRate_kHz"] * 1e3 / 1e9
    print(f"lds_march: {rep['gbps']:.0f} GB/s in {rep['elapsed_ms']:.3f} ms, "
          f"{rep['blocks']} blocks x {rep['rounds']} rounds (array width {peak:.0f} GB/s), "
          f"cus_seen {rep['cus_seen']}")
    assert rep["ok"] is True, rep
    assert rep["bad_cus"] == [] and rep["mismatched_blocks"] == 0 and rep["split_blocks"] == 0
    assert rep["cus_seen"] == cus, rep
    assert 0 < rep["gbps"] <= peak, (rep["gbps"], peak)


@needs_gpu
def test_health_report_march_wiring():
    from hivedscheduler_amd.ops import gpu_health_report

    plain = gpu_health_report(0, quick=True)
    rep = gpu_health_report(0, quick=True, lds_march=True)
    assert rep["lds_march"]["ok"] is True and rep["healthy"] is True
    assert "lds_march" not in plain
    assert set(rep) - set(plain) == {"lds_march"}
    assert set(plain) == {
        "device", "info", "hbm_gbps", "mfma_max_err_vs_fp32", "mfma_cross_cu_spread", "mfma_ok",
        "mfma_fp8_max_err_vs_fp32", "mfma_fp8_cross_cu_spread", "mfma_fp8_ok",
        "mfma_mx8_max_err_vs_fp32", "mfma_mx8_cross_cu_spread", "mfma_mx8_ok",
        "mfma_fp4_max_err_vs_fp32", "mfma_fp4_cross_cu_spread", "mfma_fp4_ok",
        "mfma_lowprec_ok", "cu_coverage", "cu_coverage_ok", "lds_errors", "healthy",
    }
