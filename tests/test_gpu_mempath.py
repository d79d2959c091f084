"""GPU tests for the memory-path probe (ops.mempath_probe): clean runs of every
section in both polarities against the host checksum, injected one-bit faults
found at their (step, offset) with their bit, the oob descriptor injection,
argument checks, the default shape and the health-report wiring. Everything
is bitwise: no tolerance."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")]

BLOCKS = 8
SEED = 3
ROUNDS = 2
M32 = 0xFFFFFFFF
SECTIONS = ("buf", "oob", "lds", "forms")


@functools.lru_cache(maxsize=None)
def probe(section, block=-1, step=-1, offset=-1, bit=0):
    """Records [BLOCKS, 4 waves, 8] as int64; each distinct launch runs once."""
    from hivedscheduler_amd.ops import get_ops

    records, ms = get_ops().mempath_probe(section, BLOCKS, ROUNDS, SEED, block, step, offset, bit)
    assert records.shape == (BLOCKS * 4, 8) and records.dtype == torch.int32 and ms > 0
    rec = records.cpu().numpy().astype(np.int64).reshape(BLOCKS, 4, 8)
    rec.setflags(write=False)
    return rec


def step_index(section, name, round=0):
    from hivedscheduler_amd.ops import mempath_steps

    steps = mempath_steps(section)
    return round * len(steps) + steps.index(name)


@pytest.mark.parametrize("section", SECTIONS)
def test_clean_run(section):
    from hivedscheduler_amd.ops import decode_hw_word, mempath_wave_checksum

    rec = probe(section)
    assert (rec[:, :, 1] == 0).all(), rec[rec[:, :, 1] != 0]
    assert (rec[:, :, 2:4] == -1).all() and (rec[:, :, 4:6] == 0).all()
    want = [mempath_wave_checksum(section, SEED, w, ROUNDS) for w in range(BLOCKS * 4)]
    assert [int(x) & M32 for x in rec[:, :, 6].ravel()] == want
    flags = set(rec[:, :, 7].ravel().tolist())
    assert flags in ({1}, {2}) if section in ("lds", "forms") else flags == {0}
    for blk in rec:
        assert len({decode_hw_word(w) for w in blk[:, 0]}) == 1, blk[:, 0]


LAST = 12288 - 4
INJECTIONS = [("buf", "buffer_load_ubyte", 0, 0), ("buf", "buffer_load_ubyte", 12287, 1),
              ("buf", "buffer_store_dwordx4", 0, 0), ("buf", "buffer_store_dwordx4", LAST, 1)]
INJ_DST = (("global_load_lds_dword", 0), ("global_load_lds_dwordx4", 4096),
           ("buffer_load_dword_lds", 2048), ("buffer_load_dwordx4_lds", 16))  # where each step's copy starts in the region
INJECTIONS += [("lds", name, dst + off, rnd) for name, dst in INJ_DST
               for off, rnd in ((0, 0), (LAST, 1))]
INJECTIONS += [("forms", "global_load_short_d16_hi", 0, 1), ("forms", "ds_read_u8_d16_hi", 12287, 0),
               ("forms", "ds_read2_b32", 0, 0), ("forms", "ds_read2st64_b32", LAST, 1)]


@pytest.mark.parametrize("section,name,offset,round", INJECTIONS)
def test_injected_bit_is_found(section, name, offset, round):
    """One flipped bit of the wave's own data: one mismatch, in the injected
    block only, at that (step, offset), with that bit in the mask that matches
    the polarity it was written in."""
    from hivedscheduler_amd.ops import mempath_pattern, mempath_steps

    block, bit = 5, 6
    step = step_index(section, name, round)
    rec = probe(section, block, step, offset, bit)
    assert int(rec[:, :, 1].sum()) == 1 and int(rec[block, 0, 1]) == 1, rec[:, :, 1]
    hit = rec[block, 0]
    assert (int(hit[2]), int(hit[3])) == (step, offset), hit
    dropped, raised = int(hit[4]) & M32, int(hit[5]) & M32
    local = step % len(mempath_steps(section))
    x = ((local + 1) * 0x9E3779B9) & M32 if "store" in name or "write" in name else 0
    src = offset - dict(INJ_DST).get(name, 0) if section == "lds" else offset
    word = (int(mempath_pattern(SEED, 4 * block, round)[src >> 2]) ^ x) >> (8 * (src & 3))
    assert (dropped, raised) == ((1 << bit, 0) if (word >> bit) & 1 else (0, 1 << bit))
    clean = rec[:, :, 1] == 0
    assert (rec[:, :, 2][clean] == -1).all() and (rec[:, :, 4:6][clean] == 0).all()


@pytest.mark.parametrize("width", [1, 16])
def test_oob_descriptor_injection(width):
    """A descriptor one element too long at the full length: exactly the
    first wholly-out access of each wave of that block returns the guard
    instead of 0, and the report names one CU."""
    from hivedscheduler_amd.ops import mempath_oob_cases, summarize_mempath

    case = next(c for c in mempath_oob_cases()
                if c["length"] == 12288 and c["width"] == width and not c["store"])
    block = 2
    rec = probe("oob", block, case["step"])
    per_wave = max(1, width // 4)
    assert rec[:, :, 1].sum() == 4 * per_wave and (rec[block, :, 1] == per_wave).all()
    assert (rec[block, :, 2] == case["step"]).all() and (rec[block, :, 3] == 12288).all()
    s = summarize_mempath(rec.reshape(-1, 8), 1.0, "oob", ROUNDS, SEED, expected_cus=1)
    assert len(s["bad_cus"]) == 1 and s["bad_cus"][0]["first_bad_step_name"] == case["name"]
    assert s["bad_cus"][0]["raised_mask"] == (0xC3A5E17B if width == 16 else 0x7B)


def test_argument_checks():
    from hivedscheduler_amd.ops import get_ops

    ops = get_ops()
    for bad in (dict(section="nope"), dict(blocks=0), dict(blocks=2 ** 16 + 1), dict(rounds=0),
                dict(blocks=2 ** 16, rounds=2), dict(inject_block=BLOCKS),
                dict(inject_block=-2), dict(inject_step=ROUNDS * 14), dict(inject_step=-2),
                dict(inject_offset=12288), dict(inject_offset=-2), dict(inject_bit=32),
                dict(inject_bit=-1), dict(inject_offset=3, inject_bit=8)):
        args = dict(section="buf", blocks=BLOCKS, rounds=ROUNDS, seed=SEED, inject_block=1,
                    inject_step=0, inject_offset=4, inject_bit=0)
        args.update(bad)
        with pytest.raises(RuntimeError):
            ops.mempath_probe(**args)


def test_default_shape_and_health_report():
    from hivedscheduler_amd.ops import get_ops, gpu_health_report

    cus = get_ops().device_info(0)["multiProcessorCount"]
    plain = gpu_health_report(0, quick=True)
    rep = gpu_health_report(0, quick=True, mempath_probe=True)
    assert set(rep) - set(plain) == {"mempath_probe"} and rep["healthy"] is True
    probe_rep = rep["mempath_probe"]
    assert probe_rep["ok"] is True and probe_rep["bad_cus"] == []
    assert probe_rep["lds_oob_writes_zero"] in (True, False)
    for name, s in probe_rep["sections"].items():
        print(f"mempath {name}: {s['elapsed_ms']:.3f} ms, {s['gbps']:.0f} GB/s, "
              f"{s['blocks']} blocks x {s['rounds']} rounds, cus_seen {s['cus_seen']}")
        assert s["ok"] is True and s["cus_seen"] == cus and s["split_blocks"] == 0, (name, s)
    assert set(plain) == {
        "device", "info", "hbm_gbps", "mfma_max_err_vs_fp32", "mfma_cross_cu_spread", "mfma_ok",
        "mfma_fp8_max_err_vs_fp32", "mfma_fp8_cross_cu_spread", "mfma_fp8_ok",
        "mfma_mx8_max_err_vs_fp32", "mfma_mx8_cross_cu_spread", "mfma_mx8_ok",
        "mfma_fp4_max_err_vs_fp32", "mfma_fp4_cross_cu_spread", "mfma_fp4_ok",
        "mfma_lowprec_ok", "cu_coverage", "cu_coverage_ok", "lds_errors", "healthy",
    }
