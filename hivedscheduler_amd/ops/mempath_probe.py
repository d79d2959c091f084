"""Memory-path probe (ops.mempath_probe): buffer addressing in every width, the
descriptor's hardware bounds check, direct-to-LDS loads and the sub-dword, d16
and wide forms, each step verified bitwise and attributed per CU. The step
lists, the pattern, the out-of-bounds offset table and the expected checksum
here mirror the kernel comment in hived_ops.hip; pure numpy apart from the
report functions.
"""
from __future__ import annotations

from .records import BadUnits, _fmix32, decode_hw_word, units_seen

MEMPATH_SECTIONS = ("buf", "oob", "lds", "forms")
SLICE_WORDS = 3072
GUARD_WORDS = 64
SLICE_BYTES = 4 * SLICE_WORDS
ROW_BYTES = 4 * (SLICE_WORDS + GUARD_WORDS)
LDS_WAVE_WORDS = 4096
GUARD_SENTINEL = 0xC3A5E17B  # every byte non-zero
LDS_SENTINEL = 0x5AA5C33C
OOB_LENGTHS = (SLICE_BYTES, SLICE_BYTES - 1, SLICE_BYTES - 3, 4, 0)
OOB_WIDTHS = (1, 2, 4, 8, 12, 16)
OOB_LANES = 16
# where in the wave's 16 KiB each direct-to-LDS step puts its copy (bytes)
LDS_DST = (0, 4096, 2048, 16, 512)
LDS_OOB_INRANGE = 32
_M32 = 0xFFFFFFFF
# default grid and rounds (BENCHMARKS.md "Memory-path probe")
_BLOCKS_PER_CU = 2
_DEFAULT_ROUNDS = 2

_NARROW = ("u8", "i8", "u16", "i16")
_D16 = ("u8_d16", "u8_d16_hi", "i8_d16", "i8_d16_hi", "u16_d16", "u16_d16_hi")
_WIDTH_NAMES = {1: "byte", 2: "short", 4: "dword", 8: "dwordx2", 12: "dwordx3", 16: "dwordx4"}
# (step name, what the step compares) per section, in kernel order
_STEPS = {
    "buf": [("buffer_load_ubyte", "u8"), ("buffer_load_sbyte", "i8"),
            ("buffer_load_ushort", "u16"), ("buffer_load_sshort", "i16")]
           + [(f"buffer_load_{_WIDTH_NAMES[w]}", "w") for w in (4, 8, 12, 16)]
           + [(f"buffer_store_{_WIDTH_NAMES[w]}", "store") for w in OOB_WIDTHS],
    "oob": [(f"len{L}_buffer_{'store' if k >= 6 else 'load'}_b{8 * OOB_WIDTHS[k % 6]}", "oob")
            for L in OOB_LENGTHS for k in range(12)] + [("guard_global_load_dword", "guard")],
    "lds": [(name, "lds_copy") for name in (
        "global_load_lds_dword", "global_load_lds_dwordx4", "buffer_load_dword_lds",
        "buffer_load_dwordx4_lds")]
           + [("buffer_load_dword_lds_out_of_range", "lds_oob")],
    "forms": list(zip(("global_load_ubyte", "global_load_sbyte", "global_load_ushort",
                       "global_load_sshort"), _NARROW))
             + list(zip(("global_load_ubyte_d16", "global_load_ubyte_d16_hi",
                         "global_load_sbyte_d16", "global_load_sbyte_d16_hi",
                         "global_load_short_d16", "global_load_short_d16_hi"), _D16))
             + [(n, "store") for n in ("global_store_byte", "global_store_byte_d16_hi",
                                       "global_store_short", "global_store_short_d16_hi")]
             + list(zip(("ds_read_u8", "ds_read_i8", "ds_read_u16", "ds_read_i16"), _NARROW))
             + [(f"ds_read_{k}", k) for k in _D16]
             + [(n, "w") for n in ("ds_read_b64", "ds_read_b96", "ds_read2_b32",
                                   "ds_read2st64_b32", "ds_read2_b64")]
             + [(n, "store") for n in ("ds_write_b8", "ds_write_b16", "ds_write_b8_d16_hi",
                                       "ds_write_b16_d16_hi", "ds_write_b64", "ds_write_b96",
                                       "ds_write_b128", "ds_write2_b32", "ds_write2st64_b32",
                                       "ds_write2_b64")],
}


def mempath_steps(section: str) -> list:
    """Step names of a section, in kernel order; the kernel reports the global
    step round*len(steps) + step."""
    return [name for name, _ in _STEPS[section]]


def _patterns(seed: int, waves, round: int):
    """np.uint32 [len(waves), 3072]: what each wave's slice holds in `round`."""
    import numpy as np

    w = np.asarray(waves, dtype=np.uint64)
    rs = ((int(seed) + int(round) * 0x9E3779B9 + w * 0x7F4A7C15) & _M32).astype(np.uint32)
    i = np.arange(SLICE_WORDS, dtype=np.uint32) * np.uint32(0x85EBCA6B)
    v = _fmix32(rs[:, None] ^ i[None, :])
    return ~v if round & 1 else v


def mempath_pattern(seed: int, wave: int, round: int):
    """The np.uint32[3072] a wave's slice holds in a round: fmix32((seed +
    round*0x9E3779B9 + wave*0x7F4A7C15) ^ (i*0x85EBCA6B)), a bijection in i,
    complemented in odd rounds."""
    return _patterns(seed, [wave], round)[0]


def _oob_lo(length: int, width: int) -> int:
    return max(0, length // width * width - (OOB_LANES // 2) * width)


def mempath_oob_cases() -> list:
    """The oob section's steps but the last: per step its descriptor length,
    access width, whether it stores, and the (byte offset, 'in' | 'out')
    accesses its lanes issue; a lane whose access would straddle the length
    issues nothing. soffset is 0 throughout. Asserts for every access that the
    address formed without the check, offset + width, stays inside the wave's
    row, and likewise under the injection's lengthened descriptor."""
    cases = []
    for li, length in enumerate(OOB_LENGTHS):
        for k in range(12):
            width = OOB_WIDTHS[k % 6]
            lo = _oob_lo(length, width)
            accesses = []
            for lane in range(OOB_LANES):
                o = lo + lane * width
                assert 0 <= o and o + width <= ROW_BYTES and o % width == 0, (length, width, o)
                if o + width <= length:
                    accesses.append((o, "in"))
                elif o >= length:
                    accesses.append((o, "out"))
            first_out = -(-length // width) * width
            assert first_out + width <= ROW_BYTES
            step = li * 12 + k
            cases.append({"step": step, "name": _STEPS["oob"][step][0], "length": length,
                          "width": width, "store": k >= 6, "lo": lo, "first_out": first_out,
                          "soffset": 0, "accesses": accesses})
    return cases


def _step_x(step: int) -> int:
    return ((step + 1) * 0x9E3779B9) & _M32


def _narrow_sums(v) -> dict:
    """Per wave: the sums of v's bytes and halfwords and how many are negative."""
    import numpy as np

    u8, u16 = v.view(np.uint8), v.view(np.uint16)
    return {"u8": u8.sum(axis=1, dtype=np.uint64), "u16": u16.sum(axis=1, dtype=np.uint64),
            "neg8": (u8 >> 7).sum(axis=1, dtype=np.uint64),
            "neg16": (u16 >> 15).sum(axis=1, dtype=np.uint64)}


def _elem_sum(kind: str, sums: dict):
    """Sum of the elements as a narrow step compares them: extended to 32 bits,
    a d16 form to 16 bits (the register's other half is not compared)."""
    import numpy as np

    base = kind.split("_")[0]
    bits = int(base[1:])
    total = sums[f"u{bits}"]
    if base[0] == "i":  # sign extension adds the upper bits of every negative element
        upper = (0xFFFF if kind != base else _M32) & ~((1 << bits) - 1)
        total = total + sums[f"neg{bits}"] * np.uint64(upper)
    return total


def _oob_sum(v):
    import numpy as np

    total = np.zeros(v.shape[0], dtype=np.uint64)
    guard = np.full((v.shape[0], GUARD_WORDS), GUARD_SENTINEL, dtype=np.uint32)
    row = np.concatenate([v, guard], axis=1)  # slice then guard
    for case in mempath_oob_cases():
        w = case["width"]
        dtype = {1: np.uint8, 2: np.uint16}.get(w, np.uint32)
        first = case["lo"] // 4
        window = np.ascontiguousarray(row[:, first:first + (OOB_LANES * w + 7) // 4])
        stored = (window ^ np.uint32(_step_x(case["step"]))).view(np.uint8)
        window = window.view(np.uint8)
        for o, where in case["accesses"]:
            if where == "out" and not case["store"]:
                continue  # an out-of-range load returns 0
            src = stored if where == "in" and case["store"] else window
            at = o - 4 * first
            total += np.ascontiguousarray(src[:, at:at + w]).view(dtype).sum(axis=1,
                                                                            dtype=np.uint64)
    return total + np.uint64(GUARD_WORDS * GUARD_SENTINEL)


def _wave_checksums(section: str, seed: int, waves, rounds: int):
    """np.uint32 [len(waves)]: the expected record field [6]."""
    import numpy as np

    waves = np.asarray(waves)
    total = np.zeros(len(waves), dtype=np.uint64)
    for r in range(0, rounds, 2):  # the even rounds hold the true polarity
        v = _patterns(seed, waves, r)
        words = v.sum(axis=1, dtype=np.uint64)
        narrow = _narrow_sums(v)
        if section == "oob":
            total += _oob_sum(v)
            continue
        for step, (_, kind) in enumerate(_STEPS[section]):
            if kind == "w":
                total += words
            elif kind == "store":
                total += (v ^ np.uint32(_step_x(step))).sum(axis=1, dtype=np.uint64)
            elif kind == "lds_copy":
                total += words + np.uint64((LDS_WAVE_WORDS - SLICE_WORDS) * LDS_SENTINEL)
            elif kind == "lds_oob":  # the out-of-range lanes' words are not summed
                total += v[:, :LDS_OOB_INRANGE].sum(axis=1, dtype=np.uint64) \
                    + np.uint64((LDS_WAVE_WORDS - 64) * LDS_SENTINEL)
            else:
                total += _elem_sum(kind, narrow)
    return (total & np.uint64(_M32)).astype(np.uint32)


def mempath_wave_checksum(section: str, seed: int, wave: int, rounds: int) -> int:
    """Expected record field [6] of a wave: the sum mod 2^32 of every value its
    steps compare in the even rounds, from the pattern alone."""
    return int(_wave_checksums(section, seed, [wave], rounds)[0])


def _section_bytes(section: str) -> int:
    """Bytes one wave moves in one round (for the reported GB/s)."""
    if section == "buf":  # fill, 8 load steps, 6 x (store + read-back)
        return (1 + 8 + 12) * SLICE_BYTES
    if section == "oob":  # fill, guard; a store step also reads back and restores
        return SLICE_BYTES + 4 * GUARD_WORDS + sum(
            len(c["accesses"]) * c["width"] * (3 if c["store"] else 1)
            for c in mempath_oob_cases())
    if section == "lds":  # fill; per step prefill and read-back of 16 KiB, the copy in and out
        return SLICE_BYTES + 5 * 2 * 4 * LDS_WAVE_WORDS + 4 * 2 * SLICE_BYTES + 2 * 256
    stores = sum(1 for _, kind in _STEPS["forms"] if kind == "store")
    return (2 + len(_STEPS["forms"]) + stores) * SLICE_BYTES


def summarize_mempath(records, elapsed_ms: float, section: str, rounds: int, seed: int,
                      expected_cus: int) -> dict:
    """Turn the per-wave records of one ops.mempath_probe launch into a verdict.

    records: [blocks*4, 8] int32 rows {hw word, mismatched elements, first bad
    global step (-1), lowest bad byte offset in that step (-1), dropped mask,
    raised mask, sum of the values compared in the even rounds, flags}. A
    block is attributed to the CU of its first wave; a block whose waves name
    different CUs counts in `split_blocks`. In the lds section the flags say
    what an out-of-range lane of a direct-to-LDS load did (1 wrote zero, 2 left
    LDS alone): reported as `lds_oob_writes_zero`, and waves that disagree, or
    saw both, make the run not ok. In the forms section they say what a d16
    load left in the other half of its register (1 kept, 2 zeroed, 4 neither):
    reported as `d16_other_half`, never judged. Pure numpy; needs no GPU.
    """
    import numpy as np

    rec = np.asarray(records).reshape(-1, 4, 8).astype(np.int64)
    blocks = int(rec.shape[0])
    steps = mempath_steps(section)
    nbytes = float(blocks) * 4 * rounds * _section_bytes(section)
    want = _wave_checksums(section, seed, np.arange(blocks * 4), rounds).reshape(blocks, 4)
    checksum_ok = bool(((rec[:, :, 6] & _M32) == want).all())
    mismatched_blocks = split_blocks = 0
    bad = BadUnits()
    for blk in rec:
        cus = [decode_hw_word(w) for w in blk[:, 0]]
        if len(set(cus)) != 1:
            split_blocks += 1
        mism = int(blk[:, 1].sum())
        if mism == 0:
            continue
        mismatched_blocks += 1
        first = min((int(w[2]), int(w[3])) for w in blk if w[1] != 0)
        bad.add(cus[0], {"blocks": 1, "mismatched_elements": mism}, first,
                {"dropped_mask": int(np.bitwise_or.reduce(blk[:, 4])) & _M32,
                 "raised_mask": int(np.bitwise_or.reduce(blk[:, 5])) & _M32})
    bad_cus = bad.entries(("first_bad_step", "first_bad_offset"))
    for e in bad_cus:
        e["first_bad_step_name"] = steps[e["first_bad_step"] % len(steps)] \
            if e["first_bad_step"] >= 0 else None
    out = {
        "gbps": nbytes / (elapsed_ms * 1e-3) / 1e9 if elapsed_ms > 0 else 0.0,
        "elapsed_ms": float(elapsed_ms),
        "blocks": blocks,
        "cus_seen": units_seen(rec[:, :, 0], decode_hw_word),
        "mismatched_blocks": mismatched_blocks,
        "checksum_ok": checksum_ok,
        "split_blocks": split_blocks,
        "bad_cus": bad_cus,
    }
    flags_ok = True
    if section == "lds":
        seen = set(int(f) for f in np.unique(rec[:, :, 7]))
        flags_ok = seen in ({1}, {2})
        out["lds_oob_writes_zero"] = (seen == {1}) if flags_ok else None
    elif section == "forms":
        seen = int(np.bitwise_or.reduce(rec[:, :, 7].ravel())) if blocks else 0
        out["d16_other_half"] = {0: None, 1: "kept", 2: "zeroed"}.get(seen, "mixed")
    else:
        flags_ok = bool((rec[:, :, 7] == 0).all())
    out["ok"] = bool(mismatched_blocks == 0 and checksum_ok and split_blocks == 0 and flags_ok
                     and out["cus_seen"] >= expected_cus)
    return out


def mempath_section_report(device: int = 0, section: str = "buf", blocks: int = None,
                           rounds: int = None, seed: int = 1, inject=None) -> dict:
    """Run one section of the memory-path probe on one GPU and summarise it.

    The default grid is two workgroups per CU, which covers every CU of an
    idle GPU (BENCHMARKS.md "Memory-path probe"), and two rounds, one per
    polarity. `inject=(block, step, offset, bit)` flips that bit of the element
    at that byte offset of what global step `step` reads, in wave 0 of that
    block (in the oob section: lengthens that block's descriptor for that
    step; offset and bit are unused): a harmless store into the wave's own
    memory that exercises detection and attribution on healthy hardware.
    """
    from . import _ops_on

    ops = _ops_on(device)
    expected_cus = ops.device_info(device)["multiProcessorCount"]
    blocks = _BLOCKS_PER_CU * expected_cus if blocks is None else int(blocks)
    rounds = _DEFAULT_ROUNDS if rounds is None else int(rounds)
    inject_args = (-1, -1, -1, 0) if inject is None else tuple(int(v) for v in inject)
    records, ms = ops.mempath_probe(section, blocks, rounds, seed, *inject_args)
    out = summarize_mempath(records.cpu().numpy(), ms, section, rounds, seed, expected_cus)
    out["rounds"] = rounds
    return out


def mempath_probe_report(device: int = 0) -> dict:
    """All four sections at the default shape: {"sections": {name: summary},
    "ok", "bad_cus" (the union, as xcc/se/sh/cu), "lds_oob_writes_zero"}."""
    from .records import place_dicts, place_keys

    sections = {name: mempath_section_report(device, name) for name in MEMPATH_SECTIONS}
    bad = set().union(*(place_keys(s["bad_cus"], 4) for s in sections.values()))
    return {"sections": sections, "ok": all(s["ok"] for s in sections.values()),
            "bad_cus": place_dicts(bad),
            "lds_oob_writes_zero": sections["lds"]["lds_oob_writes_zero"]}
