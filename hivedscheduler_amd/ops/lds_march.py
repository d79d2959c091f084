"""Full-LDS march (ops.lds_march): all 160 KiB of a CU, both bit polarities,
ds_read_b32 and ds_read_b128 read-back, timed, attributed per CU. See the
kernel comment in hived_ops.hip.
"""
from __future__ import annotations

from .records import BadUnits, _fmix32, decode_hw_word, units_seen

LDS_MARCH_WORDS = 40960  # 163840 B, the whole LDS of a CU
_LDS_MARCH_BYTES = 4 * LDS_MARCH_WORDS
# default rounds per workgroup, and workgroups per CU of the default grid
# (BENCHMARKS.md "LDS march")
_LDS_MARCH_DEFAULT_ROUNDS = 8
_LDS_MARCH_BLOCKS_PER_CU = 2


def lds_march_pattern(seed: int, round: int):
    """The np.uint32[40960] pattern p(round, i) the kernel writes in the true
    polarity: fmix32((seed + round*0x9E3779B9) ^ (i*0x85EBCA6B)). Every step
    is a bijection on 32 bits, so the 40960 values of a round are distinct.
    The complement passes write ~p."""
    import numpy as np

    rs = np.uint32((int(seed) + int(round) * 0x9E3779B9) & 0xFFFFFFFF)
    i = np.arange(LDS_MARCH_WORDS, dtype=np.uint32)
    return _fmix32(rs ^ (i * np.uint32(0x85EBCA6B)))


def lds_march_block_checksum(seed: int, rounds: int) -> int:
    """Expected sum of record field [6] over the four waves of a block: every
    word of p is read once in phase 0 and once in phase 2 of each round, so
    2 * sum_round sum_i p(round, i) mod 2^32."""
    import numpy as np

    total = sum(int(lds_march_pattern(seed, r).sum(dtype=np.uint64)) for r in range(rounds))
    return (2 * total) & 0xFFFFFFFF


def summarize_lds_march(records, elapsed_ms: float, rounds: int, seed: int,
                        expected_cus: int) -> dict:
    """Turn the per-wave records of one ops.lds_march launch into a verdict.

    records: [blocks*4, 8] int32 rows {hw word, mismatched dwords, first bad
    global pass (-1), lowest bad word in that pass (-1), dropped mask (bits
    that should be 1 and read 0), raised mask (should be 0, read 1), sum of
    the dwords read in phases 0 and 2, reserved}. The four waves of a block
    (wave // 4) are combined; a block is attributed to the CU of its first
    wave, and a block whose waves name different CUs is counted in
    `split_blocks` (one workgroup runs on one CU, so that is a fault in
    itself). Pure numpy; needs no GPU.
    """
    import numpy as np

    rec = np.asarray(records).reshape(-1, 4, 8).astype(np.int64)
    blocks = int(rec.shape[0])
    nbytes = float(blocks) * rounds * 4 * 2 * _LDS_MARCH_BYTES
    gbps = nbytes / (elapsed_ms * 1e-3) / 1e9 if elapsed_ms > 0 else 0.0
    want_sum = lds_march_block_checksum(seed, rounds)
    cus_seen = units_seen(rec[:, :, 0], decode_hw_word)
    mismatched_blocks = split_blocks = 0
    checksum_ok = True
    bad = BadUnits()
    for blk in rec:
        cus = [decode_hw_word(w) for w in blk[:, 0]]
        if len(set(cus)) != 1:
            split_blocks += 1
        if (int(blk[:, 6].sum()) & 0xFFFFFFFF) != want_sum:
            checksum_ok = False
        mism = int(blk[:, 1].sum())
        if mism == 0:
            continue
        mismatched_blocks += 1
        first = min((int(w[2]), int(w[3])) for w in blk if w[1] != 0)
        bad.add(cus[0], {"blocks": 1, "mismatched_dwords": mism}, first,
                {"dropped_mask": int(np.bitwise_or.reduce(blk[:, 4])) & 0xFFFFFFFF,
                 "raised_mask": int(np.bitwise_or.reduce(blk[:, 5])) & 0xFFFFFFFF})
    bad_cus = bad.entries(("first_bad_pass", "first_bad_word"))
    return {
        "gbps": gbps,
        "elapsed_ms": float(elapsed_ms),
        "blocks": blocks,
        "cus_seen": cus_seen,
        "mismatched_blocks": mismatched_blocks,
        "checksum_ok": checksum_ok,
        "split_blocks": split_blocks,
        "bad_cus": bad_cus,
        "ok": bool(mismatched_blocks == 0 and checksum_ok and split_blocks == 0
                   and cus_seen >= expected_cus),
    }


def lds_march_report(device: int = 0, blocks: int = None, rounds: int = None, seed: int = 1,
                     inject=None) -> dict:
    """Run the full-LDS march on one GPU and summarise it.

    The kernel takes all 160 KiB of LDS, so one workgroup is resident per CU;
    the default grid is two workgroups per CU (every CU is then covered on an
    idle GPU) and the default rounds keep the launch at about a millisecond.
    `inject=(block, word, pass, bit)` flips that bit of that LDS word in that
    block after the write of that global pass (round*4 + phase): a harmless
    store into the workgroup's own LDS that exercises detection and
    attribution on healthy hardware.
    """
    from . import _ops_on

    ops = _ops_on(device)
    expected_cus = ops.device_info(device)["multiProcessorCount"]
    blocks = _LDS_MARCH_BLOCKS_PER_CU * expected_cus if blocks is None else int(blocks)
    rounds = _LDS_MARCH_DEFAULT_ROUNDS if rounds is None else int(rounds)
    inject_args = (-1, -1, -1, 0) if inject is None else tuple(int(v) for v in inject)
    records, ms = ops.lds_march(blocks, rounds, seed, *inject_args)
    out = summarize_lds_march(records.cpu().numpy(), ms, rounds, seed, expected_cus)
    out["rounds"] = rounds
    return out
