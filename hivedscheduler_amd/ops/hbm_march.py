"""HBM march (ops.hbm_march): a bounded span of HBM, both bit polarities,
16 B per lane, a pattern unique across the whole sweep, every launch timed
by events and by device clocks per workgroup. See the kernel comment in
hived_ops.hip.
"""
from __future__ import annotations

from .records import _M64, _mix64, _u64_fields

HBM_MARCH_TILE_BYTES = 16384  # 256 threads x 16 B x 4 accesses
_HBM_MARCH_TILE_QWORDS = HBM_MARCH_TILE_BYTES // 8
# the realtime clock of the records ticks at 100 MHz
_HBM_MARCH_TICK_S = 1e-8
_HBM_MARCH_MAX_LOCATIONS = 16
_HBM_MARCH_MAX_LOG = 64


def hbm_march_pattern(seed: int, start: int, count: int):
    """The np.uint64[count] pattern p(seed, start + i) = mix64(seed ^ g) the
    kernel writes in pass 0 at the global qword indices g = start + i (byte
    offset in the sweep / 8). mix64(seed ^ .) is a bijection on 64 bits, so
    all values of a sweep are distinct. Pass 1 writes ~p."""
    import numpy as np

    g = np.arange(int(count), dtype=np.uint64) + np.uint64(int(start) & _M64)
    return _mix64(g ^ np.uint64(int(seed) & _M64))


def hbm_slow_xcds(xcds, min_xcd_ratio) -> list:
    """XCC ids whose verify_gbps is below min_xcd_ratio x the median over the
    XCDs; empty when min_xcd_ratio is None."""
    import numpy as np

    if min_xcd_ratio is None or not xcds:
        return []
    floor = float(min_xcd_ratio) * float(np.median([x["verify_gbps"] for x in xcds]))
    return sorted(int(x["xcc"]) for x in xcds if x["verify_gbps"] < floor)


def summarize_hbm_march(result: dict, expected_xcds: int, min_xcd_ratio=None) -> dict:
    """Turn the result of one ops.hbm_march call into a verdict.

    result: the dict hbm_march returns, tensors already numpy. `records` is
    [launches, blocks, 16] int32 in launch order (chunk-major, then pass,
    then write before verify), rows {hw word, tiles, clock at start lo/hi,
    clock at end lo/hi, and for verify launches mismatched qwords lo/hi,
    lowest bad global qword index lo/hi (-1,-1), dropped mask lo/hi, raised
    mask lo/hi, sum of the qwords read lo/hi}. Pure numpy; needs no GPU.

    A rate per XCD is the bytes of that XCD's workgroups' tiles over all
    launches of one kind, divided by the sum over those launches of the XCD's
    own span (latest end minus earliest start among ITS workgroups that had a
    tile, in 10 ns ticks): clocks of different XCDs are never subtracted from
    each other. `blocks` of an XCD counts its workgroups over all launches.
    """
    import numpy as np

    bytes_tested = int(result["bytes_tested"])
    chunks = int(result["chunks"])
    chunk_bytes = int(result["chunk_bytes"])
    skipped = bool(result["skipped"])
    rec = np.asarray(result["records"]).astype(np.int64)
    rec = rec.reshape(-1, rec.shape[-2] if rec.ndim >= 2 else 0, 16)
    elapsed = np.asarray(result["elapsed_ms"], dtype=np.float64).reshape(-1)
    launches = int(rec.shape[0])
    is_verify = (np.arange(launches) % 2) == 1
    chunk_of = np.arange(launches) // 4
    pass_of = (np.arange(launches) // 2) % 2

    mism = _u64_fields(rec, 6)
    first = _u64_fields(rec, 8)
    per_launch = [int(mism[l].sum()) if is_verify[l] else 0 for l in range(launches)]
    errors = sum(per_launch)
    errors_per_chunk = [sum(e for l, e in enumerate(per_launch) if chunk_of[l] == c)
                        for c in range(chunks)]
    dropped = raised = 0
    first_bad = None
    for l in range(launches):
        if not per_launch[l]:
            continue
        bad = mism[l] != 0
        dropped |= int(np.bitwise_or.reduce(_u64_fields(rec[l], 10)[bad]))
        raised |= int(np.bitwise_or.reduce(_u64_fields(rec[l], 12)[bad]))
        if first_bad is None:
            first_bad = {"offset": 8 * int(first[l][bad].min()), "pass": int(pass_of[l])}
    bad_bits = [b for b in range(64) if ((dropped | raised) >> b) & 1]

    log = np.asarray(result["log"]).astype(np.int64).reshape(-1, 4)
    rows = sorted((int(r[1]), int(r[0]) & _M64, (int(r[2]) ^ int(r[3])) & _M64) for r in log)
    bad_locations = [{"offset": 8 * idx, "chunk": (8 * idx) // chunk_bytes if chunk_bytes else 0,
                      "pass": pas, "xor": xor}
                     for pas, idx, xor in rows[:_HBM_MARCH_MAX_LOCATIONS]]

    # every launch must have visited every tile of its chunk: a loop that
    # compared nothing cannot pass
    tiles = rec[:, :, 1]
    coverage_ok = bool(launches == 4 * chunks and
                       (tiles.sum(axis=1) * _HBM_MARCH_TILE_QWORDS == chunk_bytes // 8).all())

    def chip_gbps(kind):
        ms = float(elapsed[is_verify == kind].sum())
        return 2.0 * bytes_tested / (ms * 1e-3) / 1e9 if ms > 0 else 0.0

    start = _u64_fields(rec, 2)
    end = _u64_fields(rec, 4)
    xcc = rec[:, :, 0] >> 16
    xcds = []
    for x in sorted(int(v) for v in np.unique(xcc)):
        entry = {"xcc": x, "blocks": int((xcc == x).sum())}
        for kind, key in ((False, "write_gbps"), (True, "verify_gbps")):
            nbytes = ticks = 0
            for l in np.nonzero(is_verify == kind)[0]:
                sel = (xcc[l] == x) & (tiles[l] > 0)
                if not sel.any():
                    continue
                nbytes += int(tiles[l][sel].sum()) * HBM_MARCH_TILE_BYTES
                ticks += int(end[l][sel].max()) - int(start[l][sel].min())
            entry[key] = nbytes / (ticks * _HBM_MARCH_TICK_S) / 1e9 if ticks > 0 else 0.0
        xcds.append(entry)
    rates = [x["verify_gbps"] for x in xcds]
    median = float(np.median(rates)) if rates else 0.0
    xcd_ratio = min(rates) / median if median > 0 else 0.0
    slow_xcds = hbm_slow_xcds(xcds, min_xcd_ratio)
    ok = skipped or bool(errors == 0 and coverage_ok and len(xcds) >= expected_xcds
                         and not slow_xcds)
    return {
        "bytes_tested": bytes_tested,
        "chunks": chunks,
        "skipped": skipped,
        "errors": errors,
        "errors_per_chunk": errors_per_chunk,
        "dropped_mask": dropped,
        "raised_mask": raised,
        "bad_bits": bad_bits,
        "first_bad": first_bad,
        "bad_locations": bad_locations,
        "coverage_ok": coverage_ok,
        "write_gbps": chip_gbps(False),
        "verify_gbps": chip_gbps(True),
        "xcds": xcds,
        "xcds_seen": len(xcds),
        "xcd_ratio": xcd_ratio,
        "slow_xcds": slow_xcds,
        "ok": ok,
    }


def hbm_march_report(device: int = 0, max_gib: int = 16, chunk_gib: int = 4, seed: int = 1,
                     blocks: int = 2048, inject=None, min_xcd_ratio=None,
                     max_bytes: int = None, chunk_bytes: int = None) -> dict:
    """Run the HBM march on one GPU and summarise it.

    Marches up to max_gib GiB in chunk_gib chunks (all held until the end,
    like hbm_sweep, with the same 8 GiB headroom): four launches per chunk,
    write p / verify / write ~p / verify. max_bytes and chunk_bytes override
    the GiB arguments; they exist for small test shapes. `inject=(index,
    pass, bit)` xors that bit of the qword at that global index between the
    write and the verify of that pass: a plain store into the march's own
    allocation that exercises detection and location on healthy hardware.
    min_xcd_ratio has no default: the healthy spread between XCDs is
    site-measured (docs/user-manual.md).
    """
    from . import _ops_on

    ops = _ops_on(device)
    max_bytes = int(max_gib) << 30 if max_bytes is None else int(max_bytes)
    chunk_bytes = int(chunk_gib) << 30 if chunk_bytes is None else int(chunk_bytes)
    inject_args = (-1, -1, 0) if inject is None else tuple(int(v) for v in inject)
    expected_xcds = max(1, ops.device_info(device)["multiProcessorCount"] // 32)
    res = dict(ops.hbm_march(max_bytes, chunk_bytes, seed, blocks, _HBM_MARCH_MAX_LOG,
                             *inject_args))
    for key in ("records", "elapsed_ms", "log"):
        res[key] = res[key].cpu().numpy()
    out = summarize_hbm_march(res, expected_xcds, min_xcd_ratio)
    out["expected_xcds"] = expected_xcds
    out["blocks"] = blocks
    out["elapsed_ms"] = float(res["elapsed_ms"].sum())
    return out
