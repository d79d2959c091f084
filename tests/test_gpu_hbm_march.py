"""GPU tests for the HBM march (ops.hbm_march): clean runs with fewer tiles
than workgroups and with a ragged grid-stride (host checksum per verify
launch), an injected one-bit fault located at tile, chunk and sweep edges,
bits and both polarities, offsets beyond 4 GiB, the report with per-XCD
rates against the event timing, argument checks and the health-report wiring.
Everything is bitwise: no tolerance."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

needs_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")

BLOCKS = 8
MAX_LOG = 16
SEED = 3
TILE = 16384
TILE_QWORDS = TILE // 8
M32 = 0xFFFFFFFF
M64 = (1 << 64) - 1
GIB = 1 << 30

SMALL = 19 * TILE           # one ragged chunk: 19 tiles over 8 workgroups
CHUNK_QWORDS = SMALL // 8


@functools.lru_cache(maxsize=None)
def march(max_bytes, chunk_bytes, index=-1, pas=-1, bit=0, blocks=BLOCKS):
    """One ops.hbm_march call with numpy arrays (records as int64); each
    distinct call runs once and is shared."""
    from hivedscheduler_amd.ops import get_ops

    res = dict(get_ops().hbm_march(max_bytes, chunk_bytes, SEED, blocks, MAX_LOG, index, pas, bit))
    assert res["records"].dtype == torch.int32 and res["elapsed_ms"].dtype == torch.float64
    assert res["log"].dtype == torch.int64
    for key in ("records", "elapsed_ms", "log"):
        res[key] = res[key].cpu().numpy()
        res[key].setflags(write=False)
    launches = 4 * res["chunks"]
    assert res["records"].shape == (launches, blocks, 16)
    assert res["elapsed_ms"].shape == (launches,) and (res["elapsed_ms"] > 0).all()
    assert res["log"].shape == (min(res["log_count"], MAX_LOG), 4)
    assert res["chunk_bytes"] == chunk_bytes
    assert res["bytes_tested"] == res["chunks"] * chunk_bytes
    assert res["skipped"] is (res["bytes_tested"] == 0)
    return res


def u64(rec, lo):
    """Fields [lo], [lo+1] of int32 records as Python ints (array of object)."""
    low = rec[..., lo].astype(np.int64) & M32
    high = rec[..., lo + 1].astype(np.int64) & M32
    return (high.astype(object) << 32) | low.astype(object)


def expected_sum(chunk, chunk_bytes, pas):
    from hivedscheduler_amd.ops import hbm_march_pattern

    n = chunk_bytes // 8
    p = hbm_march_pattern(SEED, chunk * n, n)
    if pas == 1:
        p = ~p
    return int(p.sum(dtype=np.uint64))      # wraps mod 2^64


def assert_records_clean(res, tile_counts, except_launch=None):
    """Every record but those of `except_launch`: the tile counts, ordered
    clocks, zeroed verify fields in write launches, no mismatch, and the sum
    of the qwords read equal to the host's pattern sum."""
    rec = res["records"].astype(np.int64)
    for l in range(rec.shape[0]):
        r = rec[l]
        assert list(r[:, 1]) == list(tile_counts), (l, r[:, 1])
        assert (r[:, 0] >> 16 < 8).all() and (r[:, 0] >= 0).all()
        assert all(e >= s > 0 for s, e in zip(u64(r, 2), u64(r, 4))), (l, r[:, 2:6])
        if l % 2 == 0:
            assert (r[:, 6:] == 0).all(), (l, r[:, 6:])
            continue
        if l == except_launch:
            continue
        assert (r[:, 6:8] == 0).all(), (l, r[:, 6:8])
        assert (r[:, 8:10] == -1).all() and (r[:, 10:14] == 0).all(), (l, r[:, 8:14])
        idle = r[:, 1] == 0
        assert (r[idle][:, 14:16] == 0).all()
        chunk, pas = l // 4, (l // 2) % 2
        assert sum(u64(r, 14)) & M64 == expected_sum(chunk, res["chunk_bytes"], pas), l


def grid_stride_counts(tiles, blocks=BLOCKS):
    return [len(range(b, tiles, blocks)) for b in range(blocks)]


@needs_gpu
def test_fewer_tiles_than_workgroups():
    res = march(3 * TILE, 3 * TILE)
    assert res["chunks"] == 1 and res["bytes_tested"] == 3 * TILE and res["log_count"] == 0
    assert grid_stride_counts(3) == [1, 1, 1, 0, 0, 0, 0, 0]
    # five workgroups had no tile and still wrote a record (hw word, clocks)
    assert_records_clean(res, [1, 1, 1, 0, 0, 0, 0, 0])
    sums = [sum(u64(res["records"][l], 14)) & M64 for l in (1, 3)]
    assert sums == [expected_sum(0, 3 * TILE, 0), expected_sum(0, 3 * TILE, 1)]
    assert sums[0] != sums[1]


@needs_gpu
def test_ragged_grid_stride():
    res = march(SMALL, SMALL)
    assert res["chunks"] == 1 and res["log_count"] == 0
    assert grid_stride_counts(19) == [3, 3, 3, 2, 2, 2, 2, 2]
    assert_records_clean(res, [3, 3, 3, 2, 2, 2, 2, 2])


def assert_single_fault(res, index, pas, bit):
    """Exactly one mismatched qword, in the verify launch of the right chunk
    and pass and in the workgroup that owns the tile, at `index`; exactly one
    log row; everything else clean. Returns (dropped, raised, want)."""
    from hivedscheduler_amd.ops import hbm_march_pattern

    chunk_qwords = res["chunk_bytes"] // 8
    tiles = chunk_qwords // TILE_QWORDS
    blocks = res["records"].shape[1]
    chunk = index // chunk_qwords
    launch = 4 * chunk + 2 * pas + 1
    block = ((index % chunk_qwords) // TILE_QWORDS) % blocks
    assert_records_clean(res, grid_stride_counts(tiles, blocks), except_launch=launch)
    r = res["records"][launch].astype(np.int64)
    mism = u64(r, 6)
    assert int(mism.sum()) == 1 and int(mism[block]) == 1, mism
    assert int(u64(r, 8)[block]) == index
    others = np.arange(blocks) != block
    assert (r[others][:, 8:10] == -1).all() and (r[others][:, 10:14] == 0).all()
    want = int(hbm_march_pattern(SEED, index, 1)[0]) ^ (M64 if pas == 1 else 0)
    assert res["log_count"] == 1
    row = [int(v) & M64 for v in res["log"][0]]
    assert row == [index, pas, want, want ^ (1 << bit)], row
    # the one wrong qword shows in the sum of what was read, and only there
    delta = ((want ^ (1 << bit)) - want) & M64
    assert sum(u64(r, 14)) & M64 == (expected_sum(chunk, res["chunk_bytes"], pas) + delta) & M64
    return int(u64(r, 10)[block]), int(u64(r, 12)[block]), want


LOCATIONS = {
    "first": 0,
    "second_qword_of_an_access": 1,
    "last_of_tile_0": TILE_QWORDS - 1,
    "first_of_next_workgroup": TILE_QWORDS,
    "first_of_chunk_1": CHUNK_QWORDS,
    "last_of_sweep": 2 * CHUNK_QWORDS - 1,
}


@needs_gpu
@pytest.mark.parametrize("where", list(LOCATIONS))
def test_location(where):
    index = LOCATIONS[where]
    pas, bit = index % 2, (7 * index + 13) % 64
    res = march(2 * SMALL, SMALL, index, pas, bit)
    assert res["chunks"] == 2
    dropped, raised, _ = assert_single_fault(res, index, pas, bit)
    assert dropped | raised == 1 << bit and dropped & raised == 0


@needs_gpu
@pytest.mark.parametrize("bit", [0, 31, 32, 63])
def test_bits_and_polarity(bit):
    """The same cell flipped after the true write (pass 0) and after the
    complement write (pass 1): a bit written 1 reads back dropped, one
    written 0 raised, never both."""
    from hivedscheduler_amd.ops import hbm_march_pattern

    index = CHUNK_QWORDS + 5 * TILE_QWORDS + 777
    one_in_pass0 = bool((int(hbm_march_pattern(SEED, index, 1)[0]) >> bit) & 1)
    masks = []
    for pas in (0, 1):
        dropped, raised, want = assert_single_fault(march(2 * SMALL, SMALL, index, pas, bit),
                                                    index, pas, bit)
        written_one = bool((want >> bit) & 1)
        assert written_one is (one_in_pass0 if pas == 0 else not one_in_pass0)
        assert (dropped, raised) == ((1 << bit, 0) if written_one else (0, 1 << bit))
        masks.append((dropped, raised))
    assert masks[0] != masks[1]


@needs_gpu
@pytest.mark.parametrize("index, pas, bit", [((1 << 32) // 8 + 1, 1, 40),
                                             (5 * GIB // 8 - 1, 0, 63)])
def test_offsets_beyond_4_gib(index, pas, bit):
    from hivedscheduler_amd.ops import summarize_hbm_march

    res = march(5 * GIB, GIB, index, pas, bit, blocks=2048)
    if res["bytes_tested"] < 5 * GIB:
        pytest.skip(f"only {res['bytes_tested']} B free for the march on this GPU")
    assert res["chunks"] == 5
    rec = res["records"].astype(np.int64)
    launch = 4 * (index // (GIB // 8)) + 2 * pas + 1
    per_launch = [int(u64(rec[l], 6).sum()) for l in range(rec.shape[0])]
    assert per_launch == [1 if l == launch else 0 for l in range(rec.shape[0])]
    found = [int(v) for v, m in zip(u64(rec[launch], 8), u64(rec[launch], 6)) if m]
    assert found == [index]
    assert res["log_count"] == 1 and int(res["log"][0][0]) == index
    assert (int(res["log"][0][2]) ^ int(res["log"][0][3])) & M64 == 1 << bit
    s = summarize_hbm_march(res, expected_xcds=1)
    assert s["first_bad"] == {"offset": 8 * index, "pass": pas}
    assert s["bad_locations"] == [{"offset": 8 * index, "chunk": index // (GIB // 8),
                                   "pass": pas, "xor": 1 << bit}]
    assert s["errors"] == 1 and s["coverage_ok"] is True


@needs_gpu
def test_report_names_the_injected_location():
    from hivedscheduler_amd.ops import hbm_march_report

    index, pas, bit = CHUNK_QWORDS + 4321, 1, 17
    rep = hbm_march_report(0, seed=SEED, blocks=BLOCKS, inject=(index, pas, bit),
                           max_bytes=2 * SMALL, chunk_bytes=SMALL)
    assert rep["ok"] is False and rep["skipped"] is False
    assert rep["errors"] == 1 and rep["errors_per_chunk"] == [0, 1]
    assert rep["first_bad"] == {"offset": 8 * index, "pass": pas}
    assert rep["bad_locations"] == [{"offset": 8 * index, "chunk": 1, "pass": pas,
                                     "xor": 1 << bit}]
    assert rep["dropped_mask"] | rep["raised_mask"] == 1 << bit
    assert rep["bad_bits"] == [bit] and rep["coverage_ok"] is True


@needs_gpu
def test_report_clean_4_gib_rates_and_clock():
    """One 4-GiB chunk at the default grid. The device span of every XCD in
    every launch lies inside that launch's event bracket, which checks the
    100 MHz realtime clock; the chip-wide read rate stays under the 8 TB/s
    spec peak (a 4-GiB chunk keeps the Infinity Cache's possible share near
    6 %): a cap against byte-count or timing errors, not a target, so no
    lower bound."""
    from hivedscheduler_amd.ops import get_ops, hbm_march_report

    rep = hbm_march_report(0, max_gib=4, chunk_gib=4)
    if rep["bytes_tested"] < 4 * GIB:
        pytest.skip("less than 4 GiB free for the march on this GPU")
    print("hbm_march 4 GiB: write %.0f verify %.0f GB/s, xcd_ratio %.3f" %
          (rep["write_gbps"], rep["verify_gbps"], rep["xcd_ratio"]))
    for x in rep["xcds"]:
        print("  xcc %d: %d blocks, write %.1f verify %.1f GB/s" %
              (x["xcc"], x["blocks"], x["write_gbps"], x["verify_gbps"]))
    expected_xcds = max(1, get_ops().device_info(0)["multiProcessorCount"] // 32)
    assert rep["ok"] is True, rep
    assert rep["errors"] == 0 and rep["coverage_ok"] is True and rep["first_bad"] is None
    assert rep["xcds_seen"] == expected_xcds == rep["expected_xcds"]
    assert 0 < rep["verify_gbps"] <= 8000.0
    res = march(4 * GIB, 4 * GIB, blocks=2048)
    if res["bytes_tested"] < 4 * GIB:
        pytest.skip("less than 4 GiB free for the march on this GPU")
    rec = res["records"].astype(np.int64)
    for l in range(rec.shape[0]):
        xcc = rec[l][:, 0] >> 16
        start, end = u64(rec[l], 2), u64(rec[l], 4)
        busy = rec[l][:, 1] > 0
        for x in np.unique(xcc):
            sel = (xcc == x) & busy
            span_ms = (max(end[sel]) - min(start[sel])) * 1e-8 * 1e3
            print("  launch %d xcc %d: span %.4f ms of %.4f ms" %
                  (l, x, span_ms, res["elapsed_ms"][l]))
            assert 0 < span_ms <= res["elapsed_ms"][l] + 0.02, (l, x)


@needs_gpu
def test_argument_checks():
    from hivedscheduler_amd.ops import get_ops

    ops = get_ops()
    good = dict(max_bytes=2 * SMALL, chunk_bytes=SMALL, seed=SEED, blocks=BLOCKS, max_log=MAX_LOG,
                inject_index=5, inject_pass=0, inject_bit=0)
    for bad in (dict(blocks=0), dict(blocks=2 ** 16 + 1),
                dict(chunk_bytes=0), dict(chunk_bytes=-TILE), dict(chunk_bytes=TILE + 8),
                dict(chunk_bytes=3 * SMALL),
                dict(max_bytes=2 ** 40 + TILE),
                dict(max_log=-1), dict(max_log=2 ** 16 + 1),
                dict(inject_index=-2), dict(inject_index=2 * SMALL // 8),
                dict(inject_pass=-2), dict(inject_pass=2),
                dict(inject_bit=-1), dict(inject_bit=64)):
        args = dict(good)
        args.update(bad)
        with pytest.raises(RuntimeError):
            ops.hbm_march(**args)
    # an index beyond the bytes actually tested is simply not applied: the
    # budget holds one whole chunk, the index lies in the remainder
    res = dict(ops.hbm_march(max_bytes=SMALL + TILE, chunk_bytes=SMALL, seed=SEED, blocks=BLOCKS,
                             max_log=MAX_LOG, inject_index=SMALL // 8 + 3, inject_pass=0,
                             inject_bit=1))
    assert res["chunks"] == 1 and res["log_count"] == 0
    # max_log 0: counted, nothing logged
    res = dict(ops.hbm_march(max_bytes=SMALL, chunk_bytes=SMALL, seed=SEED, blocks=BLOCKS,
                             max_log=0, inject_index=9, inject_pass=1, inject_bit=2))
    assert res["log_count"] == 1 and tuple(res["log"].shape) == (0, 4)


@needs_gpu
def test_health_report_march_wiring():
    from hivedscheduler_amd.ops import gpu_health_report

    plain = gpu_health_report(0, quick=True)
    rep = gpu_health_report(0, quick=True, hbm_march=True)
    assert "hbm_march" not in plain
    assert set(rep) - set(plain) == {"hbm_march"} and set(plain) - set(rep) == set()
    m = rep["hbm_march"]
    assert m["ok"] is True, m
    assert rep["healthy"] is plain["healthy"]
    if not m["skipped"]:
        assert m["errors"] == 0 and m["coverage_ok"] is True
