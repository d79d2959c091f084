"""GPU tests for the conversion probe (ops.cvt_sweep, ops.cvt_burn): every path's
whole operand table, the compare path driven by a corrupted expectation, the
stochastic-rounding brackets, clean and injected burns, argument checks and
the health-report wiring. Everything is bitwise: no tolerance."""
import pytest

torch = pytest.importorskip("torch")

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")]

from hivedscheduler_amd import ops  # noqa: E402
from hivedscheduler_amd.ops.records import place_keys  # noqa: E402

BLOCKS = 8
EXACT_PATHS = tuple(p for p in ops.CVT_PATHS if p not in ops.CVT_SR_PATHS)


def run_sweep(path, edit=None, blocks=BLOCKS):
    args = [t.clone() for t in ops.cvt_operands(path)]
    if edit:
        args = edit(*args)
    records, ms = ops.get_ops().cvt_sweep(path, *(t.cuda() for t in args), blocks)
    assert records.shape == (blocks * 4, 8) and ms > 0
    return records.cpu().numpy()


def assert_clean(rec):
    assert (rec[:, 1] == 0).all() and (rec[:, 2] == -1).all()
    assert len(set(zip(rec[:, 5], rec[:, 6]))) == 1 and (rec[:, 7] == 0).all()


@pytest.mark.parametrize("path", EXACT_PATHS)
def test_sweep(path):
    assert_clean(run_sweep(path))


# (path, entry, expected dword of the entry, bit): the second fp8 case and the
# fp4 case flip a bit of `old` that the select leaves untouched
@pytest.mark.parametrize("path,entry,dword,bit", [
    ("enc_fp8_f32", 777, 0, 3), ("enc_fp8_f32", 4535, 0, 29), ("enc_fp4_f32", 65, 1, 2),
    ("enc_fp6_f32", 70, 5, 31), ("dec_f32_fp6", 11, 17, 22), ("dec_f16_fp8", 64, 1, 15)])
def test_sweep_reports_a_corrupted_expected(path, entry, dword, bit):
    want_n = ops.cvt_operands(path)[2].numel() // ops.cvt_operands(path)[1].numel()
    at = entry * want_n + dword
    true = int(ops.cvt_operands(path)[2][at])

    def corrupt(inputs, scales, expected):
        expected[at] = ((true ^ (1 << bit)) + (1 << 31)) % (1 << 32) - (1 << 31)
        return inputs, scales, expected

    rec = run_sweep(path, corrupt)
    assert (rec[:, 1] == 1).all() and (rec[:, 2] == entry).all() and (rec[:, 3] == true).all()
    assert ((rec[:, 3] ^ rec[:, 4]) == ((1 << bit) + (1 << 31)) % (1 << 32) - (1 << 31)).all()
    s = ops.summarize_cvt_sweep(rec, 1.0, path, 1)
    assert not s["ok"] and s["mismatched_waves"] == BLOCKS * 4 and not s["checksum_spread"]


@pytest.mark.parametrize("path", ops.CVT_SR_PATHS)
def test_sr_brackets(path):
    assert_clean(run_sweep(path))
    el, exps, want = ops.cvt_elements(path)
    at = int(((want & 0xFF) != (want >> 8)).nonzero()[5])     # an input between two codes
    above = int(want[at] >> 8) + 1                            # neither neighbour

    def wrong(inputs, scales, expected):
        expected[at] = above | (above << 8)
        return inputs, scales, expected

    rec = run_sweep(path, wrong)
    pack = ops.cvt_path_info(path)["pack"]
    assert (rec[:, 1] == 1).all() and (rec[:, 2] == at // pack).all()
    assert (rec[:, 4] == (above | (above << 8))).all()
    assert all(int(g) in (int(want[at]) & 0xFF, int(want[at]) >> 8) for g in rec[:, 3])


def run_burn(section, chain=8, rounds=5, inject=(-1, -1, -1, -1), blocks=BLOCKS, expected=None):
    if expected is None:
        want = ops.cvt_burn_expected(section, 1, chain)
        expected = torch.from_numpy(want.view("int32").copy()).cuda()
    records, ms = ops.get_ops().cvt_burn(section, expected, 1, blocks, chain, rounds, *inject)
    return records.cpu().numpy(), ms


@pytest.mark.parametrize("section", ops.CVT_BURN_SECTIONS)
def test_burn_clean_and_injected(section):
    rec, ms = run_burn(section)
    assert rec.shape == (BLOCKS * 4, 8) and ms > 0
    assert (rec[:, 1] == 0).all() and (rec[:, 2:4] == -1).all() and len(set(rec[:, 4])) == 1
    wave, rnd, lane, bit = 13, 2, 37, 5
    rec, ms = run_burn(section, inject=(wave, rnd, lane, bit))
    assert rec[:, 1].sum() == 1 and tuple(rec[wave, 1:4]) == (1, rnd, lane)
    s = ops.summarize_cvt_burn(rec, ms, section, 8, 5, expected_simds=1)
    assert not s["ok"] and s["mismatched_waves"] == 1 and s["checksum_spread"]
    assert place_keys(s["bad_simds"], 5) == {ops.decode_hw_simd(rec[wave, 0])}


def _sweep_with(**change):
    def edit(inputs, scales, expected):
        t = dict(inputs=inputs, scales=scales, expected=expected)
        t.update({k: f(t[k]) for k, f in change.items()})
        return t["inputs"], t["scales"], t["expected"]
    return edit


BAD_SWEEPS = [
    ("no_such_path", {}),
    ("enc_fp8_f32", dict(edit=_sweep_with(inputs=lambda t: t.float()))),
    ("enc_fp8_f32", dict(edit=_sweep_with(scales=lambda t: t.double()))),
    ("enc_fp8_f32", dict(edit=_sweep_with(expected=lambda t: t.long()))),
    ("enc_fp8_f32", dict(edit=_sweep_with(inputs=lambda t: t[:-1]))),
    ("enc_fp8_f32", dict(edit=_sweep_with(expected=lambda t: t[2:]))),
    ("enc_fp8_f32", dict(edit=_sweep_with(scales=lambda t: t.cuda().repeat(2)[::2]))),
    ("enc_fp8_f32", dict(edit=_sweep_with(inputs=lambda t: t.repeat(2), scales=lambda t: t.repeat(2),
                                          expected=lambda t: t.repeat(2)))),   # beyond the LDS
    ("enc_fp8_f32", dict(blocks=0)),
]
BAD_BURNS = [
    ("no_such_section", {}), ("fp8", dict(blocks=0)), ("fp8", dict(rounds=0)),
    ("fp8", dict(rounds=4)), ("fp8", dict(inject=(BLOCKS * 4, 0, 0, 0))),
    ("fp8", dict(inject=(0, 5, 0, 0))), ("fp8", dict(inject=(0, 0, 64, 0))),
    ("fp8", dict(inject=(0, 0, 0, 32))), ("fp8", dict(expected=torch.zeros(64, dtype=torch.int64))),
    ("fp8", dict(expected=torch.zeros(63, dtype=torch.int32))),
]


@pytest.mark.parametrize("path,kwargs", BAD_SWEEPS)
def test_bad_sweep_arguments(path, kwargs):
    with pytest.raises(RuntimeError):
        if path not in ops.CVT_PATHS:
            i, s, e = (t.cuda() for t in ops.cvt_operands("enc_fp8_f32"))
            ops.get_ops().cvt_sweep(path, i, s, e, BLOCKS)
        else:
            run_sweep(path, **kwargs)


def test_sweep_refuses_cpu_tensors():
    with pytest.raises(RuntimeError):
        ops.get_ops().cvt_sweep("enc_fp8_f32", *ops.cvt_operands("enc_fp8_f32"), BLOCKS)


@pytest.mark.parametrize("section,kwargs", BAD_BURNS)
def test_bad_burn_arguments(section, kwargs):
    if "expected" in kwargs:
        kwargs = dict(kwargs, expected=kwargs["expected"].cuda())
    elif section not in ops.CVT_BURN_SECTIONS:
        kwargs = dict(kwargs, expected=torch.zeros(64, dtype=torch.int32).cuda())
    with pytest.raises(RuntimeError):
        run_burn(section, **kwargs)


def test_health_report():
    base = ops.gpu_health_report(0, quick=True)
    rep = ops.gpu_health_report(0, quick=True, cvt_probe=True)
    assert set(rep) - set(base) == {"cvt_probe"} and rep["healthy"]
    probe = rep["cvt_probe"]
    assert probe["ok"] and probe["bad_simds"] == [] and probe["sweep"]["ok"] and probe["burn"]["ok"]
    assert set(probe["sweep"]["paths"]) == set(ops.CVT_PATHS)
    assert set(probe["burn"]["sections"]) == set(ops.CVT_BURN_SECTIONS)
    simds = 4 * rep["info"]["multiProcessorCount"]
    for path, s in probe["sweep"]["paths"].items():
        assert s["ok"] and s["simds_seen"] == simds, path
    for section, s in probe["burn"]["sections"].items():
        print(f"{section}: chain {s['chain']} rounds {s['rounds']} {s['elapsed_ms']:.2f} ms "
              f"{s['gcvt_per_s']:.0f} Gcvt/s")
        assert s["ok"] and s["simds_seen"] == simds
