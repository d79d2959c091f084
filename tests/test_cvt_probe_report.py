"""CPU tests for the conversion probe's host mirror (ops/cvt_probe.py): the
encoder against a brute-force nearest-value search and against torch's own fp8
casts, decode of encode, the fp6 packing, the operand sets' stated conditions
and the summarisers. No GPU."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from hivedscheduler_amd import ops  # noqa: E402
from hivedscheduler_amd.ops.mx_scale import mx_decode  # noqa: E402
from hivedscheduler_amd.ops.records import place_keys  # noqa: E402

FORMATS = tuple(ops.CVT_FORMATS)
ENCODE_F32 = {"fp8": "enc_fp8_f32", "bf8": "enc_bf8_f32", "fp6": "enc_fp6_f32",
              "bf6": "enc_bf6_f32", "fp4": "enc_fp4_f32"}


def scaled_inputs(path):
    """float64 x / 2^s of every element of an encode or sr path, and its wide values."""
    info = ops.cvt_path_info(path)
    el, exps, want = ops.cvt_elements(path)
    ftype, itype = {"f32": (torch.float32, torch.int32), "f16": (torch.float16, torch.int16),
                    "bf16": (torch.bfloat16, torch.int16)}[info["wide"]]
    bits = 32 if info["wide"] == "f32" else 16
    wide = torch.where(el >= 1 << (bits - 1), el - (1 << bits), el).to(itype).view(ftype)
    return torch.ldexp(wide.double(), -exps), wide, want


@pytest.mark.parametrize("fmt", FORMATS)
def test_encode_is_nearest_ties_to_even(fmt):
    x, _, want = scaled_inputs(ENCODE_F32[fmt])
    codes = ops.cvt_finite_codes(fmt)
    table = mx_decode(ops.CVT_FORMATS[fmt], codes)
    dist = (x.unsqueeze(1) - table.unsqueeze(0)).abs()           # float64, exact here
    nearest = dist == dist.amin(dim=1, keepdim=True)
    same_sign = (codes >= codes[len(codes) // 2]).unsqueeze(0) == torch.signbit(x).unsqueeze(1)
    even = (codes % 2 == 0).unsqueeze(0)
    pick = nearest & same_sign
    pick = torch.where(pick.sum(dim=1, keepdim=True) > 1, pick & even, pick)
    assert bool((pick.sum(dim=1) == 1).all())
    assert torch.equal(codes[pick.long().argmax(dim=1)], want)
    assert len(x) >= {"fp8": 1400, "bf8": 1400, "fp6": 300, "bf6": 300, "fp4": 80}[fmt] * 6


@pytest.mark.parametrize("fmt,dtype", [("fp8", torch.float8_e4m3fn), ("bf8", torch.float8_e5m2)])
def test_encode_agrees_with_torch_fp8(fmt, dtype):
    x, _, want = scaled_inputs(ENCODE_F32[fmt])
    assert torch.equal(x.float().double(), x)
    assert torch.equal(x.float().to(dtype).view(torch.uint8).long(), want)


def test_bf16_encode_agrees_with_torch():
    x, wide, want = scaled_inputs("enc_bf16_f32")
    assert torch.equal(wide.to(torch.bfloat16).view(torch.int16).long() & 0xFFFF, want)


@pytest.mark.parametrize("fmt", FORMATS)
def test_decode_of_encode_is_identity(fmt):
    codes = ops.cvt_finite_codes(fmt)
    assert torch.equal(ops.cvt_encode_expected(fmt, ops.cvt_decode_value(fmt, codes)), codes)
    lo, hi = ops.cvt_sr_bracket(fmt, ops.cvt_decode_value(fmt, codes))
    assert torch.equal(lo, codes) and torch.equal(hi, codes)


def test_fp6_pack_round_trip_and_layout():
    codes = torch.randint(0, 64, (5, 32), generator=torch.Generator().manual_seed(0))
    words = ops.cvt_pack6(codes)
    assert torch.equal(ops.cvt_unpack6(words), codes) and int(words.max()) < 1 << 32
    # the layout mx_scale's kernels feed the MFMA: code j at bit 6j of the 192
    big = sum(int(c) << (6 * j) for j, c in enumerate(codes[0]))
    assert [int(w) for w in words[0]] == [(big >> (32 * i)) & 0xFFFFFFFF for i in range(6)]


@pytest.mark.parametrize("path", ops.CVT_PATHS)
def test_operand_set_stays_inside_its_condition(path):
    info = ops.cvt_path_info(path)
    el, exps, want = ops.cvt_elements(path)
    inputs, scales, expected = ops.cvt_operands(path)
    assert len(el) % info["pack"] == 0 and scales.numel() == len(el) // info["pack"]
    assert set(exps.tolist()) == set(ops.cvt_scale_exps(path))
    assert set(ops.CVT_SCALE_EXPS) <= set(ops.cvt_scale_exps(path)) or not info["scaled"]
    for s in set(ops.cvt_scale_exps(path)) - {64, -64}:       # more than signed zero
        assert len(set(el[exps == s].tolist())) > 2
    assert torch.equal(scales.double(), torch.ldexp(torch.ones(()).double(),
                                                    exps.view(-1, info["pack"])[:, 0]))
    finfo = torch.finfo({"f32": torch.float32, "f16": torch.float16,
                         "bf16": torch.bfloat16}[info["wide"]])
    if info["kind"] == "dec":
        value = torch.ldexp(ops.cvt_decode_value(info["format"], el), exps)
        assert set(el.tolist()) <= set(ops.cvt_finite_codes(info["format"]).tolist())
    else:
        x, wide, _ = scaled_inputs(path)
        value = wide.double()
        if info["format"] != "bf16":
            assert bool((x.abs() <= ops.cvt_max_normal(info["format"])).all())
            codes = (want & 0xFF, want >> 8) if info["kind"] == "sr" else (want,)
            for c in codes:
                assert not torch.isnan(ops.cvt_decode_value(info["format"], c)).any()
    assert bool(torch.isfinite(value).all())
    assert bool(((value.abs() >= finfo.tiny) | (value == 0)).all())
    assert bool((value.abs() <= finfo.max).all())


def records(n=16, cks=(7, 9)):
    rec = np.zeros((n, 8), dtype=np.int32)
    rec[:, 0] = [(w // 8) << 16 | (w % 8 // 4) << 8 | (w % 4) << 4 for w in range(n)]
    rec[:, 2] = -1
    rec[:, 5], rec[:, 6] = cks
    return rec


def test_summarize_cvt_sweep():
    clean = ops.summarize_cvt_sweep(records(), 1.0, "enc_fp8_f32", 16)
    assert clean["ok"] and clean["bad_simds"] == [] and clean["simds_seen"] == 16
    assert not ops.summarize_cvt_sweep(records(), 1.0, "enc_fp8_f32", 17)["ok"]
    rec = records()
    rec[5, 1:5] = (2, 40, 0x1234, 0x1235)
    s = ops.summarize_cvt_sweep(rec, 1.0, "enc_fp8_f32", 16)
    assert not s["ok"] and s["mismatched_waves"] == 1 and not s["checksum_spread"]
    assert s["first_bad"] == {"entry": 40, "got": 0x1234, "want": 0x1235}
    assert s["bad_simds"] == [{"xcc": 0, "se": 0, "sh": 0, "cu": 1, "simd": 1, "waves": 1,
                               "mismatched_entries": 2, "first_bad_entry": 40}]
    rec = records()
    rec[9, 6] ^= 1 << 20
    s = ops.summarize_cvt_sweep(rec, 1.0, "sr_fp8_f32", 16)
    assert not s["ok"] and s["checksum_spread"] and s["mismatched_waves"] == 0
    assert place_keys(s["bad_simds"], 5) == {(1, 0, 0, 0, 1)}


def test_summarize_cvt_burn():
    rec = records()
    rec[:, 3], rec[:, 4:7] = -1, (5, 0, 0)
    s = ops.summarize_cvt_burn(rec, 2.0, "fp4", 8, 5, 16)
    assert s["ok"] and s["gcvt_per_s"] == pytest.approx(4 * 64 * 16 * 8 * 5 / 2e-3 / 1e9)
    rec[13, 1:4] = (1, 2, 37)
    s = ops.summarize_cvt_burn(rec, 2.0, "fp4", 8, 5, 16)
    assert not s["ok"] and place_keys(s["bad_simds"], 5) == {(1, 0, 0, 1, 1)}
    rec = records()
    rec[:, 3], rec[:, 4:7] = -1, (5, 0, 0)
    rec[2, 4] = 6
    s = ops.summarize_cvt_burn(rec, 2.0, "fp8", 8, 5, 16)
    assert not s["ok"] and s["checksum_spread"]
    assert place_keys(s["bad_simds"], 5) == {(0, 0, 0, 0, 2)}


@pytest.mark.parametrize("section", ops.CVT_BURN_SECTIONS)
def test_burn_mirror_depends_on_every_step(section):
    a, b = ops.cvt_burn_expected(section, 1, 3), ops.cvt_burn_expected(section, 1, 4)
    assert a.dtype == np.uint32 and a.shape == (64,) and (a != b).all()
    assert len(set(a.tolist())) == 64 and (ops.cvt_burn_expected(section, 2, 3) != a).any()
