"""Conversion probe (ops.cvt_sweep, ops.cvt_burn): the gfx950 converters that
quantise to fp8 / fp6 / fp4 / bf16 on the way into the MFMA and dequantise on
the way out, attributed per SIMD. Here: the path table, the operand sets, the
host mirror on top of `mx_decode`, and the reports. See the kernel comments in
hived_ops.hip.

A path is one instruction form: `enc_<format>_<wide>` and `dec_<wide>_<format>`
are the scaled v_cvt_scalef32_pk_* forms (fp6 / bf6: 2xpk16 and pk32),
`decb_*` the scaled byte-select decode, `encu_*`, `decu_*` and `decub_*` the
unscaled v_cvt_pk_{fp8,bf8}_f32, v_cvt_pk_f32_* and v_cvt_f32_*,
`enc_bf16_f32` v_cvt_pk_bf16_f32, `sr_*` the scaled and `sru_*` the unscaled
stochastic-rounding forms. Formats are OCP: fp8 e4m3, bf8 e5m2, fp6 e2m3, bf6
e3m2, fp4 e2m1.

Operand sets. Decode: every finite code at every scale exponent of
CVT_SCALE_EXPS whose value * 2^s the wide type holds exactly as a normal
number (or zero); that only bites for f16, where 2^64 and 2^-64 leave zero
alone, so the f16 paths add 2^8 and 2^-8 (CVT_SCALE_EXPS_F16). Encode: every non-negative value
of the format and every midpoint between neighbours, times 2^s, each exactly
and one wide-type ulp above and below, with both signs, kept where the wide
value is normal (or zero) and |x / 2^s| <= max normal; expected is
round-to-nearest-even of x / 2^s, the sign of zero kept. The scale operand is
the f32 2^s: the hardware reads its exponent only.

Out of scope: NaN and infinity inputs, anything beyond max normal (saturation
and the mode bits that steer it are not the project's), denormal wide values,
and which neighbour a stochastic-rounding form picks: for those the kernel
checks only that an exact input gives its own code and any other one of its
two neighbours, and the waves' checksums are compared by consensus, which
names a SIMD that disagrees and cannot see a fault common to all.
"""
from __future__ import annotations

import functools

from .mx_scale import mx_code_count, mx_decode
from .records import (_M32, BadUnits, _fmix32, _rotl32, _u64_fields, checksum_outliers,
                      decode_hw_simd, place_dicts, place_keys, units_seen)
from .simd_probe import summarize_valu_burn

CVT_SCALE_EXPS = (0, 1, -1, 7, 64, -64)
# f16 holds nothing but zero of a format's values times 2^64 or 2^-64, so the
# f16 paths also take two scales that its range has room for
CVT_SCALE_EXPS_F16 = CVT_SCALE_EXPS + (8, -8)
CVT_FORMATS = {"fp8": 0, "bf8": 1, "fp6": 2, "bf6": 3, "fp4": 4}   # name: mx_decode's code
_BITS = {"fp8": 8, "bf8": 8, "fp6": 6, "bf6": 6, "fp4": 4, "bf16": 16}
_WIDE_BITS = {"f32": 32, "f16": 16, "bf16": 16}


def _paths() -> dict:
    """name: (kind enc|dec|sr, format, wide type, scaled, elements per entry, GOT dwords)"""
    p = {}
    for w in ("f32", "f16", "bf16"):
        for f in ("fp8", "bf8"):
            p[f"enc_{f}_{w}"] = ("enc", f, w, True, 2, 2)
    for w in ("f32", "f16", "bf16"):
        p[f"enc_fp4_{w}"] = ("enc", "fp4", w, True, 2, 4)
    for f in ("fp6", "bf6"):
        p[f"enc_{f}_f32"] = ("enc", f, "f32", True, 32, 6)
    for w in ("f32", "f16", "bf16"):
        for f in ("fp8", "bf8"):
            p[f"dec_{w}_{f}"] = ("dec", f, w, True, 4, 4 if w == "f32" else 2)
    for f in ("fp8", "bf8"):
        p[f"decb_f32_{f}"] = ("dec", f, "f32", True, 4, 4)
    for w in ("f32", "f16", "bf16"):
        p[f"dec_{w}_fp4"] = ("dec", "fp4", w, True, 8, 8 if w == "f32" else 4)
    for f in ("fp6", "bf6"):
        p[f"dec_f32_{f}"] = ("dec", f, "f32", True, 32, 32)
    for f in ("fp8", "bf8"):
        p[f"encu_{f}_f32"] = ("enc", f, "f32", False, 2, 2)
    for f in ("fp8", "bf8"):
        p[f"decu_f32_{f}"] = ("dec", f, "f32", False, 4, 4)
    for f in ("fp8", "bf8"):
        p[f"decub_f32_{f}"] = ("dec", f, "f32", False, 4, 4)
    p["enc_bf16_f32"] = ("enc", "bf16", "f32", False, 2, 1)
    for f in ("fp8", "bf8"):
        p[f"sr_{f}_f32"] = ("sr", f, "f32", True, 1, 4)
    p["sr_fp4_f32"] = ("sr", "fp4", "f32", True, 2, 8)
    for f in ("fp6", "bf6"):
        p[f"sr_{f}_f32"] = ("sr", f, "f32", True, 32, 32)
    for f in ("fp8", "bf8"):
        p[f"sru_{f}_f32"] = ("sr", f, "f32", False, 1, 4)
    return p


_PATHS = _paths()
CVT_PATHS = tuple(_PATHS)
CVT_SR_PATHS = tuple(p for p in _PATHS if _PATHS[p][0] == "sr")
CVT_BURN_SECTIONS = ("fp8", "bf8", "fp6", "fp4", "bf16")
_CVTB_ID = {s: i for i, s in enumerate(CVT_BURN_SECTIONS)}
# conversions (elements encoded plus elements decoded) per lane per step
_CVTB_PER_STEP = {"fp8": 4, "bf8": 4, "fp6": 64, "fp4": 4, "bf16": 2}
# per section, so that the timed launch at 2048 blocks takes the tens of
# milliseconds a VALU burn section takes (BENCHMARKS.md "Conversion probe")
_CVTB_DEFAULTS = {"fp8": (1024, 33), "bf8": (1024, 33), "fp6": (64, 33), "fp4": (1024, 33),
                  "bf16": (1024, 33)}


def cvt_scale_exps(path: str) -> tuple:
    """The scale exponents a path's operand set is built at."""
    _, _, wide, scaled, _, _ = _PATHS[path]
    return (0,) if not scaled else CVT_SCALE_EXPS_F16 if wide == "f16" else CVT_SCALE_EXPS


def cvt_path_info(path: str) -> dict:
    kind, fmt, wide, scaled, pack, got = _PATHS[path]
    return {"kind": kind, "format": fmt, "wide": wide, "scaled": scaled, "pack": pack, "got": got}


# --------------------------------------------------------------------------
# formats and wide types
# --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _magnitudes(fmt: str):
    """The non-negative finite values of a format, ascending; index = code."""
    import torch

    half = mx_code_count(CVT_FORMATS[fmt]) // 2
    v = mx_decode(CVT_FORMATS[fmt], torch.arange(half))
    return v[~torch.isnan(v)]


def cvt_max_normal(fmt: str) -> float:
    return float(_magnitudes(fmt)[-1])


def cvt_finite_codes(fmt: str):
    """Every code of `fmt` that is neither NaN nor infinity, as int64."""
    import torch

    n = len(_magnitudes(fmt))
    return torch.cat([torch.arange(n), torch.arange(n) + mx_code_count(CVT_FORMATS[fmt]) // 2])


def _wide_dtypes(wide: str):
    import torch

    return {"f32": (torch.float32, torch.int32), "f16": (torch.float16, torch.int16),
            "bf16": (torch.bfloat16, torch.int16)}[wide]


def _to_wide_bits(values, wide: str):
    """(bits int64, ok): the wide type's pattern of float64 `values`, and
    whether the value is held exactly as a normal number or zero."""
    import torch

    ftype, itype = _wide_dtypes(wide)
    w = values.to(ftype)
    back = w.double()
    ok = (back == values) & ((back.abs() >= torch.finfo(ftype).tiny) | (back == 0))
    return w.view(itype).long() & ((1 << _WIDE_BITS[wide]) - 1), ok


def _from_wide_bits(bits, wide: str):
    """float64 values of wide-type patterns (int64)."""
    import torch

    ftype, itype = _wide_dtypes(wide)
    n = _WIDE_BITS[wide]
    signed = torch.where(bits >= (1 << (n - 1)), bits - (1 << n), bits)
    return signed.to(itype).view(ftype).double()


def cvt_encode_expected(fmt: str, x):
    """Round-to-nearest-even of float64 `x` (already divided by the scale,
    |x| <= max normal) into `fmt`: int64 codes, the sign of zero kept. Ties go
    to the code with an even mantissa. fmt "bf16": the 16-bit pattern, by the
    integer form of the same rounding on the f32 bits."""
    import torch

    if fmt == "bf16":
        bits = x.float().view(torch.int32).long() & _M32
        return ((bits + 0x7FFF + ((bits >> 16) & 1)) >> 16) & 0xFFFF
    v = _magnitudes(fmt)
    a = x.abs()
    assert bool((a <= v[-1]).all()), "beyond max normal"
    hi = torch.searchsorted(v, a).clamp(max=len(v) - 1)
    lo = (hi - 1).clamp(min=0)
    down, up = a - v[lo], v[hi] - a
    code = torch.where(up < down, hi, torch.where(down < up, lo, torch.where(hi % 2 == 0, hi, lo)))
    return code | (torch.signbit(x).long() << (_BITS[fmt] - 1))


def cvt_sr_bracket(fmt: str, x):
    """(lo, hi) int64 codes: the neighbours of float64 `x` in `fmt`, towards
    and away from zero, equal where x is representable; sign as x."""
    import torch

    v = _magnitudes(fmt)
    a = x.abs()
    hi = torch.searchsorted(v, a).clamp(max=len(v) - 1)
    lo = torch.where(v[hi] == a, hi, hi - 1)
    sign = torch.signbit(x).long() << (_BITS[fmt] - 1)
    return lo | sign, hi | sign


def cvt_decode_value(fmt: str, codes):
    """float64 value of int64 codes (bf16: its 16-bit pattern)."""
    if fmt == "bf16":
        return _from_wide_bits(codes, "bf16")
    return mx_decode(CVT_FORMATS[fmt], codes)


def cvt_decode_expected(fmt: str, codes, exp, wide: str = "f32"):
    """(bits int64, ok): the wide type's pattern of value(code) * 2^exp, and
    whether that value is exact and normal (or zero) in the wide type."""
    import torch

    return _to_wide_bits(torch.ldexp(cvt_decode_value(fmt, codes), torch.as_tensor(exp)), wide)


def cvt_pack6(codes):
    """[..., 32] six-bit codes -> [..., 6] dwords (int64): code j at bits
    [6j, 6j + 6) of the 192, the packing mx_scale's kernels feed the MFMA."""
    import torch

    out = torch.zeros(codes.shape[:-1] + (6,), dtype=torch.int64)
    for j in range(32):
        word, at = divmod(6 * j, 32)
        c = codes[..., j].long() & 63
        out[..., word] |= (c << at) & _M32
        if at + 6 > 32:
            out[..., word + 1] |= c >> (32 - at)
    return out


def cvt_unpack6(words):
    """The inverse of cvt_pack6: [..., 6] dwords -> [..., 32] codes."""
    import torch

    out = torch.zeros(words.shape[:-1] + (32,), dtype=torch.int64)
    for j in range(32):
        word, at = divmod(6 * j, 32)
        c = (words[..., word].long() & _M32) >> at
        if at + 6 > 32:
            c = c | ((words[..., word + 1].long() & _M32) << (32 - at))
        out[..., j] = c & 63
    return out


# --------------------------------------------------------------------------
# operand sets
# --------------------------------------------------------------------------
def _encode_set(fmt: str, wide: str, exp: int):
    """Wide-type patterns (int64, sorted) of the encode operands at one scale
    exponent: see the module docstring."""
    import torch

    if fmt == "bf16":   # every mantissa in a handful of binades; exact, the tie, one ulp around
        e = torch.tensor([1, 64, 126, 127, 128, 200, 254]).view(-1, 1, 1)
        m = torch.arange(128).view(1, -1, 1)
        low = torch.tensor([0, 1, 0x7FFF, 0x8000, 0x8001, 0xFFFF]).view(1, 1, -1)
        bits = ((e << 23) | (m << 16) | low).flatten()
        bits = bits[bits < 0x7F7F8000]          # the last tie would round to infinity
    else:
        v = _magnitudes(fmt)
        base = torch.ldexp(torch.cat([v, (v[:-1] + v[1:]) / 2]), torch.tensor(exp))
        bits, ok = _to_wide_bits(base, wide)
        bits = bits[ok]
        bits = torch.cat([bits, bits + 1, torch.where(bits > 0, bits - 1, bits)])
        x = _from_wide_bits(bits, wide)
        _, ok = _to_wide_bits(x, wide)
        ok &= torch.isfinite(x) & (torch.ldexp(x, torch.tensor(-exp)).abs() <= v[-1])
        bits = bits[ok]
    bits = torch.unique(bits)
    return torch.cat([bits, bits | (1 << (_WIDE_BITS[wide] - 1))])


def _decode_set(fmt: str, wide: str, exp: int):
    codes = cvt_finite_codes(fmt)
    return codes[cvt_decode_expected(fmt, codes, exp, wide)[1]]


@functools.lru_cache(maxsize=None)
def cvt_elements(path: str):
    """The operand set of a path, element by element and before packing:
    (elements, exps, want) int64 tensors. `elements` are wide-type patterns
    (encode, sr) or codes (decode), `exps` the scale exponent of each, `want`
    the expected code (encode), wide-type pattern (decode) or bracket
    lo | hi << 8 (sr). Each scale's run is padded to whole entries by
    repeating its first element."""
    import torch

    kind, fmt, wide, scaled, pack, _ = _PATHS[path]
    elements, exps = [], []
    for s in cvt_scale_exps(path):
        el = _decode_set(fmt, wide, s) if kind == "dec" else _encode_set(fmt, wide, s)
        el = torch.cat([el, el[:1].expand(-len(el) % pack)])
        elements.append(el)
        exps.append(torch.full_like(el, s))
    elements, exps = torch.cat(elements), torch.cat(exps)
    if kind == "dec":
        want = cvt_decode_expected(fmt, elements, exps, wide)[0]
    else:
        x = torch.ldexp(_from_wide_bits(elements, wide), -exps)
        if kind == "enc":
            want = cvt_encode_expected(fmt, x)
        else:
            lo, hi = cvt_sr_bracket(fmt, x)
            want = lo | (hi << 8)
    return elements, exps, want


def _pack_fields(x, bits: int):
    """[entries, n] fields of `bits` bits -> [entries, n * bits / 32] dwords,
    field j at bit j * bits (bits divides 32)."""
    import torch

    per = 32 // bits
    x = x.view(x.shape[0], -1, per)
    return (x << (bits * torch.arange(per))).sum(dim=-1)


def cvt_old(entries: int):
    """The kernel's `old` destination of each entry, int64."""
    import numpy as np
    import torch

    e = np.arange(entries, dtype=np.uint32)
    old = _fmix32(e * np.uint32(0x9E3779B1) + np.uint32(0x85EBCA6B))
    return torch.from_numpy(old.astype(np.int64))


def _as_int32(x):
    import torch

    x = x.long() & _M32
    return torch.where(x >= (1 << 31), x - (1 << 32), x).to(torch.int32).contiguous()


@functools.lru_cache(maxsize=None)
def cvt_operands(path: str):
    """(inputs int32, scales float32, expected int32), on the CPU, as
    ops.cvt_sweep takes them (shared between callers: do not write to them)."""
    import torch

    kind, fmt, wide, scaled, pack, _ = _PATHS[path]
    elements, exps, want = (t.view(-1, pack) for t in cvt_elements(path))
    entries = elements.shape[0]
    scales = torch.ldexp(torch.ones(entries, dtype=torch.float64), exps[:, 0]).float().contiguous()
    old = cvt_old(entries)
    if kind == "dec":
        inputs = cvt_pack6(elements) if _BITS[fmt] == 6 else _pack_fields(elements, _BITS[fmt])
        expected = _pack_fields(want, _WIDE_BITS[wide])
    else:
        inputs = _pack_fields(elements, _WIDE_BITS[wide])
        if kind == "sr":
            expected = want
        elif fmt == "bf16":
            expected = _pack_fields(want, 16)
        elif _BITS[fmt] == 6:
            expected = cvt_pack6(want)
        else:     # the field lands where each select names; the rest keeps `old`
            width = 2 * _BITS[fmt]
            field = want[:, :1] | (want[:, 1:] << _BITS[fmt])
            shifts = width * torch.arange(32 // width)
            mask = ((1 << width) - 1) << shifts
            expected = (old.unsqueeze(1) & ~mask & _M32) | (field << shifts)
    return _as_int32(inputs.reshape(-1)), scales, _as_int32(expected.reshape(-1))


# --------------------------------------------------------------------------
# burn mirror
# --------------------------------------------------------------------------
_CARVE = {"fp8": (-6, 14), "bf8": (-14, 29), "fp6": (0, 2), "fp4": (0, 2), "bf16": (-100, 200)}


def _cvtb_step(section: str, s):
    """One step of the kernel's CvtBurnStep<section> on the 64 lanes at once
    (np.uint32[64]), through cvt_encode_expected and cvt_decode_expected."""
    import numpy as np
    import torch

    u32 = np.uint32
    k = ((s >> u32(3)) & u32(15)).astype(np.int64) - 8
    k2 = ((s >> u32(9)) & u32(15)).astype(np.int64) - 8
    nxt = s * u32(0x9E3779B1) + u32(0x7F4A7C15)
    emin, nexp = _CARVE[section]

    def hashed(x, mul):
        x = x * u32(mul)
        return x ^ (x >> u32(15))

    def carve(h, kk):    # float64 values of the carved f32
        e = emin + ((((h >> u32(23)) & u32(0xFF)).astype(np.int64) * nexp) >> 8)
        bits = (h & u32(0x807FFFFF)) | ((127 + e + kk).astype(u32) << u32(23))
        return torch.from_numpy(bits.view(np.float32).astype(np.float64))

    def f32_bits(code, kk):
        bits, ok = cvt_decode_expected(section, code, torch.from_numpy(kk), "f32")
        assert bool(ok.all())
        return bits.numpy().astype(u32)

    if section == "fp6":
        j = np.arange(32, dtype=u32).reshape(1, 32)
        h = hashed(s.reshape(64, 1) ^ (j * u32(0x85EBCA6B)), 0x9E3779B1)
        kk, kk2 = np.repeat(k.reshape(64, 1), 32, 1), np.repeat(k2.reshape(64, 1), 32, 1)
        code = cvt_encode_expected(section, torch.ldexp(carve(h, kk), torch.from_numpy(-kk)))
        p = cvt_pack6(code).numpy().astype(u32)
        q = f32_bits(code, kk2)
        x = nxt
        for i in range(6):
            x = x ^ _rotl32(p[:, i], 5 * i + 1)
        for jj in range(32):
            x = x ^ _rotl32(q[:, jj], jj % 31 + 1)
        return x
    h = np.stack([hashed(s, 0x85EBCA6B), hashed(s ^ u32(0xC2B2AE35), 0x27D4EB2F)], axis=1)
    kk, kk2 = np.repeat(k.reshape(64, 1), 2, 1), np.repeat(k2.reshape(64, 1), 2, 1)
    x = carve(h, kk)
    if section == "bf16":
        code = cvt_encode_expected("bf16", x).numpy().astype(u32)
        w = code[:, 0] | (code[:, 1] << u32(16))
        return nxt ^ w ^ _rotl32(w << u32(16), 7) ^ _rotl32(w & u32(0xFFFF0000), 19)
    code = cvt_encode_expected(section, torch.ldexp(x, torch.from_numpy(-kk)))
    d = f32_bits(code, kk2)
    c = code.numpy().astype(u32)
    w = c[:, 0] | (c[:, 1] << u32(_BITS[section]))
    return nxt ^ w ^ _rotl32(d[:, 0], 7) ^ _rotl32(d[:, 1], 19)


@functools.lru_cache(maxsize=None)
def cvt_burn_expected(section: str, seed: int, chain: int):
    """The 64 states (np.uint32, one per lane) every wave of ops.cvt_burn
    must hold after `chain` steps: the host mirror of the kernel."""
    import numpy as np

    if section not in _CVTB_ID:
        raise ValueError(f"unknown section {section!r}")
    lane = np.arange(64, dtype=np.uint32)
    start = np.uint32((int(seed) + (_CVTB_ID[section] + 16) * 0x9E3779B9) & _M32)
    s = _fmix32(start + lane * np.uint32(0x85EBCA6B))
    for _ in range(int(chain)):
        s = _cvtb_step(section, s)
    return s


# --------------------------------------------------------------------------
# summaries and reports
# --------------------------------------------------------------------------
def summarize_cvt_sweep(records, elapsed_ms: float, path: str, expected_simds: int) -> dict:
    """Turn the per-wave records of one ops.cvt_sweep launch into a verdict.

    records: [waves, 8] int32 rows {hw word, mismatched entries, lowest bad
    entry (-1), produced and expected dword there, checksum low / high word,
    0}. A wave is bad when it mismatched or when its checksum is not the
    majority's; it is attributed to the SIMD of its hw word. Pure numpy.
    """
    import numpy as np

    rec = np.asarray(records).reshape(-1, 8).astype(np.int64)
    simds_seen = units_seen(rec[:, 0], decode_hw_simd)
    odd = checksum_outliers(_u64_fields(rec, 5))
    bad = BadUnits()
    for row in rec[(rec[:, 1] != 0) | odd]:
        bad.add(decode_hw_simd(row[0]), {"waves": 1, "mismatched_entries": row[1]},
                (int(row[2]),) if row[1] != 0 else None)
    mismatched_waves = int((rec[:, 1] != 0).sum())
    first = rec[rec[:, 1] != 0][:1]
    return {
        "path": path,
        "elapsed_ms": float(elapsed_ms),
        "waves": int(rec.shape[0]),
        "simds_seen": simds_seen,
        "mismatched_waves": mismatched_waves,
        "checksum_spread": bool(odd.any()),
        "first_bad": ({"entry": int(first[0, 2]), "got": int(first[0, 3]) & _M32,
                       "want": int(first[0, 4]) & _M32} if len(first) else None),
        "bad_simds": bad.entries(("first_bad_entry",)),
        "ok": bool(mismatched_waves == 0 and not odd.any() and simds_seen >= expected_simds),
    }


def summarize_cvt_burn(records, elapsed_ms: float, section: str, chain: int, rounds: int,
                       expected_simds: int) -> dict:
    """summarize_valu_burn of an ops.cvt_burn launch (the record is the same)
    plus `gcvt_per_s`: 1e9 conversions per second, reported and never judged."""
    s = summarize_valu_burn(records, elapsed_ms, section, chain, rounds, expected_simds)
    done = _CVTB_PER_STEP[section] * 64.0 * s["waves"] * chain * rounds
    s["gcvt_per_s"] = done / (elapsed_ms * 1e-3) / 1e9 if elapsed_ms > 0 else 0.0
    return s


def cvt_sweep_report(device: int = 0, paths=CVT_PATHS, blocks: int = 2048) -> dict:
    """Every path's whole operand table on every SIMD. Returns {"paths":
    {path: summarize_cvt_sweep(...) + entries}, "ok", "bad_simds"}."""
    from . import _ops_on

    ops = _ops_on(device)
    expected_simds = 4 * ops.device_info(device)["multiProcessorCount"]
    out: dict = {"blocks": blocks, "paths": {}}
    bad = set()
    for path in paths:
        inputs, scales, expected = (t.cuda(device) for t in cvt_operands(path))
        records, ms = ops.cvt_sweep(path, inputs, scales, expected, blocks)
        s = summarize_cvt_sweep(records.cpu().numpy(), ms, path, expected_simds)
        s["entries"] = int(scales.numel())
        out["paths"][path] = s
        bad |= place_keys(s["bad_simds"], 5)
    out["ok"] = all(s["ok"] for s in out["paths"].values())
    out["bad_simds"] = place_dicts(bad)
    return out


def cvt_burn_report(device: int = 0, sections=CVT_BURN_SECTIONS, blocks: int = 2048,
                    chain: int = None, rounds: int = None, seed: int = 1, inject=None) -> dict:
    """Run the conversion burn for each section on one GPU. Returns
    {"sections": {section: summarize_cvt_burn(...)}, "ok", "bad_simds"}.
    chain and rounds default per section; `rounds` must be odd.
    `inject=(wave, round, lane, bit)` xors that bit into that lane's state (a
    harmless register-only fault) to exercise detection on healthy hardware."""
    import torch

    from . import _ops_on

    ops = _ops_on(device)
    inject_args = (-1, -1, -1, -1) if inject is None else tuple(int(v) for v in inject)
    expected_simds = 4 * ops.device_info(device)["multiProcessorCount"]
    out: dict = {"blocks": blocks, "sections": {}}
    bad = set()
    for section in sections:
        c = _CVTB_DEFAULTS[section][0] if chain is None else int(chain)
        r = _CVTB_DEFAULTS[section][1] if rounds is None else int(rounds)
        want = cvt_burn_expected(section, seed, c)
        expected = torch.from_numpy(want.view("int32").copy()).cuda(device)
        records, ms = ops.cvt_burn(section, expected, seed, blocks, c, r, *inject_args)
        s = summarize_cvt_burn(records.cpu().numpy(), ms, section, c, r, expected_simds)
        out["sections"][section] = s
        bad |= place_keys(s["bad_simds"], 5)
    out["ok"] = all(s["ok"] for s in out["sections"].values())
    out["bad_simds"] = place_dicts(bad)
    return out


def cvt_probe_report(device: int = 0) -> dict:
    """The conversion probe on one GPU: {"sweep": cvt_sweep_report, "burn":
    cvt_burn_report, "ok", "bad_simds"}, `ok` the AND and `bad_simds` the
    union of the two."""
    sweep = cvt_sweep_report(device)
    burn = cvt_burn_report(device)
    bad = place_keys(sweep["bad_simds"], 5) | place_keys(burn["bad_simds"], 5)
    return {"sweep": sweep, "burn": burn, "ok": bool(sweep["ok"] and burn["ok"]),
            "bad_simds": place_dicts(bad)}
