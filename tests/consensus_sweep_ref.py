"""Reference for the consensus sweep (csrc/hip/consensus_sweep.hip), written
from the sweep's description and the number formats, sharing nothing with the
C++: the step table (names, result words, operand kinds), the operand
generator (key -> fmix32 -> shaping), decoders of fp8, bf8, fp6, bf6, fp4, f16
and bf16, and the property checks the GPU tests hold a probe's dump to.

The sweep has no expected values: its verdict is a vote. What is checked
against this file is therefore the operands (bit-equal, on the CPU) and, on
the GPU, properties that hold whatever the unfixed bits are."""
import numpy as np

PARTS = ["trans", "div", "sr", "edge", "ldsx", "mfma", "smfmac"]
SEEDS = (0x1B873593, 0x9E3779B9)
BLOCK = 256
T = np.arange(BLOCK, dtype=np.uint64)
M32 = np.uint64(0xFFFFFFFF)


# ---------------------------------------------------------------- the hash
def fmix32(h):
    h = np.asarray(h, np.uint64) & M32
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85EBCA6B)) & M32
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xC2B2AE35)) & M32
    h ^= h >> np.uint64(16)
    return h


def hashv(seed, p, s, r, o):
    """h(o) of every thread of the workgroup."""
    return fmix32(np.uint64(seed) ^ (np.uint64(p << 28 | s << 20 | r << 12 | o << 8) | T))


def hashw(h, w):
    return h if w == 0 else fmix32((h + np.uint64((0x9E3779B9 * w) & 0xFFFFFFFF)) & M32)


def u(x):
    return np.uint64(x)


# ------------------------------------------------------------------ shaping
def f32_band(x, lo, n, sign=True):
    s = x & u(0x80000000) if sign else u(0)
    return s | (u(lo) + ((x >> u(23)) & u(0xFF)) % u(n)) << u(23) | (x & u(0x7FFFFF))


def f64_hi(x, lo, n, sign=True):
    s = x & u(0x80000000) if sign else u(0)
    return s | (u(lo) + ((x >> u(20)) & u(0x7FF)) % u(n)) << u(20) | (x & u(0xFFFFF))


def f16_band(y, lo, n, sign=True):
    s = y & u(0x8000) if sign else u(0)
    return s | (u(lo) + ((y >> u(10)) & u(31)) % u(n)) << u(10) | (y & u(0x3FF))


def bf16_band(y, lo, n, sign=True):
    s = y & u(0x8000) if sign else u(0)
    return s | (u(lo) + ((y >> u(7)) & u(0xFF)) % u(n)) << u(7) | (y & u(0x7F))


def bytes4(x, fp8):
    out = np.zeros_like(x)
    for i in range(4):
        b = (x >> u(8 * i)) & u(0xFF)
        if fp8:  # e4m3fn: 0x7f / 0xff are the NaNs
            b = np.where((b & u(0x7F)) == u(0x7F), b & u(0xF7), b)
        else:  # e5m2: exponent 31 is Inf / NaN
            b = np.where((b & u(0x7C)) == u(0x7C), b & u(0xBF), b)
        out |= b << u(8 * i)
    return out


def edge_float(c, s, m, mbits, emax, mid, midn):
    """Class c of a float format: quiet NaN with payload, signalling NaN,
    infinity, subnormal, zero, huge, tiny, middle."""
    quiet, inf = u(1 << (mbits - 1)), u(emax << mbits)
    sh = u(mbits)
    return np.select(
        [c == 0, c == 1, c == 2, c == 3, c == 4, c == 5, c == 6],
        [s | inf | quiet | m, s | inf | (m & (quiet - u(1))) | u(1), s | inf, s | m | u(1), s,
         s | (u(emax - 4) + m % u(4)) << sh | m, s | (u(1) + m % u(4)) << sh | m],
        s | (u(mid) + m % u(midn)) << sh | m)


def edge_f16(y):
    return edge_float((y >> u(10)) & u(7), y & u(0x8000), y & u(0x3FF), 10, 31, 12, 8)


def edge_bf16(y):
    return edge_float((y >> u(7)) & u(7), y & u(0x8000), y & u(0x7F), 7, 255, 120, 16)


def f32_bits_of_int(k):
    return np.asarray(k, np.float32).view(np.uint32).astype(np.uint64)


# target: (significand bits, lowest exponent used, exponents used, bias, exponent bits)
SR_TARGETS = {"fp8": (3, -6, 14), "bf8": (2, -12, 25), "fp4": (1, 0, 2), "fp6": (3, 0, 2), "bf6": (2, -2, 6),
              "f16": (10, -14, 29), "bf16": (7, -20, 41)}
SR_SOURCES = {"f32": (23, 127), "f16": (10, 15), "bf16": (7, 127)}


def sr_element(target, source, scaled, x, hs, r, el):
    mt, lo, n = SR_TARGETS[target]
    ms, bias = SR_SOURCES[source]
    L = ms - mt
    s = (hs % u(5)).astype(np.int64) - 2 if scaled else np.zeros(BLOCK, np.int64)
    e = (lo + (((x >> u(23)) & u(0xFF)) % u(n)).astype(np.int64) + s + bias).astype(np.uint64)
    top = (x >> u(8)) & u((1 << mt) - 1)
    rep = ((T + u(r + el)) & u(7)) == 0
    low = np.where(rep, u(0), u(1 << (L - 2)) + (x >> u(3)) % u((1 << (L - 1)) + 1))
    mant = top << u(L) | low
    if source == "f32":
        return (x & u(0x80000000)) | e << u(23) | mant
    return ((x >> u(16)) & u(0x8000)) | e << u(ms) | mant


def operand_word(kind, seed, p, s, r, o, w):
    """Word w of operand o of every thread: uint64 [256] holding 32-bit values."""
    h = hashv(seed, p, s, r, o)
    if isinstance(kind, tuple):
        _, target, source, scaled = kind
        hs = hashv(seed, p, s, r, 2)
        if source == "f32":
            return sr_element(target, source, scaled, hashw(h, w), hs, r, w)
        return (sr_element(target, source, scaled, hashw(h, 2 * w), hs, r, 2 * w) |
                sr_element(target, source, scaled, hashw(h, 2 * w + 1), hs, r, 2 * w + 1) << u(16))
    x = hashw(h, w)
    lo16, hi16 = x & u(0xFFFF), x >> u(16)
    if kind == "U32":
        return x
    if kind == "BIT":
        return x & u(1)
    if kind == "F32N":
        return f32_band(x, 1, 254)
    if kind == "F32NP":
        return f32_band(x, 1, 254, False)
    if kind == "F32X":
        return np.where(T & u(1), f32_band(x, 100, 34), f32_band(x, 1, 254))
    if kind == "F32REV":
        return f32_band(x, 97, 38)
    if kind == "F32B":
        return f32_band(x, 96, 63)
    if kind in ("F64N", "F64NP", "F64B"):
        if w == 0:
            return hashw(h, 1)
        return f64_hi(h, 992, 63) if kind == "F64B" else f64_hi(h, 1, 2046, kind == "F64N")
    if kind == "F16N":
        return f16_band(lo16, 1, 30)
    if kind == "F16NP":
        return f16_band(lo16, 1, 30, False)
    if kind == "PKF16":
        return f16_band(lo16, 8, 15) | f16_band(hi16, 8, 15) << u(16)
    if kind == "PKBF16":
        return bf16_band(lo16, 120, 15) | bf16_band(hi16, 120, 15) << u(16)
    if kind == "FP8W":
        return bytes4(x, True)
    if kind == "BF8W":
        return bytes4(x, False)
    if kind == "SCALE":
        return (u(125) + x % u(5)) << u(23)
    if kind == "SCALE8":
        out = np.zeros_like(x)
        for i in range(4):
            out |= (u(125) + ((x >> u(8 * i)) & u(0xFF)) % u(5)) << u(8 * i)
        return out
    if kind == "EXPI":
        return ((x % u(61)).astype(np.int64) - 30).astype(np.uint64) & M32
    if kind == "E32":
        return edge_float((x >> u(24)) & u(7), x & u(0x80000000), x & u(0x7FFFFF), 23, 255, 120, 16)
    if kind == "E16PK":
        return edge_f16(lo16) | edge_f16(hi16) << u(16)
    if kind == "EBFPK":
        return edge_bf16(lo16) | edge_bf16(hi16) << u(16)
    if kind == "EW32":
        sg, m, c = x & u(0x80000000), x & u(0x7FFFFF), (x >> u(24)) & u(7)
        return np.select([c == 0, c == 1, c == 2, c == 3], [sg | u(0x7FC00000) | m, sg | u(0x7F800000), sg | m | u(1), sg],
                         sg | (u(96) + m % u(64)) << u(23) | m)
    if kind == "F32U8":
        return f32_bits_of_int(((x % u(1216)).astype(np.int64) - 64) / 4.0)
    if kind == "F32NORM":
        return f32_band(x, 110, 19)
    if kind == "E64":
        c = (h >> u(24)) & u(7)
        if w:
            return edge_float(c, h & u(0x80000000), h & u(0xFFFFF), 20, 2047, 1016, 16)
        return np.where((c == 2) | (c == 4), u(0), hashw(h, 1))
    raise KeyError(kind)


# ------------------------------------------------------------ the step table
def SR(target, source, scaled=1):
    return ("SR", target, source, scaled)


def _step(part, name, words, *ops):
    """ops: (kind, words) of operands 0.., padded to four."""
    ops = list(ops) + [(None, 0)] * (4 - len(ops))
    return (part, name, words, ops)


def _steps():
    S = []
    one = lambda k: (k, 1)  # noqa: E731
    for name, k in [("v_exp_f32", "F32X"), ("v_log_f32", "F32NP"), ("v_rcp_f32", "F32N"), ("v_rsq_f32", "F32NP"),
                    ("v_sqrt_f32", "F32NP"), ("v_sin_f32", "F32REV"), ("v_cos_f32", "F32REV"),
                    ("v_rcp_iflag_f32", "F32N"), ("v_exp_legacy_f32", "F32X"), ("v_log_legacy_f32", "F32NP")]:
        S.append(_step("trans", name, 1, one(k)))
    for name, k in [("v_rcp_f64", "F64N"), ("v_rsq_f64", "F64NP"), ("v_sqrt_f64", "F64NP")]:
        S.append(_step("trans", name, 2, (k, 2)))
    for name, k in [("v_rcp_f16", "F16N"), ("v_rsq_f16", "F16NP"), ("v_sqrt_f16", "F16NP"), ("v_exp_f16", "F16N"),
                    ("v_log_f16", "F16NP")]:
        S.append(_step("trans", name, 1, one(k)))

    n32, b32, n64, b64 = one("F32N"), one("F32B"), ("F64N", 2), ("F64B", 2)
    S += [_step("div", "v_div_scale_f32", 2, n32, n32, n32),
          _step("div", "v_div_fmas_f32", 1, b32, b32, b32, one("BIT")),
          _step("div", "v_div_fixup_f32", 1, n32, n32, n32),
          _step("div", "div_f32", 1, n32, n32),
          _step("div", "v_div_scale_f64", 3, n64, n64, n64),
          _step("div", "v_div_fmas_f64", 2, b64, b64, b64, one("BIT")),
          _step("div", "v_div_fixup_f64", 2, n64, n64, n64),
          _step("div", "div_f64", 2, n64, n64),
          _step("div", "v_trig_preop_f64", 2, n64, one("U32")),
          _step("div", "v_mul_legacy_f32", 1, one("E32"), one("E32")),
          _step("div", "v_fma_legacy_f16", 1, one("E16PK"), one("E16PK"), one("E16PK")),
          _step("div", "v_mad_legacy_f16", 1, one("E16PK"), one("E16PK"), one("E16PK"))]
    S += [_step("div", f"v_cube{x}_f32", 1, b32, b32, b32) for x in ("id", "sc", "tc", "ma")]

    rnd, scale = one("U32"), one("SCALE")
    for t in ("fp8", "bf8", "f16", "bf16"):
        S.append(_step("sr", f"v_cvt_sr_{t}_f32", 1, (SR(t, "f32", 0), 1), rnd))
    for t in ("fp8", "bf8"):
        for src in ("f32", "f16", "bf16"):
            S.append(_step("sr", f"v_cvt_scalef32_sr_{t}_{src}", 1, (SR(t, src), 1), rnd, scale))
    for src, n in (("f32", 2), ("f16", 1), ("bf16", 1)):
        S.append(_step("sr", f"v_cvt_scalef32_sr_pk_fp4_{src}", 1, (SR("fp4", src), n), rnd, scale))
    for t in ("fp6", "bf6"):
        for src, n in (("f32", 32), ("f16", 16), ("bf16", 16)):
            S.append(_step("sr", f"v_cvt_scalef32_sr_pk32_{t}_{src}", 6, (SR(t, src), n), rnd, scale))
    S.append(_step("sr", "v_prng_b32", 1, one("U32")))

    e32, e16, ew = one("E32"), one("E16PK"), one("EW32")
    for name, n in [("v_add_f32", 2), ("v_mul_f32", 2), ("v_fma_f32", 3), ("v_min_f32", 2), ("v_max_f32", 2),
                    ("v_med3_f32", 3), ("v_minimum3_f32", 3), ("v_maximum3_f32", 3)]:
        S.append(_step("edge", name, 1, *[e32] * n))
    S.append(_step("edge", "v_ldexp_f32", 1, e32, one("EXPI")))
    for name in ("v_frexp_mant_f32", "v_frexp_exp_i32_f32", "v_fract_f32", "v_trunc_f32", "v_rndne_f32", "v_floor_f32",
                 "v_ceil_f32"):
        S.append(_step("edge", name, 1, e32))
    S.append(_step("edge", "v_sub_f32", 1, e32, e32))
    S += [_step("edge", f"v_pk_{op}_f32", 2, *[("E32", 2)] * n) for op, n in (("add", 2), ("mul", 2), ("fma", 3))]
    S += [_step("edge", "v_min3_f32", 1, e32, e32, e32), _step("edge", "v_max3_f32", 1, e32, e32, e32)]
    S += [_step("edge", f"v_cmp_{c}_f32", 1, e32, e32) for c in ("lt", "eq", "le", "gt", "lg", "ge")]
    S.append(_step("edge", "v_cmp_class_f32", 1, e32, one("U32")))
    for name, n in [("v_add_f16", 2), ("v_mul_f16", 2), ("v_fma_f16", 3), ("v_pk_add_f16", 2), ("v_pk_mul_f16", 2),
                    ("v_pk_fma_f16", 3), ("v_pk_min_f16", 2), ("v_pk_max_f16", 2)]:
        S.append(_step("edge", name, 1, *[e16] * n))
    S += [_step("edge", "v_pk_minimum3_f16", 1, e16, e16, e16), _step("edge", "v_pk_maximum3_f16", 1, e16, e16, e16),
          _step("edge", "v_fma_mix_f32", 1, e16, e16, e32), _step("edge", "v_fma_mixlo_f16", 1, e16, e16, e16)]
    S += [_step("edge", "v_cvt_f16_f32", 1, ew), _step("edge", "v_cvt_f32_f16", 1, e16),
          _step("edge", "v_cvt_pk_bf16_f32", 1, ew, ew), _step("edge", "v_cvt_pkrtz_f16_f32", 1, ew, ew),
          _step("edge", "v_cvt_pk_fp8_f32", 1, ew, ew), _step("edge", "v_cvt_pk_bf8_f32", 1, ew, ew),
          _step("edge", "v_cvt_f32_fp8", 1, one("U32")), _step("edge", "v_cvt_f32_bf8", 1, one("U32")),
          _step("edge", "v_cvt_i32_f32", 1, ew), _step("edge", "v_cvt_u32_f32", 1, ew),
          _step("edge", "v_cvt_scalef32_pk_fp8_f32", 1, ew, ew, scale),
          _step("edge", "v_cvt_scalef32_pk_bf8_f32", 1, ew, ew, scale),
          _step("edge", "v_cvt_scalef32_pk_fp4_f32", 1, ew, ew, scale),
          _step("edge", "v_cvt_scalef32_pk32_fp6_f16", 6, ("E16PK", 16), scale),
          _step("edge", "v_cvt_scalef32_pk32_bf6_f16", 6, ("E16PK", 16), scale),
          _step("edge", "v_cvt_scalef32_pk32_fp6_bf16", 6, ("EBFPK", 16), scale),
          _step("edge", "v_cvt_scalef32_pk32_bf6_bf16", 6, ("EBFPK", 16), scale),
          _step("edge", "v_cvt_scalef32_2xpk16_fp6_f32", 6, ("EW32", 16), ("EW32", 16), scale),
          _step("edge", "v_cvt_scalef32_2xpk16_bf6_f32", 6, ("EW32", 16), ("EW32", 16), scale),
          _step("edge", "v_cvt_pk_u8_f32", 1, one("F32U8"), one("U32"), one("U32")),
          _step("edge", "v_cvt_pknorm_i16_f32", 1, one("F32NORM"), one("F32NORM")),
          _step("edge", "v_cvt_pknorm_u16_f32", 1, one("F32NORM"), one("F32NORM"))]
    S += [_step("edge", "v_cvt_rpi_i32_f32", 1, ew), _step("edge", "v_cvt_flr_i32_f32", 1, ew),
          _step("edge", "v_cvt_f64_f32", 2, e32), _step("edge", "v_cvt_f32_f64", 1, ("E64", 2)),
          _step("edge", "v_cvt_i32_f64", 1, ("E64", 2)), _step("edge", "v_cvt_pk_f16_f32", 1, ew, ew)]
    for f in ("fp8", "bf8"):  # the byte selects 1..3 (0 is above), then the packed and the scaled widening
        S += [_step("edge", f"v_cvt_f32_{f}", 1, one("U32"))] * 3
        S += [_step("edge", f"v_cvt_pk_f32_{f}", 2, one("U32")),
              _step("edge", f"v_cvt_scalef32_pk_f32_{f}", 2, one("U32"), scale)]
    S.append(_step("edge", "v_cvt_scalef32_pk_f32_fp4", 2, one("U32"), scale))
    S += [_step("edge", f"v_cvt_scalef32_pk32_f32_{f}", 32, ("U32", 6), scale) for f in ("fp6", "bf6")]

    tile = ("U32", 8)
    S += [_step("ldsx", "ds_read_b64_tr_b8", 2, tile)] * 2 + [_step("ldsx", "ds_read_b64_tr_b4", 2, tile)] * 2
    S += [_step("ldsx", "ds_read_b96_tr_b6", 3, tile)] * 2
    S += [_step("ldsx", f"ds_{op}_rtn_f32", 2, b32, b32) for op in ("add", "min", "max")]
    S += [_step("ldsx", f"ds_{op}_rtn_f64", 4, b64, b64) for op in ("add", "min", "max")]
    S += [_step("ldsx", "ds_pk_add_rtn_f16", 2, one("PKF16"), one("PKF16")),
          _step("ldsx", "ds_pk_add_rtn_bf16", 2, one("PKBF16"), one("PKBF16")),
          _step("ldsx", "ds_cmpst_rtn_f32", 2, b32, b32, b32)]

    def mfma(name, words, ka, na, kb, nb, kc="F32B", scales=False):
        ops = [(ka, na), (kb, nb), (kc, words)] + ([("SCALE8", 2)] if scales else [])
        return _step("mfma", name, words, *ops)

    S += [mfma("v_mfma_f32_16x16x32_f16", 4, "PKF16", 4, "PKF16", 4),
          mfma("v_mfma_f32_16x16x32_bf16", 4, "PKBF16", 4, "PKBF16", 4),
          mfma("v_mfma_f32_16x16x16_f16", 4, "PKF16", 2, "PKF16", 2),
          mfma("v_mfma_f32_16x16x16_bf16", 4, "PKBF16", 2, "PKBF16", 2),
          mfma("v_mfma_f32_16x16x32_fp8_fp8", 4, "FP8W", 2, "FP8W", 2),
          mfma("v_mfma_f32_16x16x32_bf8_bf8", 4, "BF8W", 2, "BF8W", 2),
          mfma("v_mfma_f32_16x16x32_fp8_bf8", 4, "FP8W", 2, "BF8W", 2),
          mfma("v_mfma_f32_16x16x32_bf8_fp8", 4, "BF8W", 2, "FP8W", 2),
          mfma("v_mfma_f32_32x32x16_fp8_bf8", 16, "FP8W", 2, "BF8W", 2),
          mfma("v_mfma_f32_32x32x16_bf8_fp8", 16, "BF8W", 2, "FP8W", 2),
          mfma("v_mfma_i32_16x16x64_i8", 4, "U32", 4, "U32", 4, "U32"),
          mfma("v_mfma_i32_16x16x32_i8", 4, "U32", 2, "U32", 2, "U32"),
          mfma("v_mfma_f32_16x16x4_f32", 4, "F32B", 1, "F32B", 1), mfma("v_mfma_f32_4x4x4_16b_f16", 4, "PKF16", 2, "PKF16", 2),
          mfma("v_mfma_f32_4x4x4_16b_bf16", 4, "PKBF16", 2, "PKBF16", 2),
          mfma("v_mfma_f32_4x4x1_16b_f32", 4, "F32B", 1, "F32B", 1),
          mfma("v_mfma_i32_4x4x4_16b_i8", 4, "U32", 1, "U32", 1, "U32"),
          mfma("v_mfma_f64_4x4x4_4b_f64", 2, "F64B", 2, "F64B", 2, "F64B"),
          mfma("v_mfma_f32_16x16x128_f8f6f4", 4, "FP8W", 8, "FP8W", 8),
          mfma("v_mfma_f32_16x16x128_f8f6f4", 4, "BF8W", 8, "U32", 4),
          mfma("v_mfma_f32_16x16x128_f8f6f4", 4, "U32", 6, "U32", 6),
          mfma("v_mfma_f32_32x32x64_f8f6f4", 16, "FP8W", 8, "FP8W", 8),
          mfma("v_mfma_f32_32x32x64_f8f6f4", 16, "BF8W", 8, "U32", 6),
          mfma("v_mfma_scale_f32_16x16x128_f8f6f4", 4, "FP8W", 8, "FP8W", 8, scales=True),
          mfma("v_mfma_scale_f32_16x16x128_f8f6f4", 4, "BF8W", 8, "U32", 4, scales=True),
          mfma("v_mfma_scale_f32_32x32x64_f8f6f4", 16, "FP8W", 8, "U32", 6, scales=True)]

    def smfmac(name, words, ka, kb, kc="F32B"):
        # Both abid encodings run on the same operands: two result tiles of `words`.
        return _step("smfmac", name, 2 * words, (ka, 4), (kb, 8), ("U32", 1), (kc, words))

    S += [smfmac("v_smfmac_f32_16x16x64_f16", 4, "PKF16", "PKF16"), smfmac("v_smfmac_f32_16x16x64_bf16", 4, "PKBF16", "PKBF16"),
          smfmac("v_smfmac_f32_32x32x32_f16", 16, "PKF16", "PKF16"), smfmac("v_smfmac_f32_32x32x32_bf16", 16, "PKBF16", "PKBF16"),
          smfmac("v_smfmac_i32_16x16x128_i8", 4, "U32", "U32", "U32"),
          smfmac("v_smfmac_i32_32x32x64_i8", 16, "U32", "U32", "U32")]
    for shape, words in (("16x16x128", 4), ("32x32x64", 16)):
        for a, b in (("fp8", "fp8"), ("fp8", "bf8"), ("bf8", "fp8"), ("bf8", "bf8")):
            S.append(smfmac(f"v_smfmac_f32_{shape}_{a}_{b}", words, a.upper() + "W", b.upper() + "W"))
    return S


STEPS = _steps()
# The steps that are sequences, by the instructions they are about.
SEQUENCES = {"div_f32": ["v_div_scale_f32", "v_rcp_f32", "v_fma_f32", "v_div_fmas_f32", "v_div_fixup_f32"],
             "div_f64": ["v_div_scale_f64", "v_rcp_f64", "v_fma_f64", "v_div_fmas_f64", "v_div_fixup_f64"]}


def steps_of(part):
    return [s for s in STEPS if s[0] == part]


def shape(part):
    """(steps, result words per round, operand words per round)."""
    st = steps_of(part)
    return len(st), sum(s[2] for s in st), sum(n for s in st for _, n in s[3])


def rows_of(part, index):
    """The first result row of step `index` of `part` and its result words."""
    st = steps_of(part)
    return sum(s[2] for s in st[:index]), st[index][2]


def step_index(part, name, nth=0):
    return [i for i, s in enumerate(steps_of(part)) if s[1] == name][nth]


def step_operands(part, index, seed, r):
    """The operands of one step in one round: a list (one per operand) of uint32 [words, 256]."""
    p = PARTS.index(part)
    ops = steps_of(part)[index][3]
    return [np.stack([operand_word(k, seed, p, index, r, o, w) for w in range(n)]).astype(np.uint32)
            for o, (k, n) in enumerate(ops) if n]


def operands(part, seed, rounds):
    """What xs_consensus_operands returns: uint32 [rounds, operand words, 256]."""
    out = np.zeros((rounds, shape(part)[2], BLOCK), np.uint32)
    for r in range(rounds):
        row = 0
        for i in range(len(steps_of(part))):
            for words in step_operands(part, i, seed, r):
                out[r, row:row + len(words)] = words
                row += len(words)
    return out


def digest(dump):
    """The workgroup digest of a probe's dump [rounds, rows, 256]: sum(got x (2 idx + 1)) mod 2^32."""
    flat = dump.reshape(-1).astype(np.uint64)
    idx = np.arange(flat.size, dtype=np.uint64)
    return int((flat * ((u(2) * idx + u(1)) & M32) & M32).sum() & M32)


# ----------------------------------------------------------------- decoders
def decode_small(code, ebits, mbits, bias):
    """A sign / exponent / significand code without Inf or NaN (fp4, fp6, bf6, and the finite codes of fp8 / bf8)."""
    code = np.asarray(code, np.int64)
    s = np.where(code >> (ebits + mbits) & 1, -1.0, 1.0)
    e = code >> mbits & ((1 << ebits) - 1)
    m = code & ((1 << mbits) - 1)
    return s * np.where(e == 0, m * 2.0 ** (1 - bias - mbits), (1 + m * 2.0 ** -mbits) * 2.0 ** (e - bias))


FORMATS = {"fp8": (4, 3, 7), "bf8": (5, 2, 15), "fp6": (2, 3, 1), "bf6": (3, 2, 3), "fp4": (2, 1, 1),
           "f16": (5, 10, 15), "bf16": (8, 7, 127)}


def decode(fmt, code):
    """The finite value of a code of `fmt`, as float64."""
    return decode_small(code, *FORMATS[fmt])


def f32_of(bits):
    return np.asarray(bits, np.uint32).view(np.float32).astype(np.float64)


def f64_of(lo, hi):
    return (np.asarray(hi, np.uint64) << u(32) | np.asarray(lo, np.uint64)).view(np.float64)


def neighbours(fmt, value):
    """The largest code value of `fmt` at or below |value| and the smallest at or above it, signed like value."""
    ebits, mbits, _ = FORMATS[fmt]
    grid = np.unique(np.abs(decode(fmt, np.arange(1 << (ebits + mbits)))))
    grid = grid[np.isfinite(grid)]
    a = np.abs(value)
    below = grid[np.searchsorted(grid, a, side="right") - 1]
    above = grid[np.minimum(np.searchsorted(grid, a, side="left"), len(grid) - 1)]
    s = np.sign(value)
    return s * below, s * above


def sr_values(fmt, source, words):
    """The float64 values of an SR operand [words, 256] -> [elements, 256]."""
    if source == "f32":
        return f32_of(words)
    halves = np.stack([h for w in words for h in (w & 0xFFFF, w >> 16)])
    return decode(source, halves)


def unpack(words, bits, count):
    """`count` codes of `bits` bits each, packed from bit 0 of words[0] up: [words, 256] -> [count, 256]."""
    big = sum(words[i].astype(object) << (32 * i) for i in range(len(words)))
    return np.stack([np.array([(int(b) >> (bits * k)) & ((1 << bits) - 1) for b in big], np.int64) for k in range(count)])


# ---------------------------------------------------------- property checks
# Each takes a probe's dump [rounds, rows, 256] of its part at `seed` and
# returns findings; an empty list (or a dict of figures) is a pass.
def step_results(part, dump, index, r):
    row, n = rows_of(part, index)
    return dump[r, row:row + n]


def _round_to(width, x):
    return np.asarray(x, np.float64).astype({16: np.float16, 32: np.float32, 64: np.float64}[width])


def _bits_to(width, words):
    if width == 64:
        return f64_of(words[0], words[1])
    if width == 32:
        return np.asarray(words[0], np.uint32).view(np.float32)
    return (np.asarray(words[0], np.uint32) & 0xFFFF).astype(np.uint16).view(np.float16)


def _turns(x):
    return 2 * np.pi * np.fmod(x, 1.0)  # x is exact in float64 and so is its fraction


# name -> (width, f(x) in extended precision, absolute error?)
TRANS = {
    "v_exp_f32": (32, np.exp2, False), "v_log_f32": (32, np.log2, False), "v_rcp_f32": (32, lambda x: 1 / x, False),
    "v_rsq_f32": (32, lambda x: 1 / np.sqrt(x), False), "v_sqrt_f32": (32, np.sqrt, False),
    "v_sin_f32": (32, lambda x: np.sin(_turns(x)), True), "v_cos_f32": (32, lambda x: np.cos(_turns(x)), True),
    "v_rcp_iflag_f32": (32, lambda x: 1 / x, False),
    "v_rcp_f64": (64, lambda x: 1 / x, False), "v_rsq_f64": (64, lambda x: 1 / np.sqrt(x), False),
    "v_sqrt_f64": (64, np.sqrt, False),
    "v_rcp_f16": (16, lambda x: 1 / x, False), "v_rsq_f16": (16, lambda x: 1 / np.sqrt(x), False),
    "v_sqrt_f16": (16, np.sqrt, False), "v_exp_f16": (16, np.exp2, False), "v_log_f16": (16, np.log2, False),
}


def trans_errors(dump, seed):
    """{name: the largest error over the dump}: in ULP of the width at the
    reference (numpy in extended precision, rounded once to the width), for sin
    and cos the absolute error. Only lanes whose reference is a finite, non-zero
    normal of the width are measured: what the unit does with a result that
    underflows or overflows the width is left to the vote."""
    out = {}
    for i, (_, name, _, ops) in enumerate(steps_of("trans")):
        if name not in TRANS:
            continue
        width, fn, absolute = TRANS[name]
        worst = 0.0
        for r in range(dump.shape[0]):
            x = _bits_to(width, step_operands("trans", i, seed, r)[0]).astype(np.longdouble)
            got = _bits_to(width, step_results("trans", dump, i, r)).astype(np.float64)
            with np.errstate(all="ignore"):
                exact = fn(x)
                want = _round_to(width, exact)
                tiny = np.finfo(want.dtype).tiny
                ok = np.isfinite(want) & (np.abs(want) >= tiny)
                want64 = want.astype(np.float64)
                err = np.abs(got - want64) if absolute else np.abs(got - want64) / np.spacing(np.abs(want)).astype(np.float64)
            err = np.where(np.isnan(err), np.inf, err)
            assert ok.sum() >= BLOCK // 4, (name, int(ok.sum()))
            worst = max(worst, float(err[ok].max()))
        out[name] = worst
    return out


def sr_findings(dump, seed):
    """Every result must be one of the two neighbours of the exact scaled value
    in the target format (equal to it where it is representable), and across
    the operands in the middle of the gap both directions must occur."""
    bad = []
    for i, (_, name, nres, ops) in enumerate(steps_of("sr")):
        if name == "v_prng_b32":
            continue
        _, target, source, scaled = ops[0][0]
        ebits, mbits, _ = FORMATS[target]
        bits = 1 + ebits + mbits
        up = down = 0
        for r in range(dump.shape[0]):
            o = step_operands("sr", i, seed, r)
            x = sr_values(target, source, o[0]) / (f32_of(o[2][0]) if scaled else 1.0)
            res = step_results("sr", dump, i, r)
            if nres == 6:
                codes = unpack(res, 6, 32)
            elif target == "fp4":
                codes = unpack(res, 4, 2)
            else:
                codes = (res[:1] & ((1 << bits) - 1)).astype(np.int64)
            x = x[:len(codes)]  # a single conversion of a 16-bit source takes the low half
            got = decode(target, codes)
            lo, hi = neighbours(target, x)
            wrong = (got != lo) & (got != hi)
            for e, t in np.argwhere(wrong)[:4]:
                bad.append(f"{name} round {r} element {e} thread {t}: {x[e, t]!r} -> {got[e, t]!r}, "
                           f"not {lo[e, t]!r} or {hi[e, t]!r}")
            mid = hi != lo
            up += int((mid & (got == hi)).sum())
            down += int((mid & (got == lo)).sum())
        if not (up and down):
            bad.append(f"{name}: {up} rounded away from zero, {down} towards it")
    return bad


def _same_class(got, want):
    """IEEE-754 fixes the class: NaN where NaN is due, else the same bits where an infinity is due."""
    got, want = np.asarray(got), np.asarray(want)
    return (np.isnan(got) == np.isnan(want)) & (~np.isinf(want) | (got == want)) & (np.isinf(got) <= np.isinf(want))


def _bf16_of(halves):
    return (np.asarray(halves, np.uint32) << 16).astype(np.uint32).view(np.float32)


def _edge_checks():
    """name -> (operand decoders, result decoder, numpy function, how much IEEE-754 fixes).
    A decoder takes an operand's or the result's words [n, 256] and returns the
    float lanes [k, 256]. "class": NaN exactly where NaN is due, an infinity
    (with its sign) exactly where one is due. "from": the same, but an infinity
    is only held where an operand was one, the reference rounding twice or the
    format's overflow being the instruction's own. "nan": NaN in gives NaN out."""
    f32 = lambda w: np.asarray(w, np.uint32).view(np.float32)  # noqa: E731
    lo = lambda w: (np.asarray(w[:1], np.uint32) & 0xFFFF).astype(np.uint16).view(np.float16)  # noqa: E731
    hi = lambda w: (np.asarray(w[:1], np.uint32) >> 16).astype(np.uint16).view(np.float16)  # noqa: E731
    both = lambda w: np.concatenate([lo(w), hi(w)])  # noqa: E731
    bf = lambda w: _bf16_of(np.concatenate([w[:1] & 0xFFFF, w[:1] >> 16]))  # noqa: E731
    f64 = lambda w: f64_of(w[0], w[1])[None]  # noqa: E731
    wide = lambda *x: [v.astype(np.float64) for v in x]  # noqa: E731
    fma64 = lambda a, b, c: (lambda x: x[0] * x[1] + x[2])(wide(a, b, c))  # noqa: E731
    return {
        "v_add_f32": ([f32, f32], f32, np.add, "class"), "v_sub_f32": ([f32, f32], f32, np.subtract, "class"),
        "v_mul_f32": ([f32, f32], f32, np.multiply, "class"),
        "v_fma_f32": ([f32, f32, f32], f32, lambda a, b, c: fma64(a, b, c).astype(np.float32), "from"),
        "v_pk_add_f32": ([f32, f32], f32, np.add, "class"), "v_pk_mul_f32": ([f32, f32], f32, np.multiply, "class"),
        "v_pk_fma_f32": ([f32, f32, f32], f32, lambda a, b, c: fma64(a, b, c).astype(np.float32), "from"),
        "v_ldexp_f32": ([f32, lambda w: np.asarray(w, np.uint32).view(np.int32)], f32,
                        lambda a, e: np.ldexp(a, e).astype(np.float32), "class"),
        "v_trunc_f32": ([f32], f32, np.trunc, "class"), "v_rndne_f32": ([f32], f32, np.rint, "class"),
        "v_floor_f32": ([f32], f32, np.floor, "class"), "v_ceil_f32": ([f32], f32, np.ceil, "class"),
        "v_fract_f32": ([f32], f32, lambda a: a, "nan"),
        "v_add_f16": ([lo, lo], lo, np.add, "class"), "v_mul_f16": ([lo, lo], lo, np.multiply, "class"),
        "v_fma_f16": ([lo, lo, lo], lo, lambda a, b, c: fma64(a, b, c).astype(np.float16), "from"),
        "v_pk_add_f16": ([both, both], both, np.add, "class"), "v_pk_mul_f16": ([both, both], both, np.multiply, "class"),
        "v_pk_fma_f16": ([both, both, both], both, lambda a, b, c: fma64(a, b, c).astype(np.float16), "from"),
        "v_cvt_f16_f32": ([f32], lo, lambda a: a.astype(np.float16), "class"),
        "v_cvt_f32_f16": ([lo], f32, lambda a: a.astype(np.float32), "class"),
        "v_cvt_pk_f16_f32": ([f32, f32], both, lambda x: x.astype(np.float16), "class"),
        "v_cvt_pkrtz_f16_f32": ([f32, f32], both, lambda x: x.astype(np.float16), "from"),
        "v_cvt_pk_bf16_f32": ([f32, f32], bf, lambda x: x, "from"),
        "v_cvt_f64_f32": ([f32], f64, lambda a: a.astype(np.float64), "class"),
        "v_cvt_f32_f64": ([f64], f32, lambda a: a.astype(np.float32), "class"),
    }


def edge_findings(dump, seed):
    """The classes IEEE-754 fixes, on every lane and half of the steps of _edge_checks(); payloads are the vote's."""
    bad = []
    for name, (srcs, dst, fn, how) in _edge_checks().items():
        i = step_index("edge", name)
        seen_nan = seen_inf = 0
        for r in range(dump.shape[0]):
            ins = [src(o) for src, o in zip(srcs, step_operands("edge", i, seed, r))]
            if name.startswith("v_cvt_pk"):  # two sources, each to its own half: one operand of two lanes
                ins = [np.concatenate(ins)]
            got = dst(step_results("edge", dump, i, r))
            with np.errstate(all="ignore"):
                want = np.asarray(fn(*ins))
            nan_in = np.any([np.isnan(x) for x in ins], 0)
            if how == "nan":
                ok = ~nan_in | np.isnan(got)
            elif how == "from":
                from_inf = np.isinf(want) & np.any([np.isinf(x) for x in ins], 0)
                ok = (np.isnan(got) == np.isnan(want)) & (~from_inf | (got == want))
            else:
                ok = _same_class(got, want)
            seen_nan += int(np.isnan(want).sum())
            seen_inf += int(np.isinf(want).sum())
            for e, t in np.argwhere(~ok)[:4]:
                bad.append(f"{name} round {r} lane {e} thread {t}: {[x[e, t] for x in ins]} -> {got[e, t]!r}, "
                           f"class of {want[e, t]!r} expected")
        if not (seen_nan and seen_inf):
            bad.append(f"{name}: the operands led to {seen_nan} NaNs and {seen_inf} infinities")
    return bad


def div_findings(dump, seed):
    """The full division sequences against numpy's correctly rounded quotient, bit for bit."""
    bad = []
    for name, width in (("div_f32", 32), ("div_f64", 64)):
        i = step_index("div", name)
        for r in range(dump.shape[0]):
            a, b = (_bits_to(width, o) for o in step_operands("div", i, seed, r))
            with np.errstate(all="ignore"):
                want = a / b
            res = step_results("div", dump, i, r)
            got = _bits_to(width, res)
            view = np.uint64 if width == 64 else np.uint32
            wrong = got.view(view) != want.view(view)
            for t in np.argwhere(wrong).ravel()[:4]:
                bad.append(f"{name} round {r} thread {t}: {a[t]!r} / {b[t]!r} = {got[t]!r}, want {want[t]!r}")
    return bad
