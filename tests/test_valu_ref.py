"""The VALU sweep's design claims, checked on the reference alone
(tests/valu_sweep_ref.py): what csrc/hip/valu_sweep.hip's header says about its
keys, operand bands, edge rounds and exact classes."""
from fractions import Fraction

import numpy as np
import pytest

import valu_sweep_ref as ref

ROUNDS = 8
FLOAT_RESULT = {  # steps whose result words are one float each, or packed floats
    "f32": (ref.F32, 1), "f64": (ref.F64, 1), "f16": (ref.F16, 2)}


NAMED = {"int": ("v_sad_u8", "v_msad_u8"), "cvt": ("v_cvt_pknorm_i16_f32", "v_cvt_scalef32_pk32_f32_fp6")}


def test_units_steps_and_shapes_agree():
    assert list(ref.STEPS) == ref.UNITS == list(ref.SHAPES) and len(ref.UNITS) == 8
    total = 0
    for u in ref.UNITS:
        steps, words = ref.SHAPES[u]
        assert steps == len(ref.STEPS[u]) == len(set(ref.STEPS[u])) and steps < 256
        assert words == len(ref.row_names(u)) == ref.expected(u, ref.SEEDS[0], 1).shape[1]
        assert all(1 <= s[1] <= 2 for s in ref.STEPS_FULL[u])
        assert all(n in ref.STEPS[u] for n in NAMED.get(u, ()))
        total += steps
    assert total <= 192  # the record's step mask


def test_keys_are_distinct():
    k = ref.all_keys(rounds=64)
    assert len(np.unique(k)) == len(k)
    assert int(k.max()) < 1 << 31


F32x2 = [(0, ref.F32), (32, ref.F32)]
# Float results of the cvt unit: (bit offset, format) of every float in the result.
CVT_FLOATS = {
    "v_cvt_f32_i32": [(0, ref.F32)], "v_cvt_f32_u32": [(0, ref.F32)], "v_cvt_f64_f32": [(0, ref.F64)],
    "v_cvt_f32_f64": [(0, ref.F32)], "v_cvt_f64_i32": [(0, ref.F64)],
    **{f"v_cvt_f32_ubyte{i}": [(0, ref.F32)] for i in range(4)},
    "v_cvt_f16_f32": [(0, ref.F16)], "v_cvt_f32_f16": [(0, ref.F32)],
    "v_cvt_pk_f16_f32": [(0, ref.F16), (16, ref.F16)], "v_cvt_pkrtz_f16_f32": [(0, ref.F16), (16, ref.F16)],
    "v_cvt_pk_bf16_f32": [(0, ref.BF16), (16, ref.BF16)],
    "v_cvt_pk_fp8_f32": [(0, ref.E4M3), (8, ref.E4M3)], "v_cvt_pk_bf8_f32": [(0, ref.E5M2), (8, ref.E5M2)],
    **{f"v_cvt_f32_{f}:{i}": [(0, ref.F32)] for f in ("fp8", "bf8") for i in range(4)},
    "v_cvt_pk_f32_fp8": F32x2, "v_cvt_scalef32_pk_fp8_f32": [(0, ref.E4M3), (8, ref.E4M3)],
    "v_cvt_scalef32_pk_f32_fp8": F32x2, "v_cvt_scalef32_pk_f32_fp4": F32x2,
}
# Of e2m1's eight magnitudes one, 0.5, is its subnormal: v_cvt_scalef32_pk_fp4_f32 cannot keep off it, and the
# format has neither Inf nor NaN. v_cvt_scalef32_pk32_f32_fp6 returns folds; its 32 floats are checked unfolded.
CVT_NOT_FLOAT = {"v_cvt_i32_f32", "v_cvt_u32_f32", "v_cvt_rpi_i32_f32", "v_cvt_flr_i32_f32", "v_cvt_i32_f64",
                 "v_cvt_pk_u8_f32", "v_cvt_pk_i16_i32", "v_cvt_pk_u16_u32", "v_cvt_pknorm_i16_f32", "v_ashr_pk_i8_i32",
                 "v_ashr_pk_u8_i32", "v_cvt_scalef32_pk_fp4_f32", "v_cvt_scalef32_pk32_f32_fp6"}


def float_layout(unit, name, words):
    """(bit offset, format) of every float in a step's result; [] for an integer or boolean result."""
    if unit in ("f32", "f64"):
        if "_cmp_" in name or "frexp_exp" in name:
            return []
        return [(0, ref.F64)] if unit == "f64" else F32x2[:words]
    if unit == "f16":
        if name == "v_fma_mix_f32":
            return [(0, ref.F32)]
        return [(0, ref.F16), (16, ref.F16)] if "_pk_" in name else [(0, ref.F16)]
    if unit == "dot":
        return [(0, ref.F32)] if name.startswith("v_dot2") else []
    if unit == "cvt":
        assert (name in CVT_FLOATS) != (name in CVT_NOT_FLOAT), name
        return CVT_FLOATS.get(name, [])
    if unit == "trans":
        fmt = {"f32": ref.F32, "f64": ref.F64, "f16": ref.F16}[name.split(":")[0].rsplit("_", 1)[1]]
        return [(0, fmt)]
    return []


def zero_or_normal(bits, fmt):
    """An exact zero (a - a) is allowed; everything else is a normal, finite number."""
    if bits & ((1 << sum(fmt)) - 1) == 0:
        return True
    if fmt == ref.E4M3:  # e4m3fn: the top exponent holds numbers, all ones is its one NaN
        return bits >> 3 & 15 != 0 and bits & 0x7F != 0x7F
    return ref.is_normal_finite(bits, fmt)


@pytest.mark.parametrize("seed", ref.SEEDS)
def test_no_float_result_outside_the_edge_rounds_is_subnormal_infinite_or_nan(seed):
    steps = 0
    for unit in ref.UNITS:
        for sidx, (name, words, _, _, _) in enumerate(ref.STEPS_FULL[unit]):
            layout = float_layout(unit, name, words)
            steps += bool(layout)
            for r in range(2, ROUNDS):
                for v in ref.step_values(unit, sidx, seed, r) if layout else ():
                    for shift, fmt in layout:
                        bits = v >> shift & ((1 << sum(fmt) + 1) - 1)
                        assert zero_or_normal(bits, fmt), (unit, name, r, hex(bits))
    assert steps >= 95  # every float step of the eight units, not a chosen few
    sidx = ref.STEPS["cvt"].index("v_cvt_scalef32_pk32_f32_fp6")
    for r in range(2, ROUNDS):
        for a, b, c in zip(*ref.operands("cvt", sidx, seed, r)):
            assert all(zero_or_normal(v, ref.F32) for v in ref.fp6_unpack(a, b, c))


def test_the_fma_edge_triple_differs_under_double_rounding():
    a, b, c = (ref.dec(v, ref.F32) for v in ref.FMA32_TRIPLE)
    once = ref.enc(a * b + c, ref.F32)
    twice = ref.enc(ref.dec(ref.enc(a * b + c, ref.F64), ref.F64), ref.F32)
    assert once != twice
    assert ref.dec(once, ref.F32) == 2 ** 24 + 2 and ref.dec(twice, ref.F32) == 2 ** 24
    # and it is what lane 0 of round 1 of v_fma_f32 computes
    sidx = ref.STEPS["f32"].index("v_fma_f32")
    ops = ref.operands("f32", sidx, ref.SEEDS[0], 1)
    assert tuple(o[0] for o in ops) == ref.FMA32_TRIPLE
    assert ref.step_values("f32", sidx, ref.SEEDS[0], 1)[0] == once


def test_each_width_has_a_subnormal_result_for_add_and_fma():
    for unit, fmt, names in (("f32", ref.F32, ("v_add_f32", "v_fma_f32")), ("f64", ref.F64, ("v_add_f64", "v_fma_f64")),
                             ("f16", ref.F16, ("v_add_f16", "v_fma_f16"))):
        for name in names:
            vals = ref.step_values(unit, ref.STEPS[unit].index(name), ref.SEEDS[0], 1)[:16]
            mask = (1 << sum(fmt) + 1) - 1
            assert any(v & mask and not ref.is_normal_finite(v & mask, fmt) for v in vals), name


def test_rounding_steps_meet_exact_ties():
    for unit, name, dec in (("f32", "v_rndne_f32", ref.fr), ("f64", "v_rndne_f64", ref.fd)):
        a = ref.operands(unit, ref.STEPS[unit].index(name), ref.SEEDS[0], 1)[0][:16]
        assert {dec(v) for v in a} == {Fraction(2 * k + 1, 2) for k in range(-8, 8)}
    for name, fmt in (("v_cvt_f16_f32", ref.F16), ("v_cvt_pk_bf16_f32", ref.BF16), ("v_cvt_pk_fp8_f32", ref.E4M3),
                      ("v_cvt_pk_bf8_f32", ref.E5M2)):
        a = ref.operands("cvt", ref.STEPS["cvt"].index(name), ref.SEEDS[0], 1)[0]
        ties = 0
        for v in a[:16]:
            x = ref.fr(v)
            down, up = ref.dec(ref.enc(x, fmt, True), fmt), None
            ulp = Fraction(2) ** (ref.ilog2(abs(x)) - fmt[1])
            ties += x - down == ulp / 2
        assert ties >= 4, name
    for name, fmt in (("v_cvt_scalef32_pk_fp8_f32", ref.E4M3), ("v_cvt_scalef32_pk_fp4_f32", ref.E2M1)):
        a, b, c = ref.operands("cvt", ref.STEPS["cvt"].index(name), ref.SEEDS[0], 1)
        ties = 0
        for t in range(64):
            for v in (a[t], b[t]):
                x = ref.fr(v) / ref.fr(c[t])  # what is rounded is the quotient by the scale
                ulp = Fraction(2) ** (max(ref.ilog2(abs(x)), 2 - (1 << fmt[0] - 1)) - fmt[1])
                ties += abs(x) - ref.dec(ref.enc(abs(x), fmt, True), fmt) == ulp / 2
        assert ties >= 4, name
    a = ref.operands("cvt", ref.STEPS["cvt"].index("v_cvt_f32_f64"), ref.SEEDS[0], 1)[0][:8]
    assert all(ref.dec(ref.enc(ref.fd(v), ref.F32, True), ref.F32) != ref.fd(v) for v in a)


def test_class_inputs_cover_every_class():
    for unit, name, fmt in (("f32", "v_cmp_class_f32", ref.F32), ("f64", "v_cmp_class_f64", ref.F64)):
        a = ref.operands(unit, ref.STEPS[unit].index(name), ref.SEEDS[0], 2)[0]
        assert {ref.fclass(v, fmt) for v in a} == set(range(10))


@pytest.mark.parametrize("seed", ref.SEEDS)
def test_every_transcendental_argument_has_an_exactly_representable_result(seed):
    fmts = {"f32": ref.F32, "f64": ref.F64, "f16": ref.F16}
    for sidx, (name, words, kinds, _, _) in enumerate(ref.STEPS_FULL["trans"]):
        fmt = fmts[name.split(":")[0].rsplit("_", 1)[1]]
        dec = (lambda v, f=fmt: ref.dec(v, f))
        for r in range(ROUNDS):
            a = ref.operands("trans", sidx, seed, r)[0]
            vals = ref.step_values("trans", sidx, seed, r)  # exact_sqrt / exact_log2 assert exactness
            for x, v in zip(a, vals):
                x, y = dec(x), dec(v)
                assert y == 0 or ref.is_normal_finite(v, fmt)
                if "rcp" in name:
                    assert x * y == 1
                elif "rsq" in name:
                    assert x * y * y == 1 and y > 0
                elif "sqrt" in name:
                    assert y * y == x and y >= 0
                elif "exp" in name:
                    assert x.denominator == 1 and y == Fraction(2) ** int(x)
                elif "log" in name:
                    assert Fraction(2) ** int(y) == x and y.denominator == 1
                else:  # sin, cos at quarter revolutions
                    assert (4 * x).denominator == 1 and y in (-1, 0, 1)


@pytest.mark.parametrize("seed", ref.SEEDS)
def test_dot_float_operands_keep_every_partial_sum_exact(seed):
    for name, fmt in (("v_dot2_f32_f16", ref.F16), ("v_dot2_f32_bf16", ref.BF16), ("v_dot2c_f32_bf16", ref.BF16)):
        sidx = ref.STEPS["dot"].index(name)
        for r in range(ROUNDS):
            a, b, c = ref.operands("dot", sidx, seed, r)
            for x, y, z in zip(a, b, c):
                terms = [ref.dec(x & 0xFFFF, fmt) * ref.dec(y & 0xFFFF, fmt), ref.dec(x >> 16, fmt) * ref.dec(y >> 16, fmt),
                         ref.fr(z)]
                # integers, and every sum of a subset fits f16's (the narrowest) 11-bit significand
                assert all(t.denominator == 1 for t in terms)
                assert max(abs(terms[0]), abs(terms[1])) <= 225 and abs(terms[2]) <= 1023
                assert abs(terms[0]) + abs(terms[1]) + abs(terms[2]) < 2048


@pytest.mark.parametrize("seed", ref.SEEDS)
def test_every_narrowing_cvt_input_is_inside_its_targets_finite_range(seed):
    limits = {"v_cvt_f16_f32": 65504, "v_cvt_pk_f16_f32": 65504, "v_cvt_pkrtz_f16_f32": 65504,
              "v_cvt_pk_fp8_f32": 448, "v_cvt_pk_bf8_f32": 57344, "v_cvt_i32_f32": 2 ** 31 - 1,
              "v_cvt_u32_f32": 2 ** 32 - 1, "v_cvt_rpi_i32_f32": 2 ** 31 - 2, "v_cvt_flr_i32_f32": 2 ** 31 - 1,
              "v_cvt_pk_u8_f32": 255}
    for name, limit in limits.items():
        sidx = ref.STEPS["cvt"].index(name)
        n_ops = sum(k is not None and k.startswith("F32") for k in ref.STEPS_FULL["cvt"][sidx][2])
        for r in range(ROUNDS):
            ops = ref.operands("cvt", sidx, seed, r)[:n_ops]
            for x in (ref.fr(v) for o in ops for v in o):
                assert abs(x) <= limit, (name, r, x)
                if "u32" in name or "u8" in name:
                    assert x >= 0
    for name, limit, low in (("v_cvt_scalef32_pk_fp8_f32", 448, Fraction(1, 64)), ("v_cvt_scalef32_pk_fp4_f32", 6, 0)):
        sidx = ref.STEPS["cvt"].index(name)
        for r in range(ROUNDS):
            a, b, c = ref.operands("cvt", sidx, seed, r)
            for x, y, z in zip(a, b, c):
                scale = ref.fr(z)
                assert ref.ilog2(scale) in range(-2, 3) and Fraction(2) ** ref.ilog2(scale) == scale  # a power of two
                assert all(low <= abs(ref.fr(v) / scale) <= limit for v in (x, y)), (name, r)
    sidx = ref.STEPS["cvt"].index("v_cvt_pknorm_i16_f32")
    for r in range(ROUNDS):
        for x in (ref.fr(v) for o in ref.operands("cvt", sidx, seed, r)[:2] for v in o):
            # inside [-1, 1], the product exact in f32's 24 bits and never halfway between two integers
            assert abs(x) <= 1 and (x * 256).denominator == 1 and (x * 32767 * 2).denominator != 1 or x in (-1, 0, 1)
    sidx = ref.STEPS["cvt"].index("v_cvt_i32_f64")
    for r in range(ROUNDS):
        assert all(abs(ref.fd(v)) < 2 ** 31 for v in ref.operands("cvt", sidx, seed, r)[0])
    for name, kind_fmt in (("v_cvt_f32_fp8:0", ref.E4M3), ("v_cvt_f32_bf8:0", ref.E5M2)):
        a = ref.operands("cvt", ref.STEPS["cvt"].index(name), seed, 2)[0]
        top = (1 << kind_fmt[0]) - 1
        for v in a:
            for i in range(4):
                byte = v >> (8 * i) & 0xFF
                e, m = byte >> kind_fmt[1] & top, byte & ((1 << kind_fmt[1]) - 1)
                assert not (e == top and m == (1 << kind_fmt[1]) - 1) if kind_fmt == ref.E4M3 else e != top


def test_the_digest_moves_by_one_flipped_bit_as_the_header_says():
    u, seed = "int", ref.SEEDS[0]
    v = ref.expected(u, seed, 2).copy()
    d = ref.digest_of(v)
    assert d == ref.digest(u, seed, 2)
    old = int(v[0, 0, 0])
    v[0, 0, 0] ^= 1
    assert ref.digest_of(v) == (d + (int(v[0, 0, 0]) - old)) & ref.M32  # idx 0 has weight 1


def test_rounds_are_prefixes_of_one_another():
    a, b = ref.expected("bit", ref.SEEDS[1], 2), ref.expected("bit", ref.SEEDS[1], 4)
    assert np.array_equal(a, b[:2])


def test_msad_masks_on_the_reference_and_differs_from_sad():
    assert ref.msad(0x01020304, 0x00FF0004, 7) == 7 + (0xFF - 2)  # bytes 3 and 1 of b are 0: masked; byte 0 is equal
    sad, msad = (ref.STEPS["int"].index(n) for n in ("v_sad_u8", "v_msad_u8"))
    masked = 0
    for r in range(2):
        a, b, c = ref.operands("int", msad, ref.SEEDS[0], r)
        masked += sum(any(y >> s & 0xFF == 0 and x >> s & 0xFF for s in (0, 8, 16, 24)) for x, y in zip(a, b))
    assert masked >= 32  # the edge round's 0 and 1 words put zero bytes in the reference
    assert sad + 1 == msad


def test_the_fp6_fold_moves_with_any_one_bit_of_any_element():
    a, b, c = (o[5] for o in ref.operands("cvt", ref.STEPS["cvt"].index("v_cvt_scalef32_pk32_f32_fp6"), ref.SEEDS[0], 2))
    r = ref.fp6_unpack(a, b, c)
    assert len(r) == 32 and ref.fp6_fold(a, b, c) & ref.M32 == sum(v * (2 * i + 1) for i, v in enumerate(r)) & ref.M32
    # every e2m3 encoding times a power of two is exact: the element, rescaled, is the f32
    for i, v in enumerate(r):
        e = (c << 128 | b << 64 | a) >> (6 * i) & 63
        assert ref.fr(v) == ref.dec(e, ref.E2M3) * ref.fr(ref.fp6_scale(a))
    for i in range(32):
        for bit in range(32):
            moved = sum((v ^ (1 << bit if j == i else 0)) * (2 * j + 1) for j, v in enumerate(r)) & ref.M32
            assert moved != ref.fp6_fold(a, b, c) & ref.M32
