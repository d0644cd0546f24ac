"""k_matrix_sweep / k_matrix_tile on the GPU (csrc/hip/matrix_sweep.hip).

The tile test decodes the operand encodings with tables written here from the
OCP fp8 and MX (e2m3, e3m2, e2m1, E8M0) definitions and requires the product
the matrix cores return to be equal to the float64 / int64 reference: that
pins the operand lane maps, the fp6/fp4 packing, the scale byte select and
the C/D maps without trusting the C++ host reference. The sweep tests check
coverage, the digests, and that injected mis-computes are localised to their
CU, XCD and format."""
import numpy as np
import pytest

from flex_gpu_scheduler_amd.control.node_agent import GpuHealth, hip_health_fn
from flex_gpu_scheduler_amd.ops.hip_probe import ProbeError, probe

pytestmark = pytest.mark.gpu

M = 0xFFFFFFFF
FORMATS = ["f16", "f32", "f64", "fp8", "bf8", "i8", "mxfp8", "mxbf8", "mxfp6", "mxbf6", "mxfp4"]
MX = FORMATS[6:]


# ------------------------------------------------------------ decode tables
def minifloat(ebits: int, mbits: int, special=()) -> np.ndarray:
    """value[code] of a sign | exponent | mantissa format with bias
    2^(ebits-1) - 1 and gradual underflow; `special` codes are not finite."""
    bias = (1 << (ebits - 1)) - 1
    out = np.zeros(1 << (1 + ebits + mbits))
    for code in range(len(out)):
        s, e, m = code >> (ebits + mbits), (code >> mbits) & ((1 << ebits) - 1), code & ((1 << mbits) - 1)
        v = m / (1 << mbits) * 2.0 ** (1 - bias) if e == 0 else (1 + m / (1 << mbits)) * 2.0 ** (e - bias)
        out[code] = np.nan if code in special else (-v if s else v)
    return out


E4M3FN = minifloat(4, 3, special=(0x7F, 0xFF))  # OCP: no infinities, S.1111.111 is NaN
E5M2 = minifloat(5, 2, special=tuple(c for c in range(256) if (c >> 2) & 31 == 31))  # IEEE-like inf/NaN
E2M3 = minifloat(2, 3)  # MX fp6/fp4: every code is finite
E3M2 = minifloat(3, 2)
E2M1 = np.array([0, 0.5, 1, 1.5, 2, 3, 4, 6, -0.0, -0.5, -1, -1.5, -2, -3, -4, -6])
TABLES = {"fp8": E4M3FN, "bf8": E5M2, "mxfp8": E4M3FN, "mxbf8": E5M2, "mxfp6": E2M3, "mxbf6": E3M2, "mxfp4": E2M1}


def test_decode_tables_match_the_definitions():
    assert np.array_equal(minifloat(2, 1), E2M1)
    assert E4M3FN[0x7E] == 448 and E4M3FN[0x01] == 2.0 ** -9 and E4M3FN[0x38] == 1 and E4M3FN[0xC0] == -2
    assert E5M2[0x7B] == 57344 and E5M2[0x01] == 2.0 ** -16 and E5M2[0x3C] == 1 and np.isnan(E5M2[0x7C])
    assert E2M3.max() == 7.5 and E2M3[0x01] == 0.125 and E2M3[0x08] == 1
    assert E3M2.max() == 28 and E3M2[0x01] == 0.0625 and E3M2[0x0C] == 1


def decode(fmt: str, codes: np.ndarray) -> np.ndarray:
    if fmt == "f16":
        return codes.astype(np.uint16).view(np.float16).astype(np.float64)
    if fmt == "f32":
        return codes.astype(np.uint32).view(np.float32).astype(np.float64)
    if fmt == "f64":
        return codes.view(np.float64)
    if fmt == "i8":
        return codes.astype(np.uint8).view(np.int8).astype(np.int64)
    assert codes.max() < len(TABLES[fmt])
    return TABLES[fmt][codes.astype(np.int64)]


def e8m0(codes: np.ndarray) -> np.ndarray:
    assert (codes != 255).all()  # NaN
    return 2.0 ** (codes.astype(np.int64) - 127)


def reference(inp: dict, fmt: str) -> np.ndarray:
    a, b = decode(fmt, inp["a"]), decode(fmt, inp["b"])
    if inp["a_scale"] is not None:
        a = a * np.repeat(e8m0(inp["a_scale"]), 32, axis=1)
        b = b * np.repeat(e8m0(inp["b_scale"]), 32, axis=0)
    assert np.isfinite(a.astype(np.float64)).all() and np.isfinite(b.astype(np.float64)).all()
    return a @ b  # float64 (int64 for i8): exact, every partial sum is far below 2^53


def digest(tile: np.ndarray, frac: int) -> int:
    fix = np.asarray(tile, dtype=np.float64) * 2.0 ** frac
    assert np.array_equal(fix, np.round(fix)) and np.abs(fix).max() < 2 ** 31
    w = 2 * np.arange(tile.size, dtype=np.int64).reshape(tile.shape) + 1
    d = int(((fix.astype(np.int64) & M) * w).sum()) & M
    return (15 * d) & M  # four identical waves: sum_w D << w


# ----------------------------------------------------------------- fixtures
@pytest.fixture(scope="module")
def p():
    return probe()


@pytest.fixture(scope="module")
def cus(p):
    return int(p.props(0)["computeUnits"])


@pytest.fixture(scope="module")
def inputs(p):
    return {f: p.matrix_inputs(f) for f in FORMATS}


@pytest.fixture(scope="module")
def refs(inputs):
    return {f: reference(inputs[f], f) for f in FORMATS}


@pytest.fixture(scope="module")
def clean(p):
    return p.matrix_sweep(0)


def _keys(records):
    return {(r["xcd"], r["cu"]) for r in records}


# -------------------------------------------------------------------- tests
def test_format_names(p):
    assert p.matrix_formats() == FORMATS
    with pytest.raises(ValueError):
        p.matrix_sweep(0, formats=["fp5"])
    with pytest.raises(ValueError):
        p.matrix_inputs("bf16")


@pytest.mark.parametrize("fmt", FORMATS)
def test_inputs_have_the_properties_the_design_rests_on(inputs, fmt):
    inp = inputs[fmt]
    a, b = inp["a"], inp["b"]
    t, k = inp["tile"], inp["k"]
    assert a.shape == (t, k) and b.shape == (k, t)
    av, bv = decode(fmt, a), decode(fmt, b)
    assert (av < 0).any() and (av > 0).any() and (bv < 0).any() and (bv > 0).any()  # both signs
    n = min(t, k)
    assert not np.array_equal(a[:n, :n], b[:n, :n])  # A != B
    assert not np.array_equal(bv[:n, :n], bv[:n, :n].T)  # B asymmetric in (k, col)
    if fmt in ("mxfp6", "mxbf6", "mxfp4"):
        bits = 4 if fmt == "mxfp4" else 6
        assert set(np.unique(np.concatenate([a.ravel(), b.ravel()])).tolist()) == set(range(1 << bits))
        assert (np.abs(av) == TABLES[fmt][1]).any() or (np.abs(bv) == TABLES[fmt][1]).any()  # a subnormal
    if fmt == "i8":
        both = np.concatenate([av.ravel(), bv.ravel()])
        assert both.min() == -128 and both.max() == 127
    if fmt in MX:
        sa, sb = inp["a_scale"], inp["b_scale"]
        assert sa.shape == (t, k // 32) and sb.shape == (k // 32, t) and k // 32 == 4
        for s in (sa, sb):
            assert not (s == 127).all()
            assert s.min() <= 125 and s.max() >= 129  # 2^-2 .. 2^2
        assert len({tuple(r) for r in sa}) > 1 and len({tuple(c) for c in sb.T}) > 1  # rows, columns differ
        assert not np.array_equal(sa[:, 0], sa[:, 1]) and not np.array_equal(sa[:, 2], sa[:, 3])  # k-blocks differ
        assert not np.array_equal(sb[0], sb[1]) and not np.array_equal(sb[2], sb[3])
        assert not np.array_equal(sa, sb.T)
    else:
        assert inp["a_scale"] is None and inp["b_scale"] is None


@pytest.mark.parametrize("fmt", FORMATS)
def test_tile_equals_the_independent_reference(p, inputs, refs, fmt):
    got = p.matrix_tile(0, fmt)
    want = refs[fmt]
    assert got.shape == want.shape == (inputs[fmt]["tile"],) * 2
    assert got.dtype == (np.int64 if fmt == "i8" else np.float64)
    bad = np.argwhere(got != want)
    print(fmt, "mismatches:", len(bad), "first:", [(tuple(ix), got[tuple(ix)], want[tuple(ix)]) for ix in bad[:4]])
    assert np.array_equal(got, want)
    assert np.abs(want).max() > 0


@pytest.mark.parametrize("fmt", FORMATS)
def test_digest_of_the_tile_is_the_expected_and_the_swept_one(p, inputs, refs, clean, fmt):
    d = digest(refs[fmt], inputs[fmt]["frac"])
    assert d != 0
    assert p.matrix_sweep_expected([fmt]) == {fmt: d}
    assert p.matrix_sweep_expected()[fmt] == d
    assert {r["digests"][fmt] for r in clean["records"]} == {d}


def test_clean_sweep_covers_every_cu(p, cus, clean):
    s = clean["summary"]
    print("matrix_sweep defaults:", {k: s[k] for k in ("rounds", "ms", "blocks", "covered", "uncovered")})
    assert s["covered"] and s["formats"] == FORMATS
    assert len(_keys(clean["records"])) == cus
    assert _keys(clean["records"]) == _keys(p.cu_sweep(0)["records"])
    print("simd masks:", sorted({r["simd_mask"] for r in clean["records"]}))
    assert all(r["fail"] == 0 for r in clean["records"])
    assert s["bad_xcds"] == [] and s["failed_formats"] == []
    assert all(v["failed_formats"] == [] and v["cus_seen"] == v["cus_expected"] for v in s["xcds"].values())


@pytest.mark.parametrize("fmt", FORMATS)
def test_injection_is_localised_to_one_cu_and_format(p, clean, fmt):
    bit = 1 << FORMATS.index(fmt)
    xcd, cu = sorted(_keys(clean["records"]))[len(clean["records"]) // 9]
    out = p.matrix_sweep(0, inject=(xcd, cu, [fmt]))
    s = out["summary"]
    hit = [r for r in out["records"] if (r["xcd"], r["cu"]) == (xcd, cu)]
    assert hit and all(r["fail"] == bit for r in hit)
    assert all(r["fail"] == 0 for r in out["records"] if (r["xcd"], r["cu"]) != (xcd, cu))
    assert s["bad_xcds"] == [xcd]
    assert s["failed_formats"] == [fmt]
    assert s["xcds"][xcd]["failed_cus"] == [cu] and s["xcds"][xcd]["failed_formats"] == [fmt]


def test_injection_wildcard_flags_one_whole_xcd(p, clean):
    xcd = max(r["xcd"] for r in clean["records"])
    bits = 1 << FORMATS.index("f64") | 1 << FORMATS.index("mxfp4")
    out = p.matrix_sweep(0, inject=(xcd, None, ["mxfp4", "f64"]))
    s = out["summary"]
    assert s["bad_xcds"] == [xcd] and s["failed_formats"] == ["f64", "mxfp4"]
    assert s["xcds"][xcd]["failed_cus"] == sorted(c for x, c in _keys(out["records"]) if x == xcd)
    assert all((r["fail"] == bits) == (r["xcd"] == xcd) for r in out["records"])
    assert all(r["fail"] in (0, bits) for r in out["records"])


def test_format_subset_leaves_the_others_untouched(p, clean):
    sub = ["fp8", "mxbf6"]
    out = p.matrix_sweep(0, formats=sub, max_rounds=1)
    want = p.matrix_sweep_expected(sub)
    assert sorted(want) == sorted(sub) and out["summary"]["formats"] == sub
    for r in out["records"]:
        assert r["fail"] == 0
        assert {f: v for f, v in r["digests"].items() if v} == want
    # a fault injected into a format that is not selected is not computed, so not reported
    xcd = clean["records"][0]["xcd"]
    out = p.matrix_sweep(0, formats=sub, inject=(xcd, None, ["f16"]), max_rounds=1)
    assert all(r["fail"] == 0 for r in out["records"])


def test_one_block_is_uncovered_not_failed(p):
    out = p.matrix_sweep(0, blocks=1)
    s = out["summary"]
    assert len(out["records"]) == 1 and s["rounds"] == 1
    assert not s["covered"]
    assert s["bad_xcds"] == [] and out["records"][0]["fail"] == 0
    verdict = hip_health_fn(matrix=True, matrix_args={"blocks": 1})(0)
    assert verdict.ok if isinstance(verdict, GpuHealth) else verdict is True


@pytest.mark.parametrize("args", [
    dict(blocks=-1), dict(blocks=(1 << 20) + 1), dict(format_mask=0), dict(format_mask=1 << 11),
    dict(inject_xcd=16), dict(inject_xcd=-2), dict(inject_cu=256), dict(inject_cu=-2), dict(inject_formats=1 << 11),
])
def test_bad_arguments_are_refused(p, args):
    import ctypes

    a = dict(blocks=4, format_mask=1, inject_xcd=-1, inject_cu=-1, inject_formats=0)
    a.update(args)
    buf = (ctypes.c_uint32 * (16 * 4))()
    rc = p.lib.xs_matrix_sweep(0, a["blocks"], a["format_mask"], a["inject_xcd"], a["inject_cu"], a["inject_formats"],
                               buf, None, None)
    assert rc == -1000
    assert not any(buf)  # nothing ran


def test_bad_arguments_raise_from_python(p):
    with pytest.raises(ProbeError) as e:
        p.matrix_sweep(0, blocks=-1)
    assert e.value.rc == -1000
    with pytest.raises(ProbeError) as e:
        p.matrix_sweep(0, inject=(99, None, ["f16"]))
    assert e.value.rc == -1000
    assert p.lib.xs_matrix_tile(0, 11, None) == -1000
    assert p.lib.xs_matrix_sweep_expected(0, None) == -1000


def test_health_fn_with_the_matrix_sweep(p, cus, clean):
    assert hip_health_fn(matrix=True)(0)
    xcd = clean["records"][0]["xcd"]
    v = hip_health_fn(matrix=True, matrix_formats=["mxfp4", "fp8", "f32"],
                      matrix_args={"inject": (xcd, None, ["mxfp4", "fp8"])})(0)
    if cus // 32 >= 8:
        assert isinstance(v, GpuHealth) and not v and not v.ok
        assert v.bad_xcds == frozenset({xcd})
        assert v.detail["matrixFaults"] == {xcd: ["fp8", "mxfp4"]}
    else:
        assert v is False
