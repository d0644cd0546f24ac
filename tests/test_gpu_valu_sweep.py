"""k_valu_sweep and k_valu_probe on the GPU (csrc/hip/valu_sweep.hip).

Every result of every step of each unit is held bit-equal against the
reference (tests/valu_sweep_ref.py, written from IEEE-754 and the ISA's integer
definitions), so a step the host table got wrong cannot pass by agreeing with
itself. The digests of a clean sweep must be the reference's on every CU;
injected mis-compares must be localised to their CU, XCD, unit and step. Every
comparison is equality."""
import ctypes

import numpy as np
import pytest

import valu_sweep_ref as ref
from flex_gpu_scheduler_amd.control.node_agent import GpuHealth, hip_health_fn
from flex_gpu_scheduler_amd.ops.hip_probe import VALU_ROUNDS, ProbeError, probe

pytestmark = pytest.mark.gpu
ROUNDS = VALU_ROUNDS


@pytest.fixture(scope="module")
def p():
    return probe()


@pytest.fixture(scope="module")
def cus(p):
    return int(p.props(0)["computeUnits"])


@pytest.fixture(scope="module")
def clean(p):
    return p.valu_sweep(0)


@pytest.fixture(scope="module")
def target(clean):
    """(xcd, cu key) of one CU the clean sweep reached."""
    keys = sorted(_keys(clean["records"]))
    return keys[len(keys) // 7]


def _keys(records):
    return {(r["xcd"], r["cu"]) for r in records}


def _digests(seed, units=ref.UNITS, rounds=ROUNDS):
    return {u: (ref.digest(u, seed, rounds) if u in units else 0) for u in ref.UNITS}


def _is_clean(r, digests):
    return (r["fail"] == 0 and not any(r["bad"].values()) and r["bad_simds"] == 0 and r["bad_steps"] == []
            and r["digests"] == digests)


# -------------------------------------------------------------------- tests
def test_unit_names_steps_and_shapes(p):
    assert p.valu_units() == ref.UNITS
    for u in ref.UNITS:
        assert p.valu_steps(u) == ref.STEPS[u]
        assert (p.valu_shape(u)["steps"], p.valu_shape(u)["words"]) == ref.SHAPES[u]
    with pytest.raises(ValueError):
        p.valu_shape("f8")


@pytest.mark.parametrize("seed", ref.SEEDS)
@pytest.mark.parametrize("unit", ref.UNITS)
def test_probe_is_bit_equal_to_the_reference(p, unit, seed):
    got, want = p.valu_probe(0, unit, seed, rounds=2), ref.expected(unit, seed, 2)
    assert got.shape == want.shape and got.dtype == np.uint32
    names = ref.row_names(unit)
    bad = np.argwhere(got != want)
    for r, row, t in bad[:12]:
        print(f"{unit} {names[row][0]} word {names[row][1]} round {r} wave {t >> 6} lane {t & 63}: "
              f"got {got[r, row, t]:#010x} want {want[r, row, t]:#010x}")
    print(f"{unit} seed {seed:#x}: {len(bad)} of {got.size} values differ; steps {sorted({names[b[1]][0] for b in bad})}")
    assert len(bad) == 0


@pytest.mark.parametrize("seed", ref.SEEDS)
def test_digests_equal_the_reference_on_every_cu(p, clean, seed):
    want = _digests(seed)
    assert p.valu_sweep_expected(seed=seed) == want
    out = clean if seed == ref.SEEDS[0] else p.valu_sweep(0, seed=seed)
    odd = [r for r in out["records"] if r["digests"] != want]
    print(f"seed {seed:#x}: {len(odd)} of {len(out['records'])} records off the reference; first {odd[:2]}")
    assert not odd
    assert all(r["fail"] == 0 for r in out["records"]) and out["summary"]["seed"] == seed


def test_clean_sweep_covers_every_cu(p, cus, clean):
    s = clean["summary"]
    print("valu_sweep defaults:", {k: s[k] for k in ("rounds", "ms", "blocks", "covered", "uncovered", "operand_rounds")})
    print("valu_sweep_info:", p.valu_sweep_info(0))
    assert s["covered"] and s["units"] == ref.UNITS and s["operand_rounds"] == ROUNDS
    assert len(_keys(clean["records"])) == cus
    assert _keys(clean["records"]) == _keys(p.cu_sweep(0)["records"])
    bad = [r for r in clean["records"] if r["fail"]]
    print("failing records:", bad[:4])
    assert not bad
    assert all(_is_clean(r, _digests(ref.SEEDS[0])) for r in clean["records"])
    assert s["bad_xcds"] == [] and s["failed_units"] == [] and s["failed_steps"] == []
    assert all(v["failed_units"] == [] and v["cus_seen"] == v["cus_expected"] for v in s["xcds"].values())


def test_the_kernel_keeps_a_cu_to_itself_without_scratch(p):
    info = p.valu_sweep_info(0)
    assert info["blocks_per_cu"] == 1 and info["scratch_bytes"] == 0
    assert info["lds_bytes"] > (160 << 10) // 2


@pytest.mark.parametrize("unit", ref.UNITS)
def test_injection_is_localised_to_one_cu_unit_and_step(p, target, unit):
    xcd, cu = target
    out = p.valu_sweep(0, inject=(xcd, cu, [unit]))
    s = out["summary"]
    hit = [r for r in out["records"] if (r["xcd"], r["cu"]) == (xcd, cu)]
    print("hit records:", hit[:1])
    assert hit
    want = _digests(ref.SEEDS[0])
    bit = 1 << ref.UNITS.index(unit)
    first = ref.STEPS[unit][0]
    flipped = int(ref.expected(unit, ref.SEEDS[0], 1)[0, 0, 0]) ^ 1  # thread 0, round 0, row 0: idx 0, weight 1
    for r in hit:
        assert r["fail"] == bit and r["bad"] == {u: int(u == unit) for u in ref.UNITS}
        assert r["bad_steps"] == [first]
        assert r["bad_simds"] in (1, 2, 4, 8) and r["bad_simds"] & r["simd_mask"]
        assert {u: d for u, d in r["digests"].items() if u != unit} == {u: d for u, d in want.items() if u != unit}
        assert r["digests"][unit] == (want[unit] - (flipped ^ 1) + flipped) & 0xFFFFFFFF
    assert all(_is_clean(r, want) for r in out["records"] if (r["xcd"], r["cu"]) != (xcd, cu))
    assert s["bad_xcds"] == [xcd] and s["failed_units"] == [unit] and s["failed_steps"] == [first]
    assert s["xcds"][xcd]["failed_cus"] == [cu] and s["xcds"][xcd]["failed_units"] == [unit]
    assert s["xcds"][xcd]["failed_steps"] == [first]


def test_injection_wildcard_flags_one_whole_xcd(p, clean):
    xcd = max(r["xcd"] for r in clean["records"])
    out = p.valu_sweep(0, inject=(xcd, None, ["f64", "cvt"]))
    s = out["summary"]
    both = (1 << ref.UNITS.index("f64")) | (1 << ref.UNITS.index("cvt"))
    assert s["bad_xcds"] == [xcd] and s["failed_units"] == ["f64", "cvt"]
    assert s["failed_steps"] == [ref.STEPS["f64"][0], ref.STEPS["cvt"][0]]
    assert s["xcds"][xcd]["failed_cus"] == sorted(c for x, c in _keys(out["records"]) if x == xcd)
    assert all(r["fail"] == (both if r["xcd"] == xcd else 0) for r in out["records"])


def test_a_unit_subset_runs_only_those_units(p, target):
    xcd, cu = target
    sub = ["f16", "trans"]
    out = p.valu_sweep(0, units=sub, inject=(xcd, cu, ["int"]))  # not selected: not run, nothing to report
    want = _digests(ref.SEEDS[0], sub)
    assert out["summary"]["units"] == sub and out["summary"]["bad_xcds"] == []
    assert all(_is_clean(r, want) for r in out["records"])
    assert p.valu_sweep_expected(sub) == {u: want[u] for u in sub}
    with pytest.raises(ValueError):
        p.valu_sweep(0, units=["f32", "f8"])


def test_more_rounds_than_the_default(p):
    out = p.valu_sweep(0, units=["f32", "dot"], rounds=4)
    want = _digests(ref.SEEDS[0], ["f32", "dot"], 4)
    assert out["summary"]["operand_rounds"] == 4 and out["summary"]["bad_xcds"] == []
    assert all(_is_clean(r, want) for r in out["records"])


def test_one_block_is_uncovered_not_failed(p):
    out = p.valu_sweep(0, blocks=1)
    s = out["summary"]
    assert len(out["records"]) == 1 and s["rounds"] == 1
    assert not s["covered"]
    assert s["bad_xcds"] == [] and out["records"][0]["fail"] == 0
    verdict = hip_health_fn(valu=True, valu_args={"blocks": 1})(0)
    assert verdict.ok if isinstance(verdict, GpuHealth) else verdict is True


@pytest.mark.parametrize("args", [
    dict(blocks=-1), dict(blocks=(1 << 20) + 1), dict(inject_xcd=16), dict(inject_xcd=-2), dict(inject_cu=256),
    dict(inject_cu=-2), dict(unit_mask=0), dict(unit_mask=1 << 8), dict(inject_units=1 << 8), dict(rounds=0),
    dict(rounds=65),
])
def test_bad_arguments_are_refused(p, args):
    a = dict(blocks=4, unit_mask=0xFF, rounds=2, inject_xcd=-1, inject_cu=-1, inject_units=0)
    a.update(args)
    buf = (ctypes.c_uint32 * (32 * 4))()
    rc = p.lib.xs_valu_sweep(0, a["blocks"], a["unit_mask"], ref.SEEDS[0], a["rounds"], a["inject_xcd"],
                             a["inject_cu"], a["inject_units"], buf, None, None)
    assert rc == -1000
    assert not any(buf)  # nothing ran


def test_bad_arguments_raise_from_python(p):
    for kw in (dict(blocks=-1), dict(inject=(16, None, ["f32"])), dict(inject=(0, 256, ["f32"])), dict(rounds=0),
               dict(rounds=65)):
        with pytest.raises(ProbeError) as e:
            p.valu_sweep(0, **kw)
        assert e.value.rc == -1000
    assert p.lib.xs_valu_sweep_expected(0xFF, 0, 2, None) == -1000
    assert p.lib.xs_valu_sweep_expected(0, 0, 2, (ctypes.c_uint32 * 8)()) == -1000
    assert p.lib.xs_valu_shape(8, (ctypes.c_int * 2)()) == -1000
    out = np.zeros(16, np.uint32)
    assert p.lib.xs_valu_probe(0, 0, 0, 2, out.ctypes.data, out.size) == -1000  # not rounds x words x 256
    assert p.lib.xs_valu_probe(0, 8, 0, 2, out.ctypes.data, out.size) == -1000
    assert p.lib.xs_valu_probe(0, 0, 0, 0, out.ctypes.data, out.size) == -1000
    assert not out.any()


def test_health_fn_with_the_valu_sweep(p, cus, clean):
    assert hip_health_fn(valu=True)(0)
    xcd = clean["records"][0]["xcd"]
    v = hip_health_fn(valu=True, valu_units=["f64", "bit", "cvt"],
                      valu_args={"inject": (xcd, None, ["f64", "cvt"])})(0)
    if cus // 32 >= 8:
        assert isinstance(v, GpuHealth) and not v and not v.ok
        assert v.bad_xcds == frozenset({xcd})
        assert v.detail["valuFaults"] == {xcd: ["f64", "cvt"]}
        assert v.detail["valuSweep"]["units"] == ["f64", "bit", "cvt"]
        assert v.detail["valuSweep"]["failed_steps"] == [ref.STEPS["f64"][0], ref.STEPS["cvt"][0]]
    else:
        assert v is False
