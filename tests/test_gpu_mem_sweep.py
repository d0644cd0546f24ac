"""k_mem_sweep and k_mem_probe on the GPU (csrc/hip/mem_sweep.hip).

Every value a workgroup received through each route is held bit-equal against
the numpy reference (tests/mem_sweep_ref.py, which executes the stores and
loads on a byte array by the ISA's rules), so a rule the kernel's comparator
got wrong cannot pass by agreeing with itself. The digests of a clean sweep
must be the reference's on every CU; injected mis-compares must be localised
to their CU, XCD and route. Every comparison is equality."""
import ctypes

import numpy as np
import pytest

import mem_sweep_ref as ref
from flex_gpu_scheduler_amd.control.node_agent import GpuHealth, hip_health_fn
from flex_gpu_scheduler_amd.ops.hip_probe import ProbeError, probe

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def p():
    return probe()


@pytest.fixture(scope="module")
def cus(p):
    return int(p.props(0)["computeUnits"])


@pytest.fixture(scope="module")
def clean(p):
    return p.mem_sweep(0)


@pytest.fixture(scope="module")
def target(clean):
    """(xcd, cu key) of one CU the clean sweep reached."""
    keys = sorted(_keys(clean["records"]))
    return keys[len(keys) // 7]


def _keys(records):
    return {(r["xcd"], r["cu"]) for r in records}


def _digests(seed, routes=ref.ROUTES):
    return {f: (ref.digest(f, seed) if f in routes else 0) for f in ref.ROUTES}


def _is_clean(r, digests):
    return r["fail"] == 0 and not any(r["bad"].values()) and r["bad_simds"] == 0 and r["digests"] == digests


# -------------------------------------------------------------------- tests
def test_route_names_and_shapes(p):
    assert p.mem_routes() == ref.ROUTES
    for f in ref.ROUTES:
        assert (p.mem_shape(f)["steps"], p.mem_shape(f)["words"]) == ref.SHAPES[f]
    with pytest.raises(ValueError):
        p.mem_shape("l3")


@pytest.mark.parametrize("seed", ref.SEEDS)
@pytest.mark.parametrize("route", ref.ROUTES)
def test_probe_is_bit_equal_to_the_numpy_reference(p, route, seed):
    got, want = p.mem_probe(0, route, seed), ref.expected(route, seed)
    assert got.shape == want.shape and got.dtype == np.uint32
    bad = np.argwhere(got != want)
    for s, w, t in bad[:12]:
        print(f"{route} step {s} word {w} wave {t >> 6} lane {t & 63}: got {got[s, w, t]:#010x} want {want[s, w, t]:#010x}")
    print(f"{route} seed {seed:#x}: {len(bad)} of {got.size} values differ; steps {sorted({int(b[0]) for b in bad})[:40]}")
    assert len(bad) == 0


@pytest.mark.parametrize("seed", ref.SEEDS)
def test_digests_equal_the_reference_on_every_cu(p, clean, seed):
    want = _digests(seed)
    assert p.mem_sweep_expected(seed=seed) == want
    out = clean if seed == ref.SEEDS[0] else p.mem_sweep(0, seed=seed)
    odd = [r for r in out["records"] if r["digests"] != want]
    print(f"seed {seed:#x}: {len(odd)} of {len(out['records'])} records off the reference; first {odd[:2]}")
    assert not odd
    assert all(r["fail"] == 0 for r in out["records"]) and out["summary"]["seed"] == seed


def test_clean_sweep_covers_every_cu(p, cus, clean):
    s = clean["summary"]
    print("mem_sweep defaults:", {k: s[k] for k in ("rounds", "ms", "blocks", "covered", "uncovered")})
    print("mem_sweep_info:", p.mem_sweep_info(0))
    assert s["covered"] and s["routes"] == ref.ROUTES
    assert len(_keys(clean["records"])) == cus
    assert _keys(clean["records"]) == _keys(p.cu_sweep(0)["records"])
    bad = [r for r in clean["records"] if r["fail"]]
    print("failing records:", bad[:4])
    assert not bad
    assert all(_is_clean(r, _digests(ref.SEEDS[0])) for r in clean["records"])
    assert s["bad_xcds"] == [] and s["failed_routes"] == []
    assert all(v["failed_routes"] == [] and v["cus_seen"] == v["cus_expected"] for v in s["xcds"].values())


def test_the_kernel_keeps_a_cu_to_itself_without_scratch(p):
    info = p.mem_sweep_info(0)
    assert info["blocks_per_cu"] == 1 and info["scratch_bytes"] == 0
    assert info["lds_bytes"] > (160 << 10) // 2
    assert info["arena_bytes"] == ref.STRIDE


@pytest.mark.parametrize("route", ref.ROUTES)
def test_injection_is_localised_to_one_cu_and_route(p, target, route):
    xcd, cu = target
    out = p.mem_sweep(0, inject=(xcd, cu, [route]))
    s = out["summary"]
    hit = [r for r in out["records"] if (r["xcd"], r["cu"]) == (xcd, cu)]
    print("hit records:", hit[:1])
    assert hit
    want = _digests(ref.SEEDS[0])
    bit = 1 << ref.ROUTES.index(route)
    for r in hit:
        assert r["fail"] == bit and r["bad"] == {f: int(f == route) for f in ref.ROUTES}
        assert r["bad_simds"] in (1, 2, 4, 8) and r["bad_simds"] & r["simd_mask"]
        assert {f: d for f, d in r["digests"].items() if f != route} == {f: d for f, d in want.items() if f != route}
        assert r["digests"][route] == ref.digest(route, ref.SEEDS[0], flip_first=True)  # thread 0, step 0, word 0
    assert all(_is_clean(r, want) for r in out["records"] if (r["xcd"], r["cu"]) != (xcd, cu))
    assert s["bad_xcds"] == [xcd] and s["failed_routes"] == [route]
    assert s["xcds"][xcd]["failed_cus"] == [cu] and s["xcds"][xcd]["failed_routes"] == [route]


def test_a_route_subset_runs_only_those_routes(p, target):
    xcd, cu = target
    sub = ["buffer", "scalar"]
    out = p.mem_sweep(0, routes=sub, inject=(xcd, cu, ["l2"]))  # not selected: not run, nothing to report
    want = _digests(ref.SEEDS[0], sub)
    assert out["summary"]["routes"] == sub and out["summary"]["bad_xcds"] == []
    assert all(_is_clean(r, want) for r in out["records"])
    assert p.mem_sweep_expected(sub) == {f: want[f] for f in sub}


def test_bad_arguments_are_refused(p):
    with pytest.raises(ValueError):
        p.mem_sweep(0, routes=["l1", "texture"])  # an unknown route
    buf = (ctypes.c_uint32 * (32 * 4))()
    for mask, inject in ((0, 0), (1 << 7, 0), (0x7F, 1 << 7)):  # mask 0, a mask beyond all, an injection beyond all
        rc = p.lib.xs_mem_sweep(0, 4, mask, ref.SEEDS[0], -1, -1, inject, buf, None, None)
        assert rc == -1000
    for kw in (dict(blocks=-1), dict(inject=(16, None, ["l1"])), dict(inject=(0, 256, ["l1"]))):
        with pytest.raises(ProbeError) as e:
            p.mem_sweep(0, **kw)
        assert e.value.rc == -1000
    assert not any(buf)  # nothing ran
    out = np.zeros(16, np.uint32)
    assert p.lib.xs_mem_probe(0, 0, 0, out.ctypes.data, out.size) == -1000  # not steps x words x 256
    assert p.lib.xs_mem_probe(0, 7, 0, out.ctypes.data, out.size) == -1000
    assert not out.any()


def test_health_fn_with_the_mem_sweep(p, cus, clean):
    v = hip_health_fn(mem=True)(0)
    assert v and (not isinstance(v, GpuHealth) or v.detail["memFaults"] == {})
    xcd = clean["records"][0]["xcd"]
    v = hip_health_fn(mem=True, mem_routes=["atomic", "l2", "scalar"], mem_args={"inject": (xcd, None, ["l2", "scalar"])})(0)
    if cus // 32 >= 8:
        assert isinstance(v, GpuHealth) and not v and not v.ok
        assert v.bad_xcds == frozenset({xcd})
        assert v.detail["memFaults"] == {xcd: ["l2", "scalar"]}
        assert v.detail["memSweep"]["routes"] == ["atomic", "l2", "scalar"]
    else:
        assert v is False
