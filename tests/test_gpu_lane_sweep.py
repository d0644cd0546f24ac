"""k_lane_sweep and k_lane_probe on the GPU (csrc/hip/lane_sweep.hip).

Every value a workgroup received through each path is held bit-equal against
the numpy reference (tests/lane_sweep_ref.py, written from the lane maps), so a
map the kernel's comparator got wrong cannot pass by agreeing with itself. The
digests of a clean sweep must be the reference's on every CU; injected
mis-compares must be localised to their CU, XCD and path. Every comparison is
equality."""
import ctypes

import numpy as np
import pytest

import lane_sweep_ref as ref
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
    return p.lane_sweep(0)


@pytest.fixture(scope="module")
def target(clean):
    """(xcd, cu key) of one CU the clean sweep reached."""
    keys = sorted(_keys(clean["records"]))
    return keys[len(keys) // 7]


def _keys(records):
    return {(r["xcd"], r["cu"]) for r in records}


def _digests(seed, paths=ref.PATHS):
    return {f: (ref.digest(f, seed) if f in paths else 0) for f in ref.PATHS}


def _is_clean(r, digests):
    return r["fail"] == 0 and not any(r["bad"].values()) and r["bad_simds"] == 0 and r["digests"] == digests


# -------------------------------------------------------------------- tests
def test_path_names_and_shapes(p):
    assert p.lane_paths() == ref.PATHS
    for f in ref.PATHS:
        assert (p.lane_shape(f)["steps"], p.lane_shape(f)["words"]) == ref.SHAPES[f]
    with pytest.raises(ValueError):
        p.lane_shape("ldstr8")


@pytest.mark.parametrize("seed", ref.SEEDS)
@pytest.mark.parametrize("path", ref.PATHS)
def test_probe_is_bit_equal_to_the_numpy_reference(p, path, seed):
    got, want = p.lane_probe(0, path, seed), ref.expected(path, seed)
    assert got.shape == want.shape and got.dtype == np.uint32
    bad = np.argwhere(got != want)
    for s, w, t in bad[:12]:
        print(f"{path} step {s} word {w} wave {t >> 6} lane {t & 63}: got {got[s, w, t]:#010x} want {want[s, w, t]:#010x}")
    print(f"{path} seed {seed:#x}: {len(bad)} of {got.size} values differ; steps {sorted({int(b[0]) for b in bad})[:40]}")
    assert len(bad) == 0


@pytest.mark.parametrize("seed", ref.SEEDS)
def test_digests_equal_the_reference_on_every_cu(p, clean, seed):
    want = _digests(seed)
    assert p.lane_sweep_expected(seed=seed) == want
    out = clean if seed == ref.SEEDS[0] else p.lane_sweep(0, seed=seed)
    odd = [r for r in out["records"] if r["digests"] != want]
    print(f"seed {seed:#x}: {len(odd)} of {len(out['records'])} records off the reference; first {odd[:2]}")
    assert not odd
    assert all(r["fail"] == 0 for r in out["records"]) and out["summary"]["seed"] == seed


def test_clean_sweep_covers_every_cu(p, cus, clean):
    s = clean["summary"]
    print("lane_sweep defaults:", {k: s[k] for k in ("rounds", "ms", "blocks", "covered", "uncovered")})
    print("lane_sweep_info:", p.lane_sweep_info(0))
    assert s["covered"] and s["paths"] == ref.PATHS
    assert len(_keys(clean["records"])) == cus
    assert _keys(clean["records"]) == _keys(p.cu_sweep(0)["records"])
    print("simd masks:", sorted({r["simd_mask"] for r in clean["records"]}))
    bad = [r for r in clean["records"] if r["fail"]]
    print("failing records:", bad[:4])
    assert not bad
    assert all(_is_clean(r, _digests(ref.SEEDS[0])) for r in clean["records"])
    assert s["bad_xcds"] == [] and s["failed_paths"] == []
    assert all(v["failed_paths"] == [] and v["cus_seen"] == v["cus_expected"] for v in s["xcds"].values())


def test_the_kernel_keeps_a_cu_to_itself_without_scratch(p):
    info = p.lane_sweep_info(0)
    assert info["blocks_per_cu"] == 1 and info["scratch_bytes"] == 0
    assert info["lds_bytes"] > (160 << 10) // 2


@pytest.mark.parametrize("path", ref.PATHS)
def test_injection_is_localised_to_one_cu_and_path(p, target, path):
    xcd, cu = target
    out = p.lane_sweep(0, inject=(xcd, cu, [path]))
    s = out["summary"]
    hit = [r for r in out["records"] if (r["xcd"], r["cu"]) == (xcd, cu)]
    print("hit records:", hit[:1])
    assert hit
    want = _digests(ref.SEEDS[0])
    bit = 1 << ref.PATHS.index(path)
    flipped = int(ref.expected(path, ref.SEEDS[0])[0, 0, 0]) ^ 1  # thread 0, step 0, word 0: idx 0, weight 1
    for r in hit:
        assert r["fail"] == bit and r["bad"] == {f: int(f == path) for f in ref.PATHS}
        assert r["bad_simds"] in (1, 2, 4, 8) and r["bad_simds"] & r["simd_mask"]
        assert {f: d for f, d in r["digests"].items() if f != path} == {f: d for f, d in want.items() if f != path}
        assert r["digests"][path] == (want[path] - (flipped ^ 1) + flipped) & 0xFFFFFFFF
    assert all(_is_clean(r, want) for r in out["records"] if (r["xcd"], r["cu"]) != (xcd, cu))
    assert s["bad_xcds"] == [xcd] and s["failed_paths"] == [path]
    assert s["xcds"][xcd]["failed_cus"] == [cu] and s["xcds"][xcd]["failed_paths"] == [path]


def test_injection_wildcard_flags_one_whole_xcd(p, clean):
    xcd = max(r["xcd"] for r in clean["records"])
    out = p.lane_sweep(0, inject=(xcd, None, ["permlane", "ldstr"]))
    s = out["summary"]
    both = (1 << ref.PATHS.index("permlane")) | (1 << ref.PATHS.index("ldstr"))
    assert s["bad_xcds"] == [xcd] and s["failed_paths"] == ["permlane", "ldstr"]
    assert s["xcds"][xcd]["failed_cus"] == sorted(c for x, c in _keys(out["records"]) if x == xcd)
    assert all(r["fail"] == (both if r["xcd"] == xcd else 0) for r in out["records"])


def test_a_path_subset_runs_only_those_paths(p, target):
    xcd, cu = target
    sub = ["dpp", "ldsdma"]
    out = p.lane_sweep(0, paths=sub, inject=(xcd, cu, ["bpermute"]))  # not selected: not run, nothing to report
    want = _digests(ref.SEEDS[0], sub)
    assert out["summary"]["paths"] == sub and out["summary"]["bad_xcds"] == []
    assert all(_is_clean(r, want) for r in out["records"])
    assert p.lane_sweep_expected(sub) == {f: want[f] for f in sub}
    with pytest.raises(ValueError):
        p.lane_sweep(0, paths=["dpp", "shuffle"])


def test_one_block_is_uncovered_not_failed(p):
    out = p.lane_sweep(0, blocks=1)
    s = out["summary"]
    assert len(out["records"]) == 1 and s["rounds"] == 1
    assert not s["covered"]
    assert s["bad_xcds"] == [] and out["records"][0]["fail"] == 0
    verdict = hip_health_fn(lane=True, lane_args={"blocks": 1})(0)
    assert verdict.ok if isinstance(verdict, GpuHealth) else verdict is True


@pytest.mark.parametrize("args", [
    dict(blocks=-1), dict(blocks=(1 << 20) + 1), dict(inject_xcd=16), dict(inject_xcd=-2), dict(inject_cu=256),
    dict(inject_cu=-2), dict(path_mask=0), dict(path_mask=1 << 8), dict(inject_paths=1 << 8),
])
def test_bad_arguments_are_refused(p, args):
    a = dict(blocks=4, path_mask=0xFF, inject_xcd=-1, inject_cu=-1, inject_paths=0)
    a.update(args)
    buf = (ctypes.c_uint32 * (32 * 4))()
    rc = p.lib.xs_lane_sweep(0, a["blocks"], a["path_mask"], ref.SEEDS[0], a["inject_xcd"], a["inject_cu"],
                             a["inject_paths"], buf, None, None)
    assert rc == -1000
    assert not any(buf)  # nothing ran


def test_bad_arguments_raise_from_python(p):
    for kw in (dict(blocks=-1), dict(inject=(16, None, ["dpp"])), dict(inject=(0, 256, ["dpp"]))):
        with pytest.raises(ProbeError) as e:
            p.lane_sweep(0, **kw)
        assert e.value.rc == -1000
    assert p.lib.xs_lane_sweep_expected(0xFF, 0, None) == -1000
    assert p.lib.xs_lane_sweep_expected(0, 0, (ctypes.c_uint32 * 8)()) == -1000
    assert p.lib.xs_lane_shape(8, (ctypes.c_int * 2)()) == -1000
    out = np.zeros(16, np.uint32)
    assert p.lib.xs_lane_probe(0, 0, 0, out.ctypes.data, out.size) == -1000  # not steps x words x 256
    assert p.lib.xs_lane_probe(0, 8, 0, out.ctypes.data, out.size) == -1000
    assert not out.any()


def test_health_fn_with_the_lane_sweep(p, cus, clean):
    assert hip_health_fn(lane=True)(0)
    xcd = clean["records"][0]["xcd"]
    v = hip_health_fn(lane=True, lane_paths=["permlane", "ldstr", "ldsdma"],
                      lane_args={"inject": (xcd, None, ["ldstr", "ldsdma"])})(0)
    if cus // 32 >= 8:
        assert isinstance(v, GpuHealth) and not v and not v.ok
        assert v.bad_xcds == frozenset({xcd})
        assert v.detail["laneFaults"] == {xcd: ["ldstr", "ldsdma"]}
        assert v.detail["laneSweep"]["paths"] == ["permlane", "ldstr", "ldsdma"]
    else:
        assert v is False
