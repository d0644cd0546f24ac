"""k_scalar_sweep and k_scalar_probe on the GPU (csrc/hip/scalar_sweep.hip).

Every word a workgroup holds after each part is held bit-equal against the
reference (tests/scalar_sweep_ref.py, Python integers from the ISA's
definitions). The digests of a clean sweep must be the reference's on every
CU; an injected mis-compare must be localised to its CU, XCD and part. One
workgroup of 1,024 threads is the smallest shape and the only one the probe
has. Every comparison is equality."""
import numpy as np
import pytest

import scalar_sweep_ref as ref
from flex_gpu_scheduler_amd.control.node_agent import GpuHealth, hip_health_fn
from flex_gpu_scheduler_amd.ops.hip_probe import probe

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def p():
    return probe()


@pytest.fixture(scope="module")
def cus(p):
    return int(p.props(0)["computeUnits"])


@pytest.fixture(scope="module")
def clean(p):
    return {seed: p.scalar_sweep(0, seed=seed) for seed in ref.SEEDS}


@pytest.fixture(scope="module")
def target(clean):
    """(xcd, cu key) of one CU the clean sweep reached."""
    keys = sorted(_keys(clean[ref.SEEDS[0]]["records"]))
    return keys[len(keys) // 7]


def _keys(records):
    return {(r["xcd"], r["cu"]) for r in records}


def _digests(seed, parts=ref.PARTS):
    return {f: (ref.digest(f, seed) if f in parts else 0) for f in ref.PARTS}


def _is_clean(r, digests):
    return r["fail"] == 0 and not any(r["bad"].values()) and r["bad_simds"] == 0 and r["digests"] == digests


@pytest.mark.parametrize("seed", ref.SEEDS)
@pytest.mark.parametrize("part", ref.PARTS)
def test_probe_is_bit_equal_to_the_reference(p, part, seed):
    got = p.scalar_probe(0, part, seed)
    want = ref.expected(part, seed)
    assert got.shape == want.shape
    bad = np.argwhere(got != want)
    for w, t in bad[:12]:
        print(f"{part}: word {w} (of {ref.SHAPES[part][0]} steps) wave {t // 64} lane {t % 64}: "
              f"got {got[w, t]:#010x}, want {want[w, t]:#010x}")
    assert len(bad) == 0


@pytest.mark.parametrize("seed", ref.SEEDS)
def test_a_default_sweep_is_clean_on_every_cu(clean, cus, seed):
    out = clean[seed]
    s = out["summary"]
    assert s["covered"] and not any(s["uncovered"].values()) and s["cus_seen"] == cus
    assert s["bad_xcds"] == [] and s["failed_parts"] == [] and s["parts"] == ref.PARTS and s["seed"] == seed
    digests = _digests(seed)
    dirty = [r for r in out["records"] if not _is_clean(r, digests)]
    assert dirty == []
    assert all(r["simd_mask"] == 0xF for r in out["records"])  # sixteen waves: four on every SIMD


def test_the_runtime_reports_no_scratch_and_one_workgroup_per_cu(p):
    info = p.scalar_sweep_info(0)
    assert info["scratch_bytes"] == 0 and info["blocks_per_cu"] == 1
    assert info["lds_bytes"] == (2 * 8 + 2 + 8) * 1024 * 4 and info["num_regs"] <= 128


def test_an_injected_part_fails_exactly_its_cu_xcd_and_part(p, target):
    xcd, cu = target
    seed = ref.SEEDS[0]
    out = p.scalar_sweep(0, inject=(xcd, cu, ["mask"]), max_rounds=1)
    hit = [r for r in out["records"] if (r["xcd"], r["cu"]) == (xcd, cu)]
    rest = [r for r in out["records"] if (r["xcd"], r["cu"]) != (xcd, cu)]
    assert hit and all(r["fail"] == 1 << ref.PARTS.index("mask") for r in hit)
    assert all(r["bad"]["mask"] == 1 and sum(r["bad"].values()) == 1 for r in hit)
    assert all(_is_clean(r, _digests(seed)) for r in rest)
    s = out["summary"]
    assert s["bad_xcds"] == [xcd] and s["xcds"][xcd]["failed_cus"] == [cu]
    assert s["xcds"][xcd]["failed_parts"] == ["mask"] and s["failed_parts"] == ["mask"]
    v = hip_health_fn(scalar=True, scalar_args={"inject": (xcd, None, ["sgpr", "arith"]), "max_rounds": 1})(0)
    assert isinstance(v, GpuHealth) and not v.ok and v.bad_xcds == frozenset({xcd})
    assert v.detail["scalarFaults"] == {xcd: ["arith", "sgpr"]}


def test_a_subset_of_parts_leaves_the_others_digests_zero(p):
    seed = ref.SEEDS[1]
    out = p.scalar_sweep(0, parts=["sgpr", "branch"], seed=seed, max_rounds=1)
    digests = _digests(seed, ("branch", "sgpr"))
    assert all(_is_clean(r, digests) for r in out["records"]) and out["summary"]["parts"] == ["branch", "sgpr"]
