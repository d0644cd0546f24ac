"""k_fetch_sweep and k_fetch_probe on the GPU (csrc/hip/fetch_sweep.hip).

Every word a workgroup hands over is held bit-equal against the reference
(tests/fetch_sweep_ref.py, Python integers). The digests of a clean sweep must
be the reference's on every CU; an injected flip must be localised to its CU,
XCD and part. One workgroup of 256 threads is the smallest shape and the only
one the probe has; the code size is fixed by what the sweep claims and is no
parameter. Every comparison is equality."""
import numpy as np
import pytest

import fetch_sweep_ref as ref
from flex_gpu_scheduler_amd.control.node_agent import GpuHealth, hip_health_fn
from flex_gpu_scheduler_amd.ops.hip_probe import FETCH_ROUNDS, FETCH_SEED, probe

pytestmark = pytest.mark.gpu

SEEDS = (FETCH_SEED, 0x9E3779B9)


@pytest.fixture(scope="module")
def p():
    return probe()


@pytest.fixture(scope="module")
def cus(p):
    return int(p.props(0)["computeUnits"])


@pytest.fixture(scope="module")
def clean(p):
    return p.fetch_sweep(0)


@pytest.fixture(scope="module")
def target(clean):
    """(xcd, cu key) of one CU the clean sweep reached."""
    keys = sorted(_keys(clean["records"]))
    return keys[len(keys) // 7]


def _keys(records):
    return {(r["xcd"], r["cu"]) for r in records}


def _digests(seed, rounds, parts=ref.PARTS):
    return {f: (ref.digest(ref.words(f, seed, rounds)) if f in parts else 0) for f in ref.PARTS}


def _is_clean(r, digests):
    return r["fail"] == 0 and not any(r["bad"].values()) and r["bad_simds"] == 0 and r["digests"] == digests


def _hold(part, got, want):
    assert got.shape == want.shape
    bad = np.argwhere(got != want)
    for row, t in bad[:12]:
        print(f"{part}: row {row} wave {t // 64} lane {t % 64}: got {got[row, t]:#010x}, want {want[row, t]:#010x}")
    assert len(bad) == 0


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("part", ref.PARTS)
def test_probe_of_one_part_is_bit_equal_to_the_reference(p, part, seed):
    got = p.fetch_probe(0, part, seed, rounds=1)
    assert list(got) == [part]
    _hold(part, got[part], ref.words(part, seed, 1))


@pytest.mark.parametrize("seed", SEEDS)
def test_probe_of_all_parts_in_one_launch_and_the_dumps_digest_is_the_records(p, seed):
    got = p.fetch_probe(0, None, seed, rounds=1)
    assert list(got) == ref.PARTS
    for part in ref.PARTS:
        _hold(part, got[part], ref.words(part, seed, 1))
    assert (got["refill"][0] == got["refill"][1]).all()  # fetched twice, the cache invalidated between
    rec = p.fetch_sweep(0, blocks=1, seed=seed, rounds=1, max_rounds=1)["records"]
    assert len(rec) == 1 and rec[0]["fail"] == 0 and rec[0]["simd_mask"] == 0xF
    assert rec[0]["digests"] == {part: ref.digest(got[part]) for part in ref.PARTS}
    assert rec[0]["digests"] == p.fetch_sweep_expected(seed=seed, rounds=1)


def test_one_workgroup_per_cu_reaches_every_cu_clean(p, cus):
    out = p.fetch_sweep(0, blocks=cus, rounds=1, max_rounds=1)
    s = out["summary"]
    assert len(out["records"]) == cus and s["covered"] and s["cus_seen"] == cus and s["code_rounds"] == 1
    assert all(_is_clean(r, _digests(FETCH_SEED, 1)) for r in out["records"])
    assert all(r["digests"] == p.fetch_sweep_expected(rounds=1) for r in out["records"])


def test_a_default_sweep_is_clean_on_every_cu(clean, cus, p):
    s = clean["summary"]
    assert s["covered"] and not any(s["uncovered"].values()) and s["cus_seen"] == cus
    assert s["bad_xcds"] == [] and s["failed_parts"] == [] and s["parts"] == ref.PARTS
    assert s["seed"] == FETCH_SEED and s["code_rounds"] == FETCH_ROUNDS and s["blocks"] == 4 * cus
    digests = _digests(FETCH_SEED, FETCH_ROUNDS)
    assert digests == p.fetch_sweep_expected()
    assert [r for r in clean["records"] if not _is_clean(r, digests)] == []
    assert all(r["simd_mask"] == 0xF for r in clean["records"])  # four waves: one on every SIMD


def test_the_runtime_reports_no_scratch_and_one_workgroup_per_cu(p):
    info = p.fetch_sweep_info(0)
    assert info["scratch_bytes"] == 0 and info["blocks_per_cu"] == 1
    assert info["lds_bytes"] == 96 << 10 and info["num_regs"] <= 128


def test_an_injected_part_fails_exactly_its_cu_xcd_and_part(p, target):
    xcd, cu = target
    out = p.fetch_sweep(0, inject=(xcd, cu, ["align"]), max_rounds=1)
    hit = [r for r in out["records"] if (r["xcd"], r["cu"]) == (xcd, cu)]
    rest = [r for r in out["records"] if (r["xcd"], r["cu"]) != (xcd, cu)]
    assert hit and all(r["fail"] == 1 << ref.PARTS.index("align") for r in hit)
    assert all(r["bad"]["align"] == 1 and sum(r["bad"].values()) == 1 for r in hit)
    want = _digests(FETCH_SEED, FETCH_ROUNDS)
    assert all(r["digests"]["align"] == (want["align"] + (int(ref.words("align", FETCH_SEED)[0, 0]) ^ 1)
                                         - int(ref.words("align", FETCH_SEED)[0, 0])) % (1 << 32) for r in hit)
    assert all(_is_clean(r, want) for r in rest)
    s = out["summary"]
    assert s["bad_xcds"] == [xcd] and s["xcds"][xcd]["failed_cus"] == [cu]
    assert s["xcds"][xcd]["failed_parts"] == ["align"] and s["failed_parts"] == ["align"]
    v = hip_health_fn(fetch=True, fetch_args={"inject": (xcd, None, ["refill", "stream"]), "max_rounds": 1})(0)
    assert isinstance(v, GpuHealth) and not v.ok and v.bad_xcds == frozenset({xcd})
    assert v.detail["fetchFaults"] == {xcd: ["stream", "refill"]}


def test_a_subset_of_parts_leaves_the_others_digests_zero(p):
    seed = SEEDS[1]
    out = p.fetch_sweep(0, parts=["refill", "call"], seed=seed, rounds=1, max_rounds=1)
    digests = _digests(seed, 1, ("call", "refill"))
    assert all(_is_clean(r, digests) for r in out["records"]) and out["summary"]["parts"] == ["call", "refill"]


def test_two_launches_at_one_seed_give_identical_records(p, cus):
    def by_cu(out):
        return sorted((r["xcd"], r["cu"], r["fail"], tuple(r["digests"].values()), tuple(r["bad"].values()))
                      for r in out["records"])

    a, b = (p.fetch_sweep(0, blocks=cus, rounds=1, max_rounds=1) for _ in range(2))
    assert {x[2:] for x in by_cu(a)} == {x[2:] for x in by_cu(b)} and len({x[2:] for x in by_cu(a)}) == 1
    assert _keys(a["records"]) == _keys(b["records"])
