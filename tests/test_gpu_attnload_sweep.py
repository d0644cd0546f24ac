"""k_attnload_sweep and k_attnload_probe on the GPU (csrc/hip/attnload_sweep.hip).

Every element of O, l and m of every lap is held equal, as a value, to the
reference's (tests/attnload_sweep_ref.py, float64, exact) and the folds to its
folds; a clean sweep must leave the host's digests on every CU; an injected
flip must be localised to its XCD and part. Every comparison is equality."""
import numpy as np
import pytest

import attnload_sweep_ref as ref
from flex_gpu_scheduler_amd.ops.hip_probe import ATTNLOAD_KVSTEPS, ATTNLOAD_SEED, ATTNLOAD_SETS, probe

pytestmark = pytest.mark.gpu

SEEDS = (ATTNLOAD_SEED, 0x9E3779B9)
# (kvsteps, sets, laps): no rescale, prologue and epilogue only; both stages, a
# rescale and a lap boundary inside the pipeline; an odd block count, so that a
# lap starts in either stage; N = 1,024, the edge of the bound, with a set
# count that is no power of two and the wave rotation wrapping past 8.
SHAPES = ((1, 1, 1), (2, 2, 3), (3, 2, 2), (16, 3, 9))
LAPS = 5  # of the clean sweep


@pytest.fixture(scope="module")
def p():
    return probe()


@pytest.fixture(scope="module")
def cus(p):
    return int(p.props(0)["computeUnits"])


@pytest.fixture(scope="module")
def clean(p):
    return p.attnload_sweep(0, laps=LAPS)


def _is_clean(r, digests):
    return (r["fail"] == 0 and not any(r["bad"].values()) and r["bad_simds"] == 0 and r["digests"] == digests
            and (r["bad_subtiles"], r["bad_sets"], r["bad_spans"]) == (0, 0, 0))


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("kvsteps,sets,laps", SHAPES)
def test_probe_equals_the_reference(p, kvsteps, sets, laps, seed):
    got = p.attnload_probe(0, None, seed, laps, kvsteps, sets)
    assert got["out"].shape == (laps, 256, 64) and got["out"].dtype == np.float32
    assert got["l"].shape == got["m"].shape == (laps, 256)
    wants = {s: ref.attention(seed, s, kvsteps) for s in range(sets)}
    for lap in range(laps):
        want = wants[ref.set_of(lap, laps, sets)]
        for name in ("out", "l", "m"):
            bad = np.argwhere(~(got[name][lap] == want[name]))  # a NaN is a mismatch
            for at in bad[:8]:
                print(f"lap {lap} {name}{list(at)}: got {got[name][lap][tuple(at)]!r}, want {want[name][tuple(at)]!r}")
            assert len(bad) == 0, name
    want = ref.digests(seed, laps, kvsteps, sets)
    for part in ("stage", "score", "transpose"):
        assert int(got[part].sum(dtype=np.uint64)) & ref.M32 == want[part], part


def test_a_sweep_of_a_few_laps_is_clean_on_every_cu(p, clean, cus):
    s = clean["summary"]
    assert s["covered"] and s["cus_seen"] == cus and not any(s["uncovered"].values())
    assert s["bad_xcds"] == [] and s["failed_parts"] == [] and s["late_only"] == {}
    assert s["parts"] == ref.PARTS and s["laps"] == LAPS and s["blocks"] == 4 * cus
    want = ref.digests(ATTNLOAD_SEED, LAPS, ATTNLOAD_KVSTEPS, ATTNLOAD_SETS)
    assert p.attnload_sweep_expected(laps=LAPS) == want
    assert [r for r in clean["records"] if not _is_clean(r, want)] == []
    assert all(r["simd_mask"] == 0xF for r in clean["records"])
    info = p.attnload_sweep_info(0)
    assert info["scratch_bytes"] == 0 and info["blocks_per_cu"] == 1 and info["num_regs"] <= 256


@pytest.mark.parametrize("part", ref.PARTS)
def test_an_injected_part_fails_exactly_its_xcd_and_part(p, clean, part):
    xcd = sorted({r["xcd"] for r in clean["records"]})[-2]
    out = p.attnload_sweep(0, laps=1, inject=(xcd, None, [part]), max_rounds=1)
    hit = [r for r in out["records"] if r["xcd"] == xcd]
    want = ref.digests(ATTNLOAD_SEED, 1, ATTNLOAD_KVSTEPS, ATTNLOAD_SETS)
    assert hit and all(r["fail"] == 1 << ref.PARTS.index(part) and r["bad"][part] == 1 for r in hit)
    assert all(_is_clean(r, want) for r in out["records"] if r["xcd"] != xcd)
    s = out["summary"]
    assert s["bad_xcds"] == [xcd] and s["failed_parts"] == [part] and s["xcds"][xcd]["failed_parts"] == [part]
    if part in ("out", "stat"):
        assert all((r["bad_subtiles"], r["bad_sets"], r["bad_spans"]) == (1, 1, 1) for r in hit)
