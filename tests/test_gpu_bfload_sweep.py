"""k_bfload_sweep and k_bfload_probe on the GPU (csrc/hip/bfload_sweep.hip).

Every element of C of every lap is held equal, as a float32 value, to the exact
product of the reference (tests/bfload_sweep_ref.py) and the folds to its
folds; a clean sweep must leave the host's digests on every CU; an injected
flip must be localised to its XCD and part. The probe's shapes are the smallest
at which the pipeline takes each of its paths. Every comparison is equality."""
import numpy as np
import pytest

import bfload_sweep_ref as ref
from flex_gpu_scheduler_amd.ops.hip_probe import BFLOAD_KSTEPS, BFLOAD_SEED, BFLOAD_SETS, probe

pytestmark = pytest.mark.gpu

SEEDS = (BFLOAD_SEED, 0x9E3779B9)
# (ksteps, sets, laps): prologue and epilogue only; both stages and a lap
# boundary inside the pipeline; an odd step count, so that a lap starts in
# either stage; K = 256, the edge of the bound, with a set modulo that is no
# power of two and tail laps without rotation.
SHAPES = ((1, 1, 1), (2, 2, 3), (3, 2, 2), (8, 3, 7))
LAPS = 5  # of the clean sweep


@pytest.fixture(scope="module")
def p():
    return probe()


@pytest.fixture(scope="module")
def cus(p):
    return int(p.props(0)["computeUnits"])


@pytest.fixture(scope="module")
def clean(p):
    return p.bfload_sweep(0, laps=LAPS)


def _is_clean(r, digests):
    return (r["fail"] == 0 and not any(r["bad"].values()) and r["bad_simds"] == 0 and r["digests"] == digests
            and (r["bad_subtiles"], r["bad_sets"], r["bad_spans"]) == (0, 0, 0))


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("ksteps,sets,laps", SHAPES)
def test_probe_equals_the_reference(p, ksteps, sets, laps, seed):
    got = p.bfload_probe(0, None, seed, laps, ksteps, sets)
    assert got["gemm"].shape == (laps, 128, 256) and got["gemm"].dtype == np.float32
    products = {s: ref.product(seed, s, ksteps) for s in range(sets)}
    for lap in range(laps):
        want = products[ref.set_of(lap, laps, sets)]
        bad = np.argwhere(~(got["gemm"][lap] == want))  # a NaN is a mismatch
        for row, col in bad[:8]:
            print(f"lap {lap} C[{row}][{col}]: got {got['gemm'][lap, row, col]!r}, want {want[row, col]!r}")
        assert len(bad) == 0
    want = ref.digests(seed, laps, ksteps, sets)
    for part in ref.PARTS[:3]:
        assert int(got[part].sum(dtype=np.uint64)) & ref.M32 == want[part], part


def test_a_sweep_of_a_few_laps_is_clean_on_every_cu(p, clean, cus):
    s = clean["summary"]
    assert s["covered"] and s["cus_seen"] == cus and not any(s["uncovered"].values())
    assert s["bad_xcds"] == [] and s["failed_parts"] == [] and s["late_only"] == {}
    assert s["parts"] == ref.PARTS and s["laps"] == LAPS and s["blocks"] == 4 * cus
    want = ref.digests(BFLOAD_SEED, LAPS, BFLOAD_KSTEPS, BFLOAD_SETS)
    assert p.bfload_sweep_expected(laps=LAPS) == want
    assert [r for r in clean["records"] if not _is_clean(r, want)] == []
    assert all(r["simd_mask"] == 0xF for r in clean["records"])
    info = p.bfload_sweep_info(0)
    assert info["scratch_bytes"] == 0 and info["blocks_per_cu"] == 1 and info["num_regs"] <= 256


@pytest.mark.parametrize("part", ref.PARTS)
def test_an_injected_part_fails_exactly_its_xcd_and_part(p, clean, part):
    xcd = sorted({r["xcd"] for r in clean["records"]})[-2]
    out = p.bfload_sweep(0, laps=1, inject=(xcd, None, [part]), max_rounds=1)
    hit = [r for r in out["records"] if r["xcd"] == xcd]
    want = ref.digests(BFLOAD_SEED, 1, BFLOAD_KSTEPS, BFLOAD_SETS)
    assert hit and all(r["fail"] == 1 << ref.PARTS.index(part) and r["bad"][part] == 1 for r in hit)
    assert all(_is_clean(r, want) for r in out["records"] if r["xcd"] != xcd)
    s = out["summary"]
    assert s["bad_xcds"] == [xcd] and s["failed_parts"] == [part] and s["xcds"][xcd]["failed_parts"] == [part]
    if part == "gemm":
        assert all((r["bad_subtiles"], r["bad_sets"], r["bad_spans"]) == (1, 1, 1) for r in hit)
