"""k_gradload_sweep and k_gradload_probe on the GPU (csrc/hip/gradload_sweep.hip).

Every element of every register partial and of every slab read-back is held
equal to the reference's int64 sums (tests/gradload_sweep_ref.py) and the folds
to its folds; a clean sweep must leave the host's digests on every CU; an
injected flip must be localised to its XCD and part. Every comparison is
equality."""
import numpy as np
import pytest

import gradload_sweep_ref as ref
from flex_gpu_scheduler_amd.ops.hip_probe import GRADLOAD_SEED, probe

pytestmark = pytest.mark.gpu

SEEDS = (GRADLOAD_SEED, 0x9E3779B9)
# (ksteps, epoch, laps, slabs): prologue and epilogue only; the ring across lap
# boundaries and one slab reused after it was cleared; an odd step count, two
# slabs and a partial last epoch; the deepest K; the bound itself.
SHAPES = ((1, 1, 1, 1), (2, 1, 3, 1), (3, 2, 5, 2), (8, 32, 32, 1), (1, 257, 257, 1))
SWEEP = {"ksteps": 3, "epoch": 2, "laps": 5, "slabs": 2}  # of the clean sweep


@pytest.fixture(scope="module")
def p():
    return probe()


@pytest.fixture(scope="module")
def cus(p):
    return int(p.props(0)["computeUnits"])


@pytest.fixture(scope="module")
def clean(p):
    return p.gradload_sweep(0, **SWEEP)


def _is_clean(r, digests):
    return (r["fail"] == 0 and not any(r["bad"].values()) and r["bad_simds"] == 0 and r["digests"] == digests
            and (r["bad_subtiles"], r["bad_sets"], r["bad_spans"]) == (0, 0, 0))


def _equal(got, want, what):
    """got float32 == want int64 2^-7, element by element; the first few that differ are printed."""
    fix = got.astype(np.float64) * 128
    for at in np.argwhere(fix != want)[:8]:
        print(f"{what}{list(at)}: got {fix[tuple(at)]}, want {want[tuple(at)]}")
    assert (fix == want).all(), what


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("ksteps,epoch,laps,slabs", SHAPES)
def test_probe_equals_the_reference(p, ksteps, epoch, laps, slabs, seed):
    got = p.gradload_probe(0, None, seed, laps, ksteps, epoch, slabs)
    assert got["gemm"].shape == (laps, 2, 128, 128) and got["gemm"].dtype == np.float32
    assert got["accum"].shape == (-(-laps // epoch), 128, 128)
    want = np.stack([ref.partials(seed, ref.set_of(0, lap, laps, epoch), ksteps) for lap in range(laps)])
    _equal(got["gemm"], want, "partial")
    sums = ref.epoch_sums(seed, laps, ksteps, epoch)
    assert abs(sums).max() < 1 << 24
    _equal(got["accum"], sums, "slab")
    want = ref.digests(seed, laps, ksteps, epoch)
    for part in ("stage", "transpose"):
        assert int(got[part].sum(dtype=np.uint64)) & ref.M32 == want[part], part


def test_a_sweep_of_a_few_laps_is_clean_on_every_cu(p, clean, cus):
    s = clean["summary"]
    assert s["covered"] and s["cus_seen"] == cus and not any(s["uncovered"].values())
    assert s["bad_xcds"] == [] and s["failed_parts"] == [] and s["late_only"] == {}
    assert s["parts"] == ref.PARTS and s["laps"] == SWEEP["laps"] and s["blocks"] == 4 * cus
    want = ref.digests(GRADLOAD_SEED, SWEEP["laps"], SWEEP["ksteps"], SWEEP["epoch"])
    assert p.gradload_sweep_expected(**SWEEP) == want
    assert [r for r in clean["records"] if not _is_clean(r, want)] == []
    assert all(r["simd_mask"] == 0xF for r in clean["records"])
    info = p.gradload_sweep_info(0)
    assert info["scratch_bytes"] == 0 and info["blocks_per_cu"] == 1


@pytest.mark.parametrize("part", ref.PARTS)
def test_an_injected_part_fails_exactly_its_xcd_and_part(p, clean, part):
    xcd = sorted({r["xcd"] for r in clean["records"]})[-2]
    out = p.gradload_sweep(0, inject=(xcd, None, [part]), max_rounds=1, **SWEEP)
    hit = [r for r in out["records"] if r["xcd"] == xcd]
    want = ref.digests(GRADLOAD_SEED, SWEEP["laps"], SWEEP["ksteps"], SWEEP["epoch"])
    assert hit and all(r["fail"] == 1 << ref.PARTS.index(part) and r["bad"][part] == 1 for r in hit)
    assert all(_is_clean(r, want) for r in out["records"] if r["xcd"] != xcd)
    s = out["summary"]
    assert s["bad_xcds"] == [xcd] and s["failed_parts"] == [part] and s["xcds"][xcd]["failed_parts"] == [part]
    if part == "gemm":  # wave 0's sub-tile of lap 0, set 0, the first span
        assert all((r["bad_subtiles"], r["bad_sets"], r["bad_spans"]) == (1, 1, 1) for r in hit)
    if part == "accum":  # wave 0 reads sub-tile (0 + 1 + 2) & 3 back after lap 1, whose set is 1; 32 x 1 // 5 = 6
        assert all((r["bad_subtiles"], r["bad_sets"], r["bad_spans"]) == (1 << 3, 1 << 1, 1 << 6) for r in hit)
