"""k_f8load_sweep and k_f8load_probe on the GPU (csrc/hip/f8load_sweep.hip).

Every element of C of every lap is held equal, as float32 bits, to the
reference's float64 product (tests/f8load_sweep_ref.py), every dword that came
back from the ring to the reference's bf16 tile, and the operand folds to its
fold; a clean sweep must leave the host's digests on every CU; an injected flip
must be localised to its XCD and part. Every comparison is equality."""
import numpy as np
import pytest

import f8load_sweep_ref as ref
from flex_gpu_scheduler_amd.ops.hip_probe import F8LOAD_SEED, probe

pytestmark = pytest.mark.gpu

SEEDS = (F8LOAD_SEED, 0x9E3779B9)
# (ksteps, slots, laps): the read-back in the tail only; one in every lap, behind a barrier of its own; the three
# stages wrapping at an odd step count and a partial tail; the largest K; more laps than sets and a rotation tail.
SHAPES = ((1, 1, 1), (2, 1, 3), (3, 2, 5), (18, 4, 6), (1, 3, 35))
SWEEP = {"ksteps": 3, "slots": 2, "laps": 5}  # of the clean sweep


@pytest.fixture(scope="module")
def p():
    return probe()


@pytest.fixture(scope="module")
def clean(p):
    return p.f8load_sweep(0, **SWEEP)


def _is_clean(r, digests):
    return (r["fail"] == 0 and not any(r["bad"].values()) and r["bad_simds"] == 0 and r["digests"] == digests
            and (r["bad_subtiles"], r["bad_sets"], r["bad_spans"]) == (0, 0, 0))


def _equal(got, want, what):
    """got == want as uint32, element by element; the first few that differ are printed."""
    for at in np.argwhere(got != want)[:8]:
        print(f"{what}{list(at)}: got {got[tuple(at)]:#x}, want {want[tuple(at)]:#x}")
    assert (got == want).all(), what


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("ksteps,slots,laps", SHAPES)
def test_probe_equals_the_reference(p, ksteps, slots, laps, seed):
    got = p.f8load_probe(0, None, seed, laps, ksteps, slots)
    assert got["gemm"].shape == (laps, 128, 256) and got["store"].shape == (laps, 128, 128)
    sets = [ref.set_of(0, lap, laps) for lap in range(laps)]
    want = np.stack([ref.product(seed, s, ksteps) for s in sets]).astype(np.float32)
    _equal(got["gemm"].view(np.uint32), want.view(np.uint32), "C")
    _equal(got["store"], np.stack([ref.tile(seed, s, ksteps) for s in sets]), "read back")
    assert int(got["operand"].sum(dtype=np.uint64)) & ref.M32 == ref.digests(seed, laps, ksteps, slots)["operand"]


def test_a_sweep_of_a_few_laps_is_clean_on_every_cu(p, clean):
    cus, s = int(p.props(0)["computeUnits"]), clean["summary"]
    assert s["covered"] and s["cus_seen"] == cus and not any(s["uncovered"].values())
    assert s["bad_xcds"] == [] and s["failed_parts"] == [] and s["late_only"] == {}
    assert s["parts"] == ref.PARTS and s["laps"] == SWEEP["laps"] and s["blocks"] == 4 * cus
    want = ref.digests(F8LOAD_SEED, SWEEP["laps"], SWEEP["ksteps"], SWEEP["slots"])
    assert p.f8load_sweep_expected(**SWEEP) == want
    assert [r for r in clean["records"] if not _is_clean(r, want)] == []
    assert all(r["simd_mask"] == 0xF for r in clean["records"])
    info = p.f8load_sweep_info(0)
    assert info["scratch_bytes"] == 0 and info["blocks_per_cu"] == 1


@pytest.mark.parametrize("part", ref.PARTS)
def test_an_injected_part_fails_exactly_its_xcd_and_part(p, clean, part):
    xcd = sorted({r["xcd"] for r in clean["records"]})[-2]
    out = p.f8load_sweep(0, inject=(xcd, None, [part]), max_rounds=1, **SWEEP)
    hit = [r for r in out["records"] if r["xcd"] == xcd]
    want = ref.digests(F8LOAD_SEED, SWEEP["laps"], SWEEP["ksteps"], SWEEP["slots"])
    assert hit and all(r["fail"] == 1 << ref.PARTS.index(part) and r["bad"][part] == 1 for r in hit)
    assert all(_is_clean(r, want) for r in out["records"] if r["xcd"] != xcd)
    s = out["summary"]
    assert s["bad_xcds"] == [xcd] and s["failed_parts"] == [part] and s["xcds"][xcd]["failed_parts"] == [part]
    if part in ("gemm", "round"):  # wave 0's sub-tile of lap 0, set 0, the first span
        assert all((r["bad_subtiles"], r["bad_sets"], r["bad_spans"]) == (1, 1, 1) for r in hit)
    if part == "store":  # wave 0 reads region (0 + 1 + 0) & 7 of lap 0's tile, set 0, at lap 2: span 32 x 2 // 5
        assert all((r["bad_subtiles"], r["bad_sets"], r["bad_spans"]) == (1 << 1, 1, 1 << 12) for r in hit)
