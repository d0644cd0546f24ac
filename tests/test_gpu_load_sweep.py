"""k_load_sweep and k_load_probe on the GPU (csrc/hip/load_sweep.hip).

Every word of C of every lap is held bit-equal against the int64 product of the
reference (tests/load_sweep_ref.py) and the folds against its folds; a clean
sweep must leave the host's digests on every CU; an injected flip must be
localised to its XCD and part. The probe's shapes are the smallest at which
the pipeline takes each of its paths. Every comparison is equality."""
import numpy as np
import pytest

import load_sweep_ref as ref
from flex_gpu_scheduler_amd.ops.hip_probe import LOAD_KSTEPS, LOAD_SEED, LOAD_SETS, probe

pytestmark = pytest.mark.gpu

SEEDS = (LOAD_SEED, 0x9E3779B9)
# (ksteps, sets, laps): prologue and epilogue with no steady state; each stage
# used once; a stage reused; an odd count with a set modulo that is no power of
# two and both rotations (sub-tile and set) wrapped.
SHAPES = ((1, 1, 1), (2, 2, 3), (3, 2, 2), (5, 3, 9))


@pytest.fixture(scope="module")
def p():
    return probe()


@pytest.fixture(scope="module")
def cus(p):
    return int(p.props(0)["computeUnits"])


@pytest.fixture(scope="module")
def clean(p):
    return p.load_sweep(0, laps=9)


def _is_clean(r, digests):
    return (r["fail"] == 0 and not any(r["bad"].values()) and r["bad_simds"] == 0 and r["digests"] == digests
            and (r["bad_subtiles"], r["bad_sets"], r["bad_spans"]) == (0, 0, 0))


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("ksteps,sets,laps", SHAPES)
def test_probe_is_bit_equal_to_the_reference(p, ksteps, sets, laps, seed):
    got = p.load_probe(0, None, seed, laps, ksteps, sets)
    assert got["gemm"].shape == (laps, 128, 256)
    products = {s: ref.product(seed, s, ksteps) for s in range(sets)}
    for lap in range(laps):
        bad = np.argwhere(got["gemm"][lap] != products[ref.set_of(lap, laps, sets)])
        for row, col in bad[:8]:
            print(f"lap {lap} C[{row}][{col}]: got {got['gemm'][lap, row, col]}")
        assert len(bad) == 0
    want = ref.digests(seed, laps, ksteps, sets)
    assert int(got["stage"].sum(dtype=np.uint64)) & ref.M32 == want["stage"]
    assert int(got["lds"].sum(dtype=np.uint64)) & ref.M32 == want["lds"]
    assert (got["valu"] == ref.valu_final(seed, laps, ksteps)).all()


def test_a_sweep_of_nine_laps_is_clean_on_every_cu(p, clean, cus):
    s = clean["summary"]
    assert s["covered"] and s["cus_seen"] == cus and not any(s["uncovered"].values())
    assert s["bad_xcds"] == [] and s["failed_parts"] == [] and s["late_only"] == {}
    assert s["parts"] == ref.PARTS and s["laps"] == 9 and s["blocks"] == 4 * cus
    want = ref.digests(LOAD_SEED, 9, LOAD_KSTEPS, LOAD_SETS)
    assert p.load_sweep_expected(laps=9) == want
    assert [r for r in clean["records"] if not _is_clean(r, want)] == []
    assert all(r["simd_mask"] == 0xF for r in clean["records"])
    info = p.load_sweep_info(0)
    assert info["scratch_bytes"] == 0 and info["blocks_per_cu"] == 1 and info["num_regs"] <= 256


@pytest.mark.parametrize("part", ref.PARTS)
def test_an_injected_part_fails_exactly_its_xcd_and_part(p, clean, part):
    xcd = sorted({r["xcd"] for r in clean["records"]})[-2]
    out = p.load_sweep(0, laps=1, inject=(xcd, None, [part]), max_rounds=1)
    hit = [r for r in out["records"] if r["xcd"] == xcd]
    want = ref.digests(LOAD_SEED, 1, LOAD_KSTEPS, LOAD_SETS)
    assert hit and all(r["fail"] == 1 << ref.PARTS.index(part) and r["bad"][part] == 1 for r in hit)
    assert all(_is_clean(r, want) for r in out["records"] if r["xcd"] != xcd)
    s = out["summary"]
    assert s["bad_xcds"] == [xcd] and s["failed_parts"] == [part] and s["xcds"][xcd]["failed_parts"] == [part]
    if part == "gemm":
        assert all((r["bad_subtiles"], r["bad_sets"], r["bad_spans"]) == (1, 1, 1) for r in hit)
