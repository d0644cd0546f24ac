"""k_streamload_sweep and k_streamload_probe on the GPU (csrc/hip/streamload_sweep.hip).

Every element of Ct of every lap is held equal to the reference's int64 product
(tests/streamload_sweep_ref.py) and the folds to its folds; a clean sweep on a
small arena must leave the host's digests on every CU; an injected flip must be
localised to its XCD and part. Every comparison is equality."""
import numpy as np
import pytest

import streamload_sweep_ref as ref
from flex_gpu_scheduler_amd.ops.hip_probe import STREAMLOAD_DEPTH as D
from flex_gpu_scheduler_amd.ops.hip_probe import STREAMLOAD_SEED, probe

pytestmark = pytest.mark.gpu

SEEDS = (STREAMLOAD_SEED, 0x9E3779B9)
# (ksteps, panels, laps): prologue and epilogue only; the ring reaches across a
# lap boundary; the ring wraps, R = 3, two full rounds and a tail lap; an odd
# step count over two rounds and a tail; the deepest K, the whole X in LDS.
SHAPES = ((1, 8, 1), (D - 1, 8, 2), (D + 1, 24, 7), (2 * D + 3, 16, 5), (64, 8, 1))
SWEEP = {"ksteps": 5, "panels": 24, "laps": 7}  # of the clean sweep: 120 KiB, two rounds and a tail lap


@pytest.fixture(scope="module")
def p():
    return probe()


@pytest.fixture(scope="module")
def cus(p):
    return int(p.props(0)["computeUnits"])


@pytest.fixture(scope="module")
def clean(p):
    return p.streamload_sweep(0, **SWEEP)


def _is_clean(r, digests):
    return (r["fail"] == 0 and not any(r["bad"].values()) and r["bad_simds"] == 0 and r["digests"] == digests
            and (r["bad_subtiles"], r["bad_sets"], r["bad_spans"]) == (0, 0, 0))


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("ksteps,panels,laps", SHAPES)
def test_probe_equals_the_reference(p, ksteps, panels, laps, seed):
    got = p.streamload_probe(0, None, seed, laps, ksteps, panels)
    assert got["gemm"].shape == (laps, 128, 16) and got["gemm"].dtype == np.int32
    for lap in range(laps):
        for wave in range(8):
            want = ref.product(seed, ref.panel_of(0, lap, wave, laps, panels), ksteps)
            tile = got["gemm"][lap, 16 * wave:16 * wave + 16]
            for n, m in np.argwhere(tile != want)[:8]:
                print(f"lap {lap} wave {wave} Ct[{n}][{m}]: got {tile[n, m]}, want {want[n, m]}")
            assert (tile == want).all(), (lap, wave)
    want = ref.digests(seed, laps, ksteps, panels)
    for part in ("stage", "act"):
        assert int(got[part].sum(dtype=np.uint64)) & ref.M32 == want[part], part


def test_a_sweep_of_a_few_laps_is_clean_on_every_cu(p, clean, cus):
    s = clean["summary"]
    assert s["covered"] and s["cus_seen"] == cus and not any(s["uncovered"].values())
    assert s["bad_xcds"] == [] and s["failed_parts"] == [] and s["late_only"] == {}
    assert s["parts"] == ref.PARTS and s["laps"] == SWEEP["laps"] and s["blocks"] == 4 * cus
    want = ref.digests(STREAMLOAD_SEED, SWEEP["laps"], SWEEP["ksteps"], SWEEP["panels"])
    assert p.streamload_sweep_expected(**SWEEP) == want
    assert [r for r in clean["records"] if not _is_clean(r, want)] == []
    assert all(r["simd_mask"] == 0xF for r in clean["records"])
    info = p.streamload_sweep_info(0)
    assert info["scratch_bytes"] == 0 and info["blocks_per_cu"] == 1 and info["num_regs"] <= 128


@pytest.mark.parametrize("part", ref.PARTS)
def test_an_injected_part_fails_exactly_its_xcd_and_part(p, clean, part):
    xcd = sorted({r["xcd"] for r in clean["records"]})[-2]
    shape = {**SWEEP, "laps": 1}
    out = p.streamload_sweep(0, inject=(xcd, None, [part]), max_rounds=1, **shape)
    hit = [r for r in out["records"] if r["xcd"] == xcd]
    want = ref.digests(STREAMLOAD_SEED, shape["laps"], shape["ksteps"], shape["panels"])
    assert hit and all(r["fail"] == 1 << ref.PARTS.index(part) and r["bad"][part] == 1 for r in hit)
    assert all(_is_clean(r, want) for r in out["records"] if r["xcd"] != xcd)
    s = out["summary"]
    assert s["bad_xcds"] == [xcd] and s["failed_parts"] == [part] and s["xcds"][xcd]["failed_parts"] == [part]
    if part == "gemm":  # wave 0, its panel of lap 0 (group 0: one lap is a tail), the first span
        assert all((r["bad_subtiles"], r["bad_sets"], r["bad_spans"]) == (1, 1, 1) for r in hit)
