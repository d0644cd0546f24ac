"""k_regfile_sweep on the GPU (csrc/hip/regfile_sweep.hip).

The digests a clean sweep leaves are compared with the numpy reference
(tests/regfile_sweep_ref.py, written from the formulas): they are sums over
the values read back from all 512 x 64 cells of a wave in both polarities, so
a cell the statement skipped, mislabelled or corrupted through a missed wait
state changes them. Injected mis-compares must be localised to their CU, XCD,
cell, bit and file; a register complemented through the index mode must be
named by the straight-line read-back. Every comparison is equality."""
import ctypes

import pytest

import regfile_sweep_ref as ref
from flex_gpu_scheduler_amd.control.node_agent import GpuHealth, hip_health_fn
from flex_gpu_scheduler_amd.ops.hip_probe import ProbeError, probe

pytestmark = pytest.mark.gpu

NO_CELL = 0xFFFF
CLEAN = {"fail": 0, "bad_vgpr": 0, "bad_agpr": 0, "first": NO_CELL, "flip": 0, "bad_simds": 0}


@pytest.fixture(scope="module")
def p():
    return probe()


@pytest.fixture(scope="module")
def cus(p):
    return int(p.props(0)["computeUnits"])


@pytest.fixture(scope="module")
def clean(p):
    return p.regfile_sweep(0)


@pytest.fixture(scope="module")
def target(clean):
    """(xcd, cu key) of one CU the clean sweep reached."""
    keys = sorted(_keys(clean["records"]))
    return keys[len(keys) // 9]


def _keys(records):
    return {(r["xcd"], r["cu"]) for r in records}


def _is_clean(r, digest):
    return all(r[k] == v for k, v in CLEAN.items()) and r["digest"] == digest and r["simd_mask"] == 15


# -------------------------------------------------------------------- tests
def test_clean_sweep_covers_every_cu(p, cus, clean):
    s = clean["summary"]
    print("regfile_sweep defaults:", {k: s[k] for k in ("rounds", "ms", "blocks", "covered", "uncovered")})
    assert s["covered"]
    assert len(_keys(clean["records"])) == cus
    print("simd masks:", sorted({r["simd_mask"] for r in clean["records"]}))
    assert all(r["simd_mask"] == 15 for r in clean["records"])
    bad = [r for r in clean["records"] if r["fail"]]
    print("failing records:", bad[:4])
    assert not bad
    assert all(_is_clean(r, ref.group_digest(ref.SEEDS[0])) for r in clean["records"])
    assert s["bad_xcds"] == [] and s["failed_files"] == [] and s["bad_cells"] == 0
    assert all(v["failed_files"] == [] and v["cus_seen"] == v["cus_expected"] for v in s["xcds"].values())


def test_the_kernel_owns_the_whole_register_file(p):
    info = p.regfile_sweep_info(0)
    print("regfile_sweep_info:", info)
    assert info["blocks_per_cu"] == 1
    assert info["scratch_bytes"] == 0


@pytest.mark.parametrize("seed", ref.SEEDS)
def test_digest_equals_the_numpy_reference(p, clean, seed):
    want = ref.group_digest(seed)
    assert p.regfile_sweep_expected(seed) == want
    out = clean if seed == ref.SEEDS[0] else p.regfile_sweep(0, seed=seed)
    got = {r["digest"] for r in out["records"]}
    print(f"seed {seed:#x}: digests {sorted(hex(d) for d in got)[:4]}, reference {want:#x}")
    assert got == {want}
    assert all(r["fail"] == 0 for r in out["records"])
    assert out["summary"]["seed"] == seed


def test_digests_differ_between_the_seeds():
    assert ref.group_digest(ref.SEEDS[0]) != ref.group_digest(ref.SEEDS[1])


@pytest.mark.parametrize("bit", [0, 31])
@pytest.mark.parametrize("reg", [0, 7, 8, 15, 16, 255, 256, 511])
def test_injection_is_localised_to_one_cu_cell_bit_and_file(p, target, reg, bit):
    xcd, cu = target
    out = p.regfile_sweep(0, inject=(xcd, cu, reg, bit))
    s = out["summary"]
    hit = [r for r in out["records"] if (r["xcd"], r["cu"]) == (xcd, cu)]
    file_bit, file_name = (1, "vgpr") if reg < 256 else (2, "agpr")
    print("hit records:", hit[:2])
    assert hit
    for r in hit:
        assert r["bad_vgpr"] + r["bad_agpr"] == 256  # one cell x 64 lanes x 4 waves, pass 0 only
        assert (r["bad_vgpr"], r["bad_agpr"]) == ((256, 0) if reg < 256 else (0, 256))
        assert r["first"] == reg and r["flip"] == 1 << bit
        assert r["fail"] == file_bit and r["bad_simds"] == 15 and r["simd_mask"] == 15
    want = ref.group_digest(ref.SEEDS[0])
    assert all(_is_clean(r, want) for r in out["records"] if (r["xcd"], r["cu"]) != (xcd, cu))
    assert s["bad_xcds"] == [xcd] and s["failed_files"] == [file_name]
    v = s["xcds"][xcd]
    assert v["failed_cus"] == [cu] and v["failed_files"] == [file_name]
    assert v["bad_cells"] == 256 and v["flip_mask"] == f"0x{1 << bit:08x}" and v["bad_simds"] == {cu: [0, 1, 2, 3]}


def test_injection_wildcard_flags_one_whole_xcd(p, clean):
    xcd = max(r["xcd"] for r in clean["records"])
    out = p.regfile_sweep(0, inject=(xcd, None, 300, 5))
    s = out["summary"]
    assert s["bad_xcds"] == [xcd] and s["failed_files"] == ["agpr"]
    assert s["xcds"][xcd]["failed_cus"] == sorted(c for x, c in _keys(out["records"]) if x == xcd)
    assert all((r["fail"] == 2) == (r["xcd"] == xcd) for r in out["records"])
    assert all(r["fail"] in (0, 2) for r in out["records"])
    assert all(r["first"] == 300 and r["flip"] == 32 and r["bad_agpr"] == 256 for r in out["records"] if r["fail"])


@pytest.mark.parametrize("reg", [0, 7, 8, 15, 16, 128, 255])
def test_poison_through_the_index_mode_is_named_by_the_read_back(p, target, reg):
    xcd, cu = target
    out = p.regfile_sweep(0, poison=(xcd, cu, reg))
    s = out["summary"]
    hit = [r for r in out["records"] if (r["xcd"], r["cu"]) == (xcd, cu)]
    print("hit records:", hit[:2])
    assert hit
    for r in hit:
        assert r["first"] == reg  # exactly that register
        assert (r["bad_vgpr"], r["bad_agpr"]) == (4 * 64, 0)  # 64 cells per wave, pass 0 only
        assert r["flip"] == 0xFFFFFFFF and r["fail"] == 1 and r["bad_simds"] == 15
    want = ref.group_digest(ref.SEEDS[0])
    assert all(_is_clean(r, want) for r in out["records"] if (r["xcd"], r["cu"]) != (xcd, cu))
    assert s["bad_xcds"] == [xcd] and s["failed_files"] == ["vgpr"]
    assert s["xcds"][xcd]["failed_cus"] == [cu]


def test_one_block_is_uncovered_not_failed(p):
    out = p.regfile_sweep(0, blocks=1)
    s = out["summary"]
    assert len(out["records"]) == 1 and s["rounds"] == 1
    assert not s["covered"]
    assert s["bad_xcds"] == [] and out["records"][0]["fail"] == 0
    verdict = hip_health_fn(regfile=True, regfile_args={"blocks": 1})(0)
    assert verdict.ok if isinstance(verdict, GpuHealth) else verdict is True


@pytest.mark.parametrize("args", [
    dict(inject_reg=512), dict(inject_reg=-2), dict(inject_bit=32), dict(inject_bit=-1), dict(poison_reg=256),
    dict(poison_reg=-2), dict(blocks=-1), dict(blocks=(1 << 20) + 1), dict(inject_xcd=16), dict(inject_xcd=-2),
    dict(inject_cu=256), dict(inject_cu=-2),
])
def test_bad_arguments_are_refused(p, args):
    a = dict(blocks=4, inject_xcd=-1, inject_cu=-1, inject_reg=-1, inject_bit=0, poison_reg=-1)
    a.update(args)
    buf = (ctypes.c_uint32 * (16 * 4))()
    rc = p.lib.xs_regfile_sweep(0, a["blocks"], ref.SEEDS[0], a["inject_xcd"], a["inject_cu"], a["inject_reg"],
                                a["inject_bit"], a["poison_reg"], buf, None, None)
    assert rc == -1000
    assert not any(buf)  # nothing ran


def test_bad_arguments_raise_from_python(p):
    for kw in (dict(blocks=-1), dict(inject=(0, None, 512, 0)), dict(inject=(0, None, 0, 32)),
               dict(poison=(0, None, 256))):
        with pytest.raises(ProbeError) as e:
            p.regfile_sweep(0, **kw)
        assert e.value.rc == -1000
    with pytest.raises(ValueError):
        p.regfile_sweep(0, inject=(0, None, 1, 0), poison=(1, None, 1))
    assert p.lib.xs_regfile_sweep_expected(0, None) == -1000
    assert p.lib.xs_regfile_sweep_info(0, None) == -1000


def test_health_fn_with_the_register_sweep(p, cus, clean):
    assert hip_health_fn(regfile=True)(0)
    xcd = clean["records"][0]["xcd"]
    v = hip_health_fn(regfile=True, regfile_args={"inject": (xcd, None, 456, 9)})(0)
    if cus // 32 >= 8:
        assert isinstance(v, GpuHealth) and not v and not v.ok
        assert v.bad_xcds == frozenset({xcd})
        n = len([c for x, c in _keys(clean["records"]) if x == xcd])
        assert v.detail["registerFaults"] == {
            xcd: {"files": ["agpr"], "cells": 256 * n, "flipMask": "0x00000200", "simds": 4 * n}}
    else:
        assert v is False
