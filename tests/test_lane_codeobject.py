"""k_lane_sweep's code object, compiled for gfx950 without a GPU. The compiler
is free to fold a DPP move or to turn a shuffle into something else, and a path
it rewrote tests nothing: every path's instructions must be in the code under
their own names, nothing may spill, and the reduction between the paths and
the record store must not use what the sweep tests."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

from flex_gpu_scheduler_amd.build_ext import CSRC, ROCM

SRC = CSRC / "hip" / "lane_sweep.hip"
LLVM = ROCM / "llvm" / "bin"


def tool(name: str) -> str | None:
    return shutil.which(name) or (str(LLVM / name) if (LLVM / name).exists() else None)


HIPCC = shutil.which("hipcc") or (str(ROCM / "bin" / "hipcc") if (ROCM / "bin" / "hipcc").exists() else None)
pytestmark = pytest.mark.skipif(HIPCC is None or tool("llvm-readelf") is None or tool("llvm-objdump") is None,
                                reason="hipcc and the LLVM binary tools are needed")

CROSS_LANE = re.compile(r"_dpp\b|\bquad_perm|\brow_|\bwave_sh|\bwave_ro|v_permlane|ds_bpermute|ds_permute|ds_swizzle|"
                        r"v_readlane|v_writelane")


@pytest.fixture(scope="module")
def built(tmp_path_factory) -> Path:
    """The object file; -save-temps leaves the assembly (with the source's asm comments) beside it."""
    d = tmp_path_factory.mktemp("lane")
    out = d / "lane_sweep.o"
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "--no-gpu-bundle-output",
           "-save-temps=obj", f"-I{CSRC}", "-c", str(SRC), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=d)
    assert r.returncode == 0, r.stderr[-4000:]
    return out


@pytest.fixture(scope="module")
def sweep(built) -> str:
    """Disassembly of k_lane_sweep alone."""
    dis = subprocess.run([tool("llvm-objdump"), "-d", str(built)], capture_output=True, text=True, check=True).stdout
    parts = re.split(r"\n(?=[0-9a-f]+ <[^>]+>:)", dis)
    mine = [p for p in parts if re.match(r"[0-9a-f]+ <\S*k_lane_sweep\S*>:", p)]
    assert len(mine) == 1
    return mine[0]


def test_kernels_spill_nothing_and_use_no_scratch(built):
    notes = subprocess.run([tool("llvm-readelf"), "--notes", str(built)], capture_output=True, text=True, check=True).stdout
    for kernel in ("k_lane_sweep", "k_lane_probe"):
        ks = [k for k in re.split(r"\n\s+- \.agpr_count:", "\n" + notes) if kernel in k]
        assert len(ks) == 1, kernel
        k = ".agpr_count:" + ks[0]

        def field(name: str) -> int:
            m = re.search(rf"\.{name}:\s+(\d+)", k)
            assert m, name
            return int(m.group(1))

        assert field("vgpr_spill_count") == 0 and field("sgpr_spill_count") == 0
        assert field("private_segment_fixed_size") == 0
        assert field("max_flat_workgroup_size") == 256
        assert field("group_segment_fixed_size") == 0  # the LDS is dynamic: the launch sizes it to own the CU
        assert field("vgpr_count") <= 256  # one 256-thread workgroup must fit


def test_dpp_controls_are_all_there(sweep):
    dpp = re.findall(r"v_mov_b32_dpp [^\n/]*", sweep)
    text = "\n".join(dpp)
    for sel in ("[0,1,2,3]", "[1,2,3,0]", "[2,3,0,1]", "[3,0,1,2]"):
        assert f"quad_perm:{sel}" in text
    for kind in ("row_shl", "row_shr", "row_ror"):
        assert {int(n) for n in re.findall(rf"{kind}:(\d+)", text)} == set(range(1, 16)), kind
    assert {int(n) for n in re.findall(r"row_newbcast:(\d+)", text)} == set(range(16))
    for ctrl in ("row_mirror", "row_half_mirror", "row_bcast:15", "row_bcast:31", "wave_shl:1", "wave_rol:1",
                 "wave_shr:1", "wave_ror:1"):
        assert re.search(rf"{ctrl}\b", text), ctrl
    assert re.search(r"row_shr:3 row_mask:0xf bank_mask:0xf bound_ctrl:[01]", text)
    assert re.search(r"row_ror:5 row_mask:0xa bank_mask:0x5", text)
    assert len(dpp) == 75  # one move per step: none folded away, none added


def test_cross_lane_and_lds_instructions_are_there_under_their_own_names(sweep):
    ops = set(re.findall(r"^\s+([a-z][a-z0-9_]+)", sweep, re.M))
    want = {"v_permlane32_swap_b32_e32", "v_permlane16_swap_b32_e32", "v_readlane_b32", "v_writelane_b32",
            "v_readfirstlane_b32", "ds_bpermute_b32", "ds_permute_b32", "ds_swizzle_b32", "ds_read_b64_tr_b16",
            "global_load_lds_dword", "global_load_lds_dwordx3", "global_load_lds_dwordx4",
            # ldswide
            "ds_write_b64", "ds_write_b96", "ds_write_b128", "ds_write2_b32", "ds_write_b8", "ds_write_b16",
            "ds_read_b64", "ds_read_b96", "ds_read_b128", "ds_read2_b32", "ds_read2st64_b32", "ds_read_u8",
            "ds_read_i8", "ds_read_u16", "ds_read_i16",
            # ldsatomic: with return on a lane's own word, without on the common one
            "ds_add_rtn_u32", "ds_sub_rtn_u32", "ds_and_rtn_b32", "ds_or_rtn_b32", "ds_xor_rtn_b32",
            "ds_min_rtn_i32", "ds_max_rtn_i32", "ds_min_rtn_u32", "ds_max_rtn_u32", "ds_wrxchg_rtn_b32",
            "ds_cmpst_rtn_b32", "ds_add_rtn_u64", "ds_add_u32", "ds_xor_b32", "ds_max_u32", "ds_min_u32"}
    assert want <= ops, sorted(want - ops)
    assert not {o for o in ops if o.startswith(("flat_atomic", "global_atomic"))}  # the atomics stayed in LDS
    assert len(re.findall(r"ds_swizzle_b32", sweep)) == 9
    assert len(re.findall(r"v_permlane32_swap", sweep)) == 2 and len(re.findall(r"v_permlane16_swap", sweep)) == 2
    assert re.search(r"s_waitcnt vmcnt\(0\)", sweep)


def test_the_reduction_uses_nothing_the_sweep_tests(built):
    asm = next(built.parent.glob("*gfx950*.s")).read_text()
    body = asm[asm.index("k_lane_sweep"):]
    begin, end = body.index("; lane_sweep reduction begin"), body.index("; lane_sweep reduction end")
    assert 0 < begin < end
    red = body[begin:end]
    code = [ln.split(";")[0].strip() for ln in red.splitlines()]
    code = [ln for ln in code if ln and not ln.startswith(".") and not ln.endswith(":")]
    assert len(code) > 40  # the reduction is really between the markers
    used = [ln for ln in code if CROSS_LANE.search(ln)]
    assert not used, used[:5]
    assert any(ln.startswith("s_barrier") for ln in code)
    assert any(ln.startswith("ds_write") for ln in code) and any(ln.startswith("ds_read") for ln in code)
    stores = [ln for ln in code if ln.startswith("global_store_dwordx4")]
    assert len(stores) == 8  # the 128-byte record, vector stores
    # and the paths before it do use them, so the pattern is not blind: at
    # least 75 DPP moves, 4 swaps, 9 swizzles, a bpermute and a permute
    assert len([ln for ln in body[:begin].splitlines() if CROSS_LANE.search(ln.split(";")[0])]) >= 75 + 4 + 9 + 2
