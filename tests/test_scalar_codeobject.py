"""k_scalar_sweep's code object, compiled for gfx950 without a GPU. Every
instruction the header of csrc/hip/scalar_sweep.hip lists must be in the code
under its own mnemonic; each of the six conditional branches under test jumps
forward; nothing may spill, the kernel has no scratch, a workgroup is 1,024
threads and a wave gets the largest SGPR allocation there is."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

import scalar_sweep_ref as ref
from flex_gpu_scheduler_amd.build_ext import CSRC, ROCM

SRC = CSRC / "hip" / "scalar_sweep.hip"
LLVM = ROCM / "llvm" / "bin"


def tool(name: str) -> str | None:
    return shutil.which(name) or (str(LLVM / name) if (LLVM / name).exists() else None)


HIPCC = shutil.which("hipcc") or (str(ROCM / "bin" / "hipcc") if (ROCM / "bin" / "hipcc").exists() else None)
pytestmark = pytest.mark.skipif(HIPCC is None or tool("llvm-readelf") is None or tool("llvm-objdump") is None,
                                reason="hipcc and the LLVM binary tools are needed")

# The steps that are sequences, by the instruction they are about, and the forms the disassembler prints.
RENAMED = {"add128": "s_addc_u32", "sub128": "s_subb_u32", "v_addc_co_u32": "v_addc_co_u32_e64"}
ALSO = ["v_readlane_b32", "v_writelane_b32", "v_readfirstlane_b32", "v_cndmask_b32_e32", "v_cndmask_b32_e64",
        "v_add_co_u32_e64", "s_getreg_b32", "s_barrier", "s_cselect_b32", "s_cmp_lg_u32"]
BRANCHES = ["s_cbranch_scc0", "s_cbranch_scc1", "s_cbranch_vccz", "s_cbranch_vccnz", "s_cbranch_execz",
            "s_cbranch_execnz"]


@pytest.fixture(scope="module")
def built(tmp_path_factory) -> Path:
    d = tmp_path_factory.mktemp("scalar")
    out = d / "scalar_sweep.o"
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "--no-gpu-bundle-output",
           f"-I{CSRC}", "-c", str(SRC), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=d)
    assert r.returncode == 0, r.stderr[-4000:]
    return out


@pytest.fixture(scope="module")
def sweep(built) -> str:
    """Disassembly of k_scalar_sweep alone, the encodings and comments stripped."""
    dis = subprocess.run([tool("llvm-objdump"), "-d", "--no-show-raw-insn", str(built)], capture_output=True, text=True,
                         check=True).stdout
    parts = re.split(r"\n(?=[0-9a-f]+ <[^>]+>:)", dis)
    mine = [p for p in parts if re.match(r"[0-9a-f]+ <\S*k_scalar_sweep\S*>:", p)]
    assert len(mine) == 1
    return "\n".join(re.sub(r"\s*//.*$", "", line) for line in mine[0].splitlines()) + "\n"


def test_kernels_spill_nothing_use_no_scratch_and_get_the_largest_sgpr_allocation(built, sweep):
    notes = subprocess.run([tool("llvm-readelf"), "--notes", str(built)], capture_output=True, text=True, check=True).stdout
    for kernel in ("k_scalar_sweep", "k_scalar_probe"):
        ks = [k for k in re.split(r"\n\s+- \.agpr_count:", "\n" + notes) if kernel in k]
        assert len(ks) == 1, kernel
        k = ".agpr_count:" + ks[0]

        def field(name: str) -> int:
            m = re.search(rf"\.{name}:\s+(\d+)", k)
            assert m, name
            return int(m.group(1))

        assert field("vgpr_spill_count") == 0 and field("sgpr_spill_count") == 0
        assert field("private_segment_fixed_size") == 0
        assert field("max_flat_workgroup_size") == 1024
        assert field("group_segment_fixed_size") == 0  # the LDS is dynamic: the launch sizes it to own the CU
        assert field("vgpr_count") <= 128  # four waves of it on a SIMD
        # 97..112 registers are seven blocks of 16; with the trap handler's 16 a wave takes 128.
        assert 97 <= field("sgpr_count") <= 112
    assert not re.search(r"^\s+scratch_", sweep, re.M)


def test_every_listed_instruction_is_in_the_code_under_its_own_name(sweep):
    ops = set(re.findall(r"^\s+([a-z][a-z0-9_]+)", sweep, re.M))
    want = {RENAMED.get(s[1], s[1]) for s in ref.STEPS} | set(ref.MOVREL_FORMS) | set(ALSO)
    assert want <= ops, sorted(want - ops)
    assert len(want) >= 150  # distinct mnemonics; the immediates and constants of one instruction count once


def test_each_branch_under_test_jumps_forward_over_one_s_mov(sweep):
    lines = [l.strip() for l in sweep.splitlines() if l.strip()]
    for name in BRANCHES:
        # the statement's own: "s_mov_b32 s46, 1; <branch> T; s_mov_b32 s46, 2; T:"
        at = [i for i, l in enumerate(lines) if l.startswith(name + " ") and lines[i - 1] == "s_mov_b32 s46, 1"]
        assert at, name
        for i in at:
            assert lines[i + 1] == "s_mov_b32 s46, 2", (name, lines[i + 1])
            m = re.match(rf"{name} (\d+)$", lines[i])
            assert m and int(m.group(1)) == 1, lines[i]  # one instruction of one dword is skipped: forward


def test_the_sgpr_part_names_every_register_between_barriers(sweep):
    written = {int(n) for n in re.findall(r"v_readlane_b32 s(\d+), v\d+, \d+\s", sweep)}
    read = {int(n) for n in re.findall(r"v_writelane_b32 v\d+, s(\d+), \d+\s", sweep)}
    assert set(range(100)) <= written and set(range(100)) <= read
    assert re.search(r"v_readlane_b32 vcc_lo, v\d+, 42\s", sweep) and re.search(r"v_writelane_b32 v\d+, vcc_hi, 43\s", sweep)
    assert len(re.findall(r"^\s+s_barrier\s", sweep, re.M)) == 4 + 3  # four of the sgpr part, three of the two-stage reduction
