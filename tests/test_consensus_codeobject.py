"""k_consensus_sweep's code object, compiled for gfx950 without a GPU. Every
mnemonic of the step table (tests/consensus_sweep_ref.py) must be in the code
under its own name; nothing may spill, the kernels have no scratch and no
static LDS, and a workgroup is 256 threads."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

import consensus_sweep_ref as ref
from flex_gpu_scheduler_amd.build_ext import CSRC, ROCM

SRC = CSRC / "hip" / "consensus_sweep.hip"
LLVM = ROCM / "llvm" / "bin"


def tool(name: str) -> str | None:
    return shutil.which(name) or (str(LLVM / name) if (LLVM / name).exists() else None)


HIPCC = shutil.which("hipcc") or (str(ROCM / "bin" / "hipcc") if (ROCM / "bin" / "hipcc").exists() else None)
pytestmark = pytest.mark.skipif(HIPCC is None or tool("llvm-readelf") is None or tool("llvm-objdump") is None,
                                reason="hipcc and the LLVM binary tools are needed")

# What the sweep leans on besides the instructions under test.
ALSO = ["s_getreg_b32", "s_barrier", "ds_write_b32", "ds_read_b32", "v_cndmask_b32_e64", "v_cmp_ne_u32_e32"]


@pytest.fixture(scope="module")
def built(tmp_path_factory) -> Path:
    d = tmp_path_factory.mktemp("consensus")
    out = d / "consensus_sweep.o"
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "--no-gpu-bundle-output",
           f"-I{CSRC}", "-c", str(SRC), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=d)
    assert r.returncode == 0, r.stderr[-4000:]
    return out


@pytest.fixture(scope="module")
def sweep(built) -> str:
    """Disassembly of k_consensus_sweep alone, the encodings and comments stripped."""
    dis = subprocess.run([tool("llvm-objdump"), "-d", "--no-show-raw-insn", str(built)], capture_output=True, text=True,
                         check=True).stdout
    parts = re.split(r"\n(?=[0-9a-f]+ <[^>]+>:)", dis)
    mine = [p for p in parts if re.match(r"[0-9a-f]+ <\S*k_consensus_sweep\S*>:", p)]
    assert len(mine) == 1
    return "\n".join(re.sub(r"\s*//.*$", "", line) for line in mine[0].splitlines()) + "\n"


def test_kernels_spill_nothing_use_no_scratch_and_run_256_threads(built, sweep):
    notes = subprocess.run([tool("llvm-readelf"), "--notes", str(built)], capture_output=True, text=True, check=True).stdout
    for kernel in ("k_consensus_sweep", "k_consensus_probe"):
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
        # The LDS is dynamic and starts at 0: the kernel addresses its tiles from there.
        assert field("group_segment_fixed_size") == 0
        assert field("vgpr_count") <= 512  # one wave per SIMD
    assert not re.search(r"^\s+scratch_", sweep, re.M)


def test_every_step_is_in_the_code_under_its_own_mnemonic(sweep):
    ops = set(re.findall(r"^\s+([a-z][a-z0-9_]+)", sweep, re.M))
    bare = {re.sub(r"_(e32|e64|sdwa|dpp)$", "", o) for o in ops} | ops
    want = set(ALSO)
    for _, name, _, _ in ref.STEPS:
        want |= set(ref.SEQUENCES.get(name, [name]))
    assert want <= bare, sorted(want - bare)
    assert len({s[1] for s in ref.STEPS}) >= 140  # distinct steps by name; a mnemonic run with two modifiers counts once


def test_the_modifier_forms_are_in_the_code(sweep):
    """The mnemonic alone does not show a format pair, an abid, a byte select or
    an op_sel: each modifier combination the step table runs is matched on its line."""
    def lines(mnemonic):
        return [l for l in sweep.splitlines() if re.match(rf"\s+{mnemonic}(_e64|_sdwa)?\s", l)]

    for shape in ("16x16x128", "32x32x64"):
        plain = [l for l in lines(f"v_mfma_f32_{shape}_f8f6f4") if "cbsz" not in l and "blgp" not in l]
        assert plain, shape  # unscaled, fp8 x fp8
    assert any("cbsz:1 blgp:4" in l for l in lines("v_mfma_f32_16x16x128_f8f6f4"))  # bf8 x fp4
    assert any("cbsz:2 blgp:3" in l for l in lines("v_mfma_f32_16x16x128_f8f6f4"))  # fp6 x bf6
    assert any("cbsz:1 blgp:2" in l for l in lines("v_mfma_f32_32x32x64_f8f6f4"))  # bf8 x fp6
    scaled16, scaled32 = lines("v_mfma_scale_f32_16x16x128_f8f6f4"), lines("v_mfma_scale_f32_32x32x64_f8f6f4")
    assert any("cbsz" not in l and "blgp" not in l for l in scaled16) and any("cbsz:1 blgp:4" in l for l in scaled16)
    assert any("blgp:2" in l and "cbsz" not in l for l in scaled32)  # cbsz 0 is not printed: fp8 x fp6
    for _, name, _, _ in ref.steps_of("smfmac"):
        mine = lines(name)  # both abid encodings, in order; abid 0 is not printed
        assert len(mine) == 2 and all("cbsz:1" in l for l in mine), (name, mine)
        if name.endswith(("_f16", "_bf16")):
            assert "abid:1" in mine[0] and "abid:3" in mine[1], (name, mine)
        else:
            assert "abid" not in mine[0] and "abid:1" in mine[1], (name, mine)
    for fmt in ("fp8", "bf8"):
        sel = {m.group(1) for l in lines(f"v_cvt_f32_{fmt}") for m in [re.search(r"src0_sel:(BYTE_\d)", l)] if m}
        assert sel >= {"BYTE_1", "BYTE_2", "BYTE_3"}, (fmt, sel)
    assert any("op_sel:[0,1,0] op_sel_hi:[1,1,0]" in l for l in lines("v_fma_mix_f32"))
    assert any("op_sel:[1,0,0]" in l for l in lines("v_fma_mixlo_f16"))


def test_the_kernel_writes_no_mode_register_and_waits_on_no_other_workgroup(sweep):
    assert not re.search(r"^\s+s_setreg", sweep, re.M)
    assert not re.search(r"^\s+(s_sleep|global_atomic|flat_atomic|buffer_atomic)", sweep, re.M)
    # Two barriers: both of the reduction.
    assert len(re.findall(r"^\s+s_barrier\s", sweep, re.M)) == 2
