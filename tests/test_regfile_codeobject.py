"""k_regfile_sweep's code object, compiled for gfx950 without a GPU: the
kernel must be allocated the whole 512-entry register file with nothing
spilled, and its instructions must name every VGPR and every AGPR. Looks at
register names and metadata only."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

from flex_gpu_scheduler_amd.build_ext import CSRC, ROCM

SRC = CSRC / "hip" / "regfile_sweep.hip"
LLVM = ROCM / "llvm" / "bin"


def tool(name: str) -> str | None:
    return shutil.which(name) or (str(LLVM / name) if (LLVM / name).exists() else None)


HIPCC = shutil.which("hipcc") or (str(ROCM / "bin" / "hipcc") if (ROCM / "bin" / "hipcc").exists() else None)
pytestmark = pytest.mark.skipif(HIPCC is None or tool("llvm-readelf") is None or tool("llvm-objdump") is None,
                                reason="hipcc and the LLVM binary tools are needed")


@pytest.fixture(scope="module")
def obj(tmp_path_factory) -> Path:
    out = tmp_path_factory.mktemp("regfile") / "regfile_sweep.o"
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "--no-gpu-bundle-output",
           f"-I{CSRC}", "-c", str(SRC), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return out


def test_kernel_owns_the_whole_file_and_spills_nothing(obj):
    notes = subprocess.run([tool("llvm-readelf"), "--notes", str(obj)], capture_output=True, text=True, check=True).stdout
    kernels = [k for k in re.split(r"\n\s+- \.agpr_count:", "\n" + notes) if "k_regfile_sweep" in k]
    assert len(kernels) == 1
    k = ".agpr_count:" + kernels[0]

    def field(name: str) -> int:
        m = re.search(rf"\.{name}:\s+(\d+)", k)
        assert m, name
        return int(m.group(1))

    assert field("vgpr_count") == 512  # VGPRs + AGPRs: the whole file of a SIMD
    assert field("agpr_count") == 256
    assert field("vgpr_spill_count") == 0 and field("sgpr_spill_count") == 0
    assert field("private_segment_fixed_size") == 0
    assert field("max_flat_workgroup_size") == 256


def test_every_register_is_named(obj):
    dis = subprocess.run([tool("llvm-objdump"), "-d", str(obj)], capture_output=True, text=True, check=True).stdout
    written = {int(m) for m in re.findall(r"v_accvgpr_write_b32 a(\d+),", dis)}
    read = {int(m) for m in re.findall(r"v_accvgpr_read_b32 v\d+, a(\d+)", dis)}
    assert written == set(range(256))
    assert read == set(range(256))
    vgprs = {int(m) for m in re.findall(r"\bv(\d+)\b", dis)}
    assert set(range(256)) <= vgprs
    # written and read back in both passes
    assert len(re.findall(r"v_accvgpr_write_b32 a\d+,", dis)) == 512
    assert len(re.findall(r"v_accvgpr_read_b32 v\d+, a\d+", dis)) == 512
