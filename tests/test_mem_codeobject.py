"""k_mem_sweep's code object, compiled for gfx950 without a GPU. Every
instruction the header of csrc/hip/mem_sweep.hip lists must be in the code
under its own mnemonic, in the addressing form and with the cache-policy bits
the header claims for it; nothing may spill, and the kernel must have no
scratch (a flat access must never be able to resolve to private memory)."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

from flex_gpu_scheduler_amd.build_ext import CSRC, ROCM

SRC = CSRC / "hip" / "mem_sweep.hip"
LLVM = ROCM / "llvm" / "bin"


def tool(name: str) -> str | None:
    return shutil.which(name) or (str(LLVM / name) if (LLVM / name).exists() else None)


HIPCC = shutil.which("hipcc") or (str(ROCM / "bin" / "hipcc") if (ROCM / "bin" / "hipcc").exists() else None)
pytestmark = pytest.mark.skipif(HIPCC is None or tool("llvm-readelf") is None or tool("llvm-objdump") is None,
                                reason="hipcc and the LLVM binary tools are needed")

GLOBAL = """global_load_ubyte global_load_sbyte global_load_ushort global_load_sshort global_load_dword global_load_dwordx2
global_load_dwordx3 global_load_dwordx4 global_load_short_d16 global_load_short_d16_hi global_load_ubyte_d16
global_load_ubyte_d16_hi global_load_sbyte_d16 global_load_sbyte_d16_hi global_store_byte global_store_short
global_store_dword global_store_dwordx2 global_store_dwordx3 global_store_dwordx4 global_store_short_d16_hi
global_store_byte_d16_hi""".split()
BUFFER = """buffer_load_ubyte buffer_load_sbyte buffer_load_ushort buffer_load_sshort buffer_load_dword
buffer_load_dwordx2 buffer_load_dwordx3 buffer_load_dwordx4 buffer_store_byte buffer_store_short buffer_store_dword
buffer_store_dwordx2 buffer_store_dwordx3 buffer_store_dwordx4""".split()
FLAT = """flat_load_ubyte flat_load_sbyte flat_load_ushort flat_load_sshort flat_load_dword flat_load_dwordx3
flat_load_dwordx4 flat_store_byte flat_store_short flat_store_dword flat_store_dwordx2 flat_store_dwordx4""".split()
ATOMIC = """global_atomic_add global_atomic_sub global_atomic_smin global_atomic_smax global_atomic_umin global_atomic_umax
global_atomic_and global_atomic_or global_atomic_xor global_atomic_swap global_atomic_cmpswap global_atomic_inc
global_atomic_dec global_atomic_add_x2 global_atomic_smin_x2 global_atomic_umax_x2 global_atomic_swap_x2
global_atomic_cmpswap_x2 global_atomic_add_f32 global_atomic_pk_add_f16 global_atomic_pk_add_bf16 global_atomic_add_f64
global_atomic_min_f64 global_atomic_max_f64""".split()
SCALAR = """s_load_dword s_load_dwordx2 s_load_dwordx4 s_load_dwordx8 s_load_dwordx16 s_buffer_load_dword
s_buffer_load_dwordx4""".split()

V, VV, SS, S4 = r"v\d+", r"v\[\d+:\d+\]", r"s\[\d+:\d+\]", r"s\[\d+:\d+\]"
# The forms the header claims, as the disassembler prints them.
FORMS = {
    "saddr load, offsets 0-12": rf"global_load_dword {V}, {V}, {SS} offset:12\s",
    "saddr store": rf"global_store_dwordx2 {V}, {VV}, {SS}\s",
    "the most negative offset, saddr load": rf"global_load_dword {V}, {V}, {SS} offset:-4096\s",
    "the most negative offset, saddr store": rf"global_store_dword {V}, {V}, {SS} offset:-4096\s",
    "the most negative offset, vaddr store": rf"global_store_dwordx2 {VV}, {VV}, off offset:-4096\s",
    "the largest offset, vaddr load": rf"global_load_dword {V}, {VV}, off offset:4095\s",
    "the largest offset, vaddr store": rf"global_store_dword {VV}, {V}, off offset:4095\s",
    "the largest offset, saddr load": rf"global_load_dwordx2 {VV}, {V}, {SS} offset:4095\s",
    "d16_hi at a negative offset": rf"global_load_short_d16_hi {V}, {VV}, off offset:-16\s",
    "the read behind an atomic": rf"global_load_dword {V}, {VV}, off sc1\s",
    "the read behind a 64-bit atomic": rf"global_load_dwordx2 {VV}, {VV}, off sc1\s",
    "l1 plain": rf"global_load_dword {V}, {VV}, off\s",
    "l1 sc0": rf"global_load_dword {V}, {VV}, off sc0\s",
    "l2 sc1": rf"global_load_dwordx4 {VV}, {V}, {SS} sc1\s",
    "l2 nt": rf"global_load_dwordx4 {VV}, {V}, {SS} nt\s",
    "l2 plain": rf"global_load_dwordx4 {VV}, {V}, {SS}\s",
    "l2 write": rf"global_store_dwordx4 {V}, {VV}, {SS}\s",
    "buffer offen": rf"buffer_load_dword {V}, {V}, {S4}, (s\d+|0) offen offset:12\s",
    "buffer idxen": rf"buffer_store_dword {V}, {V}, {S4}, (s\d+|0) idxen offset:12\s",
    "buffer idxen load": rf"buffer_load_dwordx4 {VV}, {V}, {S4}, (s\d+|0) idxen\s",
    "buffer idxen offen": rf"buffer_store_dwordx2 {VV}, {VV}, {S4}, (s\d+|0) idxen offen\s",
    "buffer idxen offen sc1": rf"buffer_load_dwordx2 {VV}, {VV}, {S4}, (s\d+|0) idxen offen sc1\s",
    "buffer soffset": rf"buffer_load_dword {V}, {V}, {S4}, s\d+ offen\s",
    "flat offset": rf"flat_load_dword {V}, {VV} offset:12\s",
    "scalar immediate offset": rf"s_load_dwordx2 {SS}, {SS}, 0x40\s",
    "scalar SGPR offset": rf"s_load_dwordx16 {SS}, {SS}, s\d+\s",
    "scalar x8 SGPR offset": rf"s_load_dwordx8 {SS}, {SS}, s\d+\s",
    "scalar buffer": rf"s_buffer_load_dwordx4 {SS}, {S4}, s\d+\s",
    "scalar buffer dword": rf"s_buffer_load_dword s\d+, {S4}, s\d+\s",
}


@pytest.fixture(scope="module")
def built(tmp_path_factory) -> Path:
    d = tmp_path_factory.mktemp("mem")
    out = d / "mem_sweep.o"
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "--no-gpu-bundle-output",
           f"-I{CSRC}", "-c", str(SRC), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=d)
    assert r.returncode == 0, r.stderr[-4000:]
    return out


@pytest.fixture(scope="module")
def sweep(built) -> str:
    """Disassembly of k_mem_sweep alone, the encodings and comments stripped."""
    dis = subprocess.run([tool("llvm-objdump"), "-d", "--no-show-raw-insn", str(built)], capture_output=True, text=True,
                         check=True).stdout
    parts = re.split(r"\n(?=[0-9a-f]+ <[^>]+>:)", dis)
    mine = [p for p in parts if re.match(r"[0-9a-f]+ <\S*k_mem_sweep\S*>:", p)]
    assert len(mine) == 1
    return "\n".join(re.sub(r"\s*//.*$", "", line) for line in mine[0].splitlines()) + "\n"


def test_kernels_spill_nothing_and_use_no_scratch(built, sweep):
    notes = subprocess.run([tool("llvm-readelf"), "--notes", str(built)], capture_output=True, text=True, check=True).stdout
    for kernel in ("k_mem_sweep", "k_mem_probe"):
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
    assert not re.search(r"^\s+scratch_", sweep, re.M)


def test_every_listed_instruction_is_in_the_code_under_its_own_name(sweep):
    ops = set(re.findall(r"^\s+([a-z][a-z0-9_]+)", sweep, re.M))
    want = set(GLOBAL) | set(BUFFER) | set(FLAT) | set(ATOMIC) | set(SCALAR)
    assert want <= ops, sorted(want - ops)


@pytest.mark.parametrize("what", sorted(FORMS))
def test_the_forms_and_cache_policies_the_header_claims(sweep, what):
    assert re.search(FORMS[what], sweep), FORMS[what]


def test_every_atomic_returns_and_nothing_else_carries_its_bit(sweep):
    atomics = re.findall(r"^\s+(global_atomic_\S+) ([^\n]*)", sweep, re.M)
    assert len(atomics) >= 2 * 13 + 5 + 2 * 3 + 3 + 4
    assert all(args.rstrip().endswith("off sc0") for _, args in atomics), [a for a in atomics if "sc0" not in a[1]][:3]
    # Four sc0 loads a step, sixteen steps a pass, two passes: the l1 route, unrolled or not.
    assert len(re.findall(r"global_load_dword v\d+, v\[\d+:\d+\], off sc0\s", sweep)) >= 4


def test_buffer_accesses_go_through_descriptors_in_sgprs(sweep):
    lines = re.findall(r"^\s+(buffer_(?:load|store)_\S+) ([^\n]*)", sweep, re.M)
    assert lines and all(re.search(r"s\[\d+:\d+\], (s\d+|0) ", args + " ") for _, args in lines)
    modes = {tuple(m for m in ("idxen", "offen") if m in args) for _, args in lines}
    assert modes == {("idxen",), ("offen",), ("idxen", "offen")}
