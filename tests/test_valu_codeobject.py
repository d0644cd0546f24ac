"""k_valu_sweep's code object, compiled for gfx950 without a GPU. The compiler
may fuse, fold or rename what it is left to choose (plain `a * b + c` becomes
v_fmac_f32), and a step it rewrote tests something else: every step's
instruction must be in the code under its own name, nothing may spill, the
float mode must be the one the expected table is computed for, and the kernel
must not touch the MODE register."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

from flex_gpu_scheduler_amd.build_ext import CSRC, ROCM

SRC = CSRC / "hip" / "valu_sweep.hip"
LLVM = ROCM / "llvm" / "bin"


def tool(name: str) -> str | None:
    return shutil.which(name) or (str(LLVM / name) if (LLVM / name).exists() else None)


HIPCC = shutil.which("hipcc") or (str(ROCM / "bin" / "hipcc") if (ROCM / "bin" / "hipcc").exists() else None)
pytestmark = pytest.mark.skipif(HIPCC is None or tool("llvm-readelf") is None or tool("llvm-objdump") is None,
                                reason="hipcc and the LLVM binary tools are needed")

# The steps of csrc/hip/valu_sweep.hip as the disassembler prints them.
E32 = """v_add_f32 v_sub_f32 v_mul_f32 v_min_f32 v_max_f32 v_frexp_mant_f32 v_frexp_exp_i32_f32 v_fract_f32 v_trunc_f32
v_rndne_f32 v_floor_f32 v_ceil_f32 v_cmp_lt_f32 v_cmp_eq_f32 v_cmp_le_f32 v_cmp_gt_f32 v_cmp_lg_f32 v_cmp_ge_f32
v_cmp_class_f32 v_frexp_mant_f64 v_frexp_exp_i32_f64 v_fract_f64 v_trunc_f64 v_rndne_f64 v_floor_f64 v_ceil_f64
v_cmp_lt_f64 v_cmp_eq_f64 v_cmp_class_f64 v_add_f16 v_mul_f16 v_mul_u32_u24 v_mul_hi_u32_u24 v_add_co_u32
v_addc_co_u32 v_sub_co_u32 v_subb_co_u32 v_cmp_lt_u64 v_cmp_ge_i32 v_bfrev_b32 v_ffbh_u32 v_ffbl_b32 v_ffbh_i32
v_dot2c_f32_bf16 v_cvt_f32_i32 v_cvt_f32_u32 v_cvt_i32_f32 v_cvt_u32_f32 v_cvt_rpi_i32_f32 v_cvt_flr_i32_f32
v_cvt_f64_f32 v_cvt_f32_f64 v_cvt_f64_i32 v_cvt_i32_f64 v_cvt_f32_ubyte0 v_cvt_f32_ubyte1 v_cvt_f32_ubyte2
v_cvt_f32_ubyte3 v_cvt_f16_f32 v_cvt_f32_f16 v_cvt_pk_f32_fp8 v_exp_f32 v_log_f32 v_rcp_f32 v_rsq_f32 v_sqrt_f32
v_sin_f32 v_cos_f32 v_rcp_f64 v_rsq_f64 v_rcp_f16 v_rsq_f16 v_sqrt_f16 v_exp_f16 v_log_f16""".split()
PLAIN = """v_fma_f32 v_pk_add_f32 v_pk_mul_f32 v_pk_fma_f32 v_med3_f32 v_min3_f32 v_max3_f32 v_minimum3_f32 v_maximum3_f32
v_ldexp_f32 v_add_f64 v_mul_f64 v_fma_f64 v_min_f64 v_max_f64 v_ldexp_f64 v_fma_f16 v_pk_add_f16 v_pk_mul_f16
v_pk_fma_f16 v_pk_min_f16 v_pk_max_f16 v_pk_minimum3_f16 v_pk_maximum3_f16 v_fma_mix_f32 v_fma_mixlo_f16 v_mul_lo_u32
v_mul_hi_u32 v_mul_hi_i32 v_mad_u64_u32 v_mad_i64_i32 v_mad_u32_u24 v_mad_i32_i24 v_mad_u32_u16 v_pk_add_u16
v_pk_mad_i16 v_pk_mul_lo_u16 v_pk_min_i16 v_pk_max_u16 v_pk_lshlrev_b16 v_pk_ashrrev_i16 v_add3_u32 v_lshl_add_u32
v_xad_u32 v_lshl_add_u64 v_lshlrev_b64 v_lshrrev_b64 v_ashrrev_i64 v_sad_u8 v_perm_b32 v_alignbit_b32
v_alignbyte_b32 v_bfe_u32 v_bfe_i32 v_bfi_b32 v_bitop3_b32 v_bitop3_b16 v_and_or_b32 v_lshl_or_b32 v_bcnt_u32_b32
v_mbcnt_lo_u32_b32 v_mbcnt_hi_u32_b32 v_dot2_f32_f16 v_dot2_f32_bf16 v_dot4_i32_i8 v_dot4_u32_u8 v_dot8_i32_i4
v_dot8_u32_u4 v_cvt_pk_u8_f32 v_cvt_pk_f16_f32 v_cvt_pkrtz_f16_f32 v_cvt_pk_bf16_f32 v_cvt_pk_i16_i32
v_cvt_pk_u16_u32 v_ashr_pk_i8_i32 v_ashr_pk_u8_i32 v_cvt_pk_fp8_f32 v_cvt_pk_bf8_f32 v_cvt_scalef32_pk_fp8_f32
v_cvt_scalef32_pk_f32_fp8 v_cvt_scalef32_pk_fp4_f32 v_cvt_scalef32_pk_f32_fp4 v_msad_u8 v_cvt_pknorm_i16_f32
v_cvt_scalef32_pk32_f32_fp6""".split()
# The correctly rounded a / b and sqrt(a) of C++, f32 and f64.
EXPANSIONS = ["v_div_scale_f32", "v_div_fmas_f32", "v_div_fixup_f32", "v_div_scale_f64", "v_div_fmas_f64",
              "v_div_fixup_f64", "v_rcp_f32_e32", "v_rcp_f64_e32", "v_sqrt_f32_e32", "v_rsq_f64_e32"]


@pytest.fixture(scope="module")
def built(tmp_path_factory) -> Path:
    d = tmp_path_factory.mktemp("valu")
    out = d / "valu_sweep.o"
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "--no-gpu-bundle-output",
           "-save-temps=obj", f"-I{CSRC}", "-c", str(SRC), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=d)
    assert r.returncode == 0, r.stderr[-4000:]
    return out


@pytest.fixture(scope="module")
def sweep(built) -> str:
    """Disassembly of k_valu_sweep alone."""
    dis = subprocess.run([tool("llvm-objdump"), "-d", str(built)], capture_output=True, text=True, check=True).stdout
    parts = re.split(r"\n(?=[0-9a-f]+ <[^>]+>:)", dis)
    mine = [p for p in parts if re.match(r"[0-9a-f]+ <\S*k_valu_sweep\S*>:", p)]
    assert len(mine) == 1
    return mine[0]


@pytest.fixture(scope="module")
def asm(built) -> str:
    """The compiler's assembly of k_valu_sweep, with its kernel descriptor."""
    text = next(built.parent.glob("*gfx950*.s")).read_text()
    m = re.search(r"\.amdhsa_kernel \S*k_valu_sweep\S*\n.*?\.end_amdhsa_kernel", text, re.S)
    assert m
    return m.group(0)


def test_kernels_spill_nothing_and_use_no_scratch(built):
    notes = subprocess.run([tool("llvm-readelf"), "--notes", str(built)], capture_output=True, text=True, check=True).stdout
    for kernel in ("k_valu_sweep", "k_valu_probe"):
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


def test_every_step_is_in_the_code_under_its_own_name(sweep):
    ops = set(re.findall(r"^\s+([a-z][a-z0-9_]+)", sweep, re.M))
    want = {f"{m}_e32" for m in E32} | set(PLAIN) | {"v_cndmask_b32_e64", "v_cvt_f32_fp8_sdwa", "v_cvt_f32_bf8_sdwa"}
    assert want <= ops, sorted(want - ops)
    for tt in (0x96, 0xE8, 0xF0, 0xCC, 0xAA, 0x1B, 0x2D, 0xCA):
        for width in (32, 16):
            assert re.search(rf"v_bitop3_b{width} [^\n]*bitop3:{tt:#x}\b", sweep), (width, hex(tt))
    for cvt in ("fp8", "bf8"):
        assert {int(n) for n in re.findall(rf"v_cvt_f32_{cvt}_sdwa [^\n]*src0_sel:BYTE_(\d)", sweep)} == {0, 1, 2, 3}
    assert re.search(r"v_fma_mix_f32 [^\n]*op_sel:\[0,1,0\] op_sel_hi:\[1,1,0\]", sweep)
    assert re.search(r"v_fma_mixlo_f16 [^\n]*op_sel:\[1,0,0\] op_sel_hi:\[1,1,1\]", sweep)


def test_division_and_square_root_are_the_correctly_rounded_expansions(sweep):
    ops = set(re.findall(r"^\s+([a-z][a-z0-9_]+)", sweep, re.M))
    assert set(EXPANSIONS) <= ops, sorted(set(EXPANSIONS) - ops)


def test_float_mode_is_the_one_the_table_is_computed_for(asm):
    for directive, value in ((".amdhsa_float_round_mode_32", 0), (".amdhsa_float_round_mode_16_64", 0),
                             (".amdhsa_float_denorm_mode_32", 3), (".amdhsa_float_denorm_mode_16_64", 3),
                             (".amdhsa_ieee_mode", 1)):
        m = re.search(rf"{re.escape(directive)}\s+(\d+)", asm)
        assert m and int(m.group(1)) == value, directive


def test_the_kernel_never_writes_the_mode_register(sweep):
    assert "s_setreg" not in sweep
    assert "s_denorm_mode" not in sweep and "s_round_mode" not in sweep


def test_the_record_is_written_with_vector_stores(sweep):
    assert len(re.findall(r"global_store_dwordx4", sweep)) == 8  # the 128-byte record
    ops = set(re.findall(r"^\s+([a-z][a-z0-9_]+)", sweep, re.M))
    assert "s_barrier" in ops  # the reduction: plain LDS stores and loads around a barrier
    assert {o for o in ops if o.startswith("ds_")} <= {"ds_write_b32", "ds_write2_b32", "ds_write2st64_b32", "ds_read_b32",
                                                       "ds_read2_b32", "ds_read2st64_b32"}
    assert any(o.startswith("ds_write") for o in ops) and any(o.startswith("ds_read") for o in ops)
