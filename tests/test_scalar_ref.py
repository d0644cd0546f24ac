"""tests/scalar_sweep_ref.py against answers worked by hand from the ISA's
definitions: at least one per instruction, and each rule the reference's
docstring states. No GPU and no library."""
import numpy as np
import pytest

import scalar_sweep_ref as ref

M32 = 0xFFFFFFFF
TOP = 0x80000000


def fn(name, nth=0):
    """The nth step of that name (the immediates of the *k forms are 0x7fff, 0x8000, 1, 0xffff in this order)."""
    return [s[4] for s in ref.STEPS if s[1] == name][nth]


def run(name, a0=0, a1=0, b0=0, b1=0, c=0, nth=0):
    return tuple(int(v) & M32 for v in fn(name, nth)(a0, a1, b0, b1, c))


# (name, keywords of run, the words it must return: result words low first, then SCC)
HAND = [
    ("s_add_u32", dict(a0=M32, b0=1), (0, 1)),
    ("s_add_u32", dict(a0=2, b0=3, c=1), (5, 0)),
    ("s_sub_u32", dict(a0=0, b0=1), (M32, 1)),
    ("s_sub_u32", dict(a0=5, b0=5), (0, 0)),
    ("s_add_i32", dict(a0=0x7FFFFFFF, b0=1), (TOP, 1)),  # signed overflow
    ("s_add_i32", dict(a0=M32, b0=1), (0, 0)),  # -1 + 1: a carry, no overflow
    ("s_sub_i32", dict(a0=TOP, b0=1), (0x7FFFFFFF, 1)),
    ("s_sub_i32", dict(a0=0, b0=1), (M32, 0)),
    ("s_addc_u32", dict(a0=M32, b0=0, c=1), (0, 1)),
    ("s_addc_u32", dict(a0=1, b0=2, c=0), (3, 0)),
    ("s_subb_u32", dict(a0=0, b0=0, c=1), (M32, 1)),
    ("s_subb_u32", dict(a0=3, b0=1, c=1), (1, 0)),
    ("s_min_i32", dict(a0=M32, b0=1), (M32, 1)),  # -1 < 1: the first operand
    ("s_min_i32", dict(a0=7, b0=7), (7, 0)),  # equal: the second
    ("s_min_u32", dict(a0=M32, b0=1), (1, 0)),
    ("s_max_i32", dict(a0=M32, b0=1), (1, 0)),
    ("s_max_u32", dict(a0=M32, b0=1), (M32, 1)),
    ("s_absdiff_i32", dict(a0=3, b0=10), (7, 1)),
    ("s_absdiff_i32", dict(a0=9, b0=9), (0, 0)),
    ("s_abs_i32", dict(a0=TOP), (TOP, 1)),  # no positive counterpart
    ("s_abs_i32", dict(a0=M32), (1, 1)),
    ("s_abs_i32", dict(a0=0, c=1), (0, 0)),
    ("s_mul_i32", dict(a0=0x10000, b0=0x10001, c=1), (0x10000, 1)),  # SCC kept
    ("s_mul_hi_u32", dict(a0=M32, b0=M32), (0xFFFFFFFE, 0)),
    ("s_mul_hi_i32", dict(a0=M32, b0=M32, c=1), (0, 1)),  # -1 x -1 = 1
    ("s_mul_hi_i32", dict(a0=TOP, b0=2), (M32, 0)),  # -2^32
    ("s_lshl1_add_u32", dict(a0=TOP, b0=0), (0, 1)),
    ("s_lshl2_add_u32", dict(a0=1, b0=3), (7, 0)),
    ("s_lshl3_add_u32", dict(a0=0x20000000, b0=5), (5, 1)),
    ("s_lshl4_add_u32", dict(a0=1, b0=M32), (15, 1)),
    ("s_addk_i32", dict(a0=0x7FFFFFFF, nth=2), (TOP, 1)),  # + 1
    ("s_addk_i32", dict(a0=5, nth=3), (4, 0)),  # + 0xffff = -1
    ("s_addk_i32", dict(a0=0, nth=1), (0xFFFF8000, 0)),  # + 0x8000 = -32768
    ("s_addk_i32", dict(a0=1, nth=0), (0x8000, 0)),
    ("s_mulk_i32", dict(a0=3, nth=3, c=1), (0xFFFFFFFD, 1)),
    ("s_mulk_i32", dict(a0=2, nth=0), (0xFFFE, 0)),
    ("s_and_b32", dict(a0=0xF0F0, b0=0x0FF0), (0x00F0, 1)),
    ("s_and_b32", dict(a0=0xF0, b0=0x0F, c=1), (0, 0)),
    ("s_and_b64", dict(a0=1, a1=TOP, b0=0, b1=TOP), (0, TOP, 1)),
    ("s_or_b32", dict(a0=0, b0=0, c=1), (0, 0)),
    ("s_or_b64", dict(a0=1, a1=0, b0=0, b1=2), (1, 2, 1)),
    ("s_xor_b32", dict(a0=0xFF, b0=0x0F), (0xF0, 1)),
    ("s_xor_b64", dict(a0=5, a1=6, b0=5, b1=6, c=1), (0, 0, 0)),
    ("s_andn2_b32", dict(a0=0xFF, b0=0x0F), (0xF0, 1)),
    ("s_andn2_b64", dict(a0=M32, a1=M32, b0=M32, b1=0), (0, M32, 1)),
    ("s_orn2_b32", dict(a0=0, b0=M32), (0, 0)),
    ("s_orn2_b64", dict(a0=0, a1=0, b0=0xFFFFFFF0, b1=M32), (0xF, 0, 1)),
    ("s_nand_b32", dict(a0=M32, b0=M32), (0, 0)),
    ("s_nand_b64", dict(a0=1, a1=0, b0=1, b1=0), (0xFFFFFFFE, M32, 1)),
    ("s_nor_b32", dict(a0=0, b0=0xFFFF0000), (0xFFFF, 1)),
    ("s_nor_b64", dict(a0=M32, a1=0, b0=0, b1=M32), (0, 0, 0)),
    ("s_xnor_b32", dict(a0=0xAAAAAAAA, b0=0x55555555), (0, 0)),
    ("s_xnor_b64", dict(a0=0, a1=0, b0=0, b1=1), (M32, 0xFFFFFFFE, 1)),
    ("s_not_b32", dict(a0=M32, c=1), (0, 0)),
    ("s_not_b64", dict(a0=0, a1=M32), (M32, 0, 1)),
    ("s_lshl_b32", dict(a0=1, b0=32), (1, 1)),  # the count takes 5 bits
    ("s_lshl_b32", dict(a0=1, b0=63), (TOP, 1)),
    ("s_lshl_b32", dict(a0=TOP, b0=1), (0, 0)),
    ("s_lshr_b32", dict(a0=TOP, b0=31), (1, 1)),
    ("s_lshr_b32", dict(a0=TOP, b0=0x100), (TOP, 1)),
    ("s_ashr_i32", dict(a0=TOP, b0=31), (M32, 1)),
    ("s_ashr_i32", dict(a0=0x40000000, b0=63), (0, 0)),
    ("s_lshl_b64", dict(a0=1, a1=0, b0=32), (0, 1, 1)),  # the count takes 6 bits
    ("s_lshl_b64", dict(a0=1, a1=0, b0=64), (1, 0, 1)),
    ("s_lshr_b64", dict(a0=0, a1=TOP, b0=63), (1, 0, 1)),
    ("s_ashr_i64", dict(a0=0, a1=TOP, b0=32), (TOP, M32, 1)),
    ("s_bfm_b32", dict(a0=4, b0=8, c=1), (0xF00, 1)),
    ("s_bfm_b32", dict(a0=32, b0=0), (0, 0)),  # width 32 takes 5 bits: 0
    ("s_bfm_b32", dict(a0=31, b0=1), (0xFFFFFFFE, 0)),
    ("s_bfm_b64", dict(a0=33, b0=31), (TOP, M32, 0)),
    ("s_bfm_b64", dict(a0=64, b0=0), (0, 0, 0)),
    ("s_bfe_u32", dict(a0=0xABCD1234, b0=0x00080004), (0x23, 1)),
    ("s_bfe_u32", dict(a0=M32, b0=0x00000004), (0, 0)),  # width 0
    ("s_bfe_u32", dict(a0=0xF0000000, b0=0x0020001C), (0xF, 1)),  # runs past the top
    ("s_bfe_u32", dict(a0=M32, b0=0x007F0020), (M32, 1)),  # offset 32 -> 0, width 127
    ("s_bfe_i32", dict(a0=0x000000F0, b0=0x00040004), (M32, 1)),  # 0b1111 signed: -1
    ("s_bfe_i32", dict(a0=0x00000070, b0=0x00040004), (7, 1)),
    ("s_bfe_i32", dict(a0=TOP, b0=0x0020001F), (M32, 1)),  # one bit left at the top: -1
    ("s_bfe_i32", dict(a0=TOP, b0=0x0000001F), (0, 0)),
    ("s_bfe_u64", dict(a0=0, a1=0xFF, b0=0x00080020), (0xFF, 0, 1)),
    ("s_bfe_u64", dict(a0=0, a1=TOP, b0=0x0040003F), (1, 0, 1)),  # past the top
    ("s_bfe_i64", dict(a0=0, a1=TOP, b0=0x0040003F), (M32, M32, 1)),
    ("s_bfe_i64", dict(a0=M32, a1=M32, b0=0x00000000), (0, 0, 0)),
    ("s_pack_ll_b32_b16", dict(a0=0x11112222, b0=0x33334444, c=1), (0x44442222, 1)),
    ("s_pack_lh_b32_b16", dict(a0=0x11112222, b0=0x33334444), (0x33332222, 0)),
    ("s_pack_hh_b32_b16", dict(a0=0x11112222, b0=0x33334444), (0x33331111, 0)),
    ("s_brev_b32", dict(a0=1, c=1), (TOP, 1)),
    ("s_brev_b32", dict(a0=0x0000FFFF), (0xFFFF0000, 0)),
    ("s_brev_b64", dict(a0=1, a1=0), (0, TOP, 0)),
    ("s_wqm_b32", dict(a0=0x00010200), (0x000F0F00, 1)),
    ("s_wqm_b32", dict(a0=0, c=1), (0, 0)),
    ("s_wqm_b64", dict(a0=TOP, a1=1), (0xF0000000, 0xF, 1)),
    ("s_quadmask_b32", dict(a0=0x00010200), (0b10100, 1)),
    ("s_quadmask_b32", dict(a0=M32), (0xFF, 1)),
    ("s_quadmask_b64", dict(a0=0, a1=TOP), (0x8000, 0, 1)),
    ("s_bcnt0_i32_b32", dict(a0=M32, c=1), (0, 0)),
    ("s_bcnt0_i32_b32", dict(a0=0xFF), (24, 1)),
    ("s_bcnt0_i32_b64", dict(a0=0, a1=0), (64, 1)),
    ("s_bcnt1_i32_b32", dict(a0=0xF0F0), (8, 1)),
    ("s_bcnt1_i32_b32", dict(a0=0, c=1), (0, 0)),
    ("s_bcnt1_i32_b64", dict(a0=M32, a1=1), (33, 1)),
    ("s_ff0_i32_b32", dict(a0=0x0000FFFF, c=1), (16, 1)),
    ("s_ff0_i32_b32", dict(a0=M32), (M32, 0)),  # no zero bit: -1
    ("s_ff0_i32_b64", dict(a0=M32, a1=1), (33, 0)),
    ("s_ff1_i32_b32", dict(a0=0), (M32, 0)),  # no set bit: -1
    ("s_ff1_i32_b32", dict(a0=TOP), (31, 0)),
    ("s_ff1_i32_b64", dict(a0=0, a1=4), (34, 0)),
    ("s_ff1_i32_b64", dict(a0=0, a1=0, c=1), (M32, 1)),
    ("s_flbit_i32_b32", dict(a0=0), (M32, 0)),
    ("s_flbit_i32_b32", dict(a0=1), (31, 0)),
    ("s_flbit_i32_b32", dict(a0=TOP), (0, 0)),
    ("s_flbit_i32_b64", dict(a0=1, a1=0), (63, 0)),
    ("s_flbit_i32_b64", dict(a0=0, a1=0), (M32, 0)),
    ("s_flbit_i32", dict(a0=0), (M32, 0)),
    ("s_flbit_i32", dict(a0=M32), (M32, 0)),
    ("s_flbit_i32", dict(a0=1), (31, 0)),
    ("s_flbit_i32", dict(a0=TOP), (1, 0)),
    ("s_flbit_i32", dict(a0=0xFFFF0000), (16, 0)),
    ("s_flbit_i32_i64", dict(a0=M32, a1=M32), (M32, 0)),
    ("s_flbit_i32_i64", dict(a0=0, a1=M32), (32, 0)),
    ("s_sext_i32_i8", dict(a0=0x1280), (0xFFFFFF80, 0)),
    ("s_sext_i32_i8", dict(a0=0xFF7F, c=1), (0x7F, 1)),
    ("s_sext_i32_i16", dict(a0=0x12348000), (0xFFFF8000, 0)),
    ("s_bitset0_b32", dict(a0=35, b0=M32), (0xFFFFFFF7, 0)),  # bit 35 & 31 = 3
    ("s_bitset0_b64", dict(a0=35, b0=M32, b1=M32), (M32, 0xFFFFFFF7, 0)),
    ("s_bitset1_b32", dict(a0=31, b0=0, c=1), (TOP, 1)),
    ("s_bitset1_b64", dict(a0=64, b0=0, b1=0), (1, 0, 0)),  # bit 64 & 63 = 0
    ("s_bitreplicate_b64_b32", dict(a0=0x80000005), (0x33, 0xC0000000, 0)),
    ("s_cmp_eq_i32", dict(a0=5, b0=5), (1,)),
    ("s_cmp_eq_u32", dict(a0=5, b0=6), (0,)),
    ("s_cmp_lg_i32", dict(a0=5, b0=6), (1,)),
    ("s_cmp_lg_u32", dict(a0=5, b0=5), (0,)),
    ("s_cmp_gt_i32", dict(a0=1, b0=M32), (1,)),  # 1 > -1
    ("s_cmp_gt_u32", dict(a0=1, b0=M32), (0,)),
    ("s_cmp_ge_i32", dict(a0=TOP, b0=TOP), (1,)),
    ("s_cmp_ge_u32", dict(a0=0, b0=1), (0,)),
    ("s_cmp_lt_i32", dict(a0=TOP, b0=0), (1,)),
    ("s_cmp_lt_u32", dict(a0=TOP, b0=0), (0,)),
    ("s_cmp_le_i32", dict(a0=0x7FFFFFFF, b0=TOP), (0,)),
    ("s_cmp_le_u32", dict(a0=0x7FFFFFFF, b0=TOP), (1,)),
    ("s_cmp_eq_u64", dict(a0=1, a1=2, b0=1, b1=2), (1,)),
    ("s_cmp_eq_u64", dict(a0=1, a1=2, b0=1, b1=3), (0,)),
    ("s_cmp_lg_u64", dict(a0=1, a1=2, b0=1, b1=3), (1,)),
    ("s_cmpk_eq_i32", dict(a0=M32, nth=3), (1,)),  # 0xffff is -1
    ("s_cmpk_eq_u32", dict(a0=M32, nth=3), (0,)),  # 0xffff is 65535
    ("s_cmpk_eq_u32", dict(a0=0xFFFF, nth=3), (1,)),
    ("s_cmpk_lg_i32", dict(a0=0x7FFF, nth=0), (0,)),
    ("s_cmpk_lg_u32", dict(a0=0x8000, nth=1), (0,)),
    ("s_cmpk_gt_i32", dict(a0=0, nth=1), (1,)),  # 0 > -32768
    ("s_cmpk_gt_u32", dict(a0=0, nth=1), (0,)),
    ("s_cmpk_ge_i32", dict(a0=1, nth=2), (1,)),
    ("s_cmpk_ge_u32", dict(a0=0, nth=2), (0,)),
    ("s_cmpk_lt_i32", dict(a0=M32, nth=2), (1,)),
    ("s_cmpk_lt_u32", dict(a0=M32, nth=2), (0,)),
    ("s_cmpk_le_i32", dict(a0=0xFFFF8000, nth=1), (1,)),
    ("s_cmpk_le_u32", dict(a0=0xFFFF8000, nth=1), (0,)),
    ("s_bitcmp0_b32", dict(a0=0xFFFFFFFE, b0=32), (1,)),  # bit 0
    ("s_bitcmp0_b64", dict(a0=0, a1=1, b0=32), (0,)),
    ("s_bitcmp1_b32", dict(a0=TOP, b0=63), (1,)),  # bit 31
    ("s_bitcmp1_b64", dict(a0=TOP, a1=0, b0=63), (0,)),
    ("s_cselect_b32", dict(a0=1, b0=2, c=1), (1, 1)),
    ("s_cselect_b32", dict(a0=1, b0=2, c=0), (2, 0)),
    ("s_cselect_b64", dict(a0=1, a1=2, b0=3, b1=4, c=0), (3, 4, 0)),
    ("s_cmov_b32", dict(a0=9, b0=2, c=1), (9, 1)),
    ("s_cmov_b32", dict(a0=9, b0=2, c=0), (2, 0)),
    ("s_cmov_b64", dict(a0=1, a1=2, b0=3, b1=4, c=1), (1, 2, 1)),
    ("s_movk_i32", dict(nth=1, c=1), (0xFFFF8000, 1)),
    ("s_movk_i32", dict(nth=0), (0x7FFF, 0)),
    ("s_cmovk_i32", dict(b0=7, nth=3, c=1), (M32, 1)),
    ("s_cmovk_i32", dict(b0=7, nth=3, c=0), (7, 0)),
    ("s_mov_b32", dict(nth=0), (0xFFFFFFF0, 0)),
    ("s_mov_b32", dict(nth=1), (64, 0)),
    ("s_mov_b32", dict(nth=2, c=1), (0x3F800000, 1)),
    ("s_mov_b32", dict(nth=3), (0x3F000000, 0)),
    ("s_mov_b32", dict(nth=4), (0x12345678, 0)),
    ("s_cbranch_scc0", dict(c=0), (1, 0)),
    ("s_cbranch_scc0", dict(c=1), (2, 1)),
    ("s_cbranch_scc1", dict(c=1), (1, 1)),
    ("s_cbranch_scc1", dict(c=0), (2, 0)),
    ("s_cbranch_vccz", dict(a0=5, c=0), (1, 0)),  # VCC is 0 without c
    ("s_cbranch_vccz", dict(a0=5, c=1), (2, 1)),
    ("s_cbranch_vccz", dict(a0=0, a1=0, c=1), (1, 1)),
    ("s_cbranch_vccnz", dict(a0=0, a1=1, c=1), (1, 1)),
    ("s_cbranch_vccnz", dict(a0=0, a1=1, c=0), (2, 0)),
    ("s_cbranch_execz", dict(a0=0, a1=0, c=1), (1, 1)),
    ("s_cbranch_execz", dict(a0=1, c=1), (2, 1)),
    ("s_cbranch_execnz", dict(a0=1, c=1), (1, 1)),
    ("s_cbranch_execnz", dict(a0=1, c=0), (2, 0)),
    # mask steps: a is the operand, b the EXEC before; D (2), the active lanes (2), SCC, first active lane
    ("s_and_saveexec_b64", dict(a0=0xF0, b0=0x3C), (0x3C, 0, 0x30, 0, 1, 4)),
    ("s_and_saveexec_b64", dict(a0=0xF0, b0=0x0F), (0x0F, 0, 0, 0, 0, 0)),  # an empty mask: lane 0
    ("s_or_saveexec_b64", dict(a0=0, a1=TOP, b0=0, b1=0), (0, 0, 0, TOP, 1, 63)),
    ("s_xor_saveexec_b64", dict(a0=6, b0=3), (3, 0, 5, 0, 1, 0)),
    ("s_andn2_saveexec_b64", dict(a0=0xFF, b0=0x0F), (0x0F, 0, 0xF0, 0, 1, 4)),
    ("s_orn2_saveexec_b64", dict(a0=0, b0=M32, b1=M32), (M32, M32, 0, 0, 0, 0)),
    ("s_nand_saveexec_b64", dict(a0=M32, a1=M32, b0=M32, b1=M32), (M32, M32, 0, 0, 0, 0)),
    ("s_nor_saveexec_b64", dict(a0=M32, a1=0, b0=0, b1=0x7FFFFFFF), (0, 0x7FFFFFFF, 0, TOP, 1, 63)),
    ("s_xnor_saveexec_b64", dict(a0=0, a1=0, b0=M32, b1=M32), (M32, M32, 0, 0, 0, 0)),
    ("s_andn1_saveexec_b64", dict(a0=0x0F, b0=0xFF), (0xFF, 0, 0xF0, 0, 1, 4)),
    ("s_orn1_saveexec_b64", dict(a0=M32, a1=M32, b0=2), (2, 0, 2, 0, 1, 1)),
    ("s_andn1_wrexec_b64", dict(a0=0x0F, b0=0xFF), (0xF0, 0, 0xF0, 0, 1, 4)),  # D is the new EXEC
    ("s_andn2_wrexec_b64", dict(a0=0xFF, b0=0x0F), (0xF0, 0, 0xF0, 0, 1, 4)),
    ("v_cmp_lt_u32_e64", dict(a0=1, b0=M32), (1,)),
    ("v_cmp_lt_u32_e32", dict(a0=M32, b0=1), (0,)),
    ("v_cmp_eq_u32_e64", dict(a0=3, b0=3), (1,)),
    ("v_cmp_le_u32_e32", dict(a0=3, b0=3), (1,)),
    ("v_cmp_gt_u32_e64", dict(a0=TOP, b0=1), (1,)),
    ("v_cmp_ne_u32_e32", dict(a0=3, b0=3), (0,)),
    ("v_cmp_ge_u32_e64", dict(a0=0, b0=1), (0,)),
    ("v_cmp_eq_u32_e32", dict(a0=3, b0=4), (0,)),
    ("v_cmp_le_u32_e64", dict(a0=4, b0=3), (0,)),
    ("v_cmp_gt_u32_e32", dict(a0=1, b0=TOP), (0,)),
    ("v_cmp_ne_u32_e64", dict(a0=3, b0=4), (1,)),
    ("v_cmp_ge_u32_e32", dict(a0=1, b0=1), (1,)),
    ("v_addc_co_u32", dict(a0=M32, a1=M32, b0=1, b1=0), (0, 0, 1)),
    ("v_addc_co_u32", dict(a0=M32, a1=0, b0=1, b1=0), (0, 1, 0)),
]


@pytest.mark.parametrize("name,kw,want", HAND, ids=[f"{i}-{h[0]}" for i, h in enumerate(HAND)])
def test_the_reference_against_hand_worked_answers(name, kw, want):
    assert run(name, **kw) == tuple(w & M32 for w in want)


def test_every_instruction_has_a_hand_worked_answer():
    assert {s[1] for s in ref.STEPS} - {"add128", "sub128"} == {h[0] for h in HAND}


def test_the_carry_chain_is_128_bit_arithmetic():
    rng = np.random.default_rng(7)
    cases = [(M32, M32, M32, M32), (0, 0, 0, 0), (M32, 0, 1, 0), (0, 0, 1, 0)]
    cases += [tuple(int(v) for v in rng.integers(0, 1 << 32, 4)) for _ in range(200)]
    for a0, a1, b0, b1 in cases:
        x = a0 | a1 << 32 | b0 << 64 | b1 << 96
        y = b0 | b1 << 32 | a0 << 64 | a1 << 96
        got = run("add128", a0, a1, b0, b1, 1)
        assert sum(w << (32 * i) for i, w in enumerate(got[:4])) == (x + y) % (1 << 128) and got[4] == (x + y) >> 128
        got = run("sub128", a0, a1, b0, b1, 0)
        assert sum(w << (32 * i) for i, w in enumerate(got[:4])) == (x - y) % (1 << 128) and got[4] == int(x < y)
    # One word at a time, as s_add_u32 / s_addc_u32 x 3 do it.
    a0, a1, b0, b1 = M32, M32, 1, 0
    carry, out = 0, []
    for u, v in ((a0, b0), (a1, b1), (b0, a0), (b1, a1)):
        out.append((u + v + carry) & M32)
        carry = (u + v + carry) >> 32
    assert run("add128", a0, a1, b0, b1) == tuple(out) + (carry,)


def test_two_seeds_give_different_operands():
    a, b = (ref.operands(s, 0, 0, "val") for s in ref.SEEDS)
    hashed = [t for t in range(ref.BLOCK) if t % 64 >= 16]
    assert all(a[t][:4] != b[t][:4] for t in hashed)
    assert ref.SEEDS[0] != ref.SEEDS[1] and len(ref.SEEDS) == 2
    # and every step and wave its own
    assert ref.operands(ref.SEEDS[0], 0, 1, "val")[20] != a[20] and a[20] != a[64 + 20]


def test_lanes_0_to_15_are_the_edge_crossing():
    for kind, table in ref.KIND.items():
        ops = ref.operands(ref.SEEDS[0], 1, 3, kind)
        seen = set()
        for t in range(ref.BLOCK):
            w, l = divmod(t, 64)
            if l < 16:
                k = 16 * w + l
                a0, a1, b0, b1, _ = ops[t]
                assert (a0, b0, a1, b1) == (ref.EDGE[k % 5], table[k // 5 % 5], ref.EDGE[k // 25 % 5], ref.EDGE[k // 125])
                seen.add((a0, b0))
        assert seen == {(a, b) for a in ref.EDGE for b in table}  # all 25 pairs over the sixteen waves
    assert ref.EDGE == (0, 1, M32, TOP, 0x7FFFFFFF) and ref.EDGE_SHIFT[:4] == (0, 31, 32, 63)
    assert ref.EDGE_FIELD[0] >> 16 == 0 and (ref.EDGE_FIELD[1] & 31) + (ref.EDGE_FIELD[1] >> 16) > 32


def test_shapes_and_layout():
    assert ref.PARTS == ["arith", "logic", "bits", "cmp", "branch", "mask", "movrel", "sgpr"]
    for part in ref.PARTS:
        e = ref.expected(part, ref.SEEDS[0])
        assert e.dtype == np.uint32 and e.shape == (ref.SHAPES[part][1], ref.BLOCK)
        assert ref.digest(part, ref.SEEDS[0]) != ref.digest(part, ref.SEEDS[1])
    # movrel: the _b64 forms use the even indexes; movreld leaves the neighbours as they were
    assert [len(ref.movrel_indexes(f)) for f in range(4)] == [16, 8, 16, 8]
    rows = ref.movrel_words(ref.SEEDS[0], 2)
    block = [ref.hashv(ref.SEEDS[0], 6, 2, j) for j in range(16)]
    src = ref.hashv(ref.SEEDS[0], 6, 2, 16)
    assert rows[0] == src and rows[1] == block[1] and rows[2] == block[15]
    # sgpr: every register s0..s99 and VCC in exactly one phase, both polarities, 0 elsewhere
    assert sorted(ref.SGPR_PHASES[0] + ref.SGPR_PHASES[1]) == list(range(100)) + [106, 107]
    e = ref.expected("sgpr", ref.SEEDS[0])
    assert (e[0] ^ e[2])[52:64].tolist() == [M32] * 12 and not e[0][:52].any() and not e[2][:52].any()
    assert (e[4] ^ e[5])[:52].tolist() == [M32] * 52 and not e[4][52:64].any()
    assert (e[1] ^ e[3])[[0, 35, 42, 43]].tolist() == [M32] * 4 and not e[1][36:42].any() and not e[1][44:64].any()
