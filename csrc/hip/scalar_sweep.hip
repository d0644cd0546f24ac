// Scalar sweep for gfx950 (MI355X): the scalar ALU and the SGPR file of every CU.
//
// Every other sweep leans on the scalar unit for its addresses, loop counters,
// EXEC masks and branches, and none tests it. k_scalar_sweep is a sweep over
// named parts (part_sweep.h) that issues the scalar instructions of gfx950
// each under its own mnemonic, compares bit for bit, and writes and reads
// back every SGPR a wave can name.
//
// Workgroup: 1,024 threads = sixteen waves, four on each SIMD, resident
// together. The reduction takes (2 x 8 + 2 + 8) x 1,024 words = 104 KiB of LDS,
// more than half a CU's, so no two workgroups share a CU; the kernel is
// compiled to the largest SGPR allocation a wave can have (it names s0..s99
// and VCC; s100 and s101 are beyond what the compiler gives a function and
// stay untouched), so across the barrier of the `sgpr` part four disjoint allocations
// of each SIMD's SGPR file hold patterns at the same time.
//
// Parts (bit, name):
//   0 arith   1 logic   2 bits   3 cmp   4 branch   5 mask   6 movrel   7 sgpr
//
// How a scalar result is checked. A scalar instruction gives one result per
// wave, so a wave runs every step 64 times, once per operand set. Lane i
// hashes operand set i on the VALU; v_readlane_b32 with the iteration number
// as lane select brings set i to s40..s44; the instruction under test runs in
// the same asm statement; s_cselect_b32 s50, 1, 0 captures the SCC it left;
// v_writelane_b32 (lane select in M0, saved and restored in the statement)
// puts result and SCC back into lane i. After the 64 iterations every lane
// holds the result of its own operands and computes in integer C++ what it
// must have received; both enter take_word. SCC-in is set from operand c by
// s_cmp_lg_u32 s44, 0 in the same statement, for every step; a step whose
// instruction does not write SCC must return c.
//
// Operands. h(p, s, w, o, l) = fmix32(seed ^ (p << 28 | s << 20 | w << 14 |
// o << 8 | l)), p = part, s = step within the part, w = wave 0..15, l = lane,
// o = operand: 0 a0, 1 a1, 2 b0, 3 b1, 4 c (c = h & 1). a = a1:a0 and b = b1:b0
// are the 64-bit operands. Lanes 0..15 of every wave are edge lanes: with
// k = 16 w + l and E = {0, 1, 0xffffffff, 0x80000000, 0x7fffffff},
//   a0 = E[k % 5], a1 = E[k / 25 % 5], b1 = E[k / 125],
//   b0 = E[k / 5 % 5]                                          (kind VAL)
//        {0, 31, 32, 63, 1}[k / 5 % 5]                         (kind SH: shift counts, bit numbers)
//        {0x00000000, 0x0020001f, 0x00400000, 0x007f0020, 0x0001001f}[k / 5 % 5]
//                       (kind BFE: width 0, a field past the top, widths 64 and 127, one bit at 31)
// so over the sixteen waves the edges cross. c is always hashed.
//
// Rules the expectations are written from (GFX9 / CDNA ISA):
//   s_add_u32 / s_addc_u32: SCC = carry out; s_sub_u32 / s_subb_u32: SCC = borrow;
//   s_add_i32 / s_sub_i32 / s_addk_i32: SCC = signed overflow;
//   s_min / s_max: SCC = 1 when the first operand is chosen (strictly less / greater);
//   s_absdiff_i32: D = a - b in 32 bits, negated when negative; SCC = D != 0;
//   s_abs_i32: 0x80000000 stays 0x80000000; SCC = D != 0;
//   s_mul_i32, s_mul_hi_*, s_mulk_i32: SCC unchanged;
//   s_lshlN_add_u32: SCC = carry of the 64-bit sum (a << N) + b;
//   the logic forms, shifts, s_bfe, s_wqm, s_quadmask, s_bcnt, s_not, s_abs: SCC = D != 0;
//   shift counts and bit numbers take 5 bits (32-bit forms) or 6 bits (64-bit forms);
//   s_bfm: ((1 << a[4:0]) - 1) << b[4:0] (6 bits each for _b64); SCC unchanged;
//   s_bfe: offset b[4:0] (b[5:0] for 64), width b[22:16]; width 0 gives 0; a field that runs
//     past the top ends at the top; the signed forms extend from the field's last bit;
//   s_ff0 / s_ff1 / s_flbit: -1 when there is no such bit; s_flbit_i32 (signed) counts the
//     bits equal to the sign from the top, -1 for 0 and -1;
//   s_wqm: a quad with any bit set becomes all ones; s_quadmask: bit q = any bit of quad q;
//   s_bitset0 / s_bitset1: bit a[4:0] (a[5:0]) of the destination, the rest kept;
//   s_cmp*, s_cmpk* (i32 forms sign-extend the immediate, u32 forms zero-extend), s_bitcmp*: SCC only;
//   s_cselect, s_cmov, s_cmovk: by SCC-in, SCC unchanged; s_movk sign-extends;
//   branches: taken leaves 1, fall-through 2; each jumps forward over one s_mov_b32;
//   s_*_saveexec_b64 D, S: D = EXEC, EXEC = S op EXEC (andn1: ~S & EXEC, orn1: ~S | EXEC,
//     andn2: S & ~EXEC, orn2: S | ~EXEC), SCC = EXEC != 0; s_andn1/2_wrexec_b64: D = new EXEC too;
//   v_readfirstlane_b32 under an all-zero EXEC reads lane 0;
//   s_movrels: D = SGPR[S + M0]; s_movreld: SGPR[D + M0] = S.
//
// The `branch` part: s_cbranch_scc0/scc1/vccz/vccnz/execz/execnz, each taken
// or not by operand c. There is no backward branch in any asm statement here.
// The `mask` part: EXEC is set to b, the instruction runs on a, then a
// v_mov_b32 under the new mask marks the active lanes in a register zeroed
// under full EXEC and v_readfirstlane_b32 reads the lane number of the first;
// EXEC is restored and v_cmp_ne_u32 makes the marks a mask. Words: D, the
// active lanes, SCC, first lane. Its lane steps (no loop) are the VALU's side
// of the SGPR interface: v_cmp_*_u32 into an SGPR pair and into VCC with a
// v_cndmask_b32 reading it, and v_add_co_u32 / v_addc_co_u32 through a pair.
// The `movrel` part: s56..s71 take lanes 0..15 of sixteen hashed registers
// (key: step = the form 0..3, o = register; o = 16, 17 the source of movreld);
// one statement per index 0..15 (the even ones for _b64, whose M0 must be
// even), a constant of the statement, names and clobbers the block. movrels returns the word(s) read;
// movreld returns the cell(s) written and a neighbour on either side (_b32)
// or the one behind (_b64), which must be unchanged.
// The `sgpr` part: pattern p(N) = h(7, phase, w, N / 64, N % 64) for register
// N, computed per lane (lane = N % 64) on the VALU. One asm statement per
// phase writes every register of the phase with v_readlane_b32 sN, v, N, waits
// at an s_barrier that all sixteen waves reach, reads them back with
// v_writelane_b32 v, sN, N, then does the same with ~p. No scalar ALU
// instruction lies in a cell's path. Phase 0 holds s52..s99 and VCC (as
// registers 106, 107); phase 1, with the clobber sets exchanged, s0..s51.
// Words: phase 0 p low, p high, ~p low, ~p high; phase 1 p, ~p. A lane with no
// register keeps 0. Phase 1 writes s32 too, which the compiler keeps for a
// stack pointer and warns about: this kernel has no stack and no call.
//
// Wait states. Nothing inside an asm string is padded by the compiler, so the
// strings carry their own: s_nop 3 before a v_readlane_b32 / v_writelane_b32
// whose lane select (an SGPR or M0) may have been written by the VALU or was
// just written; s_nop 1 after an M0 write before s_movrel*; s_nop 1 between a
// VALU write of an SGPR pair or VCC (v_cmp, v_add_co, v_addc_co) and the VALU
// instruction that reads it as mask or carry (v_cndmask, v_addc_co); s_nop 0
// opening the `sgpr` statements, whose first v_readlane_b32 reads a VGPR that
// the VALU has just written.
//
// Every statement that writes EXEC or M0 restores it; between an EXEC write
// and its restore there is only SALU, v_mov_b32 and v_readfirstlane_b32. The
// kernel never writes the MODE register, has no scratch and no spill, and its
// only scalar memory instructions are the compiler's kernarg loads. Results
// leave the scalar unit through v_writelane_b32 / v_mov_b32 and vector stores.
//
// Record (128 bytes per workgroup): part_sweep.h's head with eight parts, a
// reserved word, and per SIMD two words of HW_REG_GPR_ALLOC as its waves read
// it: the OR of the raw words and the OR of their complements (a bit set in
// both differed between the waves). A probe's dump ends in two rows that are
// not compared: the raw HW_REG_GPR_ALLOC and HW_REG_HW_ID of every thread.
//
// Which SGPR rows were reached is NOT published. The layout assumed for
// HW_REG_GPR_ALLOC (SGPR_BASE in bits 21:16 and SGPR_SIZE in bits 27:24, both
// in units of 16 registers) does not hold on the MI355X: the four waves of a
// SIMD in one workgroup read 0x060060c0, 0x062060c4, 0x064060c8, 0x066060cc
// on every SIMD, and bits 21:16 of those overlap. Bits 27:24 are 6, which is
// the code object's 112 registers as blocks of 16 less one; bits 23:16 step by
// 0x20 per wave, which a unit of four registers would make a stride of 128.
// No document at hand confirms that unit, so no figure is derived from it.
// The sweep claims only this: the registers a wave can name, in the four
// allocations per SIMD that its waves held at the same time.
//
// The expected words of host and lanes come from one table (SCALAR_STEPS and
// the want_* functions below, as valu_sweep.hip's do); the independent
// reference is tests/scalar_sweep_ref.py.
//
// Injection: as in the other part sweeps (thread 0, word 0 of each injected
// part, registers only). blocks == 0 means 4 per CU.
//
// NOT covered: SGPR rows outside the allocations reached, s100 and s101, the
// trap-handler registers, s_setreg and the MODE / STATUS registers, s_getpc / s_swappc /
// s_call, s_set_gpr_idx_* and v_movrel*, s_memtime / s_memrealtime,
// s_sendmsg, the instruction cache, backward branches, scalar floating point
// (gfx950 has none).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <mutex>
#include <utility>

#include "hip/part_sweep.h"

#define XS_ERR_BUF g_scalar_err
#define XS_HD __host__ __device__ __forceinline__
#define XS_D __device__ __forceinline__

namespace {

xsprobe::ErrBuf g_scalar_err;

using namespace xsprobe;

constexpr int kNumParts = 8;
const char kPartNames[] = "arith,logic,bits,cmp,branch,mask,movrel,sgpr";
constexpr uint32_t kAllParts = (1u << kNumParts) - 1;
constexpr int kBlock = 1024;  // 16 waves: four per SIMD
constexpr int kMask = 5, kMovrel = 6, kSgpr = 7;
constexpr int kCoverWords = 8;

enum BKind : int { VAL, SH, BFE };
enum Cls : int { G, M, L };  // looped generic step, looped mask step, lane step

// ------------------------------------------------------------------ operands
XS_HD uint32_t hashv(uint32_t seed, uint32_t p, uint32_t s, uint32_t w, uint32_t o, uint32_t l) {
  return fmix32(seed ^ (p << 28 | s << 20 | w << 14 | o << 8 | l));
}
// Branch-free: a lane's class must not become the kernel's control flow.
XS_HD uint32_t pick5(uint32_t k, uint32_t v1, uint32_t v2, uint32_t v3, uint32_t v4) {  // v0 = 0
  return ((0u - (k == 1)) & v1) | ((0u - (k == 2)) & v2) | ((0u - (k == 3)) & v3) | ((0u - (k == 4)) & v4);
}
XS_HD uint32_t edge(uint32_t k) { return pick5(k, 1u, 0xffffffffu, 0x80000000u, 0x7fffffffu); }
XS_HD uint32_t edge_shift(uint32_t k) { return pick5(k, 31u, 32u, 63u, 1u); }
XS_HD uint32_t edge_field(uint32_t k) { return pick5(k, 0x0020001fu, 0x00400000u, 0x007f0020u, 0x0001001fu); }

struct Ops {
  uint32_t a0, a1, b0, b1, c;
};
XS_HD Ops operands(uint32_t seed, uint32_t p, uint32_t s, int bk, uint32_t t) {
  const uint32_t w = t >> 6, l = t & 63u;
  Ops o{hashv(seed, p, s, w, 0, l), hashv(seed, p, s, w, 1, l), hashv(seed, p, s, w, 2, l), hashv(seed, p, s, w, 3, l),
        hashv(seed, p, s, w, 4, l) & 1u};
  const uint32_t k = (16 * w + l) & 255u, kb = k / 5 % 5, m = 0u - (l < 16);
  o.a0 = (edge(k % 5) & m) | (o.a0 & ~m);
  o.b0 = ((bk == VAL ? edge(kb) : bk == SH ? edge_shift(kb) : edge_field(kb)) & m) | (o.b0 & ~m);
  o.a1 = (edge(k / 25 % 5) & m) | (o.a1 & ~m);
  o.b1 = (edge(k / 125) & m) | (o.b1 & ~m);
  return o;
}

// ------------------------------------------------------- what a step returns
struct Res {
  uint64_t d = 0, e = 0;  // words 0, 1 and words 2, 3
  uint32_t scc = 0, first = 0;
};
XS_HD uint32_t sx16(uint32_t v) { return static_cast<uint32_t>(static_cast<int32_t>(static_cast<int16_t>(v))); }
XS_HD uint32_t add_ov(uint32_t a, uint32_t b) { return (~(a ^ b) & (a ^ (a + b))) >> 31; }
XS_HD uint32_t sub_ov(uint32_t a, uint32_t b) { return ((a ^ b) & (a ^ (a - b))) >> 31; }
XS_HD uint32_t carry(uint32_t a, uint32_t b, uint32_t c) { return static_cast<uint32_t>((uint64_t{a} + b + c) >> 32); }
XS_HD uint32_t borrow(uint32_t a, uint32_t b, uint32_t c) { return uint64_t{b} + c > a; }
XS_HD int32_t i32(uint32_t v) { return static_cast<int32_t>(v); }
XS_HD int64_t i64(uint64_t v) { return static_cast<int64_t>(v); }
XS_HD uint64_t ones(uint32_t n) { return n >= 64 ? ~0ull : (1ull << n) - 1; }
XS_HD uint64_t bfe(uint64_t a, uint32_t off, uint32_t width, uint32_t bits, bool sign) {
  const uint32_t w = width < bits - off ? width : bits - off;  // the field ends at the top
  if (w == 0) return 0;
  uint64_t v = (a >> off) & ones(w);
  if (sign && ((v >> (w - 1)) & 1u)) v |= ~ones(w);
  return v & ones(bits);
}
XS_HD uint64_t brev(uint64_t a, int bits) { return __builtin_bitreverse64(a) >> (64 - bits); }
XS_HD uint64_t any_of_quad(uint64_t a) {  // bit 4q = any bit of quad q
  a |= a >> 1;
  a |= a >> 2;
  return a & 0x1111111111111111ull;
}
XS_HD uint64_t wqm(uint64_t a, int bits) { return (any_of_quad(a) * 0xfull) & ones(bits); }
XS_HD uint64_t quadmask(uint64_t a, int bits) {
  const uint64_t x = any_of_quad(a);
  uint64_t r = 0;
#pragma unroll
  for (int q = 0; q < 16; ++q) r |= ((x >> (4 * q)) & 1u) << q;
  return r & ones(bits / 4);
}
XS_HD uint32_t bcnt1(uint64_t a) { return static_cast<uint32_t>(__builtin_popcountll(a)); }
XS_HD uint32_t ff1(uint64_t a, int bits) {  // lowest set bit, -1 if none
  a &= ones(bits);
  return a ? static_cast<uint32_t>(__builtin_ctzll(a | 1ull << 63)) : 0xffffffffu;
}
XS_HD uint32_t flbit(uint64_t a, int bits) {  // zeros above the highest set bit, -1 if none
  a = (a & ones(bits)) << (64 - bits);
  return a ? static_cast<uint32_t>(__builtin_clzll(a | 1u)) : 0xffffffffu;
}
XS_HD uint32_t flbit_signed(uint64_t a, int bits) {  // bits equal to the sign from the top, -1 if all
  const uint64_t sign = 0ull - ((a >> (bits - 1)) & 1u);
  return flbit(a ^ sign, bits);
}
XS_HD uint64_t bitrep(uint32_t a) {  // every bit twice
  uint64_t x = a;
  x = (x | x << 16) & 0x0000ffff0000ffffull;
  x = (x | x << 8) & 0x00ff00ff00ff00ffull;
  x = (x | x << 4) & 0x0f0f0f0f0f0f0f0full;
  x = (x | x << 2) & 0x3333333333333333ull;
  x = (x | x << 1) & 0x5555555555555555ull;
  return x | x << 1;
}
XS_HD uint32_t mul_hi_u(uint32_t a, uint32_t b) { return static_cast<uint32_t>((uint64_t{a} * b) >> 32); }
XS_HD uint32_t mul_hi_i(uint32_t a, uint32_t b) {
  return static_cast<uint32_t>(static_cast<uint64_t>(int64_t{i32(a)} * int64_t{i32(b)}) >> 32);
}
// a1:a0:... the 128-bit operands of the carry chain: X = {a0, a1, b0, b1}, Y = {b0, b1, a0, a1}.
XS_HD void chain128(const Ops& o, bool sub, Res& r) {
  const uint32_t x[4] = {o.a0, o.a1, o.b0, o.b1}, y[4] = {o.b0, o.b1, o.a0, o.a1};
  uint32_t c = 0, w[4];
  for (int i = 0; i < 4; ++i) {
    w[i] = sub ? x[i] - y[i] - c : x[i] + y[i] + c;
    c = sub ? borrow(x[i], y[i], c) : carry(x[i], y[i], c);
  }
  r.d = uint64_t{w[1]} << 32 | w[0];
  r.e = uint64_t{w[3]} << 32 | w[2];
  r.scc = c;
}

// ---------------------------------------------------------- register names
// Fixed SGPRs of the looped statements, all clobbered: operands s40..s44,
// result s46..s49, SCC s50, M0 kept in s51, pairs s[52:53] s[54:55], EXEC
// kept in s[72:73]; the movrel block is s56..s71.
#define RA0 "s40"
#define RA1 "s41"
#define RA "s[40:41]"
#define RB0 "s42"
#define RB1 "s43"
#define RB "s[42:43]"
#define RD0 "s46"
#define RD1 "s47"
#define RD "s[46:47]"
#define RD2 "s48"
#define RD3 "s49"
#define XS_CLOBBER                                                                                                \
  "s40", "s41", "s42", "s43", "s44", "s45", "s46", "s47", "s48", "s49", "s50", "s51", "s52", "s53", "s54", "s55", \
      "s72", "s73", "vcc", "scc"

// Operand set i to SGPRs, result cleared, SCC-in from c. The s_nop covers a
// lane select that the compiler made with a VALU instruction.
#define XS_PRE                           \
  "s_nop 3\n"                            \
  "v_readlane_b32 s40, %[a0], %[i]\n"    \
  "v_readlane_b32 s41, %[a1], %[i]\n"    \
  "v_readlane_b32 s42, %[b0], %[i]\n"    \
  "v_readlane_b32 s43, %[b1], %[i]\n"    \
  "v_readlane_b32 s44, %[c], %[i]\n"     \
  "s_mov_b64 s[46:47], 0\n"              \
  "s_mov_b64 s[48:49], 0\n"              \
  "s_cmp_lg_u32 s44, 0\n"
// SCC out, then result words into lane i through M0.
#define XS_M0_ON             \
  "s_cselect_b32 s50, 1, 0\n" \
  "s_mov_b32 s51, m0\n"      \
  "s_mov_b32 m0, %[i]\n"     \
  "s_nop 3\n"
#define XS_M0_OFF "v_writelane_b32 %[sc], s50, m0\ns_mov_b32 m0, s51\n"
#define XS_W0 "v_writelane_b32 %[d0], s46, m0\n"
#define XS_W1 "v_writelane_b32 %[d1], s47, m0\n"
#define XS_W23 "v_writelane_b32 %[d2], s48, m0\nv_writelane_b32 %[d3], s49, m0\n"
#define XS_POST_0 XS_M0_ON XS_M0_OFF
#define XS_POST_1 XS_M0_ON XS_W0 XS_M0_OFF
#define XS_POST_2 XS_M0_ON XS_W0 XS_W1 XS_M0_OFF
#define XS_POST_4 XS_M0_ON XS_W0 XS_W1 XS_W23 XS_M0_OFF

// Branch: 1 when taken, 2 when not.
#define XS_BRANCH(INSN) "s_mov_b32 s46, 1\n" INSN " 1f\ns_mov_b32 s46, 2\n1:\n"
#define XS_EXEC_IS(SET) "s_mov_b64 s[72:73], exec\ns_mov_b64 exec, 0\n" SET
#define XS_EXEC_BACK "s_mov_b64 exec, s[72:73]"

// ------------------------------------------------------------------ the table
// X(part, class, id, name, result words, kind of b0, device text, expectation)
// The expectation sees o (Ops), a0 a1 b0 b1 c, a and b (64 bit) and fills r;
// r.scc starts as c.
#define NZ r.scc = r.d != 0
#define LOGIC2(X, ID, N32, N64, E32, E64)                                                       \
  X(1, G, ID##_b32, N32, 1, VAL, N32 " " RD0 ", " RA0 ", " RB0, r.d = uint32_t(E32); NZ)         \
  X(1, G, ID##_b64, N64, 2, VAL, N64 " " RD ", " RA ", " RB, r.d = (E64); NZ)
#define ADDK(X, ID, IMM)                                                                                          \
  X(0, G, addk_##ID, "s_addk_i32", 1, VAL, "s_mov_b32 s46, s40\ns_addk_i32 s46, " #IMM,                           \
    r.d = a0 + sx16(IMM); r.scc = add_ov(a0, sx16(IMM)))                                                          \
  X(0, G, mulk_##ID, "s_mulk_i32", 1, VAL, "s_mov_b32 s46, s40\ns_mulk_i32 s46, " #IMM, r.d = a0 * sx16(IMM))
#define CMP2(X, OP, EXPR_I, EXPR_U)                                                                  \
  X(3, G, cmp_##OP##_i32, "s_cmp_" #OP "_i32", 0, VAL, "s_cmp_" #OP "_i32 s40, s42", {              \
    const int32_t x = i32(a0), y = i32(b0);                                                          \
    r.scc = (EXPR_I);                                                                                \
  })                                                                                                 \
  X(3, G, cmp_##OP##_u32, "s_cmp_" #OP "_u32", 0, VAL, "s_cmp_" #OP "_u32 s40, s42", {              \
    const uint32_t x = a0, y = b0;                                                                   \
    r.scc = (EXPR_U);                                                                                \
  })
#define CMPK1(X, OP, ID, IMM, EXPR)                                                                    \
  X(3, G, cmpk_##OP##_i32_##ID, "s_cmpk_" #OP "_i32", 0, VAL, "s_cmpk_" #OP "_i32 s40, " #IMM, {      \
    const int32_t x = i32(a0), y = i32(sx16(IMM));                                                     \
    r.scc = (EXPR);                                                                                    \
  })                                                                                                   \
  X(3, G, cmpk_##OP##_u32_##ID, "s_cmpk_" #OP "_u32", 0, VAL, "s_cmpk_" #OP "_u32 s40, " #IMM, {      \
    const uint32_t x = a0, y = IMM;                                                                    \
    r.scc = (EXPR);                                                                                    \
  })
#define CMPK(X, OP, EXPR) \
  CMPK1(X, OP, 7fff, 0x7fff, EXPR) CMPK1(X, OP, 8000, 0x8000, EXPR) CMPK1(X, OP, 1, 1, EXPR) CMPK1(X, OP, ffff, 0xffff, EXPR)
#define MOVK(X, ID, IMM)                                                                                       \
  X(3, G, movk_##ID, "s_movk_i32", 1, VAL, "s_movk_i32 s46, " #IMM, r.d = sx16(IMM))                           \
  X(3, G, cmovk_##ID, "s_cmovk_i32", 1, VAL, "s_mov_b32 s46, s42\ns_cmovk_i32 s46, " #IMM, r.d = c ? sx16(IMM) : b0)
#define SAVEEXEC(X, ID, NAME, EXPR) \
  X(5, M, ID, NAME, 6, VAL, NAME " s[46:47], s[40:41]", r.e = (EXPR); r.d = b)
#define WREXEC(X, ID, NAME, EXPR) X(5, M, ID, NAME, 6, VAL, NAME " s[46:47], s[40:41]", r.e = (EXPR); r.d = r.e)
#define VCMP(X, OP, EXPR)                                                                                          \
  X(5, L, vcmp_##OP##_sgpr, "v_cmp_" #OP "_u32_e64", 1, VAL,                                                       \
    "v_cmp_" #OP "_u32_e64 s[52:53], %[a0], %[b0]\ns_nop 1\nv_cndmask_b32_e64 %[d0], 0, 1, s[52:53]", r.d = (EXPR)) \
  X(5, L, vcmp_##OP##_vcc, "v_cmp_" #OP "_u32_e32", 1, VAL,                                                        \
    "v_cmp_" #OP "_u32_e32 vcc, %[a0], %[b0]\ns_nop 1\nv_cndmask_b32_e32 %[d0], 0, %[one], vcc", r.d = (EXPR))

#define SCALAR_STEPS(X)                                                                                                 \
  X(0, G, add_u32, "s_add_u32", 1, VAL, "s_add_u32 s46, s40, s42", r.d = a0 + b0; r.scc = carry(a0, b0, 0))             \
  X(0, G, sub_u32, "s_sub_u32", 1, VAL, "s_sub_u32 s46, s40, s42", r.d = a0 - b0; r.scc = borrow(a0, b0, 0))            \
  X(0, G, add_i32, "s_add_i32", 1, VAL, "s_add_i32 s46, s40, s42", r.d = a0 + b0; r.scc = add_ov(a0, b0))               \
  X(0, G, sub_i32, "s_sub_i32", 1, VAL, "s_sub_i32 s46, s40, s42", r.d = a0 - b0; r.scc = sub_ov(a0, b0))               \
  X(0, G, addc_u32, "s_addc_u32", 1, VAL, "s_addc_u32 s46, s40, s42", r.d = a0 + b0 + c; r.scc = carry(a0, b0, c))      \
  X(0, G, subb_u32, "s_subb_u32", 1, VAL, "s_subb_u32 s46, s40, s42", r.d = a0 - b0 - c; r.scc = borrow(a0, b0, c))     \
  X(0, G, add128, "s_addc_u32 x3", 4, VAL,                                                                              \
    "s_add_u32 s46, s40, s42\ns_addc_u32 s47, s41, s43\ns_addc_u32 s48, s42, s40\ns_addc_u32 s49, s43, s41",            \
    chain128(o, false, r))                                                                                              \
  X(0, G, sub128, "s_subb_u32 x3", 4, VAL,                                                                              \
    "s_sub_u32 s46, s40, s42\ns_subb_u32 s47, s41, s43\ns_subb_u32 s48, s42, s40\ns_subb_u32 s49, s43, s41",            \
    chain128(o, true, r))                                                                                               \
  X(0, G, min_i32, "s_min_i32", 1, VAL, "s_min_i32 s46, s40, s42", r.scc = i32(a0) < i32(b0); r.d = r.scc ? a0 : b0)    \
  X(0, G, min_u32, "s_min_u32", 1, VAL, "s_min_u32 s46, s40, s42", r.scc = a0 < b0; r.d = r.scc ? a0 : b0)              \
  X(0, G, max_i32, "s_max_i32", 1, VAL, "s_max_i32 s46, s40, s42", r.scc = i32(a0) > i32(b0); r.d = r.scc ? a0 : b0)    \
  X(0, G, max_u32, "s_max_u32", 1, VAL, "s_max_u32 s46, s40, s42", r.scc = a0 > b0; r.d = r.scc ? a0 : b0)              \
  X(0, G, absdiff_i32, "s_absdiff_i32", 1, VAL, "s_absdiff_i32 s46, s40, s42", {                                        \
    const uint32_t v = a0 - b0;                                                                                         \
    r.d = v >> 31 ? 0u - v : v;                                                                                         \
    NZ;                                                                                                                 \
  })                                                                                                                    \
  X(0, G, abs_i32, "s_abs_i32", 1, VAL, "s_abs_i32 s46, s40", r.d = a0 >> 31 ? 0u - a0 : a0; NZ)                        \
  X(0, G, mul_i32, "s_mul_i32", 1, VAL, "s_mul_i32 s46, s40, s42", r.d = a0 * b0)                                       \
  X(0, G, mul_hi_u32, "s_mul_hi_u32", 1, VAL, "s_mul_hi_u32 s46, s40, s42", r.d = mul_hi_u(a0, b0))                     \
  X(0, G, mul_hi_i32, "s_mul_hi_i32", 1, VAL, "s_mul_hi_i32 s46, s40, s42", r.d = mul_hi_i(a0, b0))                     \
  X(0, G, lshl1_add, "s_lshl1_add_u32", 1, VAL, "s_lshl1_add_u32 s46, s40, s42", {                                      \
    const uint64_t v = (uint64_t{a0} << 1) + b0;                                                                        \
    r.d = uint32_t(v), r.scc = v >> 32 != 0;                                                                            \
  })                                                                                                                    \
  X(0, G, lshl2_add, "s_lshl2_add_u32", 1, VAL, "s_lshl2_add_u32 s46, s40, s42", {                                      \
    const uint64_t v = (uint64_t{a0} << 2) + b0;                                                                        \
    r.d = uint32_t(v), r.scc = v >> 32 != 0;                                                                            \
  })                                                                                                                    \
  X(0, G, lshl3_add, "s_lshl3_add_u32", 1, VAL, "s_lshl3_add_u32 s46, s40, s42", {                                      \
    const uint64_t v = (uint64_t{a0} << 3) + b0;                                                                        \
    r.d = uint32_t(v), r.scc = v >> 32 != 0;                                                                            \
  })                                                                                                                    \
  X(0, G, lshl4_add, "s_lshl4_add_u32", 1, VAL, "s_lshl4_add_u32 s46, s40, s42", {                                      \
    const uint64_t v = (uint64_t{a0} << 4) + b0;                                                                        \
    r.d = uint32_t(v), r.scc = v >> 32 != 0;                                                                            \
  })                                                                                                                    \
  ADDK(X, 7fff, 0x7fff) ADDK(X, 8000, 0x8000) ADDK(X, 1, 1) ADDK(X, ffff, 0xffff)                                       \
  LOGIC2(X, and, "s_and_b32", "s_and_b64", a0 & b0, a & b)                                                              \
  LOGIC2(X, or, "s_or_b32", "s_or_b64", a0 | b0, a | b)                                                                 \
  LOGIC2(X, xor, "s_xor_b32", "s_xor_b64", a0 ^ b0, a ^ b)                                                              \
  LOGIC2(X, andn2, "s_andn2_b32", "s_andn2_b64", a0 & ~b0, a & ~b)                                                      \
  LOGIC2(X, orn2, "s_orn2_b32", "s_orn2_b64", a0 | ~b0, a | ~b)                                                         \
  LOGIC2(X, nand, "s_nand_b32", "s_nand_b64", ~(a0 & b0), ~(a & b))                                                     \
  LOGIC2(X, nor, "s_nor_b32", "s_nor_b64", ~(a0 | b0), ~(a | b))                                                        \
  LOGIC2(X, xnor, "s_xnor_b32", "s_xnor_b64", ~(a0 ^ b0), ~(a ^ b))                                                     \
  X(1, G, not_b32, "s_not_b32", 1, VAL, "s_not_b32 s46, s40", r.d = ~a0; NZ)                                            \
  X(1, G, not_b64, "s_not_b64", 2, VAL, "s_not_b64 s[46:47], s[40:41]", r.d = ~a; NZ)                                   \
  X(1, G, lshl_b32, "s_lshl_b32", 1, SH, "s_lshl_b32 s46, s40, s42", r.d = a0 << (b0 & 31); NZ)                         \
  X(1, G, lshr_b32, "s_lshr_b32", 1, SH, "s_lshr_b32 s46, s40, s42", r.d = a0 >> (b0 & 31); NZ)                         \
  X(1, G, ashr_i32, "s_ashr_i32", 1, SH, "s_ashr_i32 s46, s40, s42", r.d = uint32_t(i32(a0) >> (b0 & 31)); NZ)          \
  X(1, G, lshl_b64, "s_lshl_b64", 2, SH, "s_lshl_b64 s[46:47], s[40:41], s42", r.d = a << (b0 & 63); NZ)                \
  X(1, G, lshr_b64, "s_lshr_b64", 2, SH, "s_lshr_b64 s[46:47], s[40:41], s42", r.d = a >> (b0 & 63); NZ)                \
  X(1, G, ashr_i64, "s_ashr_i64", 2, SH, "s_ashr_i64 s[46:47], s[40:41], s42", r.d = uint64_t(i64(a) >> (b0 & 63)); NZ) \
  X(1, G, bfm_b32, "s_bfm_b32", 1, SH, "s_bfm_b32 s46, s40, s42", r.d = uint32_t(ones(a0 & 31) << (b0 & 31)))           \
  X(1, G, bfm_b64, "s_bfm_b64", 2, SH, "s_bfm_b64 s[46:47], s40, s42", r.d = ones(a0 & 63) << (b0 & 63))                \
  X(1, G, bfe_u32, "s_bfe_u32", 1, BFE, "s_bfe_u32 s46, s40, s42", r.d = bfe(a0, b0 & 31, b0 >> 16 & 127, 32, false); NZ) \
  X(1, G, bfe_i32, "s_bfe_i32", 1, BFE, "s_bfe_i32 s46, s40, s42", r.d = bfe(a0, b0 & 31, b0 >> 16 & 127, 32, true); NZ) \
  X(1, G, bfe_u64, "s_bfe_u64", 2, BFE, "s_bfe_u64 s[46:47], s[40:41], s42",                                            \
    r.d = bfe(a, b0 & 63, b0 >> 16 & 127, 64, false); NZ)                                                               \
  X(1, G, bfe_i64, "s_bfe_i64", 2, BFE, "s_bfe_i64 s[46:47], s[40:41], s42",                                            \
    r.d = bfe(a, b0 & 63, b0 >> 16 & 127, 64, true); NZ)                                                                \
  X(1, G, pack_ll, "s_pack_ll_b32_b16", 1, VAL, "s_pack_ll_b32_b16 s46, s40, s42", r.d = (a0 & 0xffffu) | b0 << 16)     \
  X(1, G, pack_lh, "s_pack_lh_b32_b16", 1, VAL, "s_pack_lh_b32_b16 s46, s40, s42",                                      \
    r.d = (a0 & 0xffffu) | (b0 & 0xffff0000u))                                                                          \
  X(1, G, pack_hh, "s_pack_hh_b32_b16", 1, VAL, "s_pack_hh_b32_b16 s46, s40, s42", r.d = a0 >> 16 | (b0 & 0xffff0000u)) \
  X(2, G, brev_b32, "s_brev_b32", 1, VAL, "s_brev_b32 s46, s40", r.d = brev(a0, 32))                                    \
  X(2, G, brev_b64, "s_brev_b64", 2, VAL, "s_brev_b64 s[46:47], s[40:41]", r.d = brev(a, 64))                           \
  X(2, G, wqm_b32, "s_wqm_b32", 1, VAL, "s_wqm_b32 s46, s40", r.d = wqm(a0, 32); NZ)                                    \
  X(2, G, wqm_b64, "s_wqm_b64", 2, VAL, "s_wqm_b64 s[46:47], s[40:41]", r.d = wqm(a, 64); NZ)                           \
  X(2, G, quadmask_b32, "s_quadmask_b32", 1, VAL, "s_quadmask_b32 s46, s40", r.d = quadmask(a0, 32); NZ)                \
  X(2, G, quadmask_b64, "s_quadmask_b64", 2, VAL, "s_quadmask_b64 s[46:47], s[40:41]", r.d = quadmask(a, 64); NZ)       \
  X(2, G, bcnt0_b32, "s_bcnt0_i32_b32", 1, VAL, "s_bcnt0_i32_b32 s46, s40", r.d = 32 - bcnt1(a0); NZ)                   \
  X(2, G, bcnt0_b64, "s_bcnt0_i32_b64", 1, VAL, "s_bcnt0_i32_b64 s46, s[40:41]", r.d = 64 - bcnt1(a); NZ)               \
  X(2, G, bcnt1_b32, "s_bcnt1_i32_b32", 1, VAL, "s_bcnt1_i32_b32 s46, s40", r.d = bcnt1(a0); NZ)                        \
  X(2, G, bcnt1_b64, "s_bcnt1_i32_b64", 1, VAL, "s_bcnt1_i32_b64 s46, s[40:41]", r.d = bcnt1(a); NZ)                    \
  X(2, G, ff0_b32, "s_ff0_i32_b32", 1, VAL, "s_ff0_i32_b32 s46, s40", r.d = ff1(~a0, 32))                               \
  X(2, G, ff0_b64, "s_ff0_i32_b64", 1, VAL, "s_ff0_i32_b64 s46, s[40:41]", r.d = ff1(~a, 64))                           \
  X(2, G, ff1_b32, "s_ff1_i32_b32", 1, VAL, "s_ff1_i32_b32 s46, s40", r.d = ff1(a0, 32))                                \
  X(2, G, ff1_b64, "s_ff1_i32_b64", 1, VAL, "s_ff1_i32_b64 s46, s[40:41]", r.d = ff1(a, 64))                            \
  X(2, G, flbit_b32, "s_flbit_i32_b32", 1, VAL, "s_flbit_i32_b32 s46, s40", r.d = flbit(a0, 32))                        \
  X(2, G, flbit_b64, "s_flbit_i32_b64", 1, VAL, "s_flbit_i32_b64 s46, s[40:41]", r.d = flbit(a, 64))                    \
  X(2, G, flbit_i32, "s_flbit_i32", 1, VAL, "s_flbit_i32 s46, s40", r.d = flbit_signed(a0, 32))                         \
  X(2, G, flbit_i64, "s_flbit_i32_i64", 1, VAL, "s_flbit_i32_i64 s46, s[40:41]", r.d = flbit_signed(a, 64))             \
  X(2, G, sext_i8, "s_sext_i32_i8", 1, VAL, "s_sext_i32_i8 s46, s40", r.d = uint32_t(int32_t(int8_t(a0))))              \
  X(2, G, sext_i16, "s_sext_i32_i16", 1, VAL, "s_sext_i32_i16 s46, s40", r.d = sx16(a0))                                \
  X(2, G, bitset0_b32, "s_bitset0_b32", 1, VAL, "s_mov_b32 s46, s42\ns_bitset0_b32 s46, s40", r.d = b0 & ~(1u << (a0 & 31))) \
  X(2, G, bitset0_b64, "s_bitset0_b64", 2, VAL, "s_mov_b64 s[46:47], s[42:43]\ns_bitset0_b64 s[46:47], s40",            \
    r.d = b & ~(1ull << (a0 & 63)))                                                                                     \
  X(2, G, bitset1_b32, "s_bitset1_b32", 1, VAL, "s_mov_b32 s46, s42\ns_bitset1_b32 s46, s40", r.d = b0 | 1u << (a0 & 31)) \
  X(2, G, bitset1_b64, "s_bitset1_b64", 2, VAL, "s_mov_b64 s[46:47], s[42:43]\ns_bitset1_b64 s[46:47], s40",            \
    r.d = b | 1ull << (a0 & 63))                                                                                        \
  X(2, G, bitreplicate, "s_bitreplicate_b64_b32", 2, VAL, "s_bitreplicate_b64_b32 s[46:47], s40", r.d = bitrep(a0))     \
  CMP2(X, eq, x == y, x == y) CMP2(X, lg, x != y, x != y) CMP2(X, gt, x > y, x > y)                                     \
  CMP2(X, ge, x >= y, x >= y) CMP2(X, lt, x < y, x < y) CMP2(X, le, x <= y, x <= y)                                     \
  X(3, G, cmp_eq_u64, "s_cmp_eq_u64", 0, VAL, "s_cmp_eq_u64 s[40:41], s[42:43]", r.scc = a == b)                        \
  X(3, G, cmp_lg_u64, "s_cmp_lg_u64", 0, VAL, "s_cmp_lg_u64 s[40:41], s[42:43]", r.scc = a != b)                        \
  CMPK(X, eq, x == y) CMPK(X, lg, x != y) CMPK(X, gt, x > y) CMPK(X, ge, x >= y) CMPK(X, lt, x < y) CMPK(X, le, x <= y) \
  X(3, G, bitcmp0_b32, "s_bitcmp0_b32", 0, SH, "s_bitcmp0_b32 s40, s42", r.scc = !((a0 >> (b0 & 31)) & 1u))             \
  X(3, G, bitcmp0_b64, "s_bitcmp0_b64", 0, SH, "s_bitcmp0_b64 s[40:41], s42", r.scc = !((a >> (b0 & 63)) & 1u))         \
  X(3, G, bitcmp1_b32, "s_bitcmp1_b32", 0, SH, "s_bitcmp1_b32 s40, s42", r.scc = (a0 >> (b0 & 31)) & 1u)                \
  X(3, G, bitcmp1_b64, "s_bitcmp1_b64", 0, SH, "s_bitcmp1_b64 s[40:41], s42", r.scc = (a >> (b0 & 63)) & 1u)            \
  X(3, G, cselect_b32, "s_cselect_b32", 1, VAL, "s_cselect_b32 s46, s40, s42", r.d = c ? a0 : b0)                       \
  X(3, G, cselect_b64, "s_cselect_b64", 2, VAL, "s_cselect_b64 s[46:47], s[40:41], s[42:43]", r.d = c ? a : b)          \
  X(3, G, cmov_b32, "s_cmov_b32", 1, VAL, "s_mov_b32 s46, s42\ns_cmov_b32 s46, s40", r.d = c ? a0 : b0)                 \
  X(3, G, cmov_b64, "s_cmov_b64", 2, VAL, "s_mov_b64 s[46:47], s[42:43]\ns_cmov_b64 s[46:47], s[40:41]", r.d = c ? a : b) \
  MOVK(X, 7fff, 0x7fff) MOVK(X, 8000, 0x8000) MOVK(X, 1, 1) MOVK(X, ffff, 0xffff)                                       \
  X(3, G, mov_m16, "s_mov_b32", 1, VAL, "s_mov_b32 s46, -16", r.d = 0xfffffff0u)                                        \
  X(3, G, mov_64, "s_mov_b32", 1, VAL, "s_mov_b32 s46, 64", r.d = 64)                                                   \
  X(3, G, mov_1f, "s_mov_b32", 1, VAL, "s_mov_b32 s46, 1.0", r.d = 0x3f800000u)                                         \
  X(3, G, mov_hf, "s_mov_b32", 1, VAL, "s_mov_b32 s46, 0.5", r.d = 0x3f000000u)                                         \
  X(3, G, mov_lit, "s_mov_b32", 1, VAL, "s_mov_b32 s46, 0x12345678", r.d = 0x12345678u)                                 \
  X(4, G, br_scc0, "s_cbranch_scc0", 1, VAL, XS_BRANCH("s_cbranch_scc0"), r.d = c ? 2 : 1)                              \
  X(4, G, br_scc1, "s_cbranch_scc1", 1, VAL, XS_BRANCH("s_cbranch_scc1"), r.d = c ? 1 : 2)                              \
  X(4, G, br_vccz, "s_cbranch_vccz", 1, VAL, "s_mov_b64 vcc, 0\ns_cmov_b64 vcc, s[40:41]\n" XS_BRANCH("s_cbranch_vccz"), \
    r.d = (c ? a : 0) == 0 ? 1 : 2)                                                                                     \
  X(4, G, br_vccnz, "s_cbranch_vccnz", 1, VAL,                                                                          \
    "s_mov_b64 vcc, 0\ns_cmov_b64 vcc, s[40:41]\n" XS_BRANCH("s_cbranch_vccnz"), r.d = (c ? a : 0) != 0 ? 1 : 2)        \
  X(4, G, br_execz, "s_cbranch_execz", 1, VAL,                                                                          \
    XS_EXEC_IS("s_cmov_b64 exec, s[40:41]\n") XS_BRANCH("s_cbranch_execz") XS_EXEC_BACK, r.d = (c ? a : 0) == 0 ? 1 : 2) \
  X(4, G, br_execnz, "s_cbranch_execnz", 1, VAL,                                                                        \
    XS_EXEC_IS("s_cmov_b64 exec, s[40:41]\n") XS_BRANCH("s_cbranch_execnz") XS_EXEC_BACK, r.d = (c ? a : 0) != 0 ? 1 : 2) \
  SAVEEXEC(X, and_saveexec, "s_and_saveexec_b64", a & b)                                                                \
  SAVEEXEC(X, or_saveexec, "s_or_saveexec_b64", a | b)                                                                  \
  SAVEEXEC(X, xor_saveexec, "s_xor_saveexec_b64", a ^ b)                                                                \
  SAVEEXEC(X, andn2_saveexec, "s_andn2_saveexec_b64", a & ~b)                                                           \
  SAVEEXEC(X, orn2_saveexec, "s_orn2_saveexec_b64", a | ~b)                                                             \
  SAVEEXEC(X, nand_saveexec, "s_nand_saveexec_b64", ~(a & b))                                                           \
  SAVEEXEC(X, nor_saveexec, "s_nor_saveexec_b64", ~(a | b))                                                             \
  SAVEEXEC(X, xnor_saveexec, "s_xnor_saveexec_b64", ~(a ^ b))                                                           \
  SAVEEXEC(X, andn1_saveexec, "s_andn1_saveexec_b64", ~a & b)                                                           \
  SAVEEXEC(X, orn1_saveexec, "s_orn1_saveexec_b64", ~a | b)                                                             \
  WREXEC(X, andn1_wrexec, "s_andn1_wrexec_b64", ~a & b)                                                                 \
  WREXEC(X, andn2_wrexec, "s_andn2_wrexec_b64", a & ~b)                                                                 \
  VCMP(X, lt, a0 < b0) VCMP(X, eq, a0 == b0) VCMP(X, le, a0 <= b0)                                                      \
  VCMP(X, gt, a0 > b0) VCMP(X, ne, a0 != b0) VCMP(X, ge, a0 >= b0)                                                      \
  X(5, L, vadd_co, "v_addc_co_u32", 3, VAL,                                                                             \
    "v_add_co_u32_e64 %[d0], s[52:53], %[a0], %[b0]\ns_nop 1\n"                                                         \
    "v_addc_co_u32_e64 %[d1], s[54:55], %[a1], %[b1], s[52:53]\ns_nop 1\n"                                              \
    "v_cndmask_b32_e64 %[d2], 0, 1, s[54:55]",                                                                          \
    r.d = a + b; r.e = carry(a1, b1, carry(a0, b0, 0)))

#define X(P, C, ID, NAME, NW, BK, DEV, ...) G_##ID,
enum StepId : int { SCALAR_STEPS(X) kNumSteps };
#undef X

struct StepInfo {
  int part, cls, nw, bk;
};
#define X(P, C, ID, NAME, NW, BK, DEV, ...) {P, C, NW, BK},
constexpr StepInfo kSteps[kNumSteps] = {SCALAR_STEPS(X)};
#undef X

// What a lane must hold after step ID.
#define X(P, C, ID, NAME, NW, BK, DEV, ...)                                      \
  XS_HD void want_##ID(const Ops& o, Res& r) {                                    \
    const uint32_t a0 = o.a0, a1 = o.a1, b0 = o.b0, b1 = o.b1, c = o.c;           \
    const uint64_t a = uint64_t{a1} << 32 | a0, b = uint64_t{b1} << 32 | b0;      \
    (void)a0, (void)a1, (void)b0, (void)b1, (void)c, (void)a, (void)b;            \
    r.scc = c;                                                                    \
    __VA_ARGS__;                                                                         \
    if (kSteps[G_##ID].cls == M) r.scc = r.e != 0, r.first = r.e ? ff1(r.e, 64) : 0u; \
  }
SCALAR_STEPS(X)
#undef X

XS_HD constexpr int step_words(int g) {
  return kSteps[g].cls == G ? kSteps[g].nw + 1 : kSteps[g].nw;  // G: the result words and SCC
}
XS_HD constexpr int part_first(int p) {
  int g = 0;
  while (g < kNumSteps && kSteps[g].part < p) ++g;
  return g;
}
XS_HD constexpr int word_base(int g) {  // word of step g's first within its part
  int w = 0;
  for (int i = part_first(kSteps[g].part); i < g; ++i) w += step_words(i);
  return w;
}
constexpr bool parts_in_order() {
  for (int g = 1; g < kNumSteps; ++g)
    if (kSteps[g].part < kSteps[g - 1].part) return false;
  return true;
}
static_assert(parts_in_order(), "SCALAR_STEPS lists the parts in order");

// movrel: forms 0 movrels_b32, 1 movrels_b64, 2 movreld_b32, 3 movreld_b64.
constexpr int kMovrelBlock = 16;
XS_HD constexpr int movrel_indexes(int f) { return f & 1 ? 8 : 16; }
XS_HD constexpr int movrel_index(int f, int k) { return f & 1 ? 2 * k : k; }  // M0 is even for the _b64 forms
XS_HD constexpr int movrel_words(int f) { return f == 0 ? 1 : f == 1 ? 2 : 3; }
XS_HD constexpr int movrel_base(int f, int k) {
  int w = 0;
  for (int i = 0; i < f; ++i) w += movrel_indexes(i) * movrel_words(i);
  return w + k * movrel_words(f);
}
constexpr int kMovrelSteps = 48, kMovrelWords = movrel_base(4, 0);
constexpr int kSgprSteps = 2, kSgprWords = 6;

struct Shape {
  int steps, words;
};
constexpr Shape shape_of(int p) {
  if (p == kMovrel) return {kMovrelSteps, kMovrelWords};
  if (p == kSgpr) return {kSgprSteps, kSgprWords};
  int w = 0;
  for (int g = part_first(p); g < part_first(p + 1); ++g) w += step_words(g);
  return {part_first(p + 1) - part_first(p), w};
}
constexpr Shape kShape[kNumParts] = {shape_of(0), shape_of(1), shape_of(2), shape_of(3),
                                     shape_of(4), shape_of(5), shape_of(6), shape_of(7)};

// movrel: the word thread t must hold at word `w` (0..2) of form f, M0 = k.
XS_HD uint32_t want_movrel(uint32_t seed, int f, int k, int w, uint32_t t) {
  const uint32_t wave = t >> 6, l = t & 63u;
  auto blk = [&](int j) { return hashv(seed, kMovrel, f, wave, j & 15, l); };
  auto src = [&](int j) { return hashv(seed, kMovrel, f, wave, 16 + j, l); };
  switch (f) {
    case 0: return blk(k);
    case 1: return blk(k + w);
    case 2: return w == 0 ? src(0) : w == 1 ? blk(k + 1) : blk(k + 15);
    default: return w < 2 ? src(w) : blk(k + 2);
  }
}

// sgpr: register N of phase ph is lane N % 64 of word N / 64; 0 where a lane has none.
XS_HD bool sgpr_cell(int ph, int hi, uint32_t l) {
  if (ph == 1) return !hi && l < 52;
  return hi ? l < 36 || l == 42 || l == 43 : l >= 52;
}
XS_HD uint32_t sgpr_pattern(uint32_t seed, int ph, int hi, uint32_t t) { return hashv(seed, kSgpr, ph, t >> 6, hi, t & 63u); }
XS_HD uint32_t want_sgpr(uint32_t seed, int w, uint32_t t) {  // words: ph0 p lo, p hi, ~p lo, ~p hi; ph1 p, ~p
  const int ph = w >= 4, hi = ph ? 0 : w & 1, neg = ph ? w == 5 : w >= 2;
  if (!sgpr_cell(ph, hi, t & 63u)) return 0;
  const uint32_t p = sgpr_pattern(seed, ph, hi, t);
  return neg ? ~p : p;
}

constexpr uint32_t kLdsUsed = part_reduction_words<kBlock>(kNumParts, kCoverWords) * 4;
static_assert(kLdsUsed > kLdsExclusive, "no two workgroups share a CU");

struct ScalarRecord {
  PartRecordHead<kNumParts> head;
  uint32_t reserved;
  uint32_t gpr_alloc[kCoverWords];  // per SIMD: OR of its waves' HW_REG_GPR_ALLOC, OR of the complements
  uint32_t pad[2];
};
static_assert(sizeof(ScalarRecord) == 128, "one 128-byte record per workgroup");

using Expect = PartExpect<kNumParts>;

// ------------------------------------------------------------------- device
struct Ctx {
  uint32_t seed, t, inj;  // seed and inj may be per-lane copies of uniform values
  uint32_t* dump;  // k_scalar_probe only
};

// The empty statement keeps the tally a running sum: left to itself the
// compiler holds every step's words back and adds them up at the end.
XS_D void take(const Ctx& c, Tally& y, int part, uint32_t word, uint32_t got, uint32_t want) {
  take_word(y, c.dump, word * kBlock + c.t, got, want, (c.inj >> part) & 1u);
  asm volatile("" : "+v"(y.bad), "+v"(y.digest));
}

// The iteration number as an SGPR, whatever register class the compiler gave the counter.
#define XS_ITER [i] "s"(__builtin_amdgcn_readfirstlane(i))
#define XS_OPERANDS [a0] "v"(o.a0), [a1] "v"(o.a1), [b0] "v"(o.b0), [b1] "v"(o.b1), [c] "v"(o.c)

#define RUN_G(P, ID, NW, BK, DEV)                                                                              \
  {                                                                                                            \
    uint32_t d0 = 0, d1 = 0, d2 = 0, d3 = 0, sc = 0;                                                           \
    _Pragma("nounroll") for (uint32_t i = 0; i < 64; ++i)                                                      \
        asm volatile(XS_PRE DEV "\n" XS_POST_##NW                                                              \
                     : [d0] "+v"(d0), [d1] "+v"(d1), [d2] "+v"(d2), [d3] "+v"(d3), [sc] "+v"(sc)               \
                     : XS_OPERANDS, XS_ITER                                                                 \
                     : XS_CLOBBER);                                                                            \
    const uint32_t got[5] = {d0, d1, d2, d3, 0}, want[5] = {uint32_t(r.d), uint32_t(r.d >> 32), uint32_t(r.e), \
                                                            uint32_t(r.e >> 32), 0};                           \
    _Pragma("unroll") for (int w = 0; w < NW; ++w) take(c, y, P, base + w, got[w], want[w]);                   \
    take(c, y, P, base + NW, sc, r.scc);                                                                       \
  }

// EXEC = b, the instruction on a, marks under the new mask, EXEC restored.
#define RUN_M(P, ID, NW, BK, DEV)                                                                                 \
  {                                                                                                               \
    uint32_t d0 = 0, d1 = 0, d2 = 0, d3 = 0, sc = 0, fl = 0, act;                                                 \
    _Pragma("nounroll") for (uint32_t i = 0; i < 64; ++i)                                                         \
        asm volatile(XS_PRE                                                                                       \
                     "v_mov_b32 %[act], 0\n"                                                                      \
                     "s_mov_b64 s[72:73], exec\n"                                                                 \
                     "s_mov_b64 exec, s[42:43]\n" DEV "\n"                                                        \
                     "s_cselect_b32 s50, 1, 0\n"                                                                  \
                     "v_mov_b32 %[act], 1\n"                                                                      \
                     "v_readfirstlane_b32 s54, %[lid]\n"                                                          \
                     "s_mov_b64 exec, s[72:73]\n"                                                                 \
                     "v_cmp_ne_u32_e64 s[48:49], 0, %[act]\n"                                                     \
                     "s_mov_b32 s51, m0\n"                                                                        \
                     "s_mov_b32 m0, %[i]\n"                                                                       \
                     "s_nop 3\n" XS_W0 XS_W1 XS_W23 "v_writelane_b32 %[fl], s54, m0\n" XS_M0_OFF                  \
                     : [d0] "+v"(d0), [d1] "+v"(d1), [d2] "+v"(d2), [d3] "+v"(d3), [sc] "+v"(sc), [fl] "+v"(fl),  \
                       [act] "=&v"(act)                                                                           \
                     : XS_OPERANDS, XS_ITER, [lid] "v"(lane)                                                   \
                     : XS_CLOBBER);                                                                               \
    take(c, y, P, base, d0, uint32_t(r.d));                                                                       \
    take(c, y, P, base + 1, d1, uint32_t(r.d >> 32));                                                             \
    take(c, y, P, base + 2, d2, uint32_t(r.e));                                                                   \
    take(c, y, P, base + 3, d3, uint32_t(r.e >> 32));                                                             \
    take(c, y, P, base + 4, sc, r.scc);                                                                           \
    take(c, y, P, base + 5, fl, r.first);                                                                         \
  }

// Once per lane, no loop: the VALU's side of the SGPR interface.
#define RUN_L(P, ID, NW, BK, DEV)                                                                \
  {                                                                                              \
    uint32_t d0, d1 = 0, d2 = 0;                                                                 \
    asm volatile(DEV                                                                             \
                 : [d0] "=&v"(d0), [d1] "+v"(d1), [d2] "+v"(d2)                                  \
                 : XS_OPERANDS, [one] "v"(one)                                                   \
                 : "s52", "s53", "s54", "s55", "vcc");                                           \
    take(c, y, P, base, d0, uint32_t(r.d));                                                      \
    if (NW == 3) take(c, y, P, base + 1, d1, uint32_t(r.d >> 32));                               \
    if (NW == 3) take(c, y, P, base + 2, d2, uint32_t(r.e));                                     \
  }

template <int PART>
XS_D void run_table_part(const Ctx& c, Tally& y) {
  const uint32_t lane = c.t & 63u, one = 1;
  (void)lane, (void)one;
#define X(P, C, ID, NAME, NW, BK, DEV, ...)                                        \
  if constexpr (P == PART) {                                                        \
    constexpr int g = G_##ID, base = word_base(g);                                  \
    uint32_t tt = c.t; /* opaque: the step's operands are hashed here, not earlier */ \
    asm volatile("" : "+v"(tt));                                                    \
    const Ops o = operands(c.seed, P, g - part_first(P), BK, tt);                   \
    Res r;                                                                          \
    want_##ID(o, r);                                                                \
    RUN_##C(P, ID, NW, BK, DEV)                                                     \
  }
  SCALAR_STEPS(X)
#undef X
}

// ---- movrel ----------------------------------------------------------------
#define XS_BLK(J) "v_readlane_b32 s[56+" #J "], %[b" #J "], %[i]\n"
#define XS_BLK_LOAD                                                                             \
  XS_BLK(0) XS_BLK(1) XS_BLK(2) XS_BLK(3) XS_BLK(4) XS_BLK(5) XS_BLK(6) XS_BLK(7) XS_BLK(8) XS_BLK(9) \
  XS_BLK(10) XS_BLK(11) XS_BLK(12) XS_BLK(13) XS_BLK(14) XS_BLK(15)
#define XS_BLK_IN                                                                                                      \
  [b0] "v"(b[0]), [b1] "v"(b[1]), [b2] "v"(b[2]), [b3] "v"(b[3]), [b4] "v"(b[4]), [b5] "v"(b[5]), [b6] "v"(b[6]),      \
      [b7] "v"(b[7]), [b8] "v"(b[8]), [b9] "v"(b[9]), [b10] "v"(b[10]), [b11] "v"(b[11]), [b12] "v"(b[12]),            \
      [b13] "v"(b[13]), [b14] "v"(b[14]), [b15] "v"(b[15])
#define XS_BLK_CLOBBER                                                                                              \
  "s40", "s41", "s46", "s47", "s48", "s51", "s56", "s57", "s58", "s59", "s60", "s61", "s62", "s63", "s64", "s65", "s66", \
      "s67", "s68", "s69", "s70", "s71"
// M0 = index K for the instruction, then = i for the write-back, then restored.
#define XS_MOVREL(BODY, BACK)                                                                                  \
  asm volatile("s_nop 3\n" XS_BLK_LOAD                                                                         \
               "v_readlane_b32 s40, %[s0], %[i]\n"                                                             \
               "v_readlane_b32 s41, %[s1], %[i]\n"                                                             \
               "s_mov_b32 s51, m0\n"                                                                           \
               "s_mov_b32 m0, %[k]\n"                                                                          \
               "s_nop 1\n" BODY "\n"                                                                           \
               "s_mov_b32 m0, %[i]\n"                                                                          \
               "s_nop 3\n" BACK "s_mov_b32 m0, s51\n"                                                          \
               : [d0] "+v"(d0), [d1] "+v"(d1), [d2] "+v"(d2)                                                   \
               : XS_BLK_IN, [s0] "v"(s0), [s1] "v"(s1), XS_ITER, [k] "i"(K), [k1] "i"((K + 1) & 15),        \
                 [k2] "i"((K + 2) & 15), [k15] "i"((K + 15) & 15)                                              \
               : XS_BLK_CLOBBER)

template <int F, int KI>
XS_D void run_movrel_index(const Ctx& c, Tally& y, const uint32_t (&b)[16], uint32_t s0, uint32_t s1) {
  constexpr int K = movrel_index(F, KI);
  uint32_t d0 = 0, d1 = 0, d2 = 0;
#pragma nounroll
  for (uint32_t i = 0; i < 64; ++i) {
    if constexpr (F == 0)
      XS_MOVREL("s_movrels_b32 s46, s56", "v_writelane_b32 %[d0], s46, m0\n");
    else if constexpr (F == 1)
      XS_MOVREL("s_movrels_b64 s[46:47], s[56:57]",
                "v_writelane_b32 %[d0], s46, m0\nv_writelane_b32 %[d1], s47, m0\n");
    else if constexpr (F == 2)
      XS_MOVREL("s_movreld_b32 s56, s40",
                "v_writelane_b32 %[d0], s[56+%[k]], m0\nv_writelane_b32 %[d1], s[56+%[k1]], m0\n"
                "v_writelane_b32 %[d2], s[56+%[k15]], m0\n");
    else
      XS_MOVREL("s_movreld_b64 s[56:57], s[40:41]",
                "v_writelane_b32 %[d0], s[56+%[k]], m0\nv_writelane_b32 %[d1], s[56+%[k1]], m0\n"
                "v_writelane_b32 %[d2], s[56+%[k2]], m0\n");
  }
  const uint32_t got[3] = {d0, d1, d2};
#pragma unroll
  for (int w = 0; w < movrel_words(F); ++w)
    take(c, y, kMovrel, movrel_base(F, KI) + w, got[w], want_movrel(c.seed, F, K, w, c.t));
}

template <int F, int... Ks>
XS_D void run_movrel_form(const Ctx& c, Tally& y, std::integer_sequence<int, Ks...>) {
  const uint32_t wave = c.t >> 6, l = c.t & 63u;
  uint32_t b[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) b[j] = hashv(c.seed, kMovrel, F, wave, j, l);
  const uint32_t s0 = hashv(c.seed, kMovrel, F, wave, 16, l), s1 = hashv(c.seed, kMovrel, F, wave, 17, l);
  (run_movrel_index<F, Ks>(c, y, b, s0, s1), ...);
}

XS_D void run_movrel(const Ctx& c, Tally& y) {
  run_movrel_form<0>(c, y, std::make_integer_sequence<int, 16>{});
  run_movrel_form<1>(c, y, std::make_integer_sequence<int, 8>{});
  run_movrel_form<2>(c, y, std::make_integer_sequence<int, 16>{});
  run_movrel_form<3>(c, y, std::make_integer_sequence<int, 8>{});
}

// ---- sgpr ------------------------------------------------------------------
// COUNT registers from FIRST: sN <- lane N - OFF of SRC, and back into DST.
#define XS_SG_WRITE(FIRST, COUNT, OFF, SRC) \
  ".set xs_n, " #FIRST "\n.rept " #COUNT "\nv_readlane_b32 s[xs_n], " SRC ", xs_n-" #OFF "\n.set xs_n, xs_n+1\n.endr\n"
#define XS_SG_READ(FIRST, COUNT, OFF, DST) \
  ".set xs_n, " #FIRST "\n.rept " #COUNT "\nv_writelane_b32 " DST ", s[xs_n], xs_n-" #OFF "\n.set xs_n, xs_n+1\n.endr\n"
#define XS_S10(d) \
  "s" #d "0", "s" #d "1", "s" #d "2", "s" #d "3", "s" #d "4", "s" #d "5", "s" #d "6", "s" #d "7", "s" #d "8", "s" #d "9"

XS_D void run_sgpr(const Ctx& c, Tally& y) {
  {  // phase 0: s52..s99 and VCC
    const uint32_t plo = sgpr_pattern(c.seed, 0, 0, c.t), phi = sgpr_pattern(c.seed, 0, 1, c.t), nlo = ~plo, nhi = ~phi;
    uint32_t o0 = 0, o1 = 0, o2 = 0, o3 = 0;
    asm volatile(
        "s_nop 0\n"
        XS_SG_WRITE(52, 12, 0, "%[plo]") XS_SG_WRITE(64, 36, 64, "%[phi]")
        "v_readlane_b32 vcc_lo, %[phi], 42\nv_readlane_b32 vcc_hi, %[phi], 43\n"
        "s_barrier\n"
        XS_SG_READ(52, 12, 0, "%[o0]") XS_SG_READ(64, 36, 64, "%[o1]")
        "v_writelane_b32 %[o1], vcc_lo, 42\nv_writelane_b32 %[o1], vcc_hi, 43\n"
        XS_SG_WRITE(52, 12, 0, "%[nlo]") XS_SG_WRITE(64, 36, 64, "%[nhi]")
        "v_readlane_b32 vcc_lo, %[nhi], 42\nv_readlane_b32 vcc_hi, %[nhi], 43\n"
        "s_barrier\n"
        XS_SG_READ(52, 12, 0, "%[o2]") XS_SG_READ(64, 36, 64, "%[o3]")
        "v_writelane_b32 %[o3], vcc_lo, 42\nv_writelane_b32 %[o3], vcc_hi, 43\n"
        : [o0] "+v"(o0), [o1] "+v"(o1), [o2] "+v"(o2), [o3] "+v"(o3)
        : [plo] "v"(plo), [phi] "v"(phi), [nlo] "v"(nlo), [nhi] "v"(nhi)
        : "s52", "s53", "s54", "s55", "s56", "s57", "s58", "s59", XS_S10(6), XS_S10(7), XS_S10(8), XS_S10(9), "vcc");
    const uint32_t got[4] = {o0, o1, o2, o3};
#pragma unroll
    for (int w = 0; w < 4; ++w) take(c, y, kSgpr, w, got[w], want_sgpr(c.seed, w, c.t));
  }
  {  // phase 1: s0..s51
    const uint32_t p = sgpr_pattern(c.seed, 1, 0, c.t), n = ~p;
    uint32_t o0 = 0, o1 = 0;
    asm volatile("s_nop 0\n" XS_SG_WRITE(0, 52, 0, "%[p]") "s_barrier\n" XS_SG_READ(0, 52, 0, "%[o0]")
                 XS_SG_WRITE(0, 52, 0, "%[n]") "s_barrier\n" XS_SG_READ(0, 52, 0, "%[o1]")
                 : [o0] "+v"(o0), [o1] "+v"(o1)
                 : [p] "v"(p), [n] "v"(n)
                 : "s0", "s1", "s2", "s3", "s4", "s5", "s6", "s7", "s8", "s9", XS_S10(1), XS_S10(2), XS_S10(3),
                   XS_S10(4), "s50", "s51");
    take(c, y, kSgpr, 4, o0, want_sgpr(c.seed, 4, c.t));
    take(c, y, kSgpr, 5, o1, want_sgpr(c.seed, 5, c.t));
  }
}

// `mask` is workgroup-uniform: every wave takes the same way to the barriers of run_sgpr.
XS_D void run_parts(const Ctx& c, uint32_t mask, Tally (&y)[kNumParts]) {
  if (mask & 1u) run_table_part<0>(c, y[0]);
  if (mask & 2u) run_table_part<1>(c, y[1]);
  if (mask & 4u) run_table_part<2>(c, y[2]);
  if (mask & 8u) run_table_part<3>(c, y[3]);
  if (mask & 16u) run_table_part<4>(c, y[4]);
  if (mask & 32u) run_table_part<5>(c, y[5]);
  if (mask & 64u) run_movrel(c, y[6]);
}

// The two statements of run_sgpr clobber between them every SGPR there is, so
// a scalar value that lived across both would be spilled. The kernels run the
// `sgpr` part first and carry their arguments across it in VGPRs, by hand.
XS_D uint32_t to_vgpr(uint32_t s) {
  uint32_t v;
  asm volatile("v_mov_b32 %0, %1" : "=v"(v) : "s"(s));
  return v;
}
XS_D uint32_t to_sgpr(uint32_t v) { return __builtin_amdgcn_readfirstlane(v); }
template <typename T>
struct Held {
  static_assert(sizeof(T) % 4 == 0, "whole words");
  uint32_t v[sizeof(T) / 4];
  XS_D explicit Held(const T& x) {
    uint32_t w[sizeof(T) / 4];
    __builtin_memcpy(w, &x, sizeof(T));
#pragma unroll
    for (size_t q = 0; q < sizeof(T) / 4; ++q) v[q] = to_vgpr(w[q]);
  }
  XS_D T get() const {
    uint32_t w[sizeof(T) / 4];
#pragma unroll
    for (size_t q = 0; q < sizeof(T) / 4; ++q) w[q] = to_sgpr(v[q]);
    T x;
    __builtin_memcpy(&x, w, sizeof(T));
    return x;
  }
};

// HW_REG_GPR_ALLOC, raw: see the header for why it is not interpreted.
XS_D uint32_t gpr_alloc() {
  uint32_t v;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_GPR_ALLOC)" : "=s"(v));
  return v;
}

struct SweepArgs {
  ScalarRecord* records;
  uint32_t part_mask, seed;
  int inject_xcd, inject_cu;
  uint32_t inject_parts, pad;
  Expect expect;
};

__global__ __launch_bounds__(kBlock) void k_scalar_sweep(SweepArgs args) {
  extern __shared__ uint32_t scalar_lds[];
  const uint32_t t = threadIdx.x;
  Tally y[kNumParts];
  const Held<SweepArgs> held(args);
  {
    // An injection into `sgpr` is applied by the host-side digest only if the
    // flipped word shows: the flip needs (xcd, cu), read here, before the part.
    const uint32_t vseed = held.v[3], vmask = held.v[2];
    const uint32_t hw0 = hw_id();
    const bool inj0 = inject_selected(args.inject_xcd, args.inject_cu, xcc_id(), cu_key(hw0));
    const uint32_t vinj = inj0 ? held.v[6] : 0u;
    if (to_sgpr(vmask) & 128u) run_sgpr(Ctx{vseed, t, vinj, nullptr}, y[kSgpr]);
  }
  const SweepArgs a = held.get();
  const uint32_t xcd = xcc_id();
  const uint32_t hw = hw_id();
  const uint32_t cu = cu_key(hw);
  const uint32_t simd = simd_id(hw);
  const bool inject = inject_selected(a.inject_xcd, a.inject_cu, xcd, cu);
  const Ctx c{a.seed, t, inject ? a.inject_parts : 0u, nullptr};
  run_parts(c, a.part_mask, y);

  const uint32_t alloc = gpr_alloc();
  uint32_t cover[kCoverWords];
#pragma unroll
  for (uint32_t q = 0; q < 4; ++q) {
    cover[2 * q] = simd == q ? alloc : 0u;
    cover[2 * q + 1] = simd == q ? ~alloc : 0u;
  }
  reduce_parts<kNumParts, kCoverWords, kBlock>(scalar_lds, t, simd, y, cover, a.part_mask, a.expect, xcd, cu,
                                               &a.records[blockIdx.x]);
}

struct ProbeArgs {
  uint32_t* dump;
  uint32_t part, seed, words, pad;
};

// One workgroup; dump holds the part's words x 1,024, then a row of raw
// HW_REG_GPR_ALLOC and a row of HW_REG_HW_ID.
__global__ __launch_bounds__(kBlock) void k_scalar_probe(ProbeArgs args) {
  const uint32_t t = threadIdx.x;
  Tally y[kNumParts];
  const Held<ProbeArgs> held(args);
  if (to_sgpr(held.v[2]) == kSgpr) {
    // The dump pointer as two VGPRs: a per-lane address is what a vector store takes anyway.
    uint32_t* dump = reinterpret_cast<uint32_t*>(uint64_t{held.v[1]} << 32 | held.v[0]);
    run_sgpr(Ctx{held.v[3], t, 0u, dump}, y[kSgpr]);
  }
  const ProbeArgs a = held.get();
  const Ctx c{a.seed, t, 0u, a.dump};
  run_parts(c, 1u << a.part, y);
  a.dump[a.words * kBlock + t] = gpr_alloc();
  a.dump[(a.words + 1) * kBlock + t] = hw_id();
}

// --------------------------------------------------------------------- host
using WantFn = void (*)(const Ops&, Res&);
#define X(P, C, ID, NAME, NW, BK, DEV, ...) [](const Ops& o, Res& r) { want_##ID(o, r); },
const WantFn kWant[kNumSteps] = {SCALAR_STEPS(X)};
#undef X

// The words of part p, [word][1024], into `sink(word, t, value)`.
template <typename Sink>
void expected_part(int p, uint32_t seed, Sink&& sink) {
  if (p == kSgpr) {
    for (int w = 0; w < kSgprWords; ++w)
      for (uint32_t t = 0; t < kBlock; ++t) sink(w, t, want_sgpr(seed, w, t));
    return;
  }
  if (p == kMovrel) {
    for (int f = 0; f < 4; ++f)
      for (int k = 0; k < movrel_indexes(f); ++k)
        for (int w = 0; w < movrel_words(f); ++w)
          for (uint32_t t = 0; t < kBlock; ++t) sink(movrel_base(f, k) + w, t, want_movrel(seed, f, movrel_index(f, k), w, t));
    return;
  }
  int base = 0;
  for (int g = part_first(p); g < part_first(p + 1); ++g) {
    const StepInfo si = kSteps[g];
    for (uint32_t t = 0; t < kBlock; ++t) {
      const Ops o = operands(seed, p, g - part_first(p), si.bk, t);
      Res r;
      kWant[g](o, r);
      const uint32_t w[6] = {uint32_t(r.d), uint32_t(r.d >> 32), uint32_t(r.e), uint32_t(r.e >> 32), r.scc, r.first};
      if (si.cls == G) {
        for (int q = 0; q < si.nw; ++q) sink(base + q, t, w[q]);
        sink(base + si.nw, t, r.scc);
      } else {
        for (int q = 0; q < si.nw; ++q) sink(base + q, t, w[q]);
      }
    }
    base += step_words(g);
  }
}

uint32_t expected_digest(int p, uint32_t seed) {
  uint32_t d = 0;
  expected_part(p, seed, [&](int w, uint32_t t, uint32_t v) { d += v * (2u * (uint32_t(w) * kBlock + t) + 1u); });
  return d;
}

// The node agent sweeps with one seed again and again: keep the last.
void expected(uint32_t part_mask, uint32_t seed, Expect* e) {
  static std::mutex mu;
  static bool have = false;
  static uint32_t have_seed = 0;
  static uint32_t all[kNumParts];
  std::lock_guard<std::mutex> g(mu);
  if (!have || have_seed != seed) {
    for (int p = 0; p < kNumParts; ++p) all[p] = expected_digest(p, seed);
    have = true;
    have_seed = seed;
  }
  for (int p = 0; p < kNumParts; ++p) e->digest[p] = (part_mask >> p) & 1u ? all[p] : 0u;
}

}  // namespace

extern "C" {

const char* xs_scalar_sweep_last_error() { return g_scalar_err; }

// Part names, comma-separated, in bit order.
const char* xs_scalar_parts() { return kPartNames; }

// out2 = {steps, words per thread}.
int xs_scalar_shape(int part, int* out2) {
  if (part < 0 || part >= kNumParts || !out2) return kBadArgs;
  out2[0] = kShape[part].steps;
  out2[1] = kShape[part].words;
  return 0;
}

// One workgroup runs `part` and stores every word it received: out[word][1024],
// then a row of raw HW_REG_GPR_ALLOC and a row of HW_REG_HW_ID, which are not
// part of the comparison; n_words = (words + 2) x 1024.
int xs_scalar_probe(int dev, int part, uint32_t seed, uint32_t* out, size_t n_words) {
  if (part < 0 || part >= kNumParts || !out) return kBadArgs;
  const uint32_t words = static_cast<uint32_t>(kShape[part].words);
  const size_t n = static_cast<size_t>(words + 2) * kBlock;
  if (n_words != n) return kBadArgs;
  return launch_probe(g_scalar_err, dev, reinterpret_cast<const void*>(k_scalar_probe), kBlock, 0, out, n,
                      [&](dim3 grid, dim3 block, size_t smem, void* dump) {
                        hipLaunchKernelGGL(k_scalar_probe, grid, block, smem, 0,
                                           ProbeArgs{static_cast<uint32_t*>(dump), static_cast<uint32_t>(part), seed,
                                                     words, 0u});
                      });
}

// Host only. out8[p] = the workgroup digest a healthy CU leaves for part p, 0
// for a part outside part_mask.
int xs_scalar_sweep_expected(uint32_t part_mask, uint32_t seed, uint32_t* out8) {
  if (bad_part_mask(part_mask, kAllParts) || !out8) return kBadArgs;
  Expect e;
  expected(part_mask, seed, &e);
  for (int p = 0; p < kNumParts; ++p) out8[p] = e.digest[p];
  return 0;
}

// What the runtime reports for k_scalar_sweep on `dev`: out4 = {registers per
// lane, scratch bytes per lane, dynamic LDS bytes per workgroup, workgroups
// that fit on a CU at once}.
int xs_scalar_sweep_info(int dev, int* out4) {
  if (!out4) return kBadArgs;
  XS_CHECK(hipSetDevice(dev));
  size_t smem = 0;
  if (int rc = exclusive_lds(g_scalar_err, dev, kLdsUsed, &smem)) return rc;
  return kernel_info(g_scalar_err, reinterpret_cast<const void*>(k_scalar_sweep), kBlock, smem, out4);
}

// One sweep launch of `blocks` workgroups (0: 4 per CU). Writes `blocks`
// 128-byte records to records_out. inject_xcd / inject_cu: -1 is none / any,
// values below -1 are refused. Returns 0, -1000 for bad arguments (nothing is
// launched), or a negative HIP error.
int xs_scalar_sweep(int dev, int blocks, uint32_t part_mask, uint32_t seed, int inject_xcd, int inject_cu,
                    uint32_t inject_parts, void* records_out, int* n_records, double* ms) {
  if (bad_part_mask(part_mask, kAllParts) || (inject_parts & ~kAllParts)) return kBadArgs;
  Expect e;
  expected(part_mask, seed, &e);
  return launch_sweep(g_scalar_err, {dev, blocks, inject_xcd, inject_cu, records_out, n_records, ms},
                      reinterpret_cast<const void*>(k_scalar_sweep), kBlock, kLdsUsed, sizeof(ScalarRecord),
                      [&](dim3 grid, dim3 block, size_t smem, void* rec) {
                        hipLaunchKernelGGL(k_scalar_sweep, grid, block, smem, 0,
                                           SweepArgs{static_cast<ScalarRecord*>(rec), part_mask, seed, inject_xcd,
                                                     inject_cu, inject_parts, 0u, e});
                      });
}

}  // extern "C"
