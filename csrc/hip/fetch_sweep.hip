// Fetch sweep for gfx950 (MI355X): the instruction fetch path and the
// instruction cache of every CU.
//
// Every other sweep rests on the CU fetching the instruction bytes the
// compiler wrote, unaltered, and none tests it: their kernels are a few KiB
// run front to back. k_fetch_sweep is a sweep over named parts (part_sweep.h)
// whose test data is its own code.
//
// A step folds a 32-bit literal, a constant inside an instruction's encoding,
// into a per-lane accumulator `acc`. Step j of a run of steps has kind j & 3;
// L is its literal, s = s25, C = s26 = 0x5bd1e995 (set at the head of every asm
// statement), t the thread number in a VGPR:
//   every step   v_alignbit_b32 acc, acc, acc, 27      acc = rotl(acc, 5): order matters
//   kind 0  V    v_xor_b32 acc, L, acc                 VOP2 + literal           16 B
//   kind 1  S    s_xor_b32 s, C, L                     SOP2 + literal
//                v_xor_b32 acc, s, acc                                          20 B
//   kind 2  K    s_addk_i32 s, L[15:0]                 SOPK simm16 (sign-extended), on the s of kind 1
//                v_xor_b32 acc, s, acc                                          16 B
//   kind 3  X    v_xad_u32 acc, acc, C, t              VOP3, no literal: acc = (acc ^ C) + t,
//                                                      so line offsets shift    16 B
// Every step is a bijection of acc, so a difference never dies. A flipped bit b
// of a V literal flips a bit of acc. Of an S literal: it flips bit b of acc,
// and the K step then XORs a run of bits that starts at b (the carry of the
// add) onto a difference rotated to b + 5: not zero. Of a K immediate: acc
// takes that run alone.
// L(r, i) = fmix32(r << 20 | i) | 0x01000100 for step i of region r (fmix32:
// part_sweep.h). The OR keeps L out of the inline constants 0..64 and the float
// ones, so a kind has one size (-16..-1 keep both bits: the tests hold that no
// step's literal is one, and every step to its size); a collision the OR
// creates is accepted (the reference counts the distinct literals of every region). The assembler generates the code,
// inside inline asm, with .rept / .set: fmix32 is six .set lines there.
// The final acc depends on every literal in the order executed, so a wrong bit
// in a fetched literal or a fetch from a wrong address changes it; a wrong bit
// in an opcode dword changes it or traps.
//
// A run of steps that must fill B bytes holds as many steps, in kind order
// from kind 0, as fit, then s_nop 0: 16 B = 1 step, 64 B = 3 steps + 3 nops,
// 1 KiB = 60 + 1, 16 KiB = 963 + 3, a stream segment (8 KiB less its 4-byte
// return) = 481 + 3, a call block (64 B less its return) = 3 + 2.
//
// Regions (r: first step index of each run):
//   0 stream    32 segments; segment s starts at i = 512 s
//   1..4 loop   the 16 B, 64 B, 1 KiB and 16 KiB bodies; i from 0
//   5 call      256 blocks and the extra block (b = 256); block b starts at i = 4 b
//   6 align     17 targets; target k has the one literal i = k
//
// Parts (bit, name), rows of 256 words each (row x 256 + thread is the flat index):
//   0 stream  256 KiB of straight-line steps as 32 callable segments of exactly
//             8 KiB, each ending in s_setpc_b64. Wave w calls all 32, starting
//             at segment 8 w and wrapping, so the four SIMDs fetch from four
//             places at once and every wave fetches every line. 256 KiB is four
//             times the capacity believed of the instruction cache (64 KiB per
//             pair of CUs, 64-byte lines: public CDNA3 material, assumed for
//             CDNA4; see the README for what was measured). Which level served
//             a fetch is not observed. Row k: acc after the wave's k-th call.
//   1 loop    bodies of 16 B, 64 B, 1 KiB and 16 KiB, each under a backward
//             s_cbranch_scc1 that counts an SGPR down from an immediate
//             (2048, 512, 64 and 16 trips). Body b keeps one acc over the
//             rounds. Row b x rounds + r: acc after round r.
//   2 call    256 blocks of 64 B. A round visits each once in the order
//             (a i + b) & 255, a odd: h = fmix32(seed + 0x9e3779b9 (r + 1)),
//             a = (h & 0xff) | 1, b = (h >> 8) & 0xff. v_readfirstlane_b32
//             brings the index to an SGPR; s_getpc_b64 and s_swappc_b64 reach
//             the block, s_setpc_b64 returns. Every visit then reaches the
//             extra block by a direct s_call_b64 and leaves by an s_branch
//             over it. Row r: acc after round r.
//   3 align   32 trampoline blocks of 64 B, reached by the same computed jump,
//             each an s_branch to one of 17 targets: target k < 16 begins at
//             dword k of a 64-byte line with an 8-byte v_xor_b32 acc, L, acc
//             (at k = 15 opcode and literal lie in different lines), target 16
//             begins 4 bytes before a multiple of 4096 from the kernel's
//             symbol, which is aligned to 4096. Then the rotate, then the
//             return. Trampoline j goes to target j (j < 17) or j - 17. Row j.
//   4 refill  one trip of the 16 KiB body (the same bytes as `loop`'s: one
//             statement serves both), then s_icache_inv, 16 s_nop 0 and a
//             taken branch, then one trip again from the same start value: the
//             second must be refetched. Rows 0 and 1 are equal by construction.
// `rounds` multiplies the trips of `loop` and the rounds of `call`.
//
// Start values: fmix32(seed ^ (part << 28 | sub << 16 | thread)), sub = the
// body for `loop`, else 0. The seed cannot enter the literals, which are
// compile-time: it enters the start values and the `call` order.
//
// Safety rules.
//   * The code object is never written: there is no self-modifying code.
//   * A computed jump target is always base + ((index & (N-1)) << log2(block
//     bytes)) over N equal-size aligned blocks, N a power of two; the base is
//     s_getpc_b64 plus a label difference the assembler folds. A wrong operand
//     can only select another valid block.
//   * Every backward branch counts down an SGPR that the same asm statement
//     set from an immediate; no trip count comes from memory or from a hash.
//   * Every statement names what it clobbers (s[20:26], SCC) and writes
//     nothing else; EXEC, M0 and VCC are never written.
//   * The kernel never writes the MODE register, has no scratch and no spill,
//     and its results leave through vector stores only.
//   * No wave waits on another workgroup.
//
// Judging. The device compares digests by integer equality with the host's
// (reduce_parts); it holds no table of expected words, so a record's `bad`
// counts only an injection and the SIMD of a fault is not named. The host
// walks the same region tables in expected_rows(); the independent reference
// is tests/fetch_sweep_ref.py, and tests/test_fetch_codeobject.py holds the
// bytes of the code object to it.
//
// Record (128 bytes per workgroup): part_sweep.h's head with five parts.
// Injection: as in the other part sweeps. blocks == 0 means 4 per CU. The
// sweep allocates nothing but its records.
//
// k_fetch_probe dumps the rows of the selected parts of one workgroup, one
// part after the other in bit order. With the mask 1 << 5 alone it times
// instead: for k = 1..32 it calls segments 0..k-1 once untimed and then
// `rounds` times between two s_memtime reads; row k - 1 holds every thread's
// clocks, for a footprint of 8 k KiB.
//
// NOT covered: which cache level served a fetch; whether every set and way
// was reached; the instruction TLB beyond the one page crossing; s_setprio,
// s_sleep, s_sethalt and the trap handler; code above 256 KiB; a fault that
// only another kernel's code layout would hit (the sweep's own bytes are the
// only ones it proves); the SIMD of a fault; the neighbour CU that shares the
// cache (the record names the CU that ran).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <mutex>
#include <vector>

#include "hip/part_sweep.h"

#define XS_ERR_BUF g_fetch_err
#define XS_HD __host__ __device__ __forceinline__
#define XS_D __device__ __forceinline__

namespace {

using namespace xsprobe;

ErrBuf g_fetch_err = "";

constexpr int kNumParts = 5;
const char kPartNames[] = "stream,loop,call,align,refill";
constexpr uint32_t kAllParts = (1u << kNumParts) - 1;
constexpr uint32_t kClockMask = 1u << kNumParts;  // xs_fetch_probe: the timing mode
constexpr int kBlock = kPartBlock;
constexpr int kStream = 0, kLoop = 1, kCall = 2, kAlign = 3, kRefill = 4;
constexpr uint32_t kMaxRounds = 64;

// Regions and what fills them.
constexpr uint32_t kRegStream = 0, kRegLoop0 = 1, kRegCall = 5, kRegAlign = 6;
constexpr uint32_t kSegments = 32, kSegmentSteps = 481, kSegmentStride = 512;
constexpr uint32_t kLoopSteps[4] = {1, 3, 60, 963};
constexpr uint32_t kLoopTrips[4] = {2048, 512, 64, 16};
constexpr uint32_t kCallBlocks = 256, kBlockSteps = 3, kBlockStride = 4;
constexpr uint32_t kTrampolines = 32, kTargets = 17;

// Rows of a part: fixed + per_round x rounds.
struct Shape {
  uint32_t fixed, per_round;
};
constexpr Shape kShape[kNumParts] = {{kSegments, 0}, {0, 4}, {0, 1}, {kTrampolines, 0}, {2, 0}};
XS_HD constexpr uint32_t part_rows(int p, uint32_t rounds) { return kShape[p].fixed + kShape[p].per_round * rounds; }

XS_HD uint32_t start_value(uint32_t seed, uint32_t part, uint32_t sub, uint32_t t) {
  return fmix32(seed ^ (part << 28 | sub << 16 | t));
}
// The `call` order of round r: block (a i + b) & 255, a odd.
XS_HD uint32_t call_hash(uint32_t seed, uint32_t r) { return fmix32(seed + 0x9e3779b9u * (r + 1u)); }
XS_HD uint32_t call_a(uint32_t h) { return (h & 0xffu) | 1u; }
XS_HD uint32_t call_b(uint32_t h) { return (h >> 8) & 0xffu; }
XS_HD constexpr uint32_t target_of(uint32_t j) { return j < kTargets ? j : j - kTargets; }

constexpr uint32_t kLdsUsed = part_reduction_words(kNumParts, 0) * 4;

struct FetchRecord {
  PartRecordHead<kNumParts> head;
  uint32_t reserved;
  uint32_t pad[16];
};
static_assert(sizeof(FetchRecord) == 128, "one 128-byte record per workgroup");

using Expect = PartExpect<kNumParts>;

// ------------------------------------------------------------------- device
// The assembler's side of a step. A statement defines the macros it uses and
// purges them; xs_i and xs_h are assembler variables, set before every use.
#define XS_STEP_MACROS                                          \
  ".macro xs_lit r\n"                                           \
  ".set xs_h, ((\\r) << 20) | xs_i\n"                           \
  ".set xs_h, (xs_h ^ (xs_h >> 16)) & 0xffffffff\n"             \
  ".set xs_h, (xs_h * 0x85ebca6b) & 0xffffffff\n"               \
  ".set xs_h, (xs_h ^ (xs_h >> 13)) & 0xffffffff\n"             \
  ".set xs_h, (xs_h * 0xc2b2ae35) & 0xffffffff\n"               \
  ".set xs_h, ((xs_h ^ (xs_h >> 16)) | 0x01000100) & 0xffffffff\n" \
  ".endm\n"                                                     \
  ".macro xs_step r, acc, t\n"                                  \
  "xs_lit \\r\n"                                                \
  "v_alignbit_b32 \\acc, \\acc, \\acc, 27\n"                    \
  ".if (xs_i & 3) == 0\n"                                       \
  "v_xor_b32 \\acc, xs_h, \\acc\n"                              \
  ".elseif (xs_i & 3) == 1\n"                                   \
  "s_xor_b32 s25, s26, xs_h\n"                                  \
  "v_xor_b32 \\acc, s25, \\acc\n"                               \
  ".elseif (xs_i & 3) == 2\n"                                   \
  "s_addk_i32 s25, ((xs_h & 0xffff) ^ 0x8000) - 0x8000\n"       \
  "v_xor_b32 \\acc, s25, \\acc\n"                               \
  ".else\n"                                                     \
  "v_xad_u32 \\acc, \\acc, s26, \\t\n"                          \
  ".endif\n"                                                    \
  ".set xs_i, xs_i + 1\n"                                       \
  ".endm\n"                                                     \
  ".macro xs_nops n\n"                                          \
  ".rept \\n\n"                                                 \
  "s_nop 0\n"                                                   \
  ".endr\n"                                                     \
  ".endm\n"
#define XS_PURGE ".purgem xs_lit\n.purgem xs_step\n.purgem xs_nops\n"
// The compiler sizes a statement by its lines, which .rept hides from it; its
// branches across a statement must reach. It does read a .space, so every
// statement opens with one the assembler skips, of at least the statement's bytes.
#define XS_SIZE(BYTES) ".if 0\n.space " #BYTES "\n.endif\n"
#define XS_CLOBBER "s20", "s21", "s22", "s23", "s24", "s25", "s26", "scc"

// s[20:21] = base + ((index & (N-1)) << SHIFT), then the call. `A` is the
// label behind s_getpc_b64, `BASE` that of block 0.
#define XS_HEAD "s_mov_b32 s25, 0\ns_mov_b32 s26, 0x5bd1e995\n"
#define XS_JUMP(INDEX, N, SHIFT, A, BASE)         \
  XS_HEAD                                         \
  "s_getpc_b64 s[20:21]\n" A ":\n"                \
  "s_and_b32 s24, " INDEX ", " #N " - 1\n"        \
  "s_lshl_b32 s24, s24, " #SHIFT "\n"             \
  "s_add_u32 s20, s20, s24\n"                     \
  "s_addc_u32 s21, s21, 0\n"                      \
  "s_add_u32 s20, s20, " BASE " - " A "\n"        \
  "s_addc_u32 s21, s21, 0\n"                      \
  "s_swappc_b64 s[22:23], s[20:21]\n"

// One call of stream segment `seg` (uniform).
XS_D uint32_t call_segment(uint32_t acc, uint32_t t, uint32_t seg) {
  asm volatile(XS_STEP_MACROS
               XS_SIZE(266400)
               XS_JUMP("%[seg]", 32, 13, "xs_fetch_stream_pc_%=", "xs_fetch_stream_%=")
               // the end is beyond an s_branch's reach: a jump by a folded constant
               "s_getpc_b64 s[20:21]\n"
               "xs_fetch_stream_out_%=:\n"
               "s_add_u32 s20, s20, xs_fetch_stream_end_%= - xs_fetch_stream_out_%=\n"
               "s_addc_u32 s21, s21, 0\n"
               "s_setpc_b64 s[20:21]\n"
               ".p2align 12\n"
               "xs_fetch_stream_%=:\n"
               ".set xs_s, 0\n"
               ".rept 32\n"
               ".set xs_i, xs_s * 512\n"
               ".rept 481\n"
               "xs_step 0, %[acc], %[t]\n"
               ".endr\n"
               "xs_nops 3\n"
               "s_setpc_b64 s[22:23]\n"
               ".set xs_s, xs_s + 1\n"
               ".endr\n"
               "xs_fetch_stream_end_%=:\n"
               XS_PURGE
               : [acc] "+v"(acc)
               : [seg] "s"(seg), [t] "v"(t)
               : XS_CLOBBER);
  return acc;
}

// TRIPS trips of loop body B (region 1 + B): STEPS steps and NOPS s_nop 0.
#define XS_LOOP(B, STEPS, NOPS, TRIPS)                 \
  asm volatile(XS_STEP_MACROS                          \
               XS_SIZE(1280)                           \
               XS_HEAD                                 \
               "s_movk_i32 s24, " #TRIPS "\n"          \
               ".p2align 6\n"                          \
               "xs_fetch_loop" #B "_%=:\n"             \
               ".set xs_i, 0\n"                        \
               ".rept " #STEPS "\n"                    \
               "xs_step 1 + " #B ", %[acc], %[t]\n"       \
               ".endr\n"                               \
               "xs_nops " #NOPS "\n"                   \
               "xs_fetch_loop" #B "_end_%=:\n"         \
               "s_sub_u32 s24, s24, 1\n"               \
               "s_cmp_lg_u32 s24, 0\n"                 \
               "s_cbranch_scc1 xs_fetch_loop" #B "_%=\n" \
               XS_PURGE                                \
               : [acc] "+v"(acc)                       \
               : [t] "v"(c.t)                          \
               : XS_CLOBBER)

// The 16 KiB body: 16 trips, or one when `once` (uniform) is not 0. Both
// counts are immediates of this statement.
XS_D uint32_t loop_16k(uint32_t acc, uint32_t t, uint32_t once) {
  asm volatile(XS_STEP_MACROS
               XS_SIZE(16640)
               XS_HEAD
               "s_movk_i32 s24, 16\n"
               "s_cmp_eq_u32 %[once], 0\n"
               "s_cbranch_scc1 xs_fetch_loop3_%=\n"
               "s_movk_i32 s24, 1\n"
               ".p2align 6\n"
               "xs_fetch_loop3_%=:\n"
               ".set xs_i, 0\n"
               ".rept 963\n"
               "xs_step 4, %[acc], %[t]\n"
               ".endr\n"
               "xs_nops 3\n"
               "xs_fetch_loop3_end_%=:\n"
               "s_sub_u32 s24, s24, 1\n"
               "s_cmp_lg_u32 s24, 0\n"
               "s_cbranch_scc1 xs_fetch_loop3_%=\n"
               XS_PURGE
               : [acc] "+v"(acc)
               : [once] "s"(once), [t] "v"(t)
               : XS_CLOBBER);
  return acc;
}

// One visit: block `blk` (uniform) by the computed jump, the extra block by s_call_b64.
XS_D uint32_t call_block(uint32_t acc, uint32_t t, uint32_t blk) {
  asm volatile(XS_STEP_MACROS
               XS_SIZE(16896)
               XS_JUMP("%[blk]", 256, 6, "xs_fetch_call_pc_%=", "xs_fetch_call_%=")
               "s_call_b64 s[22:23], xs_fetch_extra_%=\n"
               "s_branch xs_fetch_call_end_%=\n"
               ".p2align 6\n"
               "xs_fetch_extra_%=:\n"
               ".set xs_i, 4 * 256\n"
               ".rept 3\n"
               "xs_step 5, %[acc], %[t]\n"
               ".endr\n"
               "xs_nops 2\n"
               "s_setpc_b64 s[22:23]\n"
               ".p2align 6\n"
               "xs_fetch_call_%=:\n"
               ".set xs_s, 0\n"
               ".rept 256\n"
               ".set xs_i, 4 * xs_s\n"
               ".rept 3\n"
               "xs_step 5, %[acc], %[t]\n"
               ".endr\n"
               "xs_nops 2\n"
               "s_setpc_b64 s[22:23]\n"
               ".set xs_s, xs_s + 1\n"
               ".endr\n"
               "xs_fetch_call_end_%=:\n"
               XS_PURGE
               : [acc] "+v"(acc)
               : [blk] "s"(blk), [t] "v"(t)
               : XS_CLOBBER);
  return acc;
}

// A trampoline block and target K < 16 (xs_i == K there).
#define XS_TRAMP(K) "s_branch xs_fetch_t" #K "_%=\n.p2align 6\n"
#define XS_TRAMP15 \
  XS_TRAMP(0) XS_TRAMP(1) XS_TRAMP(2) XS_TRAMP(3) XS_TRAMP(4) XS_TRAMP(5) XS_TRAMP(6) XS_TRAMP(7) XS_TRAMP(8) \
  XS_TRAMP(9) XS_TRAMP(10) XS_TRAMP(11) XS_TRAMP(12) XS_TRAMP(13) XS_TRAMP(14)
#define XS_TARGET(K) "xs_nops " #K "\nxs_fetch_t" #K "_%=:\nxs_target\n.p2align 7\n"

// One visit of trampoline `j` (uniform) and the target it branches to.
XS_D uint32_t call_target(uint32_t acc, uint32_t j) {
  asm volatile(XS_STEP_MACROS
               ".macro xs_target\n"
               "xs_lit 6\n"
               "v_xor_b32 %[acc], xs_h, %[acc]\n"
               "v_alignbit_b32 %[acc], %[acc], %[acc], 27\n"
               "s_setpc_b64 s[22:23]\n"
               ".set xs_i, xs_i + 1\n"
               ".endm\n"
               XS_SIZE(16384)
               XS_JUMP("%[j]", 32, 6, "xs_fetch_align_pc_%=", "xs_fetch_tramp_%=")
               "s_branch xs_fetch_align_end_%=\n"
               ".p2align 6\n"
               "xs_fetch_tramp_%=:\n"
               XS_TRAMP15 XS_TRAMP(15) XS_TRAMP(16) XS_TRAMP15
               // targets 0..15: 128 bytes apart, target k at dword k of its first line
               ".p2align 7\n"
               ".set xs_i, 0\n"
               XS_TARGET(0) XS_TARGET(1) XS_TARGET(2) XS_TARGET(3) XS_TARGET(4) XS_TARGET(5) XS_TARGET(6) XS_TARGET(7)
               XS_TARGET(8) XS_TARGET(9) XS_TARGET(10) XS_TARGET(11) XS_TARGET(12) XS_TARGET(13) XS_TARGET(14)
               XS_TARGET(15)
               // target 16: its opcode dword ends a 4 KiB page of the kernel, its literal begins the next
               ".p2align 12\n"
               "xs_nops 1023\n"
               "xs_fetch_t16_%=:\n"
               "xs_target\n"
               "xs_fetch_align_end_%=:\n"
               ".purgem xs_target\n"
               XS_PURGE
               : [acc] "+v"(acc)
               : [j] "s"(j)
               : XS_CLOBBER);
  return acc;
}

struct Ctx {
  uint32_t seed, t, rounds, inj;
  uint32_t* dump;            // k_fetch_probe only
  uint32_t off[kNumParts];   // word offset of a part's rows in the dump
};

XS_D void take_at(const Ctx& c, Tally& y, uint32_t off, bool injected, uint32_t row, uint32_t got) {
  take_word(y, c.dump ? c.dump + off : nullptr, row * kBlock + c.t, got, got, injected);
}
template <int PART>
XS_D void take(const Ctx& c, Tally& y, uint32_t row, uint32_t got) {
  take_at(c, y, c.off[PART], (c.inj >> PART) & 1u, row, got);
}
XS_D uint32_t uniform(uint32_t v) { return __builtin_amdgcn_readfirstlane(v); }

// clock_reps 0: the part. Otherwise the timing mode of k_fetch_probe; the
// segment statement is one, so its bytes are the part's.
XS_D void run_stream(const Ctx& c, Tally& y, uint32_t clock_reps) {
  uint32_t acc = start_value(c.seed, kStream, 0, c.t);
#pragma nounroll
  for (uint32_t span = clock_reps ? 1u : kSegments; span <= kSegments; ++span) {
    const uint32_t calls = clock_reps ? (clock_reps + 1u) * span : kSegments;
    uint32_t seg = clock_reps ? 0u : (8u * (c.t >> 6)) & (kSegments - 1u);
    uint64_t t0 = 0;
#pragma nounroll
    for (uint32_t k = 0; k < calls; ++k) {
      if (clock_reps && k == span) t0 = clock64();
      acc = call_segment(acc, c.t, uniform(seg));
      if (!clock_reps) take<kStream>(c, y, k, acc);
      seg = seg + 1u == span ? 0u : seg + 1u;
    }
    if (clock_reps) c.dump[(span - 1u) * kBlock + c.t] = static_cast<uint32_t>(clock64() - t0);
  }
}

XS_D void run_small_loops(const Ctx& c, Tally& y) {
  uint32_t acc = start_value(c.seed, kLoop, 0, c.t);
#pragma nounroll
  for (uint32_t r = 0; r < c.rounds; ++r) {
    XS_LOOP(0, 1, 0, 2048);
    take<kLoop>(c, y, r, acc);
  }
  acc = start_value(c.seed, kLoop, 1, c.t);
#pragma nounroll
  for (uint32_t r = 0; r < c.rounds; ++r) {
    XS_LOOP(1, 3, 3, 512);
    take<kLoop>(c, y, c.rounds + r, acc);
  }
  acc = start_value(c.seed, kLoop, 2, c.t);
#pragma nounroll
  for (uint32_t r = 0; r < c.rounds; ++r) {
    XS_LOOP(2, 60, 1, 64);
    take<kLoop>(c, y, 2u * c.rounds + r, acc);
  }
}

// The 16 KiB body serves `loop` (job 0) and the two passes of `refill` (jobs
// 1 and 2) from one statement, so from one copy of its bytes.
XS_D void run_16k(const Ctx& c, uint32_t mask, Tally& loop, Tally& refill) {
#pragma nounroll
  for (uint32_t job = 0; job < 3; ++job) {
    const bool is_loop = job == 0;
    if (!((mask >> (is_loop ? kLoop : kRefill)) & 1u)) continue;
    if (job == 2)
      asm volatile("s_icache_inv\n"
                   ".rept 16\n"
                   "s_nop 0\n"
                   ".endr\n"
                   "s_branch xs_fetch_inv_%=\n"
                   "s_nop 0\n"
                   "xs_fetch_inv_%=:\n" ::
                       : "memory");
    uint32_t acc = start_value(c.seed, is_loop ? kLoop : kRefill, is_loop ? 3u : 0u, c.t);
    const uint32_t n = is_loop ? c.rounds : 1u;
    const uint32_t off = is_loop ? c.off[kLoop] : c.off[kRefill];
    const bool injected = (c.inj >> (is_loop ? kLoop : kRefill)) & 1u;
    Tally y;
#pragma nounroll
    for (uint32_t r = 0; r < n; ++r) {
      acc = loop_16k(acc, c.t, uniform(is_loop ? 0u : 1u));
      take_at(c, y, off, injected, is_loop ? 3u * c.rounds + r : job - 1u, acc);
    }
    if (is_loop)
      loop.bad += y.bad, loop.digest += y.digest;
    else
      refill.bad += y.bad, refill.digest += y.digest;
  }
}

XS_D void run_call(const Ctx& c, Tally& y) {
  uint32_t acc = start_value(c.seed, kCall, 0, c.t);
#pragma nounroll
  for (uint32_t r = 0; r < c.rounds; ++r) {
    const uint32_t h = call_hash(c.seed, r), a = call_a(h), b = call_b(h);
#pragma nounroll
    for (uint32_t i = 0; i < kCallBlocks; ++i) acc = call_block(acc, c.t, uniform((a * i + b) & (kCallBlocks - 1u)));
    take<kCall>(c, y, r, acc);
  }
}

XS_D void run_align(const Ctx& c, Tally& y) {
  uint32_t acc = start_value(c.seed, kAlign, 0, c.t);
#pragma nounroll
  for (uint32_t j = 0; j < kTrampolines; ++j) {
    acc = call_target(acc, uniform(j));
    take<kAlign>(c, y, j, acc);
  }
}

// clock_reps: as run_stream's. One call of it serves the part and the timing
// mode, so a kernel holds the segments once.
XS_D void run_parts(const Ctx& c, uint32_t mask, uint32_t clock_reps, Tally (&y)[kNumParts]) {
  if ((mask & (1u << kStream)) || clock_reps) run_stream(c, y[kStream], clock_reps);
  if (mask & (1u << kLoop)) run_small_loops(c, y[kLoop]);
  if (mask & (1u << kCall)) run_call(c, y[kCall]);
  if (mask & (1u << kAlign)) run_align(c, y[kAlign]);
  run_16k(c, mask, y[kLoop], y[kRefill]);
}

// aligned(4096): `align`'s page crossing is placed from the kernel's symbol.
__global__ __launch_bounds__(kBlock) __attribute__((aligned(4096))) void k_fetch_sweep(
    FetchRecord* __restrict__ records, uint32_t part_mask, uint32_t seed, uint32_t rounds, int inject_xcd,
    int inject_cu, uint32_t inject_parts, Expect expect) {
  extern __shared__ uint32_t fetch_lds[];
  const uint32_t t = threadIdx.x;
  const uint32_t xcd = xcc_id();
  const uint32_t hw = hw_id();
  const uint32_t cu = cu_key(hw);
  const uint32_t simd = simd_id(hw);
  const bool inject = inject_selected(inject_xcd, inject_cu, xcd, cu);
  const Ctx c{seed, t, rounds, inject ? inject_parts : 0u, nullptr, {}};

  Tally y[kNumParts];
  run_parts(c, part_mask, 0, y);

  reduce_parts<kNumParts, 0>(fetch_lds, t, simd, y, nullptr, part_mask, expect, xcd, cu, &records[blockIdx.x]);
}

struct Offsets {
  uint32_t off[kNumParts];
};

// One workgroup. part_mask within kAllParts: dump holds the rows of the
// selected parts at `at`. part_mask == kClockMask: dump holds 32 rows of clocks
// and `rounds` is the timed repeats.
__global__ __launch_bounds__(kBlock) __attribute__((aligned(4096))) void k_fetch_probe(
    uint32_t* __restrict__ dump, uint32_t part_mask, uint32_t seed, uint32_t rounds, Offsets at) {
  Ctx c{seed, threadIdx.x, rounds, 0u, dump, {}};
  for (int p = 0; p < kNumParts; ++p) c.off[p] = at.off[p];
  Tally y[kNumParts];
  run_parts(c, part_mask, part_mask == kClockMask ? rounds : 0u, y);
}

// --------------------------------------------------------------------- host
uint32_t literal(uint32_t region, uint32_t i) { return fmix32(region << 20 | i) | 0x01000100u; }

constexpr uint32_t kC = 0x5bd1e995u;  // s26

// A lane, its thread number and the s25 of its wave.
struct Lane {
  uint32_t acc, t, s;
  void step(uint32_t region, uint32_t i) {
    const uint32_t l = literal(region, i);
    acc = rotl32(acc, 5);
    switch (i & 3u) {
      case 0: acc ^= l; break;
      case 1: s = kC ^ l, acc ^= s; break;
      case 2: s += static_cast<uint32_t>(static_cast<int32_t>(static_cast<int16_t>(l & 0xffffu))), acc ^= s; break;
      default: acc = (acc ^ kC) + t; break;
    }
  }
  void run(uint32_t region, uint32_t first, uint32_t steps) {
    for (uint32_t j = 0; j < steps; ++j) step(region, first + j);
  }
};

// out[row][256] of part p.
void expected_rows(int p, uint32_t seed, uint32_t rounds, uint32_t* out) {
  for (uint32_t t = 0; t < kBlock; ++t) {
    auto put = [&](uint32_t row, uint32_t v) { out[row * kBlock + t] = v; };
    Lane l{start_value(seed, p, 0, t), t, 0};
    switch (p) {
      case kStream:
        for (uint32_t k = 0; k < kSegments; ++k) {
          const uint32_t seg = (8u * (t >> 6) + k) & (kSegments - 1u);
          l.run(kRegStream, seg * kSegmentStride, kSegmentSteps);
          put(k, l.acc);
        }
        break;
      case kLoop:
        for (uint32_t b = 0; b < 4; ++b) {
          l.acc = start_value(seed, kLoop, b, t);
          for (uint32_t r = 0; r < rounds; ++r) {
              for (uint32_t trip = 0; trip < kLoopTrips[b]; ++trip) l.run(kRegLoop0 + b, 0, kLoopSteps[b]);
            put(b * rounds + r, l.acc);
          }
        }
        break;
      case kCall:
        for (uint32_t r = 0; r < rounds; ++r) {
          const uint32_t h = call_hash(seed, r), a = call_a(h), b = call_b(h);
          for (uint32_t i = 0; i < kCallBlocks; ++i) {
              l.run(kRegCall, kBlockStride * ((a * i + b) & (kCallBlocks - 1u)), kBlockSteps);
            l.run(kRegCall, kBlockStride * kCallBlocks, kBlockSteps);
          }
          put(r, l.acc);
        }
        break;
      case kAlign:
        for (uint32_t j = 0; j < kTrampolines; ++j) {
          l.acc = rotl32(l.acc ^ literal(kRegAlign, target_of(j)), 5);
          put(j, l.acc);
        }
        break;
      default:
        l.run(kRegLoop0 + 3, 0, kLoopSteps[3]);
        put(0, l.acc);
        put(1, l.acc);
        break;
    }
  }
}

uint32_t digest_of(const uint32_t* v, size_t n) {
  uint32_t d = 0;
  for (size_t i = 0; i < n; ++i) d += v[i] * (2u * static_cast<uint32_t>(i) + 1u);
  return d;
}

bool bad_rounds(uint32_t r) { return r < 1 || r > kMaxRounds; }

// The node agent sweeps with one seed and round count again and again: keep the last digests.
std::mutex g_digest_mu;
uint32_t g_seed = 0, g_rounds = 0, g_have = 0, g_digest[kNumParts];

void expected_digests(uint32_t mask, uint32_t seed, uint32_t rounds, uint32_t* out) {
  std::lock_guard<std::mutex> g(g_digest_mu);
  if (g_seed != seed || g_rounds != rounds) g_have = 0, g_seed = seed, g_rounds = rounds;
  std::vector<uint32_t> rows;
  for (int p = 0; p < kNumParts; ++p) {
    out[p] = 0;
    if (!((mask >> p) & 1u)) continue;
    if (!((g_have >> p) & 1u)) {
      rows.assign(static_cast<size_t>(part_rows(p, rounds)) * kBlock, 0u);
      expected_rows(p, seed, rounds, rows.data());
      g_digest[p] = digest_of(rows.data(), rows.size());
      g_have |= 1u << p;
    }
    out[p] = g_digest[p];
  }
}

}  // namespace

extern "C" {

const char* xs_fetch_sweep_last_error() { return g_fetch_err; }

// Part names, comma-separated, in bit order.
const char* xs_fetch_parts() { return kPartNames; }

// out2 = {rows whatever the rounds, rows per round}: a part hands over
// out2[0] + out2[1] x rounds rows of 256 words.
int xs_fetch_shape(int part, int* out2) {
  if (part < 0 || part >= kNumParts || !out2) return kBadArgs;
  out2[0] = static_cast<int>(kShape[part].fixed);
  out2[1] = static_cast<int>(kShape[part].per_round);
  return 0;
}

// One workgroup runs the parts of part_mask and stores every word, one part's
// rows [row][256] after the other in bit order; n_words is their sum. With
// part_mask == 1 << 5 it times instead (see the head of this file): `rounds`
// timed repeats, out = [32][256] clocks.
int xs_fetch_probe(int dev, uint32_t part_mask, uint32_t seed, uint32_t rounds, uint32_t* out, size_t n_words) {
  const bool clocks = part_mask == kClockMask;
  if ((!clocks && bad_part_mask(part_mask, kAllParts)) || !out || bad_rounds(rounds)) return kBadArgs;
  Offsets at{};
  size_t n = clocks ? static_cast<size_t>(kSegments) * kBlock : 0;
  if (!clocks)
    for (int p = 0; p < kNumParts; ++p) {
      at.off[p] = static_cast<uint32_t>(n);
      if ((part_mask >> p) & 1u) n += static_cast<size_t>(part_rows(p, rounds)) * kBlock;
    }
  if (n_words != n) return kBadArgs;
  return launch_probe(g_fetch_err, dev, reinterpret_cast<const void*>(k_fetch_probe), kBlock, 0, out, n,
                      [&](dim3 grid, dim3 block, size_t smem, void* dump) {
                        hipLaunchKernelGGL(k_fetch_probe, grid, block, smem, 0, static_cast<uint32_t*>(dump),
                                           part_mask, seed, rounds, at);
                      });
}

// Host only. out5[p] = the workgroup digest a healthy CU leaves for part p, 0
// for a part outside part_mask.
int xs_fetch_sweep_expected(uint32_t part_mask, uint32_t seed, uint32_t rounds, uint32_t* out5) {
  if (bad_part_mask(part_mask, kAllParts) || bad_rounds(rounds) || !out5) return kBadArgs;
  expected_digests(part_mask, seed, rounds, out5);
  return 0;
}

// What the runtime reports for k_fetch_sweep on `dev`: out4 = {registers per
// lane, scratch bytes per lane, dynamic LDS bytes per workgroup, workgroups
// that fit on a CU at once}.
int xs_fetch_sweep_info(int dev, int* out4) {
  return sweep_info(g_fetch_err, dev, reinterpret_cast<const void*>(k_fetch_sweep), kBlock, true, out4);
}

// One sweep launch of `blocks` workgroups (0: 4 per CU). Writes `blocks`
// 128-byte records to records_out. inject_xcd / inject_cu: -1 is none / any,
// values below -1 are refused. Returns 0, -1000 for bad arguments (nothing is
// launched), or a negative HIP error.
int xs_fetch_sweep(int dev, int blocks, uint32_t part_mask, uint32_t seed, uint32_t rounds, int inject_xcd,
                   int inject_cu, uint32_t inject_parts, void* records_out, int* n_records, double* ms) {
  if (bad_part_mask(part_mask, kAllParts) || bad_rounds(rounds) || (inject_parts & ~kAllParts)) return kBadArgs;
  Expect e;
  expected_digests(part_mask, seed, rounds, e.digest);
  return launch_sweep(g_fetch_err, {dev, blocks, inject_xcd, inject_cu, records_out, n_records, ms},
                      reinterpret_cast<const void*>(k_fetch_sweep), kBlock, kLdsUsed, sizeof(FetchRecord),
                      [&](dim3 grid, dim3 block, size_t smem, void* rec) {
                        hipLaunchKernelGGL(k_fetch_sweep, grid, block, smem, 0, static_cast<FetchRecord*>(rec),
                                           part_mask, seed, rounds, inject_xcd, inject_cu, inject_parts, e);
                      });
}

}  // extern "C"

