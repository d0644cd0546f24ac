// Register-file sweep for gfx950 (MI355X): every cell of every SIMD's unified
// VGPR/AGPR file, written and read back in both polarities.
//
// The file is 512 entries x 64 lanes x 4 B = 128 KiB per SIMD (MI355X_MICROARCH,
// "Register files"). k_regfile_sweep is one launch of 256-thread workgroups
// (4 waves: one per SIMD) compiled to 256 VGPRs + 256 AGPRs per lane, so a
// wave is allocated the whole file of its SIMD: every physical row is reached
// whatever the allocator's base, and no second sweep workgroup fits on the CU.
// A grid of 4 x CUs reaches every CU of an idle device. Every workgroup is
// self-contained (no waiting on another workgroup, no spinning on memory, no
// inter-workgroup atomics) and records where it ran.
//
// Cells and pattern. Cell r = 0..511 of a wave: r < 256 is v[r], r >= 256 is
// a[r-256]. With c(r) = (((r+1) * 0x9E3779B1) mod 2^32) ^ seed, pass 0 writes
// p0(r,l) = c(r) * (2l+1) mod 2^32 into lane l and pass 1 writes ~p0. For the
// seeds in use all 32,768 cells of a wave hold distinct values, so a register
// that reads back another register's or another lane's data mis-compares.
//
// The hot path is ONE asm statement per wave that names its registers
// literally (C++ arrays give no say over which physical registers are touched,
// and they spill). In each pass every register under test is written first and
// only then is every one read back, so a cell holds its value while all the
// others are written. The statement uses VALU, v_accvgpr_read/write and SALU
// compare/select only: no MFMA, no memory operation. The one branch in it
// steps over the poison sequence below, which no production sweep executes.
//
// Scratch and phases. Eight registers are scratch: s+0 the lane multiplier
// 2l+1, s+1 and s+2 temporaries, s+3 the mis-compare counts (VGPR cells in bits
// 15:0, AGPR cells in bits 31:16), s+4 `first`, s+5 `flip`, s+6 and s+7 the
// digests of pass 0 and pass 1. The scratch set is itself swept:
//   phase A  scratch v0..v7,  tests v8..v255 and a0..a255, pass 0 then pass 1;
//   (v0..v7 are copied to v8..v15)
//   phase B  scratch v8..v15, tests v0..v7,                pass 0 then pass 1.
//
// Per-lane accumulators, reduced over the wave in C++ after the statement:
// bad_vgpr / bad_agpr count the (cell, lane) pairs that mis-compared over both
// passes; first = lowest r that mis-compared, 0xffff if none; flip = OR of
// got ^ expected; D_s = sum_{r,l} got_s(r,l) * (2(64r+l)+1) mod 2^32 over the
// value READ from the register. Wave digest D_0 ^ rotl(D_1, 16); workgroup
// digest sum_w D_w << w (15 D on a healthy CU), compared on the device with
// expect_digest; a digest mismatch with no cell mismatch sets both fail bits.
//
// Record (64 bytes per workgroup, vector stores): xcd, cu, simd_mask, fail
// (bit 0: a VGPR cell, bit 1: an AGPR cell), bad_vgpr, bad_agpr, first, flip,
// digest, bad_simds (SIMD ids whose wave mis-compared), six reserved words.
// xcd is HW_REG_XCC_ID, cu is bits [15:8] of HW_REG_HW_ID (SE, SH and CU id),
// as in cu_sweep.hip.
//
// Injection (testing the comparator and the localisation on a healthy GPU): a
// workgroup on inject_xcd whose CU key is inject_cu (or any, with -1) XORs
// 1 << inject_bit, in pass 0, in every lane of every wave, into the value read
// back from cell inject_reg. Registers only: no access changes. Its record
// shows bad_vgpr + bad_agpr == 256, first == inject_reg, flip == 1 << inject_bit.
//
// Poison (an independent address path; VGPR half only). The write loop and the
// read loop draw r from the same assembler symbol, so a loop that skipped or
// mislabelled a register would still pass the digest. The selected workgroup
// therefore can complement physical VGPR poison_reg (0..255) between pass 0's
// write phase and read phase through the hardware's index mode
// (s_set_gpr_idx_on <sgpr>, gpr_idx(SRC0,DST); v_not_b32 v0, v0;
// s_set_gpr_idx_off; M0 saved and restored in the statement), in the phase
// where that register is under test. The straight-line read-back must then
// name exactly r == poison_reg with 64 bad cells per wave.
//
// NOT covered: the SGPR file (one wave cannot own it), the caches, and any
// register-file row beyond 512 entries per lane per SIMD: coverage rests on
// the file being exactly that size.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>

#include "hip/sweep_common.h"

#define XS_ERR_BUF g_regfile_err

namespace {

xsprobe::ErrBuf g_regfile_err;

using namespace xsprobe;

constexpr int kBlock = 256;  // 4 waves: one per SIMD
constexpr int kCells = 512;  // VGPR + AGPR entries per lane
constexpr uint32_t kNone = 0xffffffffu;

enum : uint32_t { kFailVgpr = 1, kFailAgpr = 2 };

struct RegfileRecord {
  uint32_t xcd, cu, simd_mask, fail;
  uint32_t bad_vgpr, bad_agpr, first, flip;
  uint32_t digest, bad_simds, reserved[6];
};
static_assert(sizeof(RegfileRecord) == 64, "one 64-byte record per workgroup");

// ---- the text of the statement ---------------------------------------------
// Assembler symbols: xs_s = first scratch register of the phase, xs_n = the
// register under test (index into v[] or a[]). R is the cell number as text.

// s+1 <- p0(R, lane)
#define XS_EXPECT(R)                                                  \
  "v_mov_b32 v[xs_s+1], ((" R "+1)*0x9e3779b1)&0xffffffff\n"          \
  "v_xor_b32 v[xs_s+1], %[seed], v[xs_s+1]\n"                         \
  "v_mul_lo_u32 v[xs_s+1], v[xs_s+1], v[xs_s]\n"

#define XS_NOT_0
#define XS_NOT_1 "v_not_b32 v[xs_s+1], v[xs_s+1]\n"

#define XS_WRITE_V(P) XS_EXPECT("xs_n") XS_NOT_##P "v_mov_b32 v[xs_n], v[xs_s+1]\n"
#define XS_WRITE_A(P) XS_EXPECT("xs_n+256") XS_NOT_##P "v_accvgpr_write_b32 a[xs_n], v[xs_s+1]\n"

// s+2 <- the cell, in pass 0 with the injected bit where R is inject_reg.
#define XS_INJECT(R)                         \
  "s_cmp_eq_u32 %[injreg], " R "\n"          \
  "s_cselect_b32 %[tmp], %[injmask], 0\n"    \
  "s_nop 0\n"                                \
  "v_xor_b32 v[xs_s+2], %[tmp], v[xs_s+2]\n"
#define XS_GOT_V_0 "v_mov_b32 v[xs_s+2], v[xs_n]\n" XS_INJECT("xs_n")
#define XS_GOT_V_1 "v_mov_b32 v[xs_s+2], v[xs_n]\n"
#define XS_GOT_A_0 "v_accvgpr_read_b32 v[xs_s+2], a[xs_n]\n" XS_INJECT("xs_n+256")
#define XS_GOT_A_1 "v_accvgpr_read_b32 v[xs_s+2], a[xs_n]\n"

// Digest of pass P from the value read, then compare: INC is added to s+3 per
// mis-compared lane (1 for a VGPR cell, 0x10000 for an AGPR cell).
#define XS_CHECK_CELL(R, P, INC)                                       \
  "v_add_u32 v[xs_s+1], 128*(" R "), v[xs_s]\n"                        \
  "v_mul_lo_u32 v[xs_s+1], v[xs_s+1], v[xs_s+2]\n"                     \
  "v_add_u32 v[xs_s+6+" #P "], v[xs_s+6+" #P "], v[xs_s+1]\n"          \
  XS_EXPECT(R) XS_NOT_##P                                              \
  "v_xor_b32 v[xs_s+1], v[xs_s+1], v[xs_s+2]\n"                        \
  "v_or_b32 v[xs_s+5], v[xs_s+5], v[xs_s+1]\n"                         \
  "v_cmp_ne_u32 vcc, 0, v[xs_s+1]\n"                                   \
  "v_min_u32 v[xs_s+2], " R ", v[xs_s+4]\n"                            \
  "v_cndmask_b32 v[xs_s+4], v[xs_s+4], v[xs_s+2], vcc\n"               \
  "v_mov_b32 v[xs_s+2], " #INC "\n"                                    \
  "v_cndmask_b32 v[xs_s+2], 0, v[xs_s+2], vcc\n"                       \
  "v_add_u32 v[xs_s+3], v[xs_s+3], v[xs_s+2]\n"

#define XS_READ_V(P) XS_GOT_V_##P XS_CHECK_CELL("xs_n", P, 1)
#define XS_READ_A(P) XS_GOT_A_##P XS_CHECK_CELL("xs_n+256", P, 0x10000)

// BODY once for each of COUNT registers from FIRST on.
#define XS_LOOP(FIRST, COUNT, BODY) \
  ".set xs_n, " #FIRST "\n.rept " #COUNT "\n" BODY ".set xs_n, xs_n+1\n.endr\n"

// Complement v[SREG] through the index mode unless SREG is -1.
#define XS_POISON(SREG)                            \
  "s_cmp_lg_u32 " SREG ", -1\n"                    \
  "s_cbranch_scc0 1f\n"                            \
  "s_mov_b32 %[keep], m0\n"                        \
  "s_nop 0\n"                                      \
  "s_set_gpr_idx_on " SREG ", gpr_idx(SRC0,DST)\n" \
  "s_nop 1\n"                                      \
  "v_not_b32 v0, v0\n"                             \
  "s_nop 1\n"                                      \
  "s_set_gpr_idx_off\n"                            \
  "s_mov_b32 m0, %[keep]\n"                        \
  "s_nop 0\n"                                      \
  "1:\n"

// Clobber lists: every VGPR and AGPR but the five outputs v11..v15.
#define XS_R10(f, d) f #d "0", f #d "1", f #d "2", f #d "3", f #d "4", f #d "5", f #d "6", f #d "7", f #d "8", f #d "9"
#define XS_R100(f, h)                                                                                      \
  XS_R10(f, h##0), XS_R10(f, h##1), XS_R10(f, h##2), XS_R10(f, h##3), XS_R10(f, h##4), XS_R10(f, h##5),    \
      XS_R10(f, h##6), XS_R10(f, h##7), XS_R10(f, h##8), XS_R10(f, h##9)
#define XS_R20_255(f)                                                                                       \
  XS_R10(f, 2), XS_R10(f, 3), XS_R10(f, 4), XS_R10(f, 5), XS_R10(f, 6), XS_R10(f, 7), XS_R10(f, 8),         \
      XS_R10(f, 9), XS_R100(f, 1), XS_R10(f, 20), XS_R10(f, 21), XS_R10(f, 22), XS_R10(f, 23), XS_R10(f, 24), \
      f "250", f "251", f "252", f "253", f "254", f "255"
#define XS_CLOBBER_V \
  "v0", "v1", "v2", "v3", "v4", "v5", "v6", "v7", "v8", "v9", "v10", "v16", "v17", "v18", "v19", XS_R20_255("v")
#define XS_CLOBBER_A \
  "a0", "a1", "a2", "a3", "a4", "a5", "a6", "a7", "a8", "a9", XS_R10("a", 1), XS_R20_255("a")

__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(1, 1))) void k_regfile_sweep(
    RegfileRecord* __restrict__ records, uint32_t seed, int inject_xcd, int inject_cu, int inject_reg, int inject_bit,
    int poison_reg, uint32_t expect_digest) {
  __shared__ uint32_t part[kBlock / 64][8];
  // Nothing per-lane may be live across the statement: every register is its.
  // `wave` is an operand of the statement, which pins its readfirstlane ahead
  // of it (threadIdx.x would otherwise stay live in v0 and spill).
  uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t xcd = xcc_id();
  const uint32_t hw = hw_id();
  const uint32_t cu = cu_key(hw);
  const uint32_t simd = simd_id(hw);
  const bool selected = inject_selected(inject_xcd, inject_cu, xcd, cu);
  const uint32_t injreg =
      __builtin_amdgcn_readfirstlane(selected && inject_reg >= 0 ? static_cast<uint32_t>(inject_reg) : kNone);
  const uint32_t injmask = __builtin_amdgcn_readfirstlane(1u << (inject_bit & 31));
  // The poison goes to the phase in which its register is under test.
  const uint32_t poison_a =
      __builtin_amdgcn_readfirstlane(selected && poison_reg >= 8 ? static_cast<uint32_t>(poison_reg) : kNone);
  const uint32_t poison_b = __builtin_amdgcn_readfirstlane(
      selected && poison_reg >= 0 && poison_reg < 8 ? static_cast<uint32_t>(poison_reg) : kNone);
  const uint32_t sseed = __builtin_amdgcn_readfirstlane(seed);

  uint32_t bad, first, flip, d0, d1, keep, tmp;
  asm volatile(
      // scratch of phase A: lane multiplier and empty accumulators
      ".set xs_s, 0\n"
      "v_mbcnt_lo_u32_b32 v0, -1, 0\n"
      "v_mbcnt_hi_u32_b32 v0, -1, v0\n"
      "v_lshl_add_u32 v0, v0, 1, 1\n"
      "v_mov_b32 v3, 0\n"
      "v_mov_b32 v4, 0xffff\n"
      "v_mov_b32 v5, 0\n"
      "v_mov_b32 v6, 0\n"
      "v_mov_b32 v7, 0\n"
      // phase A, pass 0
      XS_LOOP(8, 248, XS_WRITE_V(0)) XS_LOOP(0, 256, XS_WRITE_A(0))
      XS_POISON("%[poison_a]")
      XS_LOOP(8, 248, XS_READ_V(0)) XS_LOOP(0, 256, XS_READ_A(0))
      // phase A, pass 1
      XS_LOOP(8, 248, XS_WRITE_V(1)) XS_LOOP(0, 256, XS_WRITE_A(1))
      XS_LOOP(8, 248, XS_READ_V(1)) XS_LOOP(0, 256, XS_READ_A(1))
      // the scratch set moves to v8..v15
      ".set xs_n, 0\n.rept 8\nv_mov_b32 v[xs_n+8], v[xs_n]\n.set xs_n, xs_n+1\n.endr\n"
      ".set xs_s, 8\n"
      // phase B, both passes
      XS_LOOP(0, 8, XS_WRITE_V(0))
      XS_POISON("%[poison_b]")
      XS_LOOP(0, 8, XS_READ_V(0))
      XS_LOOP(0, 8, XS_WRITE_V(1))
      XS_LOOP(0, 8, XS_READ_V(1))
      : "={v11}"(bad), "={v12}"(first), "={v13}"(flip), "={v14}"(d0), "={v15}"(d1), [keep] "=&s"(keep),
        [tmp] "=&s"(tmp), "+s"(wave)
      : [seed] "s"(sseed), [injreg] "s"(injreg), [injmask] "s"(injmask), [poison_a] "s"(poison_a),
        [poison_b] "s"(poison_b)
      : XS_CLOBBER_V, XS_CLOBBER_A, "vcc", "scc");

  const uint32_t lane = __lane_id();
  const uint32_t bad_v = wave_sum(bad & 0xffffu), bad_a = wave_sum(bad >> 16);
  const uint32_t digest = wave_sum(d0) ^ rotl32(wave_sum(d1), 16);
  const uint32_t first_w = wave_min(first), flip_w = wave_or(flip);
  if (lane == 0) {
    uint32_t* s = part[wave];
    s[0] = bad_v;
    s[1] = bad_a;
    s[2] = first_w;
    s[3] = flip_w;
    s[4] = digest;
    s[5] = 1u << simd;
  }
  __syncthreads();
  if (wave == 0 && lane == 0) {
    uint32_t bv = 0, ba = 0, f1 = 0xffffu, fl = 0, dg = 0, simds = 0, bad_simds = 0;
    for (int w = 0; w < kBlock / 64; ++w) {
      const uint32_t* s = part[w];
      bv += s[0];
      ba += s[1];
      f1 = min(f1, s[2]);
      fl |= s[3];
      dg += s[4] << w;
      simds |= s[5];
      if (s[0] | s[1]) bad_simds |= s[5];
    }
    uint32_t fail = (bv ? kFailVgpr : 0u) | (ba ? kFailAgpr : 0u);
    if (!fail && dg != expect_digest) fail = kFailVgpr | kFailAgpr;
    u32x4* out = reinterpret_cast<u32x4*>(&records[blockIdx.x]);
    out[0] = u32x4{xcd, cu, simds, fail};
    out[1] = u32x4{bv, ba, f1, fl};
    out[2] = u32x4{dg, bad_simds, 0u, 0u};
    out[3] = u32x4{0u, 0u, 0u, 0u};
  }
}

// The workgroup digest a healthy CU leaves, from the same formulas.
uint32_t expected_digest(uint32_t seed) {
  uint32_t d[2] = {0, 0};
  for (uint32_t r = 0; r < kCells; ++r) {
    const uint32_t c = ((r + 1u) * 0x9e3779b1u) ^ seed;
    for (uint32_t l = 0; l < 64; ++l) {
      const uint32_t p0 = c * (2u * l + 1u), w = 2u * (64u * r + l) + 1u;
      d[0] += p0 * w;
      d[1] += ~p0 * w;
    }
  }
  const uint32_t wave = d[0] ^ rotl32(d[1], 16);
  uint32_t out = 0;
  for (int w = 0; w < kBlock / 64; ++w) out += wave << w;
  return out;
}

}  // namespace

extern "C" {

const char* xs_regfile_sweep_last_error() { return g_regfile_err; }

int xs_regfile_sweep_expected(uint32_t seed, uint32_t* out) {
  if (!out) return kBadArgs;
  *out = expected_digest(seed);
  return 0;
}

// out3 = {numRegs as the runtime reports it, scratch bytes per lane, active
// 256-thread workgroups per CU}.
int xs_regfile_sweep_info(int dev, int* out3) {
  return sweep_info(g_regfile_err, dev, reinterpret_cast<const void*>(k_regfile_sweep), kBlock, false, out3);
}

// One sweep launch of `blocks` workgroups (0: 4 per CU). Writes `blocks`
// 64-byte records to records_out (the caller's buffer holds at least that
// many; with blocks == 0, 4 x computeUnits). inject_xcd -1: no workgroup is
// selected; inject_reg -1 / poison_reg -1: that mode is off. Returns 0, -1000
// for bad arguments (nothing is launched), or a negative HIP error.
int xs_regfile_sweep(int dev, int blocks, uint32_t seed, int inject_xcd, int inject_cu, int inject_reg, int inject_bit,
                     int poison_reg, void* records_out, int* n_records, double* ms) {
  if (inject_reg < -1 || inject_reg >= kCells || inject_bit < 0 || inject_bit > 31) return kBadArgs;
  if (poison_reg < -1 || poison_reg > 255) return kBadArgs;
  const uint32_t expect = expected_digest(seed);
  return launch_sweep(g_regfile_err, {dev, blocks, inject_xcd, inject_cu, records_out, n_records, ms},
                      reinterpret_cast<const void*>(k_regfile_sweep), kBlock, 0, sizeof(RegfileRecord),
                      [&](dim3 grid, dim3 block, size_t smem, void* rec) {
                        hipLaunchKernelGGL(k_regfile_sweep, grid, block, smem, 0, static_cast<RegfileRecord*>(rec), seed,
                                           inject_xcd, inject_cu, inject_reg, inject_bit, poison_reg, expect);
                      });
}

}  // extern "C"
