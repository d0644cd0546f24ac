// Lane sweep for gfx950 (MI355X): the cross-lane network and the non-trivial
// LDS access paths of every CU.
//
// The other sweeps compute in one lane and touch LDS with ds_write_b32 /
// ds_read_b32 at a lane's own addresses; the only cross-lane operation among
// them is the __shfl_xor that reduces their digests. k_lane_sweep is the same
// kind of launch (256-thread workgroups, 4 waves: one per SIMD, each holding
// more than half of a CU's LDS, 4 x CUs of them, every workgroup
// self-contained: no waiting on another workgroup, no spinning on memory, no
// inter-workgroup atomics) and moves hashed values through the DPP shifters,
// v_permlane*_swap, v_readlane / v_writelane, the LDS crossbar and the wide,
// sub-dword, transposed, atomic and DMA paths of LDS. Everything is data
// movement or exact integer arithmetic: one right answer, no tolerance.
//
// Values. fmix32 is the murmur3 finaliser, a bijection of 32 bits (part_sweep.h).
//   src(p, s, w, l) = fmix32(seed ^ (p << 24 | s << 12 | w << 6 | l))
//   aux(p, s, w, l) = fmix32(seed ^ (1 << 28 | p << 24 | s << 12 | w << 6 | l))
// p = path, s = step, l = lane (0..63), w = 4 * wave + word (a step has at
// most four words; the four waves of a workgroup carry different values).
// aux supplies the operands that are not moved (DPP `old`, atomic operands).
// All keys of a launch differ, so all values do: one delivered from the wrong
// lane, step, word or wave mis-compares. The 16-bit tiles of `ldstr` hold
// e(i) = (i * 0x9e37 + seed) mod 2^16, i = ((stride * 4 + wave) * 16 + row) * 64
// + col < 8192: an odd multiplier, a bijection on 16 bits.
//
// Paths (bit, name, steps x words per step). Thread t = 64 * wave + lane l.
//  0 dpp       75 x 1  v_mov_b32 DPP, `old` = aux, so a lane without a source
//                      keeps old. Steps: 0-3 quad_perm [0,1,2,3] [1,2,3,0]
//                      [2,3,0,1] [3,0,1,2]; 4-18 row_shl:1..15; 19-33
//                      row_shr:1..15; 34-48 row_ror:1..15; 49 row_mirror; 50
//                      row_half_mirror; 51 row_bcast15; 52 row_bcast31; 53
//                      wave_shl:1; 54 wave_rol:1; 55 wave_shr:1; 56 wave_ror:1;
//                      57-72 row_newbcast:0..15; 73 row_shr:3 bound_ctrl (an
//                      absent source reads 0); 74 row_ror:5 row_mask:0xa
//                      bank_mask:0x5 (other lanes keep old).
//  1 permlane   4 x 2  steps 0, 1 v_permlane32_swap, steps 2, 3
//                      v_permlane16_swap, through the builtins (the compiler
//                      resolves the VALU-write -> permlane hazard). vdst =
//                      src(word 0), src = src(word 1); word 0 is vdst after
//                      the swap, word 1 is src after it.
//  2 readlane 133 x 1  0-63 v_readlane_b32 of lane s (uniform index); 64-127
//                      v_writelane_b32 of aux(s, lane 0) into lane s - 64 of
//                      src; 128-132 v_readfirstlane_b32 with EXEC = lanes >= f,
//                      f = 0, 1, 31, 32, 63 (lanes below f keep aux).
//  3 bpermute 137 x 1  0-63 ds_bpermute_b32 addr = 4 * ((l + s) % 64); 64-127
//                      ds_permute_b32 with the same addresses (s - 64);
//                      128-132 ds_swizzle_b32 bit-mask mode and:0x1f xor:1, 2,
//                      4, 8, 16; 133 and:0x10 (broadcast of lanes 0 / 16 of a
//                      half); 134 and:0x1f or:3; 135, 136 quad-perm mode
//                      [3,2,1,0] and [1,2,3,0].
//  4 ldswide  112 x 4  step = 7 * rot + combo, rot = 0..15. A wave's tile is
//                      64 slots of 16 B; lane l uses slot (l + rot) % 64, so
//                      over the steps it touches dwords 4((l + rot) % 64) + j:
//                      all 64 banks. x0..x3 = src(words 0..3). Combos:
//                        0 ds_write_b128            -> 2 x ds_read_b64
//                        1 2 x ds_write_b64         -> ds_read_b128
//                        2 ds_write_b96 + b32       -> 2 x ds_read2_b32
//                        3 2 x ds_write2_b32        -> ds_read_b96 + ds_read_b32
//                        4 8 x ds_write_b8 (x0, x1) -> u16(x0 lo) i16(x0 hi) i16(x1 lo) u16(x1 hi)
//                        5 4 x ds_write_b16 (x0, x1)-> u8(x0 b0) i8(x0 b1) i8(x1 b2) u8(x1 b3)
//                        6 ds_write_b128            -> 2 x ds_read2st64_b32 at dword D =
//                          (l + rot) % 64: dwords D, D+64, D+128, D+192 of the tile
//                          (other lanes' slots; dword d is word d % 4 of the lane
//                          whose slot is d / 4).
//                      i8 / i16 results are sign-extended.
//  5 ldstr     32 x 2  ds_read_b64_tr_b16 over a [16][64] tile of e(i), written
//                      with plain stores. Steps 0-15 row stride 128 B, 16-31
//                      136 B. The tile has 4 x 4 blocks of 4 rows x 16 columns;
//                      in step k (mod 16) lane group g = l >> 4 reads block
//                      b = (k + 5g) % 16 (block row b >> 2, block column b & 3):
//                      every group reads every block. EXEC is all ones, every
//                      address is in bounds and 8-byte aligned.
//  6 ldsatomic 13 x 4  steps 0-10: add, sub, and, or, xor, min_i32, max_i32,
//                      min_u32, max_u32, exchange, compare-swap with return on
//                      the lane's own word, two data sets j = 0, 1: the word
//                      holds a = src(word 2j), the operand is b = aux(word
//                      2j); word 2j is the returned value (a), word 2j+1 the
//                      final value. Compare-swap compares with a (j = 0: the
//                      swap happens) and with a ^ 1 (j = 1: it does not). Step
//                      11: the 64-bit add, a = src(words 0, 1), b = aux(words 0,
//                      1) (low, high): words 0, 1 returned, words 2, 3 final.
//                      Step 12: all 256 lanes hit one word per operation with
//                      ds_add_u32, ds_xor_b32, ds_max_u32, ds_min_u32 of
//                      src(word j) onto aux(word j, thread 0); every lane reads
//                      the four final values.
//  7 ldsdma     6 x 4  global_load_lds from a read-only buffer G laid out
//                      [step][wave][64][4] with G = src(step, word j, lane q)
//                      (the host fills it once per call). Lane l fetches
//                      element q = ((2s + 3) * l + s) % 64: steps 0, 1 four
//                      _dword (word j into plane j: base + 256j + 4l); steps
//                      2, 3 one _dwordx3 (base + 16l, see the maps) and a
//                      _dword for word 3 (base + 1024 + 4l); steps 4, 5 one
//                      _dwordx4 (base + 16l).
//                      The LDS destination is wave-linear, the SOURCE address
//                      is permuted. s_waitcnt vmcnt(0) and a barrier precede
//                      the read-back with plain ds_read_b32.
//
// Lane maps the comparator is written from (destination lane l reads source
// lane; a row is 16 lanes):
//   quad_perm          (l & ~3) + sel[l & 3]
//   row_shl:n          l + n while it stays in the row, else no source
//   row_shr:n          l - n while it stays in the row, else no source
//   row_ror:n          (l & ~15) | ((l - n) & 15)
//   wave_shl:1         l + 1; lane 63 has no source      wave_rol:1 wraps
//   wave_shr:1         l - 1; lane 0 has no source       wave_ror:1 wraps
//   row_mirror         (l & ~15) | (15 - (l & 15))
//   row_half_mirror    (l & ~7) | (7 - (l & 7))
//   row_bcast15        lane 15 of row r goes to all of row r + 1; row 0 reads itself
//   row_bcast31        lane 31 goes to rows 2 and 3; rows 0 and 1 read themselves
//   row_newbcast:n     lane n of its own row
//   row_mask bit r enables lanes 16r..16r+15, bank_mask bit b the lanes with
//   (l & 15) >> 2 == b; a disabled lane keeps old
//   v_permlane32_swap vdst, src   lanes 32-63 of vdst <-> lanes 0-31 of src
//   v_permlane16_swap vdst, src   vdst 16-31 <-> src 0-15, vdst 48-63 <-> src 32-47
//   ds_bpermute        dst[l] = src[(addr[l] >> 2) & 63]
//   ds_permute         dst[(addr[l] >> 2) & 63] = src[l]
//   ds_swizzle (bits)  within 32 lanes, ((l & and) | or) ^ xor
//   ds_swizzle (quad)  as quad_perm
//   ds_read_b64_tr_b16 per group of 16 lanes, lane 4q + p supplies the address
//                      of row q, columns 4p..4p+3; lane i receives column i of
//                      the four rows, row q in element q (rows 0, 1 in word 0)
//   global_load_lds    LDS address = M0 base + instruction offset + lane * size
//                      for _dword and _dwordx4; _dwordx3 steps 16 B per lane
// Every map is a bijection of the source cells onto the (lane, word) cells it
// fills, or exactly the stated fan-out (tests/test_lane_ref.py).
// What the hardware settled (the first probe against the numpy reference
// differed in exactly these cells, every other map stood as written): a row
// that row_bcast15 / row_bcast31 gives no source does not keep `old`, it
// receives the lane's own src (the broadcasts are documented only under
// row_mask 0xa / 0xc, where those rows are disabled); and
// global_load_lds_dwordx3 lays a lane's 12 bytes at lane * 16, not lane * 12
// (written for lane * 12, lane l read back lane 3l/4's words).
//
// Comparison. Each lane computes what it must receive with integer VALU only
// (the hash of the source lane under the map), counts mismatches per path and
// accumulates D_p += got * (2 idx + 1), idx = (step * words + word) * 256 + t.
// part_sweep.h's reduce_parts() makes the record of the 256 threads' counts
// and digests, with plain LDS words and a barrier: no shuffle, DPP or permute,
// so the sweep does not lean on what it tests.
//
// Record (128 bytes per workgroup): part_sweep.h's head with a path per part,
// eleven reserved words. xcd is HW_REG_XCC_ID, cu is bits [15:8] of
// HW_REG_HW_ID, as in cu_sweep.hip.
//
// Injection (testing the comparator and the localisation on a healthy GPU): a
// workgroup on inject_xcd whose CU key is inject_cu (or any, with -1) flips
// bit 0 of the value thread 0 received in step 0, word 0 of each path in
// inject_paths before comparing. Registers only. A path that is not selected
// is not run, so an injection into it reports nothing.
//
// k_lane_probe is one workgroup of the same device code with a dump pointer:
// it stores every received value of one path as [step][word][256]. That is
// what tests/test_gpu_lane_sweep.py holds against tests/lane_sweep_ref.py.
//
// NOT covered: the 8-, 6- and 4-bit transposed reads (ds_read_b64_tr_b8,
// ds_read_b64_tr_b4, ds_read_b96_tr_b6: their lane maps are in no document at
// hand, so a reference for them could only be copied from the hardware), the
// floating-point and packed LDS atomics, the SGPR file, and the caches.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <mutex>
#include <utility>
#include <vector>

#include "hip/part_sweep.h"

#define XS_ERR_BUF g_lane_err
#define XS_HD __host__ __device__ __forceinline__
#define XS_D __device__ __forceinline__

namespace {

xsprobe::ErrBuf g_lane_err;

using namespace xsprobe;

typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x3 __attribute__((ext_vector_type(3)));

enum Path : int { kDpp, kPermlane, kReadlane, kBpermute, kLdsWide, kLdsTr, kLdsAtomic, kLdsDma, kNumPaths };
const char kPathNames[] = "dpp,permlane,readlane,bpermute,ldswide,ldstr,ldsatomic,ldsdma";
constexpr uint32_t kAllPaths = (1u << kNumPaths) - 1;

struct Shape {
  int steps, words;
};
constexpr Shape kShape[kNumPaths] = {{75, 1}, {4, 2}, {133, 1}, {137, 1}, {112, 4}, {32, 2}, {13, 4}, {6, 4}};

constexpr int kBlock = kPartBlock;

// LDS layout in bytes from the start of the allocation.
constexpr uint32_t kRedBytes = part_reduction_words(kNumPaths, 0) * 4;
constexpr uint32_t kTileOff = kRedBytes;                     // per wave: 4 KiB
constexpr uint32_t kTileBytes = 4096;
constexpr uint32_t kAtomOff = kTileOff + 4 * kTileBytes;     // per thread: 8 B
constexpr uint32_t kCommonOff = kAtomOff + kBlock * 8;       // 4 words every lane hits
constexpr uint32_t kLdsUsed = kCommonOff + 16;
static_assert(kTileOff % 16 == 0 && kAtomOff % 8 == 0 && kLdsUsed <= (64u << 10), "LDS layout");

constexpr int kTrRows = 16, kTrCols = 64;
constexpr uint32_t kTrStride[2] = {128, 136};  // a power of two, and one padded by 8 B
static_assert(15 * 136 + 2 * (48 + 12) + 8 <= kTileBytes, "the padded tile fits");

constexpr int kDmaSteps = 6;
constexpr size_t kDmaWords = static_cast<size_t>(kDmaSteps) * 4 * 64 * 4;

struct LaneRecord {
  PartRecordHead<kNumPaths> head;
  uint32_t reserved[11];
};
static_assert(sizeof(LaneRecord) == 128, "one 128-byte record per workgroup");

using Expect = PartExpect<kNumPaths>;

// ------------------------------------------------------------------- values
// t = 64 * wave + lane; the word field of the key is 4 * wave + word.
XS_HD uint32_t srcv(uint32_t seed, uint32_t p, uint32_t s, uint32_t word, uint32_t t) {
  return fmix32(seed ^ (p << 24 | s << 12 | (4u * (t >> 6) + word) << 6 | (t & 63u)));
}
XS_HD uint32_t auxv(uint32_t seed, uint32_t p, uint32_t s, uint32_t word, uint32_t t) {
  return fmix32(seed ^ (1u << 28 | p << 24 | s << 12 | (4u * (t >> 6) + word) << 6 | (t & 63u)));
}
XS_HD uint32_t at_lane(uint32_t t, uint32_t lane) { return (t & ~63u) | (lane & 63u); }

// --------------------------------------------------------------------- maps
struct DppStep {
  uint32_t ctrl, row_mask, bank_mask, bound_ctrl;
};
XS_HD constexpr DppStep dpp_step(int s) {
  constexpr uint32_t quad[4] = {0xe4, 0x39, 0x4e, 0x93};
  if (s < 4) return {quad[s], 0xf, 0xf, 0};
  if (s < 19) return {0x100u + static_cast<uint32_t>(s - 3), 0xf, 0xf, 0};   // row_shl:1..15
  if (s < 34) return {0x110u + static_cast<uint32_t>(s - 18), 0xf, 0xf, 0};  // row_shr:1..15
  if (s < 49) return {0x120u + static_cast<uint32_t>(s - 33), 0xf, 0xf, 0};  // row_ror:1..15
  if (s == 49) return {0x140, 0xf, 0xf, 0};                                  // row_mirror
  if (s == 50) return {0x141, 0xf, 0xf, 0};                                  // row_half_mirror
  if (s == 51) return {0x142, 0xf, 0xf, 0};                                  // row_bcast15
  if (s == 52) return {0x143, 0xf, 0xf, 0};                                  // row_bcast31
  if (s == 53) return {0x130, 0xf, 0xf, 0};                                  // wave_shl:1
  if (s == 54) return {0x134, 0xf, 0xf, 0};                                  // wave_rol:1
  if (s == 55) return {0x138, 0xf, 0xf, 0};                                  // wave_shr:1
  if (s == 56) return {0x13c, 0xf, 0xf, 0};                                  // wave_ror:1
  if (s < 73) return {0x150u + static_cast<uint32_t>(s - 57), 0xf, 0xf, 0};  // row_newbcast:0..15
  if (s == 73) return {0x113, 0xf, 0xf, 1};                                  // row_shr:3 bound_ctrl
  return {0x125, 0xa, 0x5, 0};                                               // row_ror:5, partial masks
}
// Source lane of destination lane l, -1 when it has none.
XS_HD constexpr int dpp_src(uint32_t ctrl, int l) {
  const int n = static_cast<int>(ctrl & 15u), r = l & 15;
  if (ctrl < 0x100) return (l & ~3) + static_cast<int>((ctrl >> (2 * (l & 3))) & 3u);
  if (ctrl < 0x110) return r + n <= 15 ? l + n : -1;
  if (ctrl < 0x120) return r >= n ? l - n : -1;
  if (ctrl < 0x130) return (l & ~15) | ((l - n) & 15);
  if (ctrl == 0x130) return l < 63 ? l + 1 : -1;
  if (ctrl == 0x134) return (l + 1) & 63;
  if (ctrl == 0x138) return l > 0 ? l - 1 : -1;
  if (ctrl == 0x13c) return (l - 1) & 63;
  if (ctrl == 0x140) return (l & ~15) | (15 - r);
  if (ctrl == 0x141) return (l & ~7) | (7 - (l & 7));
  if (ctrl == 0x142) return l >= 16 ? (l & ~15) - 1 : l;
  if (ctrl == 0x143) return l >= 32 ? 31 : l;
  return (l & ~15) | n;  // row_newbcast
}

// ds_swizzle offsets of bpermute steps 128..136.
XS_HD constexpr uint32_t swizzle_pattern(int k) {
  if (k < 5) return (1u << k) << 10 | 0x1fu;
  if (k == 5) return 0x10u;
  if (k == 6) return 3u << 5 | 0x1fu;
  return k == 7 ? 0x8000u | 0x1bu : 0x8000u | 0x39u;
}
XS_HD constexpr int swizzle_src(uint32_t pat, int l) {
  if (pat & 0x8000u) return (l & ~3) + static_cast<int>((pat >> (2 * (l & 3))) & 3u);
  const int a = static_cast<int>(pat & 31u), o = static_cast<int>((pat >> 5) & 31u), x = static_cast<int>((pat >> 10) & 31u);
  return (l & 32) | ((((l & 31) & a) | o) ^ x);
}

XS_HD uint32_t tr_elem(uint32_t seed, uint32_t stride_idx, uint32_t wave, uint32_t row, uint32_t col) {
  const uint32_t i = ((stride_idx * 4u + wave) * kTrRows + row) * kTrCols + col;
  return (i * 0x9e37u + seed) & 0xffffu;
}

XS_HD uint32_t dma_perm(uint32_t s, uint32_t l) { return ((2u * s + 3u) * l + s) & 63u; }

XS_HD uint32_t atomic_apply(int op, uint32_t a, uint32_t b) {
  switch (op) {
    case 0: return a + b;
    case 1: return a - b;
    case 2: return a & b;
    case 3: return a | b;
    case 4: return a ^ b;
    case 5: return static_cast<uint32_t>(std::min(static_cast<int32_t>(a), static_cast<int32_t>(b)));
    case 6: return static_cast<uint32_t>(std::max(static_cast<int32_t>(a), static_cast<int32_t>(b)));
    case 7: return std::min(a, b);
    case 8: return std::max(a, b);
    default: return b;  // exchange
  }
}

// ------------------------------------------------- what a lane must receive
XS_HD uint32_t want_dpp(uint32_t seed, int s, uint32_t t) {
  const DppStep d = dpp_step(s);
  const int l = static_cast<int>(t & 63u);
  const uint32_t old = auxv(seed, kDpp, s, 0, t);
  if (!((d.row_mask >> (l >> 4)) & 1u) || !((d.bank_mask >> ((l & 15) >> 2)) & 1u)) return old;
  const int from = dpp_src(d.ctrl, l);
  if (from < 0) return d.bound_ctrl ? 0u : old;
  return srcv(seed, kDpp, s, 0, at_lane(t, from));
}

XS_HD uint32_t want_permlane(uint32_t seed, int s, int word, uint32_t t) {
  const uint32_t l = t & 63u;
  const uint32_t span = s < 2 ? 32u : 16u;
  const bool upper = (l & span) != 0;
  // word 0: vdst after the swap; its upper lanes hold src's lower lanes.
  if (word == 0) return upper ? srcv(seed, kPermlane, s, 1, at_lane(t, l - span)) : srcv(seed, kPermlane, s, 0, t);
  return upper ? srcv(seed, kPermlane, s, 1, t) : srcv(seed, kPermlane, s, 0, at_lane(t, l + span));
}

XS_HD constexpr int first_lane(int k) { return k == 0 ? 0 : k == 1 ? 1 : k == 2 ? 31 : k == 3 ? 32 : 63; }

XS_HD uint32_t want_readlane(uint32_t seed, int s, uint32_t t) {
  const uint32_t l = t & 63u;
  if (s < 64) return srcv(seed, kReadlane, s, 0, at_lane(t, s));
  if (s < 128)
    return l == static_cast<uint32_t>(s - 64) ? auxv(seed, kReadlane, s, 0, at_lane(t, 0)) : srcv(seed, kReadlane, s, 0, t);
  const uint32_t f = static_cast<uint32_t>(first_lane(s - 128));
  return l >= f ? srcv(seed, kReadlane, s, 0, at_lane(t, f)) : auxv(seed, kReadlane, s, 0, t);
}

XS_HD uint32_t want_bpermute(uint32_t seed, int s, uint32_t t) {
  const uint32_t l = t & 63u;
  if (s < 64) return srcv(seed, kBpermute, s, 0, at_lane(t, l + s));
  if (s < 128) return srcv(seed, kBpermute, s, 0, at_lane(t, l - (s - 64)));
  return srcv(seed, kBpermute, s, 0, at_lane(t, swizzle_src(swizzle_pattern(s - 128), static_cast<int>(l))));
}

XS_HD uint32_t sext(uint32_t v, int bits) {
  return static_cast<uint32_t>(static_cast<int32_t>(v << (32 - bits)) >> (32 - bits));
}

XS_HD uint32_t want_ldswide(uint32_t seed, int s, int word, uint32_t t) {
  const int rot = s / 7, combo = s % 7;
  if (combo < 4) return srcv(seed, kLdsWide, s, word, t);
  const uint32_t x0 = srcv(seed, kLdsWide, s, 0, t), x1 = srcv(seed, kLdsWide, s, 1, t);
  if (combo == 4) {
    switch (word) {
      case 0: return x0 & 0xffffu;
      case 1: return sext(x0 >> 16, 16);
      case 2: return sext(x1 & 0xffffu, 16);
      default: return x1 >> 16;
    }
  }
  if (combo == 5) {
    switch (word) {
      case 0: return x0 & 0xffu;
      case 1: return sext((x0 >> 8) & 0xffu, 8);
      case 2: return sext((x1 >> 16) & 0xffu, 8);
      default: return x1 >> 24;
    }
  }
  // combo 6: dword d of the tile is word d % 4 of the lane whose slot is d / 4.
  const uint32_t d = ((t & 63u) + rot) % 64u + 64u * word;
  return srcv(seed, kLdsWide, s, d & 3u, at_lane(t, (d >> 2) - rot));
}

XS_HD uint32_t want_ldstr(uint32_t seed, int s, int word, uint32_t t) {
  const uint32_t l = t & 63u, wave = t >> 6, h = s / 16, k = s % 16;
  const uint32_t b = (k + 5u * (l >> 4)) % 16u, row = 4u * (b >> 2) + 2u * word, col = 16u * (b & 3u) + (l & 15u);
  return tr_elem(seed, h, wave, row, col) | tr_elem(seed, h, wave, row + 1, col) << 16;
}

XS_HD uint32_t want_ldsatomic(uint32_t seed, int s, int word, uint32_t t) {
  if (s < 11) {
    const int j = word >> 1;
    const uint32_t a = srcv(seed, kLdsAtomic, s, 2 * j, t), b = auxv(seed, kLdsAtomic, s, 2 * j, t);
    if (!(word & 1)) return a;
    if (s == 10) return j == 0 ? b : a;
    return atomic_apply(s, a, b);
  }
  if (s == 11) {
    const uint64_t a = srcv(seed, kLdsAtomic, s, 0, t) | static_cast<uint64_t>(srcv(seed, kLdsAtomic, s, 1, t)) << 32;
    const uint64_t b = auxv(seed, kLdsAtomic, s, 0, t) | static_cast<uint64_t>(auxv(seed, kLdsAtomic, s, 1, t)) << 32;
    const uint64_t r = word < 2 ? a : a + b;
    return static_cast<uint32_t>(r >> (32 * (word & 1)));
  }
  constexpr int ops[4] = {0, 4, 8, 7};  // add, xor, max_u32, min_u32
  uint32_t v = auxv(seed, kLdsAtomic, s, word, 0);
  for (uint32_t u = 0; u < kBlock; ++u) v = atomic_apply(ops[word], v, srcv(seed, kLdsAtomic, s, word, u));
  return v;
}

XS_HD uint32_t want_ldsdma(uint32_t seed, int s, int word, uint32_t t) {
  return srcv(seed, kLdsDma, s, word, at_lane(t, dma_perm(s, t & 63u)));
}

XS_HD uint32_t want(int p, uint32_t seed, int s, int word, uint32_t t) {
  switch (p) {
    case kDpp: return want_dpp(seed, s, t);
    case kPermlane: return want_permlane(seed, s, word, t);
    case kReadlane: return want_readlane(seed, s, t);
    case kBpermute: return want_bpermute(seed, s, t);
    case kLdsWide: return want_ldswide(seed, s, word, t);
    case kLdsTr: return want_ldstr(seed, s, word, t);
    case kLdsAtomic: return want_ldsatomic(seed, s, word, t);
    default: return want_ldsdma(seed, s, word, t);
  }
}

// ------------------------------------------------------------------- device
struct Ctx {
  uint32_t seed, t, lane, wave, inj;
  uint32_t* dump;  // k_lane_probe only
};

template <int P>
XS_D void take(const Ctx& c, Tally& y, uint32_t step, uint32_t word, uint32_t got, uint32_t expect) {
  take_word(y, c.dump, (step * kShape[P].words + word) * kBlock + c.t, got, expect, (c.inj >> P) & 1u);
}

// The value leaves the compiler's sight here, so the instruction that made it
// is not folded into its consumer.
XS_D uint32_t opaque(uint32_t v) {
  asm volatile("" : "+v"(v));
  return v;
}

#define XS_LGKM "\n\ts_waitcnt lgkmcnt(0)"
XS_D void ds_w128(uint32_t a, u32x4 v) { asm volatile("ds_write_b128 %0, %1" XS_LGKM ::"v"(a), "v"(v) : "memory"); }
XS_D void ds_w96(uint32_t a, u32x3 v) { asm volatile("ds_write_b96 %0, %1" XS_LGKM ::"v"(a), "v"(v) : "memory"); }
XS_D void ds_w64(uint32_t a, u32x2 v) { asm volatile("ds_write_b64 %0, %1" XS_LGKM ::"v"(a), "v"(v) : "memory"); }
XS_D void ds_w32(uint32_t a, uint32_t v) { asm volatile("ds_write_b32 %0, %1" XS_LGKM ::"v"(a), "v"(v) : "memory"); }
XS_D void ds_w16(uint32_t a, uint32_t v) { asm volatile("ds_write_b16 %0, %1" XS_LGKM ::"v"(a), "v"(v) : "memory"); }
XS_D void ds_w8(uint32_t a, uint32_t v) { asm volatile("ds_write_b8 %0, %1" XS_LGKM ::"v"(a), "v"(v) : "memory"); }
XS_D void ds_w2x32(uint32_t a, uint32_t x, uint32_t y) {
  asm volatile("ds_write2_b32 %0, %1, %2 offset1:1" XS_LGKM ::"v"(a), "v"(x), "v"(y) : "memory");
}
#define XS_DS_READ(name, type, text)                                      \
  XS_D type name(uint32_t a) {                                            \
    type r;                                                               \
    asm volatile(text " %0, %1" XS_LGKM : "=&v"(r) : "v"(a) : "memory"); \
    return r;                                                             \
  }
XS_DS_READ(ds_r128, u32x4, "ds_read_b128")
XS_DS_READ(ds_r96, u32x3, "ds_read_b96")
XS_DS_READ(ds_r64, u32x2, "ds_read_b64")
XS_DS_READ(ds_r32, uint32_t, "ds_read_b32")
XS_DS_READ(ds_ru8, uint32_t, "ds_read_u8")
XS_DS_READ(ds_ri8, uint32_t, "ds_read_i8")
XS_DS_READ(ds_ru16, uint32_t, "ds_read_u16")
XS_DS_READ(ds_ri16, uint32_t, "ds_read_i16")
XS_DS_READ(ds_rtr16, u32x2, "ds_read_b64_tr_b16")
#undef XS_DS_READ
XS_D u32x2 ds_r2x32(uint32_t a) {
  u32x2 r;
  asm volatile("ds_read2_b32 %0, %1 offset1:1" XS_LGKM : "=&v"(r) : "v"(a) : "memory");
  return r;
}
XS_D u32x2 ds_r2st64(uint32_t a) {
  u32x2 r;
  asm volatile("ds_read2st64_b32 %0, %1 offset1:1" XS_LGKM : "=&v"(r) : "v"(a) : "memory");
  return r;
}

template <int S>
XS_D void dpp_one(const Ctx& c, Tally& y) {
  constexpr DppStep d = dpp_step(S);
  const uint32_t x = srcv(c.seed, kDpp, S, 0, c.t), old = auxv(c.seed, kDpp, S, 0, c.t);
  const uint32_t got = opaque(static_cast<uint32_t>(__builtin_amdgcn_update_dpp(
      static_cast<int>(old), static_cast<int>(x), d.ctrl, d.row_mask, d.bank_mask, d.bound_ctrl != 0)));
  take<kDpp>(c, y, S, 0, got, want_dpp(c.seed, S, c.t));
}
template <int... S>
XS_D void run_dpp(const Ctx& c, Tally& y, std::integer_sequence<int, S...>) {
  (dpp_one<S>(c, y), ...);
}

XS_D void run_permlane(const Ctx& c, Tally& y) {
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const uint32_t a = srcv(c.seed, kPermlane, s, 0, c.t), b = srcv(c.seed, kPermlane, s, 1, c.t);
    const auto r = s < 2 ? __builtin_amdgcn_permlane32_swap(a, b, false, false)
                         : __builtin_amdgcn_permlane16_swap(a, b, false, false);
    take<kPermlane>(c, y, s, 0, opaque(r[0]), want_permlane(c.seed, s, 0, c.t));
    take<kPermlane>(c, y, s, 1, opaque(r[1]), want_permlane(c.seed, s, 1, c.t));
  }
}

// Lane `lane` of `old` <- `v`; both scalars are wave-uniform. One instruction
// reads one SGPR, so the lane select goes through M0 (saved and restored: the
// compiler owns it). The s_nop covers the M0 write.
XS_D uint32_t writelane(uint32_t old, uint32_t v, int lane) {
  uint32_t keep;
  asm volatile("s_mov_b32 %1, m0\n\ts_mov_b32 m0, %3\n\ts_nop 3\n\tv_writelane_b32 %0, %2, m0\n\ts_mov_b32 m0, %1"
               : "+v"(old), "=&s"(keep)
               : "s"(v), "s"(lane));
  return old;
}

template <int K>
XS_D void readfirst_one(const Ctx& c, Tally& y) {
  constexpr int s = 128 + K;
  const uint32_t x = srcv(c.seed, kReadlane, s, 0, c.t);
  uint32_t got = auxv(c.seed, kReadlane, s, 0, c.t);
  if (c.lane >= static_cast<uint32_t>(first_lane(K))) got = __builtin_amdgcn_readfirstlane(x);
  take<kReadlane>(c, y, s, 0, opaque(got), want_readlane(c.seed, s, c.t));
}

XS_D void run_readlane(const Ctx& c, Tally& y) {
  const uint32_t t0 = __builtin_amdgcn_readfirstlane(c.t & ~63u);  // lane 0 of this wave, uniform
  for (int s = 0; s < 64; ++s) {
    const uint32_t x = srcv(c.seed, kReadlane, s, 0, c.t);
    take<kReadlane>(c, y, s, 0, opaque(__builtin_amdgcn_readlane(x, s)), want_readlane(c.seed, s, c.t));
  }
  for (int s = 64; s < 128; ++s) {
    const uint32_t x = srcv(c.seed, kReadlane, s, 0, c.t);
    const uint32_t v = auxv(c.seed, kReadlane, s, 0, t0);
    take<kReadlane>(c, y, s, 0, writelane(x, v, s - 64), want_readlane(c.seed, s, c.t));
  }
  readfirst_one<0>(c, y);
  readfirst_one<1>(c, y);
  readfirst_one<2>(c, y);
  readfirst_one<3>(c, y);
  readfirst_one<4>(c, y);
}

template <int K>
XS_D void swizzle_one(const Ctx& c, Tally& y) {
  constexpr int s = 128 + K;
  const uint32_t x = srcv(c.seed, kBpermute, s, 0, c.t);
  const uint32_t got = static_cast<uint32_t>(__builtin_amdgcn_ds_swizzle(static_cast<int>(x), swizzle_pattern(K)));
  take<kBpermute>(c, y, s, 0, opaque(got), want_bpermute(c.seed, s, c.t));
}
template <int... K>
XS_D void run_swizzle(const Ctx& c, Tally& y, std::integer_sequence<int, K...>) {
  (swizzle_one<K>(c, y), ...);
}

XS_D void run_bpermute(const Ctx& c, Tally& y) {
  for (int s = 0; s < 128; ++s) {
    const uint32_t x = srcv(c.seed, kBpermute, s, 0, c.t);
    const int addr = static_cast<int>(((c.lane + static_cast<uint32_t>(s)) & 63u) * 4u);
    const int got = s < 64 ? __builtin_amdgcn_ds_bpermute(addr, static_cast<int>(x))
                           : __builtin_amdgcn_ds_permute(addr, static_cast<int>(x));
    take<kBpermute>(c, y, s, 0, opaque(static_cast<uint32_t>(got)), want_bpermute(c.seed, s, c.t));
  }
  run_swizzle(c, y, std::make_integer_sequence<int, 9>{});
}

XS_D void run_ldswide(const Ctx& c, Tally& y) {
  const uint32_t tile = kTileOff + c.wave * kTileBytes;
  for (int rot = 0; rot < 16; ++rot) {
    const uint32_t slot = tile + 16u * ((c.lane + static_cast<uint32_t>(rot)) & 63u);
#pragma unroll
    for (int combo = 0; combo < 7; ++combo) {
      const int s = 7 * rot + combo;
      uint32_t x[4], g[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) x[j] = srcv(c.seed, kLdsWide, s, j, c.t);
      if (combo == 0) {
        ds_w128(slot, u32x4{x[0], x[1], x[2], x[3]});
        const u32x2 lo = ds_r64(slot), hi = ds_r64(slot + 8);
        g[0] = lo[0], g[1] = lo[1], g[2] = hi[0], g[3] = hi[1];
      } else if (combo == 1) {
        ds_w64(slot, u32x2{x[0], x[1]});
        ds_w64(slot + 8, u32x2{x[2], x[3]});
        const u32x4 r = ds_r128(slot);
        g[0] = r[0], g[1] = r[1], g[2] = r[2], g[3] = r[3];
      } else if (combo == 2) {
        ds_w96(slot, u32x3{x[0], x[1], x[2]});
        ds_w32(slot + 12, x[3]);
        const u32x2 lo = ds_r2x32(slot), hi = ds_r2x32(slot + 8);
        g[0] = lo[0], g[1] = lo[1], g[2] = hi[0], g[3] = hi[1];
      } else if (combo == 3) {
        ds_w2x32(slot, x[0], x[1]);
        ds_w2x32(slot + 8, x[2], x[3]);
        const u32x3 r = ds_r96(slot);
        g[0] = r[0], g[1] = r[1], g[2] = r[2], g[3] = ds_r32(slot + 12);
      } else if (combo == 4) {
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          ds_w8(slot + b, x[0] >> (8 * b));
          ds_w8(slot + 4 + b, x[1] >> (8 * b));
        }
        g[0] = ds_ru16(slot), g[1] = ds_ri16(slot + 2), g[2] = ds_ri16(slot + 4), g[3] = ds_ru16(slot + 6);
      } else if (combo == 5) {
        ds_w16(slot, x[0]);
        ds_w16(slot + 2, x[0] >> 16);
        ds_w16(slot + 4, x[1]);
        ds_w16(slot + 6, x[1] >> 16);
        g[0] = ds_ru8(slot), g[1] = ds_ri8(slot + 1), g[2] = ds_ri8(slot + 6), g[3] = ds_ru8(slot + 7);
      } else {
        ds_w128(slot, u32x4{x[0], x[1], x[2], x[3]});
        const uint32_t d = tile + 4u * ((c.lane + static_cast<uint32_t>(rot)) & 63u);
        const u32x2 lo = ds_r2st64(d), hi = ds_r2st64(d + 512);
        g[0] = lo[0], g[1] = lo[1], g[2] = hi[0], g[3] = hi[1];
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) take<kLdsWide>(c, y, s, j, g[j], want_ldswide(c.seed, s, j, c.t));
    }
  }
}

XS_D void run_ldstr(const Ctx& c, Tally& y, uint32_t* lds) {
  const uint32_t tile = kTileOff + c.wave * kTileBytes;
  const uint32_t i = c.lane & 15u, g = c.lane >> 4;
  for (uint32_t h = 0; h < 2; ++h) {
    const uint32_t stride = h ? kTrStride[1] : kTrStride[0];
    // Plain stores, two elements per word: word n of the tile's 512.
    for (uint32_t n = c.lane; n < kTrRows * kTrCols / 2; n += 64) {
      const uint32_t row = n / (kTrCols / 2), cw = n % (kTrCols / 2);
      lds[(tile + row * stride) / 4 + cw] =
          tr_elem(c.seed, h, c.wave, row, 2 * cw) | tr_elem(c.seed, h, c.wave, row, 2 * cw + 1) << 16;
    }
    for (uint32_t k = 0; k < 16; ++k) {
      const uint32_t b = (k + 5u * g) % 16u;
      // Lane 4q + p of the group: row q of the block, columns 4p..4p+3.
      const uint32_t addr = tile + (4u * (b >> 2) + (i >> 2)) * stride + 2u * (16u * (b & 3u) + 4u * (i & 3u));
      const u32x2 r = ds_rtr16(addr);
      const int s = static_cast<int>(16 * h + k);
      take<kLdsTr>(c, y, s, 0, r[0], want_ldstr(c.seed, s, 0, c.t));
      take<kLdsTr>(c, y, s, 1, r[1], want_ldstr(c.seed, s, 1, c.t));
    }
  }
}

template <int OP>
XS_D uint32_t own_atomic(uint32_t* p, uint32_t a, uint32_t b) {
  constexpr int order = __ATOMIC_RELAXED, scope = __HIP_MEMORY_SCOPE_WORKGROUP;
  int* ip = reinterpret_cast<int*>(p);
  if constexpr (OP == 0) return __hip_atomic_fetch_add(p, b, order, scope);
  if constexpr (OP == 1) return __hip_atomic_fetch_sub(p, b, order, scope);
  if constexpr (OP == 2) return __hip_atomic_fetch_and(p, b, order, scope);
  if constexpr (OP == 3) return __hip_atomic_fetch_or(p, b, order, scope);
  if constexpr (OP == 4) return __hip_atomic_fetch_xor(p, b, order, scope);
  if constexpr (OP == 5) return static_cast<uint32_t>(__hip_atomic_fetch_min(ip, static_cast<int>(b), order, scope));
  if constexpr (OP == 6) return static_cast<uint32_t>(__hip_atomic_fetch_max(ip, static_cast<int>(b), order, scope));
  if constexpr (OP == 7) return __hip_atomic_fetch_min(p, b, order, scope);
  if constexpr (OP == 8) return __hip_atomic_fetch_max(p, b, order, scope);
  if constexpr (OP == 9) return __hip_atomic_exchange(p, b, order, scope);
  if constexpr (OP == 10) {
    __hip_atomic_compare_exchange_strong(p, &a, b, order, order, scope);  // a: the compare value in, the old value out
    return a;
  }
}

template <int OP>
XS_D void atomic_one(const Ctx& c, Tally& y, uint32_t* own) {
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const uint32_t a = srcv(c.seed, kLdsAtomic, OP, 2 * j, c.t), b = auxv(c.seed, kLdsAtomic, OP, 2 * j, c.t);
    *static_cast<volatile uint32_t*>(own) = a;
    const uint32_t ret = own_atomic<OP>(own, OP == 10 ? a ^ static_cast<uint32_t>(j) : a, b);
    const uint32_t fin = *static_cast<volatile uint32_t*>(own);
    take<kLdsAtomic>(c, y, OP, 2 * j, ret, want_ldsatomic(c.seed, OP, 2 * j, c.t));
    take<kLdsAtomic>(c, y, OP, 2 * j + 1, fin, want_ldsatomic(c.seed, OP, 2 * j + 1, c.t));
  }
}
template <int... OP>
XS_D void run_atomic_ops(const Ctx& c, Tally& y, uint32_t* own, std::integer_sequence<int, OP...>) {
  (atomic_one<OP>(c, y, own), ...);
}

XS_D void run_ldsatomic(const Ctx& c, Tally& y, uint32_t* lds) {
  uint32_t* own = lds + kAtomOff / 4 + 2 * c.t;
  run_atomic_ops(c, y, own, std::make_integer_sequence<int, 11>{});
  {
    constexpr int s = 11;
    const uint64_t a = srcv(c.seed, kLdsAtomic, s, 0, c.t) | static_cast<uint64_t>(srcv(c.seed, kLdsAtomic, s, 1, c.t)) << 32;
    const uint64_t b = auxv(c.seed, kLdsAtomic, s, 0, c.t) | static_cast<uint64_t>(auxv(c.seed, kLdsAtomic, s, 1, c.t)) << 32;
    unsigned long long* own64 = reinterpret_cast<unsigned long long*>(own);
    *static_cast<volatile unsigned long long*>(own64) = a;
    const uint64_t ret = __hip_atomic_fetch_add(own64, static_cast<unsigned long long>(b), __ATOMIC_RELAXED,
                                                __HIP_MEMORY_SCOPE_WORKGROUP);
    const uint64_t fin = *static_cast<volatile unsigned long long*>(own64);
    const uint32_t g[4] = {static_cast<uint32_t>(ret), static_cast<uint32_t>(ret >> 32), static_cast<uint32_t>(fin),
                           static_cast<uint32_t>(fin >> 32)};
#pragma unroll
    for (int j = 0; j < 4; ++j) take<kLdsAtomic>(c, y, s, j, g[j], want_ldsatomic(c.seed, s, j, c.t));
  }
  {
    // All 256 lanes on one word per operation. Inline asm: for a uniform
    // address the compiler would replace the atomics by a DPP reduction.
    constexpr int s = 12;
    volatile uint32_t* common = lds + kCommonOff / 4;
    if (c.t == 0) {
#pragma unroll
      for (int j = 0; j < 4; ++j) common[j] = auxv(c.seed, kLdsAtomic, s, j, 0);
    }
    __syncthreads();
    const uint32_t a = kCommonOff;
    asm volatile(
        "ds_add_u32 %0, %1\n\tds_xor_b32 %0, %2 offset:4\n\tds_max_u32 %0, %3 offset:8\n\tds_min_u32 %0, %4 "
        "offset:12" XS_LGKM ::"v"(a),
        "v"(srcv(c.seed, kLdsAtomic, s, 0, c.t)), "v"(srcv(c.seed, kLdsAtomic, s, 1, c.t)),
        "v"(srcv(c.seed, kLdsAtomic, s, 2, c.t)), "v"(srcv(c.seed, kLdsAtomic, s, 3, c.t))
        : "memory");
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; ++j) take<kLdsAtomic>(c, y, s, j, common[j], want_ldsatomic(c.seed, s, j, c.t));
    __syncthreads();
  }
}

typedef __attribute__((address_space(1))) const void* GlobalPtr;
typedef __attribute__((address_space(3))) void* LdsPtr;

// The size is a literal: the builtin takes no template parameter.
XS_D void lds_dma4(const uint32_t* src, uint32_t* lds_dst) {
  __builtin_amdgcn_global_load_lds((GlobalPtr)src, (LdsPtr)lds_dst, 4, 0, 0);
}
XS_D void lds_dma12(const uint32_t* src, uint32_t* lds_dst) {
  __builtin_amdgcn_global_load_lds((GlobalPtr)src, (LdsPtr)lds_dst, 12, 0, 0);
}
XS_D void lds_dma16(const uint32_t* src, uint32_t* lds_dst) {
  __builtin_amdgcn_global_load_lds((GlobalPtr)src, (LdsPtr)lds_dst, 16, 0, 0);
}

XS_D void run_ldsdma(const Ctx& c, Tally& y, uint32_t* lds, const uint32_t* __restrict__ dma_src) {
  uint32_t* tile = lds + (kTileOff + c.wave * kTileBytes) / 4;  // wave-uniform
  volatile uint32_t* back = tile;
#pragma unroll
  for (int s = 0; s < kDmaSteps; ++s) {
    const uint32_t* elem = dma_src + ((static_cast<uint32_t>(s) * 4u + c.wave) * 64u + dma_perm(s, c.lane)) * 4u;
    uint32_t g[4];
    __syncthreads();  // the tile's previous readers are done
    if (s < 2) {
      lds_dma4(elem, tile);
      lds_dma4(elem + 1, tile + 64);
      lds_dma4(elem + 2, tile + 128);
      lds_dma4(elem + 3, tile + 192);
    } else if (s < 4) {
      lds_dma12(elem, tile);
      lds_dma4(elem + 3, tile + 256);
    } else {
      lds_dma16(elem, tile);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; ++j)
      g[j] = s < 2 ? back[64 * j + c.lane] : s < 4 && j == 3 ? back[256 + c.lane] : back[4 * c.lane + j];
#pragma unroll
    for (int j = 0; j < 4; ++j) take<kLdsDma>(c, y, s, j, g[j], want_ldsdma(c.seed, s, j, c.t));
  }
}

XS_D void run_paths(const Ctx& c, uint32_t mask, uint32_t* lds, const uint32_t* dma_src, Tally (&y)[kNumPaths]) {
  if (mask & (1u << kDpp)) run_dpp(c, y[kDpp], std::make_integer_sequence<int, kShape[kDpp].steps>{});
  if (mask & (1u << kPermlane)) run_permlane(c, y[kPermlane]);
  if (mask & (1u << kReadlane)) run_readlane(c, y[kReadlane]);
  if (mask & (1u << kBpermute)) run_bpermute(c, y[kBpermute]);
  if (mask & (1u << kLdsWide)) run_ldswide(c, y[kLdsWide]);
  if (mask & (1u << kLdsTr)) run_ldstr(c, y[kLdsTr], lds);
  if (mask & (1u << kLdsAtomic)) run_ldsatomic(c, y[kLdsAtomic], lds);
  if (mask & (1u << kLdsDma)) run_ldsdma(c, y[kLdsDma], lds, dma_src);
}

__global__ __launch_bounds__(kBlock) void k_lane_sweep(LaneRecord* __restrict__ records,
                                                      const uint32_t* __restrict__ dma_src, uint32_t path_mask,
                                                      uint32_t seed, int inject_xcd, int inject_cu,
                                                      uint32_t inject_paths, Expect expect) {
  extern __shared__ uint32_t lane_lds[];
  const uint32_t t = threadIdx.x;
  const uint32_t xcd = xcc_id();
  const uint32_t hw = hw_id();
  const uint32_t cu = cu_key(hw);
  const uint32_t simd = simd_id(hw);
  const bool inject = inject_selected(inject_xcd, inject_cu, xcd, cu);
  const Ctx c{seed, t, t & 63u, t >> 6, inject ? inject_paths : 0u, nullptr};

  Tally y[kNumPaths];
  run_paths(c, path_mask, lane_lds, dma_src, y);

  // The markers bound the reduction for tests/test_lane_codeobject.py.
  asm volatile("; lane_sweep reduction begin" ::: "memory");
  reduce_parts<kNumPaths, 0>(lane_lds, t, simd, y, nullptr, path_mask, expect, xcd, cu, &records[blockIdx.x]);
  asm volatile("; lane_sweep reduction end" ::: "memory");
}

// One workgroup; dump holds steps x words x 256 words of path `path`.
__global__ __launch_bounds__(kBlock) void k_lane_probe(uint32_t* __restrict__ dump, const uint32_t* __restrict__ dma_src,
                                                      int path, uint32_t seed) {
  extern __shared__ uint32_t lane_lds[];
  const uint32_t t = threadIdx.x;
  const Ctx c{seed, t, t & 63u, t >> 6, 0u, dump};
  Tally y[kNumPaths];
  run_paths(c, 1u << path, lane_lds, dma_src, y);
}

// --------------------------------------------------------------------- host
uint32_t expected_digest(int p, uint32_t seed) {
  uint32_t d = 0;
  const Shape sh = kShape[p];
  for (int s = 0; s < sh.steps; ++s)
    for (int w = 0; w < sh.words; ++w) {
      // Step 12 of ldsatomic is the same for every thread.
      const bool same = p == kLdsAtomic && s == 12;
      const uint32_t v0 = same ? want(p, seed, s, w, 0) : 0u;
      for (uint32_t t = 0; t < kBlock; ++t) {
        const uint32_t idx = (static_cast<uint32_t>(s) * sh.words + w) * kBlock + t;
        d += (same ? v0 : want(p, seed, s, w, t)) * (2u * idx + 1u);
      }
    }
  return d;
}

// The node agent sweeps with one seed again and again: keep the last.
void expected(uint32_t path_mask, uint32_t seed, Expect* e) {
  static std::mutex mu;
  static bool have = false;
  static uint32_t have_seed = 0;
  static uint32_t all[kNumPaths];
  std::lock_guard<std::mutex> g(mu);
  if (!have || have_seed != seed) {
    for (int p = 0; p < kNumPaths; ++p) all[p] = expected_digest(p, seed);
    have = true;
    have_seed = seed;
  }
  for (int p = 0; p < kNumPaths; ++p) e->digest[p] = (path_mask >> p) & 1u ? all[p] : 0u;
}

// The LDS-DMA source: [step][wave][64][4] of src(ldsdma, step, word, lane).
int fill_dma_source(uint32_t seed, DevMem& buf) {
  std::vector<uint32_t> g(kDmaWords);
  for (uint32_t s = 0; s < kDmaSteps; ++s)
    for (uint32_t t = 0; t < kBlock; ++t)
      for (uint32_t j = 0; j < 4; ++j) g[(s * kBlock + t) * 4 + j] = srcv(seed, kLdsDma, s, j, t);
  XS_CHECK(hipMalloc(&buf.p, kDmaWords * 4));
  XS_CHECK(hipMemcpy(buf.p, g.data(), kDmaWords * 4, hipMemcpyHostToDevice));
  return 0;
}

}  // namespace

extern "C" {

const char* xs_lane_sweep_last_error() { return g_lane_err; }

// Path names, comma-separated, in bit order.
const char* xs_lane_paths() { return kPathNames; }

// out2 = {steps, words per step}.
int xs_lane_shape(int path, int* out2) {
  if (path < 0 || path >= kNumPaths || !out2) return kBadArgs;
  out2[0] = kShape[path].steps;
  out2[1] = kShape[path].words;
  return 0;
}

// One workgroup runs `path` and stores every value it received:
// out[step][word][256], n_words = steps x words x 256.
int xs_lane_probe(int dev, int path, uint32_t seed, uint32_t* out, size_t n_words) {
  if (path < 0 || path >= kNumPaths || !out) return kBadArgs;
  const size_t n = static_cast<size_t>(kShape[path].steps) * kShape[path].words * kBlock;
  if (n_words != n) return kBadArgs;
  DevMem dma;
  return launch_probe(
      g_lane_err, dev, reinterpret_cast<const void*>(k_lane_probe), kBlock, kLdsUsed, out, n,
      [&](dim3 grid, dim3 block, size_t smem, void* dump) {
        hipLaunchKernelGGL(k_lane_probe, grid, block, smem, 0, static_cast<uint32_t*>(dump), dma.as<const uint32_t>(),
                           path, seed);
      },
      [&] { return fill_dma_source(seed, dma); });
}

// Host only. out8[p] = the workgroup digest a healthy CU leaves for path p, 0
// for a path outside path_mask.
int xs_lane_sweep_expected(uint32_t path_mask, uint32_t seed, uint32_t* out8) {
  if (bad_part_mask(path_mask, kAllPaths) || !out8) return kBadArgs;
  Expect e;
  expected(path_mask, seed, &e);
  for (int p = 0; p < kNumPaths; ++p) out8[p] = e.digest[p];
  return 0;
}

// What the runtime reports for k_lane_sweep on `dev`: out4 = {registers per
// lane, scratch bytes per lane, dynamic LDS bytes per workgroup, workgroups
// that fit on a CU at once}.
int xs_lane_sweep_info(int dev, int* out4) {
  return sweep_info(g_lane_err, dev, reinterpret_cast<const void*>(k_lane_sweep), kBlock, true, out4);
}

// One sweep launch of `blocks` workgroups (0: 4 per CU). Writes `blocks`
// 128-byte records to records_out (the caller's buffer holds at least that
// many; with blocks == 0, 4 x computeUnits). Returns 0, -1000 for bad
// arguments (nothing is launched), or a negative HIP error.
int xs_lane_sweep(int dev, int blocks, uint32_t path_mask, uint32_t seed, int inject_xcd, int inject_cu,
                  uint32_t inject_paths, void* records_out, int* n_records, double* ms) {
  if (bad_part_mask(path_mask, kAllPaths) || (inject_paths & ~kAllPaths)) return kBadArgs;
  Expect e;
  expected(path_mask, seed, &e);
  DevMem dma;
  return launch_sweep(
      g_lane_err, {dev, blocks, inject_xcd, inject_cu, records_out, n_records, ms},
      reinterpret_cast<const void*>(k_lane_sweep), kBlock, kLdsUsed, sizeof(LaneRecord),
      [&](dim3 grid, dim3 block, size_t smem, void* rec) {
        hipLaunchKernelGGL(k_lane_sweep, grid, block, smem, 0, static_cast<LaneRecord*>(rec), dma.as<const uint32_t>(),
                           path_mask, seed, inject_xcd, inject_cu, inject_paths, e);
      },
      [&] { return fill_dma_source(seed, dma); });
}

}  // extern "C"
