// Memory-path sweep for gfx950 (MI355X): what lies between a wave's registers
// and HBM, on every CU. The vector-memory instructions (address generation,
// width and sign handling, the d16 merges), the buffer descriptor's stride and
// range check, the flat apertures, the memory-side atomic units, the vector L1
// of the CU, the L2 of its XCD, and the scalar data cache.
//
// k_mem_sweep is the same kind of launch as k_lane_sweep (256-thread
// workgroups, 4 waves: one per SIMD, each holding more than half of a CU's
// LDS, 4 x CUs of them, every workgroup self-contained). Everything is data
// movement or arithmetic with one exact answer: no tolerance.
//
// The arena. One device allocation holds a private slab per workgroup, keyed
// by blockIdx.x, 144 KiB apart:
//   [  0 KiB,   4 KiB)  guard band
//   [  4 KiB, 132 KiB)  the tile: `l2` uses all 128 KiB, `l1` its first 16 KiB
//   [132 KiB, 136 KiB)  work area of gwidth, flat and atomic: 1 KiB per wave,
//                       64 slots of 16 B
//   [136 KiB, 140 KiB)  buffer area of `buffer`, laid out the same way
//   [140 KiB, 144 KiB)  guard band
// The host fills the whole arena, guard bands included, with the sentinel
// sent(i) = i * 0x9e3779b1 ^ 0xa5a5a5a5 (i = the word's index in its 144 KiB,
// so that every workgroup's digest is the same) before the launch and checks
// every guard band after it: a stray store is error -1004. No workgroup touches another's slab, so the sweep needs no
// cross-workgroup ordering and no agent-scope fence. Within a workgroup a value
// written by one wave and read by another is separated by __syncthreads(), and
// every asm statement ends with its own s_waitcnt, so nothing is in flight
// behind it. A read that follows an atomic on the same word is a load with sc1:
// atomics execute at the memory side and do not refresh the CU's L1.
//
// Values. fmix32 is the murmur3 finaliser, a bijection of 32 bits (part_sweep.h).
//   src(r, s, w, l) = fmix32(seed ^ (r << 24 | s << 12 | w << 6 | l))
//   aux(r, s, w, l) = fmix32(seed ^ (1 << 28 | r << 24 | s << 12 | w << 6 | l))
//   til(r, d)       = fmix32(seed ^ (2 << 28 | r << 24 | d))     tile dword d
//   new(r, d)       = fmix32(seed ^ (3 << 28 | r << 24 | d))     a rewritten dword
// r = route, s = step, l = lane (0..63), w = 4 * wave + word. All keys of a
// launch differ, so all values do. Thread t = 64 * wave + lane l. x0..x3 =
// src(words 0..3), a0..a3 = aux(words 0..3) of the step.
// slot(k, l) = ((2k + 3) * l + k) % 64: the 16-byte slot of its wave's KiB
// that lane l uses in step k; odd multiplier, a bijection, and neighbouring
// lanes are 16 * (2k + 3) bytes apart, never the access width.
//
// Routes (bit, name, steps x words per step).
//  0 gwidth  18 x 4  global_load / global_store, step = 9 * v + combo, slot(step, l)
//                    at address A. `saddr` = slab base in SGPRs + 32-bit voffset.
//                      0 global_store_dwordx4        -> 4 x global_load_dword saddr, offset:0/4/8/12
//                      1 global_store_dwordx3 + global_store_dword offset:12 -> global_load_dwordx4
//                      2 2 x global_store_dwordx2 saddr -> global_load_dwordx3 + global_load_dword offset:12
//                      3 4 x global_store_dword      -> 2 x global_load_dwordx2
//                      4 8 x global_store_byte (x0, x1) -> ushort(x0 lo) sshort(x0 hi) sshort(x1 lo) ushort(x1 hi)
//                      5 4 x global_store_short (x0, x1) -> ubyte(x0 b0) sbyte(x0 b1) sbyte(x1 b2) ubyte(x1 b3)
//                      6 global_store_dwordx2 (x0, x1), then into registers that hold a0..a3:
//                        global_load_short_d16 at A, global_load_short_d16_hi at A + 2 (vaddr A + 18,
//                        offset:-16), global_load_ubyte_d16 at A + 5, global_load_sbyte_d16_hi at A + 7
//                      7 global_store_dwordx2 (a0, a1), global_store_short_d16_hi x0 at A,
//                        global_store_byte_d16_hi x1 at A + 5 -> global_load_dwordx2 (words 0, 1);
//                        global_load_ubyte_d16_hi at A + 1 into a2, global_load_sbyte_d16 at A + 5 into a3
//                      8 the immediate offset's ends, 4095 and -4096:
//                        global_store_dword vaddr A - 4095 offset:4095 -> global_load_dword saddr offset:-4096
//                        global_store_dword saddr offset:-4096 -> global_load_dword vaddr offset:4095
//                        global_store_dwordx2 vaddr offset:-4096 -> global_load_dwordx2 saddr offset:4095
//                    sbyte / sshort results are sign-extended.
//  1 buffer  12 x 4  buffer_load / buffer_store, step = 6 * v + combo, slot(step, l) of
//                    the wave's KiB of the buffer area. Two descriptors per wave, both
//                    over that KiB and both ending inside it: R (stride 0, num_records
//                    768 bytes) and S (stride 16, num_records 48). A lane whose slot is
//                    48 or higher is wholly out of range: its loads return 0, its stores
//                    are dropped. index = slot, offset = byte in the slot.
//                      0 buffer_store_dwordx4 R offen -> 4 x buffer_load_dword R offen offset:0/4/8/12
//                      1 4 x buffer_store_dword S idxen offset:0/4/8/12 -> buffer_load_dwordx4 S idxen
//                      2 2 x buffer_store_dwordx2 S idxen offen -> buffer_load_dwordx3 R offen +
//                        buffer_load_dword R offen, SGPR soffset 12
//                      3 buffer_store_dwordx3 R offen + buffer_store_dword R offen, SGPR soffset 12
//                        -> 2 x buffer_load_dwordx2 S idxen offen sc1
//                      4 4 x buffer_store_byte (x0) + 2 x buffer_store_short (x1) R offen ->
//                        buffer_load_ubyte (x0 b0) buffer_load_sbyte (x0 b3) buffer_load_ushort (x1 lo)
//                        buffer_load_sshort (x1 hi)
//                      5 buffer_store_dwordx4 R offen -> global_load_dwordx4 of the slot: a lane
//                        out of range reads the host's sentinel, which nothing has overwritten
//  2 flat     8 x 4  flat_load / flat_store through generic pointers, step = 4 * v + combo,
//                    slot(step, l). A lane with (l + step) odd uses its slot of the wave's
//                    KiB of LDS, the others their slot of the work area: both apertures in
//                    every instruction. No pointer to private memory.
//                      0 flat_store_dwordx4 -> 4 x flat_load_dword offset:0/4/8/12
//                      1 4 x flat_store_dword -> flat_load_dwordx4
//                      2 2 x flat_store_dwordx2 -> flat_load_dwordx3 + flat_load_dword offset:12
//                      3 2 x flat_store_short (x0) + 4 x flat_store_byte (x1) -> flat_load_ushort (x0 lo)
//                        flat_load_sshort (x0 hi) flat_load_ubyte (x1 b0) flat_load_sbyte (x1 b3)
//  3 atomic  25 x 4  global atomics with return (sc0), each lane on its own slot(step, l)
//                    of the work area. The word is set with global_store_dword and read
//                    after the atomic with global_load_dword sc1.
//                    Steps 0-12: add sub smin smax umin umax and or xor swap cmpswap inc dec,
//                    two data sets j = 0, 1: the word holds a = src(word 2j), the operand
//                    is b = aux(word 2j); word 2j is the returned value, word 2j + 1 the
//                    word left in memory. cmpswap compares with a (j = 0: it swaps) and
//                    a ^ 1 (j = 1: it does not). For j = 1, inc has b = a on even lanes
//                    (the wrap to 0) and b = 0xffffffff on odd ones; dec has a = 0 on even
//                    lanes (the wrap to b) and b = 0xffffffff on odd ones.
//                    Steps 13-17: add_x2 smin_x2 umax_x2 swap_x2 cmpswap_x2 on a = src(words
//                    0, 1), b = aux(words 0, 1) (low, high): words 0, 1 returned, words 2,
//                    3 left. cmpswap_x2 compares with a on even lanes, a ^ 1 on odd ones.
//                    Steps 18-20: global_atomic_add_f32, pk_add_f16, pk_add_bf16, data sets as in
//                    steps 0-12, operands small integers (below), every sum exact.
//                    Steps 21-23: global_atomic_add_f64, min_f64, max_f64, words as in 13-17.
//                    Step 24: all 256 lanes on one word per operation, the four words of
//                    slot 0 of wave 0, which hold aux(word j, thread 0): global_atomic_add of
//                    1, global_atomic_or of 1 << (t % 32), global_atomic_umax and
//                    global_atomic_xor of src(word j). Only the four final words are taken
//                    (sc1 loads by every lane): the returns depend on the arrival order.
//  4 l1      64 x 4  a 16 KiB tile, half the vector L1: 128 lines of 32 dwords, dword d =
//                    til(4, d), written once with global_store_dwordx4 (thread t the 16-byte
//                    chunks t + 256 i). Four passes p, each of 64 global_load_dword per lane,
//                    four to a step (step = 16 p + i / 4, word = i % 4): plain loads in passes
//                    0 and 2, sc0 loads in 1 and 3. Load i of wave w reads line pair
//                    q = (m[p] * i + 17 w + p) % 64, m = {5, 13, 27, 45}: lane l line
//                    2q + ((l >> 5) ^ (i & 1)), dword (5 (l % 32) + i) % 32 of it. Before pass
//                    2, wave 0 rewrites one dword per line: lane l the dword (5 l + 3) % 32 of
//                    lines l and l + 64 with new(4, d); after a barrier passes 2 and 3 of every
//                    wave must see it.
//  5 l2     512 x 4  the 128 KiB tile, four times the L1: 8192 chunks of 16 B, dword d =
//                    til(5, d), written with global_store_dwordx4. Four passes p, each of 128
//                    global_load_dwordx4 per lane through saddr (step = 128 p + i): pass 0 sc1,
//                    pass 1 nt, passes 2 and 3 plain. Load i of wave w reads chunk group
//                    g = (m[p] * i + 37 w + p) % 128, m = {5, 29, 67, 111}: lane l chunk
//                    64 g + (9 l + 5 p) % 64. Between passes 2 and 3 the tile is rewritten with
//                    the complement.
//  6 scalar   8 x 36 the scalar data cache, from a read-only table of 1024 dwords that the
//                    host uploads before the launch, tab(i) = til(6, i). The kernel never
//                    writes it. Per step the seven instructions s_load_dword, _dwordx2,
//                    _dwordx4, _dwordx8, _dwordx16, s_buffer_load_dword, _dwordx4 (n = 0..6, of
//                    1, 2, 4, 8, 16, 1, 4 dwords; words 0, 1-2, 3-6, 7-14, 15-30, 31, 32-35)
//                    read at dword offset o = (aux(8 * step + n, word 0 of wave w, lane 0) %
//                    (1024 / size)) * size, wave-uniform, in an SGPR; _dwordx2 takes the immediate offset
//                    0x40 from a base moved back by as much. Every lane receives the same
//                    SGPR value, moved to a VGPR.
//
// The ISA's rules the comparator is written from:
//   load ubyte / ushort   zero-extend, sbyte / sshort sign-extend to 32 bits
//   load *_d16            bits [15:0] of the destination <- the (extended) value, [31:16] <- 0
//   load *_d16_hi         bits [31:16] <- the value, [15:0] <- 0 (the hardware's rule, see below)
//   store byte / short    the low 8 / 16 bits of the data register; *_d16_hi: bits [23:16] / [31:16]
//   saddr form            address = SGPR pair + voffset + immediate; vaddr form: VGPR pair + immediate
//   buffer, stride 0      address = base + soffset + voffset + immediate; out of range when
//                         voffset + immediate + size > num_records (whether soffset is part
//                         of the check makes no difference here: every access lies inside or outside either way)
//   buffer, idxen         address = base + soffset + index * stride + voffset + immediate; out of
//                         range when index >= num_records
//   out of range          a load returns 0, a store is dropped
//   inc                   mem = old >= b ? 0 : old + 1       dec   mem = old == 0 || old > b ? b : old - 1
//   cmpswap               data = {new, compare}: mem = old == compare ? new : old
//   smin / smax signed, umin / umax unsigned; every atomic returns old
//   float atomics         the word and the operand are the integers below in the format, made
//                         from the hashes h = src (the word) and h = aux (the operand) of the
//                         data set (of word 0 for f64):
//                           f32   word 4096 + h[11:0]; operand +-(1024 + h[9:0])
//                           f16   low half 256 + h[7:0], high half 256 + h[15:8], word and operand
//                           bf16  low half 64 + h[4:0], high half 64 + h[12:8], word and operand
//                           f64 add   word 2^30 + h[29:0]; operand +-(2^29 + h[28:0])
//                           f64 min, max   word and operand +-(2^30 + h[29:0])
//                         +- is bit 31 of h. Every operand and result is an integer that fits
//                         the format's significand: exact, finite, normal, never zero.
//
// What the hardware settled (the first probe against the numpy reference
// differed in exactly these cells, every other rule stood as written): the ISA
// text has a d16 load keep the other half of its destination; the MI355X, whose
// register file is ECC-protected and written a dword at a time, writes zero
// there (the compiler knows: with sramecc on it never relies on the kept
// half). The destinations still hold a0..a3 before the load, so a part that
// kept the half would mis-compare. The d16_hi STORES behave as documented.
//
// Comparison. Each lane computes what it must receive with integer VALU only
// (float results as the bit pattern of the integer), counts mismatches per
// route and accumulates D_r += got * (2 idx + 1), idx = (step * words + word)
// * 256 + t. part_sweep.h's reduce_parts() makes the record.
//
// Record (128 bytes per workgroup): part_sweep.h's head with a route per part,
// thirteen reserved words.
//
// Injection: as in lane_sweep.hip, bit 0 of the value thread 0 received in
// step 0, word 0 of each route in inject_routes. Registers only.
//
// k_mem_probe is one workgroup of the same device code with a dump pointer: it
// stores every received value of one route as [step][word][256]. That is what
// tests/test_gpu_mem_sweep.py holds against tests/mem_sweep_ref.py.
//
// What is claimed. Every value passes from registers through the address
// unit, the L1, the L2 and back. The tile sizes make l1's re-reads fit the L1
// and l2's exceed it; WHICH level served a given read is the hardware's choice
// and the sweep does not observe it. Whether every L2 set is reached is not
// claimed.
//
// NOT covered: an access partly outside a buffer's range, buffer atomics, the
// typed (format) buffer instructions, swizzled buffers, flat access to
// private memory, global_load_lds (lane_sweep.hip has it), the 64-bit integer
// atomics other than the five listed, f32 / f16 min and max atomics, scalar
// loads across a page boundary, the Infinity Cache and the instruction cache.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <mutex>
#include <utility>
#include <vector>

#include "hip/part_sweep.h"

#define XS_ERR_BUF g_mem_err
#define XS_HD __host__ __device__ __forceinline__
#define XS_D __device__ __forceinline__

namespace {

xsprobe::ErrBuf g_mem_err;

using namespace xsprobe;

typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x3 __attribute__((ext_vector_type(3)));
typedef uint32_t u32x8 __attribute__((ext_vector_type(8)));
typedef uint32_t u32x16 __attribute__((ext_vector_type(16)));

enum Route : int { kGwidth, kBuffer, kFlat, kAtomic, kL1, kL2, kScalar, kNumRoutes };
const char kRouteNames[] = "gwidth,buffer,flat,atomic,l1,l2,scalar";
constexpr uint32_t kAllRoutes = (1u << kNumRoutes) - 1;

struct Shape {
  int steps, words;
};
constexpr Shape kShape[kNumRoutes] = {{18, 4}, {12, 4}, {8, 4}, {25, 4}, {64, 4}, {512, 4}, {8, 36}};

constexpr int kBlock = kPartBlock;
constexpr int kUnswept = -1003;
constexpr int kStrayStore = -1004;

// The slab, in bytes from its guard band's start.
constexpr uint32_t kGuard = 4096;
constexpr uint32_t kTileBytes = 128u << 10;
constexpr uint32_t kL1Bytes = 16u << 10;
constexpr uint32_t kWorkOff = kTileBytes;  // from the slab's first byte behind the guard band
constexpr uint32_t kBufOff = kWorkOff + 4096;
constexpr uint32_t kSlabBytes = kBufOff + 4096;
constexpr size_t kStride = kGuard + kSlabBytes + kGuard;
static_assert(kStride == (144u << 10), "144 KiB per workgroup");
constexpr uint32_t kWaveBytes = 1024, kSlot = 16;
constexpr uint32_t kRangeSlots = 48, kRangeBytes = kRangeSlots * kSlot;  // where the descriptors end

constexpr uint32_t kTableWords = 1024;
constexpr size_t kHostGroup = 64;  // workgroups' worth of arena the host builds or checks at a time

// LDS: the reduction's words, then a KiB per wave for `flat`.
constexpr uint32_t kRedBytes = part_reduction_words(kNumRoutes, 0) * 4;
constexpr uint32_t kFlatLdsOff = kRedBytes;
constexpr uint32_t kLdsUsed = kFlatLdsOff + 4 * kWaveBytes;
static_assert(kFlatLdsOff % 16 == 0 && kLdsUsed <= (64u << 10), "LDS layout");

struct MemRecord {
  PartRecordHead<kNumRoutes> head;
  uint32_t reserved[13];
};
static_assert(sizeof(MemRecord) == 128, "one 128-byte record per workgroup");

using Expect = PartExpect<kNumRoutes>;

// ------------------------------------------------------------------- values
XS_HD uint32_t srcv(uint32_t seed, uint32_t r, uint32_t s, uint32_t word, uint32_t t) {
  return fmix32(seed ^ (r << 24 | s << 12 | (4u * (t >> 6) + word) << 6 | (t & 63u)));
}
XS_HD uint32_t auxv(uint32_t seed, uint32_t r, uint32_t s, uint32_t word, uint32_t t) {
  return fmix32(seed ^ (1u << 28 | r << 24 | s << 12 | (4u * (t >> 6) + word) << 6 | (t & 63u)));
}
XS_HD uint32_t tilv(uint32_t seed, uint32_t r, uint32_t d) { return fmix32(seed ^ (2u << 28 | r << 24 | d)); }
XS_HD uint32_t newv(uint32_t seed, uint32_t r, uint32_t d) { return fmix32(seed ^ (3u << 28 | r << 24 | d)); }
// word_index: of the word in its workgroup's 144 KiB, guard band included.
XS_HD uint32_t sentinel(uint32_t word_index) { return word_index * 0x9e3779b1u ^ 0xa5a5a5a5u; }

XS_HD uint32_t slot_of(uint32_t k, uint32_t l) { return ((2u * k + 3u) * l + k) & 63u; }

XS_HD uint32_t sext(uint32_t v, int bits) {
  return static_cast<uint32_t>(static_cast<int32_t>(v << (32 - bits)) >> (32 - bits));
}

// The bit pattern of the integer `mag` > 0 in a binary format of `mant`
// explicit significand bits and exponent bias `bias`; mag < 2^(mant + 1).
XS_HD uint64_t fp_bits(uint64_t mag, int mant, int bias) {
  const int e = 63 - __builtin_clzll(mag);
  return static_cast<uint64_t>(e + bias) << mant | (mag - (1ull << e)) << (mant - e);
}
XS_HD uint32_t f32_of(int32_t v) {
  return v < 0 ? 0x80000000u | static_cast<uint32_t>(fp_bits(static_cast<uint64_t>(-static_cast<int64_t>(v)), 23, 127))
               : static_cast<uint32_t>(fp_bits(static_cast<uint64_t>(v), 23, 127));
}
XS_HD uint64_t f64_of(int64_t v) {
  return v < 0 ? 1ull << 63 | fp_bits(static_cast<uint64_t>(-v), 52, 1023) : fp_bits(static_cast<uint64_t>(v), 52, 1023);
}
XS_HD uint32_t f16_of(uint32_t v) { return static_cast<uint32_t>(fp_bits(v, 10, 15)); }
XS_HD uint32_t bf16_of(uint32_t v) { return static_cast<uint32_t>(fp_bits(v, 7, 127)); }

// ------------------------------------------------------------ atomic operands
enum AtomOp : int {
  kAdd, kSub, kSmin, kSmax, kUmin, kUmax, kAnd, kOr, kXor, kSwap, kCmpswap, kInc, kDec,  // 0-12
  kAddX2, kSminX2, kUmaxX2, kSwapX2, kCmpswapX2,                                         // 13-17
  kAddF32, kPkAddF16, kPkAddBf16,                                                        // 18-20
  kAddF64, kMinF64, kMaxF64,                                                             // 21-23
  kContended                                                                             // 24
};

struct Atom32 {
  uint32_t a, b, cmp;  // the word, the operand, cmpswap's compare value
};
// Steps 0-12 and 18-20, data set j.
XS_HD Atom32 atom32(uint32_t seed, int op, int j, uint32_t t) {
  const uint32_t ha = srcv(seed, kAtomic, op, 2 * j, t), hb = auxv(seed, kAtomic, op, 2 * j, t);
  Atom32 o{ha, hb, ha ^ static_cast<uint32_t>(j)};
  const bool odd = t & 1u;
  if (op == kInc && j == 1) o.b = odd ? 0xffffffffu : ha;
  if (op == kDec && j == 1) {
    if (odd) o.b = 0xffffffffu;
    else o.a = 0;
  }
  if (op == kAddF32) {
    const int32_t m = static_cast<int32_t>(0x400u | (hb & 0x3ffu));
    o.a = f32_of(static_cast<int32_t>(0x1000u | (ha & 0xfffu)));
    o.b = f32_of(hb >> 31 ? -m : m);
  }
  if (op == kPkAddF16) {
    o.a = f16_of(256u + (ha & 0xffu)) | f16_of(256u + ((ha >> 8) & 0xffu)) << 16;
    o.b = f16_of(256u + (hb & 0xffu)) | f16_of(256u + ((hb >> 8) & 0xffu)) << 16;
  }
  if (op == kPkAddBf16) {
    o.a = bf16_of(64u + (ha & 31u)) | bf16_of(64u + ((ha >> 8) & 31u)) << 16;
    o.b = bf16_of(64u + (hb & 31u)) | bf16_of(64u + ((hb >> 8) & 31u)) << 16;
  }
  return o;
}
// The word an atomic of steps 0-12, 18-20 leaves.
XS_HD uint32_t atom32_result(uint32_t seed, int op, int j, uint32_t t) {
  const Atom32 o = atom32(seed, op, j, t);
  const uint32_t a = o.a, b = o.b;
  const uint32_t ha = srcv(seed, kAtomic, op, 2 * j, t), hb = auxv(seed, kAtomic, op, 2 * j, t);
  switch (op) {
    case kAdd: return a + b;
    case kSub: return a - b;
    case kSmin: return static_cast<uint32_t>(std::min(static_cast<int32_t>(a), static_cast<int32_t>(b)));
    case kSmax: return static_cast<uint32_t>(std::max(static_cast<int32_t>(a), static_cast<int32_t>(b)));
    case kUmin: return std::min(a, b);
    case kUmax: return std::max(a, b);
    case kAnd: return a & b;
    case kOr: return a | b;
    case kXor: return a ^ b;
    case kSwap: return b;
    case kCmpswap: return a == o.cmp ? b : a;
    case kInc: return a >= b ? 0u : a + 1u;
    case kDec: return a == 0u || a > b ? b : a - 1u;
    case kAddF32: {
      const int32_t m = static_cast<int32_t>(0x400u | (hb & 0x3ffu));
      return f32_of(static_cast<int32_t>(0x1000u | (ha & 0xfffu)) + (hb >> 31 ? -m : m));
    }
    case kPkAddF16:
      return f16_of(512u + (ha & 0xffu) + (hb & 0xffu)) | f16_of(512u + ((ha >> 8) & 0xffu) + ((hb >> 8) & 0xffu)) << 16;
    default:  // kPkAddBf16
      return bf16_of(128u + (ha & 31u) + (hb & 31u)) | bf16_of(128u + ((ha >> 8) & 31u) + ((hb >> 8) & 31u)) << 16;
  }
}

struct Atom64 {
  uint64_t a, b, cmp, result;
};
// Steps 13-17 and 21-23.
XS_HD Atom64 atom64(uint32_t seed, int op, uint32_t t) {
  const uint32_t a0 = srcv(seed, kAtomic, op, 0, t), a1 = srcv(seed, kAtomic, op, 1, t);
  const uint32_t b0 = auxv(seed, kAtomic, op, 0, t), b1 = auxv(seed, kAtomic, op, 1, t);
  Atom64 o{a0 | static_cast<uint64_t>(a1) << 32, b0 | static_cast<uint64_t>(b1) << 32, 0, 0};
  o.cmp = o.a ^ (t & 1u);
  switch (op) {
    case kAddX2: o.result = o.a + o.b; break;
    case kSminX2: o.result = static_cast<uint64_t>(std::min(static_cast<int64_t>(o.a), static_cast<int64_t>(o.b))); break;
    case kUmaxX2: o.result = std::max(o.a, o.b); break;
    case kSwapX2: o.result = o.b; break;
    case kCmpswapX2: o.result = o.a == o.cmp ? o.b : o.a; break;
    case kAddF64: {
      const int64_t ai = static_cast<int64_t>((a0 & 0x3fffffffu) | 0x40000000u);
      const int64_t bm = static_cast<int64_t>((b0 & 0x1fffffffu) | 0x20000000u), bi = b0 >> 31 ? -bm : bm;
      o.a = f64_of(ai), o.b = f64_of(bi), o.result = f64_of(ai + bi);
      break;
    }
    default: {  // kMinF64, kMaxF64
      const int64_t am = static_cast<int64_t>((a0 & 0x3fffffffu) | 0x40000000u), ai = a0 >> 31 ? -am : am;
      const int64_t bm = static_cast<int64_t>((b0 & 0x3fffffffu) | 0x40000000u), bi = b0 >> 31 ? -bm : bm;
      o.a = f64_of(ai), o.b = f64_of(bi);
      o.result = f64_of(op == kMinF64 ? std::min(ai, bi) : std::max(ai, bi));
    }
  }
  return o;
}

// The operand of thread t in the contended step, word j.
XS_HD uint32_t contended_operand(uint32_t seed, int j, uint32_t t) {
  return j == 0 ? 1u : j == 1 ? 1u << (t & 31u) : srcv(seed, kAtomic, kContended, j, t);
}

// --------------------------------------------------------------- tile maps
// The dword of the l1 tile that load i (0..63) of pass p reads in thread t.
XS_HD uint32_t l1_dword(uint32_t p, uint32_t i, uint32_t t) {
  constexpr uint32_t mul[4] = {5, 13, 27, 45};
  const uint32_t l = t & 63u, w = t >> 6;
  const uint32_t q = (mul[p] * i + 17u * w + p) & 63u;
  const uint32_t line = 2u * q + ((l >> 5) ^ (i & 1u));
  return line * 32u + ((5u * (l & 31u) + i) & 31u);
}
// Whether wave 0 rewrites dword d of the l1 tile before pass 2.
XS_HD bool l1_rewritten(uint32_t d) {
  const uint32_t line = d >> 5;
  return (d & 31u) == ((5u * (line & 63u) + 3u) & 31u);
}
// The 16-byte chunk of the l2 tile that load i (0..127) of pass p reads in thread t.
XS_HD uint32_t l2_chunk(uint32_t p, uint32_t i, uint32_t t) {
  constexpr uint32_t mul[4] = {5, 29, 67, 111};
  const uint32_t l = t & 63u, w = t >> 6;
  const uint32_t g = (mul[p] * i + 37u * w + p) & 127u;
  return 64u * g + ((9u * l + 5u * p) & 63u);
}

// Scalar route: sizes and first words of the seven instructions.
XS_HD constexpr uint32_t scalar_size(int n) {
  return n == 0 ? 1 : n == 1 ? 2 : n == 2 ? 4 : n == 3 ? 8 : n == 4 ? 16 : n == 5 ? 1 : 4;
}
XS_HD constexpr uint32_t scalar_first(int n) {
  return n == 0 ? 0 : n == 1 ? 1 : n == 2 ? 3 : n == 3 ? 7 : n == 4 ? 15 : n == 5 ? 31 : 32;
}
// The dword offset instruction n of step s reads at in the wave of thread t.
XS_HD uint32_t scalar_offset(uint32_t seed, int s, int n, uint32_t t) {
  const uint32_t size = scalar_size(n);
  return auxv(seed, kScalar, 8u * s + n, 0, t & ~63u) % (kTableWords / size) * size;
}

// ------------------------------------------------- what a lane must receive
XS_HD uint32_t want_gwidth(uint32_t seed, int s, int word, uint32_t t) {
  const int combo = s % 9;
  const uint32_t x0 = srcv(seed, kGwidth, s, 0, t), x1 = srcv(seed, kGwidth, s, 1, t);
  switch (combo) {
    case 4:
      switch (word) {
        case 0: return x0 & 0xffffu;
        case 1: return sext(x0 >> 16, 16);
        case 2: return sext(x1 & 0xffffu, 16);
        default: return x1 >> 16;
      }
    case 5:
      switch (word) {
        case 0: return x0 & 0xffu;
        case 1: return sext((x0 >> 8) & 0xffu, 8);
        case 2: return sext((x1 >> 16) & 0xffu, 8);
        default: return x1 >> 24;
      }
    case 6:
      switch (word) {
        case 0: return x0 & 0xffffu;
        case 1: return x0 & 0xffff0000u;
        case 2: return (x1 >> 8) & 0xffu;
        default: return (sext(x1 >> 24, 8) & 0xffffu) << 16;
      }
    case 7: {
      const uint32_t a0 = auxv(seed, kGwidth, s, 0, t), a1 = auxv(seed, kGwidth, s, 1, t);
      switch (word) {
        case 0: return (a0 & 0xffff0000u) | (x0 >> 16);
        case 1: return (a1 & 0xffff00ffu) | ((x1 >> 16) & 0xffu) << 8;
        case 2: return (x0 >> 24) << 16;
        default: return sext((x1 >> 16) & 0xffu, 8) & 0xffffu;
      }
    }
    default: return srcv(seed, kGwidth, s, word, t);
  }
}

XS_HD uint32_t want_buffer(uint32_t seed, int s, int word, uint32_t t) {
  const int combo = s % 6;
  const uint32_t slot = slot_of(s, t & 63u);
  if (slot >= kRangeSlots)
    return combo == 5 ? sentinel((kGuard + kBufOff + (t >> 6) * kWaveBytes + slot * kSlot) / 4u + word) : 0u;
  if (combo != 4) return srcv(seed, kBuffer, s, word, t);
  const uint32_t x0 = srcv(seed, kBuffer, s, 0, t), x1 = srcv(seed, kBuffer, s, 1, t);
  switch (word) {
    case 0: return x0 & 0xffu;
    case 1: return sext(x0 >> 24, 8);
    case 2: return x1 & 0xffffu;
    default: return sext(x1 >> 16, 16);
  }
}

XS_HD uint32_t want_flat(uint32_t seed, int s, int word, uint32_t t) {
  if (s % 4 != 3) return srcv(seed, kFlat, s, word, t);
  const uint32_t x0 = srcv(seed, kFlat, s, 0, t), x1 = srcv(seed, kFlat, s, 1, t);
  switch (word) {
    case 0: return x0 & 0xffffu;
    case 1: return sext(x0 >> 16, 16);
    case 2: return x1 & 0xffu;
    default: return sext(x1 >> 24, 8);
  }
}

// The contended step's four final words: the same for every thread.
struct Contended {
  uint32_t v[4];
};
XS_HD Contended contended_final(uint32_t seed) {
  Contended c;
  for (int j = 0; j < 4; ++j) c.v[j] = auxv(seed, kAtomic, kContended, j, 0);
  for (uint32_t u = 0; u < kBlock; ++u) {
    c.v[0] += contended_operand(seed, 0, u);
    c.v[1] |= contended_operand(seed, 1, u);
    c.v[2] = std::max(c.v[2], contended_operand(seed, 2, u));
    c.v[3] ^= contended_operand(seed, 3, u);
  }
  return c;
}

XS_HD uint32_t want_atomic(uint32_t seed, int s, int word, uint32_t t, const Contended& fin) {
  if (s == kContended) return fin.v[word];
  if (s <= kDec || (s >= kAddF32 && s <= kPkAddBf16))
    return word & 1 ? atom32_result(seed, s, word >> 1, t) : atom32(seed, s, word >> 1, t).a;
  const Atom64 o = atom64(seed, s, t);
  return static_cast<uint32_t>((word < 2 ? o.a : o.result) >> (32 * (word & 1)));
}

XS_HD uint32_t want_l1(uint32_t seed, int s, int word, uint32_t t) {
  const uint32_t p = static_cast<uint32_t>(s) >> 4, i = 4u * (static_cast<uint32_t>(s) & 15u) + word;
  const uint32_t d = l1_dword(p, i, t);
  return p >= 2 && l1_rewritten(d) ? newv(seed, kL1, d) : tilv(seed, kL1, d);
}

XS_HD uint32_t want_l2(uint32_t seed, int s, int word, uint32_t t) {
  const uint32_t p = static_cast<uint32_t>(s) >> 7, i = static_cast<uint32_t>(s) & 127u;
  const uint32_t v = tilv(seed, kL2, 4u * l2_chunk(p, i, t) + word);
  return p == 3 ? ~v : v;
}

XS_HD uint32_t want_scalar(uint32_t seed, int s, int word, uint32_t t) {
  int n = 6;
  while (static_cast<uint32_t>(word) < scalar_first(n)) --n;
  return tilv(seed, kScalar, scalar_offset(seed, s, n, t) + word - scalar_first(n));
}

// ------------------------------------------------------------------- device
struct Ctx {
  uint32_t seed, t, lane, wave, inj;
  uint32_t* dump;   // k_mem_probe only
  uint8_t* slab;    // the workgroup's slab behind its guard band, wave-uniform
};

template <int R>
XS_D void take(const Ctx& c, Tally& y, uint32_t step, uint32_t word, uint32_t got, uint32_t expect) {
  take_word(y, c.dump, (step * kShape[R].words + word) * kBlock + c.t, got, expect, (c.inj >> R) & 1u);
}

XS_D uint32_t rfl(uint32_t v) { return static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(v))); }

// Every statement waits for what it issued. The s_nop 4 opening a statement
// that reads SGPRs covers a readfirstlane just before it.
#define XS_VM "\n\ts_waitcnt vmcnt(0)"
#define XS_FLATW "\n\ts_waitcnt vmcnt(0) lgkmcnt(0)"
#define XS_SN "s_nop 4\n\t"

typedef uint64_t gaddr;  // a global or generic address in a VGPR pair

// op vdata..., vaddr form: text is "mnemonic" and tail is " offset:N sc1" or "".
#define XS_GSTORE(name, type, text, tail)                                                   \
  XS_D void name(gaddr a, type v) {                                                         \
    asm volatile(text " %0, %1, off" tail "\n\ts_nop 1" XS_VM ::"v"(a), "v"(v) : "memory"); \
  }
#define XS_GLOAD(name, type, text, tail)                                           \
  XS_D type name(gaddr a) {                                                        \
    type r;                                                                        \
    asm volatile(text " %0, %1, off" tail XS_VM : "=&v"(r) : "v"(a) : "memory"); \
    return r;                                                                      \
  }
// A d16 load merges into `r`.
#define XS_GLOAD16(name, text, tail)                                           \
  XS_D uint32_t name(gaddr a, uint32_t r) {                                    \
    asm volatile(text " %0, %1, off" tail XS_VM : "+v"(r) : "v"(a) : "memory"); \
    return r;                                                                  \
  }
#define XS_SSTORE(name, type, text, tail)                                                                \
  XS_D void name(const uint8_t* base, uint32_t off, type v) {                                            \
    asm volatile(XS_SN text " %0, %1, %2" tail "\n\ts_nop 1" XS_VM ::"v"(off), "v"(v), "s"(base) : "memory"); \
  }
#define XS_SLOAD(name, type, text, tail)                                                             \
  XS_D type name(const uint8_t* base, uint32_t off) {                                                \
    type r;                                                                                          \
    asm volatile(XS_SN text " %0, %1, %2" tail XS_VM : "=&v"(r) : "v"(off), "s"(base) : "memory"); \
    return r;                                                                                        \
  }

XS_GSTORE(g_st_x4, u32x4, "global_store_dwordx4", "")
XS_GSTORE(g_st_x3, u32x3, "global_store_dwordx3", "")
XS_GSTORE(g_st_x2, u32x2, "global_store_dwordx2", "")
XS_GSTORE(g_st_x1, uint32_t, "global_store_dword", "")
XS_GSTORE(g_st_x1_o12, uint32_t, "global_store_dword", " offset:12")
XS_GSTORE(g_st_x1_max, uint32_t, "global_store_dword", " offset:4095")
XS_GSTORE(g_st_x2_min, u32x2, "global_store_dwordx2", " offset:-4096")
XS_GSTORE(g_st_b8, uint32_t, "global_store_byte", "")
XS_GSTORE(g_st_b16, uint32_t, "global_store_short", "")
XS_GSTORE(g_st_b16_hi, uint32_t, "global_store_short_d16_hi", "")
XS_GSTORE(g_st_b8_hi_o5, uint32_t, "global_store_byte_d16_hi", " offset:5")
XS_SSTORE(s_st_x2, u32x2, "global_store_dwordx2", "")
XS_SSTORE(s_st_x1_min, uint32_t, "global_store_dword", " offset:-4096")
XS_SSTORE(s_st_x4, u32x4, "global_store_dwordx4", "")

XS_GLOAD(g_ld_x4, u32x4, "global_load_dwordx4", "")
XS_GLOAD(g_ld_x3, u32x3, "global_load_dwordx3", "")
XS_GLOAD(g_ld_x2, u32x2, "global_load_dwordx2", "")
XS_GLOAD(g_ld_x1_o12, uint32_t, "global_load_dword", " offset:12")
XS_GLOAD(g_ld_x1_max, uint32_t, "global_load_dword", " offset:4095")
XS_GLOAD(g_ld_x1_sc1, uint32_t, "global_load_dword", " sc1")
XS_GLOAD(g_ld_x2_sc1, u32x2, "global_load_dwordx2", " sc1")
XS_GLOAD(g_ld_u8, uint32_t, "global_load_ubyte", "")
XS_GLOAD(g_ld_i8, uint32_t, "global_load_sbyte", "")
XS_GLOAD(g_ld_u16, uint32_t, "global_load_ushort", "")
XS_GLOAD(g_ld_i16, uint32_t, "global_load_sshort", "")
XS_GLOAD16(g_ld_d16, "global_load_short_d16", "")
XS_GLOAD16(g_ld_d16_hi_m16, "global_load_short_d16_hi", " offset:-16")
XS_GLOAD16(g_ld_u8_d16_o5, "global_load_ubyte_d16", " offset:5")
XS_GLOAD16(g_ld_i8_d16_hi_o7, "global_load_sbyte_d16_hi", " offset:7")
XS_GLOAD16(g_ld_u8_d16_hi_o1, "global_load_ubyte_d16_hi", " offset:1")
XS_GLOAD16(g_ld_i8_d16_o5, "global_load_sbyte_d16", " offset:5")
XS_SLOAD(s_ld_x1, uint32_t, "global_load_dword", "")
XS_SLOAD(s_ld_x1_o4, uint32_t, "global_load_dword", " offset:4")
XS_SLOAD(s_ld_x1_o8, uint32_t, "global_load_dword", " offset:8")
XS_SLOAD(s_ld_x1_o12, uint32_t, "global_load_dword", " offset:12")
XS_SLOAD(s_ld_x1_min, uint32_t, "global_load_dword", " offset:-4096")
XS_SLOAD(s_ld_x2_max, u32x2, "global_load_dwordx2", " offset:4095")

XS_D void run_gwidth(const Ctx& c, Tally& y) {
  const uint32_t tile = kWorkOff + c.wave * kWaveBytes;
  for (int v = 0; v < 2; ++v) {
#pragma unroll
    for (int combo = 0; combo < 9; ++combo) {
      const int s = 9 * v + combo;
      const uint32_t off = tile + kSlot * slot_of(s, c.lane);  // from the slab
      const gaddr A = reinterpret_cast<gaddr>(c.slab) + off;
      uint32_t x[4], a[4], g[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) x[j] = srcv(c.seed, kGwidth, s, j, c.t), a[j] = auxv(c.seed, kGwidth, s, j, c.t);
      if (combo == 0) {
        g_st_x4(A, u32x4{x[0], x[1], x[2], x[3]});
        g[0] = s_ld_x1(c.slab, off), g[1] = s_ld_x1_o4(c.slab, off), g[2] = s_ld_x1_o8(c.slab, off);
        g[3] = s_ld_x1_o12(c.slab, off);
      } else if (combo == 1) {
        g_st_x3(A, u32x3{x[0], x[1], x[2]});
        g_st_x1_o12(A, x[3]);
        const u32x4 r = g_ld_x4(A);
        g[0] = r[0], g[1] = r[1], g[2] = r[2], g[3] = r[3];
      } else if (combo == 2) {
        s_st_x2(c.slab, off, u32x2{x[0], x[1]});
        s_st_x2(c.slab, off + 8, u32x2{x[2], x[3]});
        const u32x3 r = g_ld_x3(A);
        g[0] = r[0], g[1] = r[1], g[2] = r[2], g[3] = g_ld_x1_o12(A);
      } else if (combo == 3) {
#pragma unroll
        for (int j = 0; j < 4; ++j) g_st_x1(A + 4 * j, x[j]);
        const u32x2 lo = g_ld_x2(A), hi = g_ld_x2(A + 8);
        g[0] = lo[0], g[1] = lo[1], g[2] = hi[0], g[3] = hi[1];
      } else if (combo == 4) {
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          g_st_b8(A + b, x[0] >> (8 * b));
          g_st_b8(A + 4 + b, x[1] >> (8 * b));
        }
        g[0] = g_ld_u16(A), g[1] = g_ld_i16(A + 2), g[2] = g_ld_i16(A + 4), g[3] = g_ld_u16(A + 6);
      } else if (combo == 5) {
        g_st_b16(A, x[0]);
        g_st_b16(A + 2, x[0] >> 16);
        g_st_b16(A + 4, x[1]);
        g_st_b16(A + 6, x[1] >> 16);
        g[0] = g_ld_u8(A), g[1] = g_ld_i8(A + 1), g[2] = g_ld_i8(A + 6), g[3] = g_ld_u8(A + 7);
      } else if (combo == 6) {
        g_st_x2(A, u32x2{x[0], x[1]});
        g[0] = g_ld_d16(A, a[0]);
        g[1] = g_ld_d16_hi_m16(A + 18, a[1]);
        g[2] = g_ld_u8_d16_o5(A, a[2]);
        g[3] = g_ld_i8_d16_hi_o7(A, a[3]);
      } else if (combo == 7) {
        g_st_x2(A, u32x2{a[0], a[1]});
        g_st_b16_hi(A, x[0]);
        g_st_b8_hi_o5(A, x[1]);
        const u32x2 r = g_ld_x2(A);
        g[0] = r[0], g[1] = r[1];
        g[2] = g_ld_u8_d16_hi_o1(A, a[2]);
        g[3] = g_ld_i8_d16_o5(A, a[3]);
      } else {
        g_st_x1_max(A - 4095, x[0]);
        g[0] = s_ld_x1_min(c.slab, off + 4096);
        s_st_x1_min(c.slab, off + 4 + 4096, x[1]);
        g[1] = g_ld_x1_max(A + 4 - 4095);
        g_st_x2_min(A + 8 + 4096, u32x2{x[2], x[3]});
        const u32x2 r = s_ld_x2_max(c.slab, off + 8 - 4095);
        g[2] = r[0], g[3] = r[1];
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) take<kGwidth>(c, y, s, j, g[j], want_gwidth(c.seed, s, j, c.t));
    }
  }
}

// ------------------------------------------------------------------- buffer
// text " vdata, vaddr, srsrc, soffset" flags; `va` is the offset, the index, or
// {index, offset} for idxen offen.
#define XS_BSTORE(name, type, atype, text, flags)                                                                     \
  XS_D void name(u32x4 rsrc, atype va, uint32_t soff, type v) {                                                       \
    asm volatile(XS_SN text " %0, %1, %2, %3 " flags "\n\ts_nop 1" XS_VM ::"v"(v), "v"(va), "s"(rsrc), "s"(soff) : "memory"); \
  }
#define XS_BLOAD(name, type, atype, text, flags)                                                                  \
  XS_D type name(u32x4 rsrc, atype va, uint32_t soff) {                                                           \
    type r;                                                                                                       \
    asm volatile(XS_SN text " %0, %1, %2, %3 " flags XS_VM : "=&v"(r) : "v"(va), "s"(rsrc), "s"(soff) : "memory"); \
    return r;                                                                                                     \
  }
XS_BSTORE(b_st_x4_off, u32x4, uint32_t, "buffer_store_dwordx4", "offen")
XS_BSTORE(b_st_x3_off, u32x3, uint32_t, "buffer_store_dwordx3", "offen")
XS_BSTORE(b_st_x1_off, uint32_t, uint32_t, "buffer_store_dword", "offen")
XS_BSTORE(b_st_x1_idx, uint32_t, uint32_t, "buffer_store_dword", "idxen")
XS_BSTORE(b_st_x1_idx4, uint32_t, uint32_t, "buffer_store_dword", "idxen offset:4")
XS_BSTORE(b_st_x1_idx8, uint32_t, uint32_t, "buffer_store_dword", "idxen offset:8")
XS_BSTORE(b_st_x1_idx12, uint32_t, uint32_t, "buffer_store_dword", "idxen offset:12")
XS_BSTORE(b_st_x2_both, u32x2, u32x2, "buffer_store_dwordx2", "idxen offen")
XS_BSTORE(b_st_b8_off, uint32_t, uint32_t, "buffer_store_byte", "offen")
XS_BSTORE(b_st_b16_off, uint32_t, uint32_t, "buffer_store_short", "offen")
XS_BLOAD(b_ld_x1_off, uint32_t, uint32_t, "buffer_load_dword", "offen")
XS_BLOAD(b_ld_x1_off4, uint32_t, uint32_t, "buffer_load_dword", "offen offset:4")
XS_BLOAD(b_ld_x1_off8, uint32_t, uint32_t, "buffer_load_dword", "offen offset:8")
XS_BLOAD(b_ld_x1_off12, uint32_t, uint32_t, "buffer_load_dword", "offen offset:12")
XS_BLOAD(b_ld_x4_idx, u32x4, uint32_t, "buffer_load_dwordx4", "idxen")
XS_BLOAD(b_ld_x3_off, u32x3, uint32_t, "buffer_load_dwordx3", "offen")
XS_BLOAD(b_ld_x2_both_sc1, u32x2, u32x2, "buffer_load_dwordx2", "idxen offen sc1")
XS_BLOAD(b_ld_u8_off, uint32_t, uint32_t, "buffer_load_ubyte", "offen")
XS_BLOAD(b_ld_i8_off, uint32_t, uint32_t, "buffer_load_sbyte", "offen")
XS_BLOAD(b_ld_u16_off, uint32_t, uint32_t, "buffer_load_ushort", "offen")
XS_BLOAD(b_ld_i16_off, uint32_t, uint32_t, "buffer_load_sshort", "offen")

// A descriptor over `base`: every word wave-uniform through readfirstlane.
XS_D u32x4 descriptor(const uint8_t* base, uint32_t stride, uint32_t num_records) {
  const uint64_t b = reinterpret_cast<uint64_t>(base);
  return u32x4{rfl(static_cast<uint32_t>(b)),
               rfl((static_cast<uint32_t>(b >> 32) & 0xffffu) | stride << 16),
               rfl(num_records), rfl(0x00020000u)};
}

XS_D void run_buffer(const Ctx& c, Tally& y) {
  const uint32_t tile = kBufOff + rfl(c.wave) * kWaveBytes;
  const u32x4 R = descriptor(c.slab + tile, 0, kRangeBytes), S = descriptor(c.slab + tile, kSlot, kRangeSlots);
  const uint32_t zero = rfl(0u), twelve = rfl(12u);
  for (int v = 0; v < 2; ++v) {
#pragma unroll
    for (int combo = 0; combo < 6; ++combo) {
      const int s = 6 * v + combo;
      const uint32_t slot = slot_of(s, c.lane), off = kSlot * slot;
      uint32_t x[4], g[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) x[j] = srcv(c.seed, kBuffer, s, j, c.t);
      if (combo == 0) {
        b_st_x4_off(R, off, zero, u32x4{x[0], x[1], x[2], x[3]});
        g[0] = b_ld_x1_off(R, off, zero), g[1] = b_ld_x1_off4(R, off, zero), g[2] = b_ld_x1_off8(R, off, zero);
        g[3] = b_ld_x1_off12(R, off, zero);
      } else if (combo == 1) {
        b_st_x1_idx(S, slot, zero, x[0]);
        b_st_x1_idx4(S, slot, zero, x[1]);
        b_st_x1_idx8(S, slot, zero, x[2]);
        b_st_x1_idx12(S, slot, zero, x[3]);
        const u32x4 r = b_ld_x4_idx(S, slot, zero);
        g[0] = r[0], g[1] = r[1], g[2] = r[2], g[3] = r[3];
      } else if (combo == 2) {
        b_st_x2_both(S, u32x2{slot, 0u}, zero, u32x2{x[0], x[1]});
        b_st_x2_both(S, u32x2{slot, 8u}, zero, u32x2{x[2], x[3]});
        const u32x3 r = b_ld_x3_off(R, off, zero);
        g[0] = r[0], g[1] = r[1], g[2] = r[2], g[3] = b_ld_x1_off(R, off, twelve);
      } else if (combo == 3) {
        b_st_x3_off(R, off, zero, u32x3{x[0], x[1], x[2]});
        b_st_x1_off(R, off, twelve, x[3]);
        const u32x2 lo = b_ld_x2_both_sc1(S, u32x2{slot, 0u}, zero), hi = b_ld_x2_both_sc1(S, u32x2{slot, 8u}, zero);
        g[0] = lo[0], g[1] = lo[1], g[2] = hi[0], g[3] = hi[1];
      } else if (combo == 4) {
#pragma unroll
        for (int b = 0; b < 4; ++b) b_st_b8_off(R, off + b, zero, x[0] >> (8 * b));
        b_st_b16_off(R, off + 4, zero, x[1]);
        b_st_b16_off(R, off + 6, zero, x[1] >> 16);
        g[0] = b_ld_u8_off(R, off, zero), g[1] = b_ld_i8_off(R, off + 3, zero);
        g[2] = b_ld_u16_off(R, off + 4, zero), g[3] = b_ld_i16_off(R, off + 6, zero);
      } else {
        b_st_x4_off(R, off, zero, u32x4{x[0], x[1], x[2], x[3]});
        const u32x4 r = g_ld_x4(reinterpret_cast<gaddr>(c.slab) + tile + off);
        g[0] = r[0], g[1] = r[1], g[2] = r[2], g[3] = r[3];
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) take<kBuffer>(c, y, s, j, g[j], want_buffer(c.seed, s, j, c.t));
    }
  }
}

// --------------------------------------------------------------------- flat
#define XS_FSTORE(name, type, text, tail)                                                  \
  XS_D void name(gaddr a, type v) {                                                        \
    asm volatile(text " %0, %1" tail "\n\ts_nop 1" XS_FLATW ::"v"(a), "v"(v) : "memory"); \
  }
#define XS_FLOAD(name, type, text, tail)                                        \
  XS_D type name(gaddr a) {                                                     \
    type r;                                                                     \
    asm volatile(text " %0, %1" tail XS_FLATW : "=&v"(r) : "v"(a) : "memory"); \
    return r;                                                                   \
  }
XS_FSTORE(f_st_x4, u32x4, "flat_store_dwordx4", "")
XS_FSTORE(f_st_x2, u32x2, "flat_store_dwordx2", "")
XS_FSTORE(f_st_x1, uint32_t, "flat_store_dword", "")
XS_FSTORE(f_st_b16, uint32_t, "flat_store_short", "")
XS_FSTORE(f_st_b8, uint32_t, "flat_store_byte", "")
XS_FLOAD(f_ld_x4, u32x4, "flat_load_dwordx4", "")
XS_FLOAD(f_ld_x3, u32x3, "flat_load_dwordx3", "")
XS_FLOAD(f_ld_x1, uint32_t, "flat_load_dword", "")
XS_FLOAD(f_ld_x1_o4, uint32_t, "flat_load_dword", " offset:4")
XS_FLOAD(f_ld_x1_o8, uint32_t, "flat_load_dword", " offset:8")
XS_FLOAD(f_ld_x1_o12, uint32_t, "flat_load_dword", " offset:12")
XS_FLOAD(f_ld_u16, uint32_t, "flat_load_ushort", "")
XS_FLOAD(f_ld_i16, uint32_t, "flat_load_sshort", "")
XS_FLOAD(f_ld_u8, uint32_t, "flat_load_ubyte", "")
XS_FLOAD(f_ld_i8, uint32_t, "flat_load_sbyte", "")

XS_D void run_flat(const Ctx& c, Tally& y, uint32_t* lds) {
  uint8_t* lds_tile = reinterpret_cast<uint8_t*>(lds) + kFlatLdsOff + c.wave * kWaveBytes;  // a generic pointer
  uint8_t* mem_tile = c.slab + kWorkOff + c.wave * kWaveBytes;
  for (int v = 0; v < 2; ++v) {
#pragma unroll
    for (int combo = 0; combo < 4; ++combo) {
      const int s = 4 * v + combo;
      const uint32_t off = kSlot * slot_of(s, c.lane);
      const gaddr A = reinterpret_cast<gaddr>((c.lane + s) & 1u ? lds_tile + off : mem_tile + off);
      uint32_t x[4], g[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) x[j] = srcv(c.seed, kFlat, s, j, c.t);
      if (combo == 0) {
        f_st_x4(A, u32x4{x[0], x[1], x[2], x[3]});
        g[0] = f_ld_x1(A), g[1] = f_ld_x1_o4(A), g[2] = f_ld_x1_o8(A), g[3] = f_ld_x1_o12(A);
      } else if (combo == 1) {
#pragma unroll
        for (int j = 0; j < 4; ++j) f_st_x1(A + 4 * j, x[j]);
        const u32x4 r = f_ld_x4(A);
        g[0] = r[0], g[1] = r[1], g[2] = r[2], g[3] = r[3];
      } else if (combo == 2) {
        f_st_x2(A, u32x2{x[0], x[1]});
        f_st_x2(A + 8, u32x2{x[2], x[3]});
        const u32x3 r = f_ld_x3(A);
        g[0] = r[0], g[1] = r[1], g[2] = r[2], g[3] = f_ld_x1_o12(A);
      } else {
        f_st_b16(A, x[0]);
        f_st_b16(A + 2, x[0] >> 16);
#pragma unroll
        for (int b = 0; b < 4; ++b) f_st_b8(A + 4 + b, x[1] >> (8 * b));
        g[0] = f_ld_u16(A), g[1] = f_ld_i16(A + 2), g[2] = f_ld_u8(A + 4), g[3] = f_ld_i8(A + 7);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) take<kFlat>(c, y, s, j, g[j], want_flat(c.seed, s, j, c.t));
    }
  }
}

// ------------------------------------------------------------------- atomic
#define XS_RMW(name, type, dtype, text)                                                          \
  XS_D type name(gaddr a, dtype b) {                                                                \
    type r;                                                                                         \
    asm volatile(text " %0, %1, %2, off sc0" XS_VM : "=&v"(r) : "v"(a), "v"(b) : "memory"); \
    return r;                                                                                       \
  }
XS_RMW(at_add, uint32_t, uint32_t, "global_atomic_add")
XS_RMW(at_sub, uint32_t, uint32_t, "global_atomic_sub")
XS_RMW(at_smin, uint32_t, uint32_t, "global_atomic_smin")
XS_RMW(at_smax, uint32_t, uint32_t, "global_atomic_smax")
XS_RMW(at_umin, uint32_t, uint32_t, "global_atomic_umin")
XS_RMW(at_umax, uint32_t, uint32_t, "global_atomic_umax")
XS_RMW(at_and, uint32_t, uint32_t, "global_atomic_and")
XS_RMW(at_or, uint32_t, uint32_t, "global_atomic_or")
XS_RMW(at_xor, uint32_t, uint32_t, "global_atomic_xor")
XS_RMW(at_swap, uint32_t, uint32_t, "global_atomic_swap")
XS_RMW(at_cmpswap, uint32_t, u32x2, "global_atomic_cmpswap")
XS_RMW(at_inc, uint32_t, uint32_t, "global_atomic_inc")
XS_RMW(at_dec, uint32_t, uint32_t, "global_atomic_dec")
XS_RMW(at_add_x2, u32x2, u32x2, "global_atomic_add_x2")
XS_RMW(at_smin_x2, u32x2, u32x2, "global_atomic_smin_x2")
XS_RMW(at_umax_x2, u32x2, u32x2, "global_atomic_umax_x2")
XS_RMW(at_swap_x2, u32x2, u32x2, "global_atomic_swap_x2")
XS_RMW(at_cmpswap_x2, u32x2, u32x4, "global_atomic_cmpswap_x2")
XS_RMW(at_add_f32, uint32_t, uint32_t, "global_atomic_add_f32")
XS_RMW(at_pk_add_f16, uint32_t, uint32_t, "global_atomic_pk_add_f16")
XS_RMW(at_pk_add_bf16, uint32_t, uint32_t, "global_atomic_pk_add_bf16")
XS_RMW(at_add_f64, u32x2, u32x2, "global_atomic_add_f64")
XS_RMW(at_min_f64, u32x2, u32x2, "global_atomic_min_f64")
XS_RMW(at_max_f64, u32x2, u32x2, "global_atomic_max_f64")

template <int OP>
XS_D uint32_t atomic32(gaddr a, const Atom32& o) {
  if constexpr (OP == kAdd) return at_add(a, o.b);
  if constexpr (OP == kSub) return at_sub(a, o.b);
  if constexpr (OP == kSmin) return at_smin(a, o.b);
  if constexpr (OP == kSmax) return at_smax(a, o.b);
  if constexpr (OP == kUmin) return at_umin(a, o.b);
  if constexpr (OP == kUmax) return at_umax(a, o.b);
  if constexpr (OP == kAnd) return at_and(a, o.b);
  if constexpr (OP == kOr) return at_or(a, o.b);
  if constexpr (OP == kXor) return at_xor(a, o.b);
  if constexpr (OP == kSwap) return at_swap(a, o.b);
  if constexpr (OP == kCmpswap) return at_cmpswap(a, u32x2{o.b, o.cmp});
  if constexpr (OP == kInc) return at_inc(a, o.b);
  if constexpr (OP == kDec) return at_dec(a, o.b);
  if constexpr (OP == kAddF32) return at_add_f32(a, o.b);
  if constexpr (OP == kPkAddF16) return at_pk_add_f16(a, o.b);
  if constexpr (OP == kPkAddBf16) return at_pk_add_bf16(a, o.b);
}
template <int OP>
XS_D u32x2 atomic64(gaddr a, const Atom64& o) {
  const u32x2 b{static_cast<uint32_t>(o.b), static_cast<uint32_t>(o.b >> 32)};
  if constexpr (OP == kAddX2) return at_add_x2(a, b);
  if constexpr (OP == kSminX2) return at_smin_x2(a, b);
  if constexpr (OP == kUmaxX2) return at_umax_x2(a, b);
  if constexpr (OP == kSwapX2) return at_swap_x2(a, b);
  if constexpr (OP == kCmpswapX2)
    return at_cmpswap_x2(a, u32x4{b[0], b[1], static_cast<uint32_t>(o.cmp), static_cast<uint32_t>(o.cmp >> 32)});
  if constexpr (OP == kAddF64) return at_add_f64(a, b);
  if constexpr (OP == kMinF64) return at_min_f64(a, b);
  if constexpr (OP == kMaxF64) return at_max_f64(a, b);
}

template <int OP>
XS_D void atomic_one(const Ctx& c, Tally& y, const Contended& fin) {
  const gaddr A = reinterpret_cast<gaddr>(c.slab) + kWorkOff + c.wave * kWaveBytes + kSlot * slot_of(OP, c.lane);
  if constexpr (OP <= kDec || (OP >= kAddF32 && OP <= kPkAddBf16)) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const Atom32 o = atom32(c.seed, OP, j, c.t);
      g_st_x1(A + 8 * j, o.a);
      const uint32_t ret = atomic32<OP>(A + 8 * j, o);
      const uint32_t left = g_ld_x1_sc1(A + 8 * j);
      take<kAtomic>(c, y, OP, 2 * j, ret, want_atomic(c.seed, OP, 2 * j, c.t, fin));
      take<kAtomic>(c, y, OP, 2 * j + 1, left, want_atomic(c.seed, OP, 2 * j + 1, c.t, fin));
    }
  } else {
    const Atom64 o = atom64(c.seed, OP, c.t);
    g_st_x2(A, u32x2{static_cast<uint32_t>(o.a), static_cast<uint32_t>(o.a >> 32)});
    const u32x2 ret = atomic64<OP>(A, o);
    const u32x2 left = g_ld_x2_sc1(A);
    const uint32_t g[4] = {ret[0], ret[1], left[0], left[1]};
#pragma unroll
    for (int j = 0; j < 4; ++j) take<kAtomic>(c, y, OP, j, g[j], want_atomic(c.seed, OP, j, c.t, fin));
  }
}
template <int... OP>
XS_D void run_atomic_ops(const Ctx& c, Tally& y, const Contended& fin, std::integer_sequence<int, OP...>) {
  (atomic_one<OP>(c, y, fin), ...);
}

XS_D void run_atomic(const Ctx& c, Tally& y, const Contended& fin) {
  run_atomic_ops(c, y, fin, std::make_integer_sequence<int, kContended>{});
  // All 256 lanes on the four words of slot 0 of wave 0.
  const gaddr common = reinterpret_cast<gaddr>(c.slab) + kWorkOff;
  __syncthreads();
  if (c.t == 0) {
#pragma unroll
    for (int j = 0; j < 4; ++j) g_st_x1(common + 4 * j, auxv(c.seed, kAtomic, kContended, j, 0));
  }
  __syncthreads();
  (void)at_add(common, contended_operand(c.seed, 0, c.t));
  (void)at_or(common + 4, contended_operand(c.seed, 1, c.t));
  (void)at_umax(common + 8, contended_operand(c.seed, 2, c.t));
  (void)at_xor(common + 12, contended_operand(c.seed, 3, c.t));
  __syncthreads();
#pragma unroll
  for (int j = 0; j < 4; ++j)
    take<kAtomic>(c, y, kContended, j, g_ld_x1_sc1(common + 4 * j), want_atomic(c.seed, kContended, j, c.t, fin));
  __syncthreads();
}

// ----------------------------------------------------------------------- l1
// Four loads and one wait: the step's four words.
#define XS_LOAD4(name, flags)                                                                                        \
  XS_D void name(gaddr a0, gaddr a1, gaddr a2, gaddr a3, uint32_t (&g)[4]) {                                         \
    asm volatile("global_load_dword %0, %4, off" flags "\n\tglobal_load_dword %1, %5, off" flags                     \
                 "\n\tglobal_load_dword %2, %6, off" flags "\n\tglobal_load_dword %3, %7, off" flags XS_VM           \
                 : "=&v"(g[0]), "=&v"(g[1]), "=&v"(g[2]), "=&v"(g[3])                                                \
                 : "v"(a0), "v"(a1), "v"(a2), "v"(a3)                                                                \
                 : "memory");                                                                                        \
  }
XS_LOAD4(l1_load4_plain, "")
XS_LOAD4(l1_load4_sc0, " sc0")

template <int P>
XS_D void l1_pass(const Ctx& c, Tally& y) {
  const gaddr T = reinterpret_cast<gaddr>(c.slab);
  for (uint32_t k = 0; k < 16; ++k) {
    uint32_t g[4];
    gaddr a[4];
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) a[j] = T + 4u * l1_dword(P, 4 * k + j, c.t);
    if constexpr (P & 1) l1_load4_sc0(a[0], a[1], a[2], a[3], g);
    else l1_load4_plain(a[0], a[1], a[2], a[3], g);
#pragma unroll
    for (int j = 0; j < 4; ++j) take<kL1>(c, y, 16 * P + k, j, g[j], want_l1(c.seed, 16 * P + k, j, c.t));
  }
}

XS_D void run_l1(const Ctx& c, Tally& y) {
  const gaddr T = reinterpret_cast<gaddr>(c.slab);
  __syncthreads();
  for (uint32_t i = 0; i < kL1Bytes / 16 / kBlock; ++i) {
    const uint32_t chunk = c.t + kBlock * i, d = 4 * chunk;
    g_st_x4(T + 16 * chunk,
            u32x4{tilv(c.seed, kL1, d), tilv(c.seed, kL1, d + 1), tilv(c.seed, kL1, d + 2), tilv(c.seed, kL1, d + 3)});
  }
  __syncthreads();
  l1_pass<0>(c, y);
  l1_pass<1>(c, y);
  __syncthreads();
  if (c.wave == 0) {
#pragma unroll
    for (uint32_t h = 0; h < 2; ++h) {
      const uint32_t d = (c.lane + 64 * h) * 32 + ((5 * c.lane + 3) & 31u);
      g_st_x1(T + 4 * d, newv(c.seed, kL1, d));
    }
  }
  __syncthreads();
  l1_pass<2>(c, y);
  l1_pass<3>(c, y);
  __syncthreads();
}

// ----------------------------------------------------------------------- l2
XS_SLOAD(l2_ld_sc1, u32x4, "global_load_dwordx4", " sc1")
XS_SLOAD(l2_ld_nt, u32x4, "global_load_dwordx4", " nt")
XS_SLOAD(l2_ld_plain, u32x4, "global_load_dwordx4", "")

XS_D void l2_write(const Ctx& c, uint32_t flip) {
  for (uint32_t i = 0; i < kTileBytes / 16 / kBlock; ++i) {
    const uint32_t chunk = c.t + kBlock * i, d = 4 * chunk;
    s_st_x4(c.slab, 16 * chunk,
            u32x4{tilv(c.seed, kL2, d) ^ flip, tilv(c.seed, kL2, d + 1) ^ flip, tilv(c.seed, kL2, d + 2) ^ flip,
                  tilv(c.seed, kL2, d + 3) ^ flip});
  }
}

template <int P>
XS_D void l2_pass(const Ctx& c, Tally& y) {
  for (uint32_t i = 0; i < 128; ++i) {
    const uint32_t off = 16u * l2_chunk(P, i, c.t);
    u32x4 r;
    if constexpr (P == 0) r = l2_ld_sc1(c.slab, off);
    else if constexpr (P == 1) r = l2_ld_nt(c.slab, off);
    else r = l2_ld_plain(c.slab, off);
#pragma unroll
    for (int j = 0; j < 4; ++j) take<kL2>(c, y, 128 * P + i, j, r[j], want_l2(c.seed, 128 * P + i, j, c.t));
  }
}

XS_D void run_l2(const Ctx& c, Tally& y) {
  __syncthreads();
  l2_write(c, 0u);
  __syncthreads();
  l2_pass<0>(c, y);
  l2_pass<1>(c, y);
  l2_pass<2>(c, y);
  __syncthreads();
  l2_write(c, 0xffffffffu);
  __syncthreads();
  l2_pass<3>(c, y);
  __syncthreads();
}

// ------------------------------------------------------------------- scalar
#define XS_LGKM "\n\ts_waitcnt lgkmcnt(0)"
#define XS_SMEM(name, type, text)                                                                \
  XS_D type name(const uint32_t* base, uint32_t off) {                                           \
    type r;                                                                                      \
    asm volatile(XS_SN text " %0, %1, %2" XS_LGKM : "=&s"(r) : "s"(base), "s"(off) : "memory"); \
    return r;                                                                                    \
  }
XS_SMEM(sm_x1, uint32_t, "s_load_dword")
XS_SMEM(sm_x4, u32x4, "s_load_dwordx4")
XS_SMEM(sm_x8, u32x8, "s_load_dwordx8")
XS_SMEM(sm_x16, u32x16, "s_load_dwordx16")
XS_D u32x2 sm_x2_imm(const uint32_t* base) {
  u32x2 r;
  asm volatile(XS_SN "s_load_dwordx2 %0, %1, 0x40" XS_LGKM : "=&s"(r) : "s"(base) : "memory");
  return r;
}
#define XS_SBUF(name, type, text)                                                                \
  XS_D type name(u32x4 rsrc, uint32_t off) {                                                     \
    type r;                                                                                      \
    asm volatile(XS_SN text " %0, %1, %2" XS_LGKM : "=&s"(r) : "s"(rsrc), "s"(off) : "memory"); \
    return r;                                                                                    \
  }
XS_SBUF(sb_x1, uint32_t, "s_buffer_load_dword")
XS_SBUF(sb_x4, u32x4, "s_buffer_load_dwordx4")

// The SGPR value in a VGPR, out of the compiler's sight.
XS_D uint32_t to_vgpr(uint32_t s) {
  uint32_t v = s;
  asm volatile("" : "+v"(v));
  return v;
}

XS_D void run_scalar(const Ctx& c, Tally& y, const uint32_t* __restrict__ table) {
  const uint32_t t0 = rfl(c.t & ~63u);  // lane 0 of this wave, uniform
  const u32x4 rsrc = descriptor(reinterpret_cast<const uint8_t*>(table), 0, kTableWords * 4);
  for (int s = 0; s < kShape[kScalar].steps; ++s) {
    uint32_t o[7];
#pragma unroll
    for (int n = 0; n < 7; ++n) o[n] = rfl(4u * scalar_offset(c.seed, s, n, t0));
    uint32_t g[36];
    g[0] = to_vgpr(sm_x1(table, o[0]));
    {
      // The base moved back by the immediate offset; uniform, so it stays in SGPRs.
      const uint64_t b = reinterpret_cast<uint64_t>(table) + o[1] - 0x40;
      const uint32_t lo = rfl(static_cast<uint32_t>(b));
      const uint32_t hi = rfl(static_cast<uint32_t>(b >> 32));
      const u32x2 r = sm_x2_imm(reinterpret_cast<const uint32_t*>(lo | static_cast<uint64_t>(hi) << 32));
      g[1] = to_vgpr(r[0]), g[2] = to_vgpr(r[1]);
    }
    {
      const u32x4 r = sm_x4(table, o[2]);
#pragma unroll
      for (int j = 0; j < 4; ++j) g[3 + j] = to_vgpr(r[j]);
    }
    {
      const u32x8 r = sm_x8(table, o[3]);
#pragma unroll
      for (int j = 0; j < 8; ++j) g[7 + j] = to_vgpr(r[j]);
    }
    {
      const u32x16 r = sm_x16(table, o[4]);
#pragma unroll
      for (int j = 0; j < 16; ++j) g[15 + j] = to_vgpr(r[j]);
    }
    g[31] = to_vgpr(sb_x1(rsrc, o[5]));
    {
      const u32x4 r = sb_x4(rsrc, o[6]);
#pragma unroll
      for (int j = 0; j < 4; ++j) g[32 + j] = to_vgpr(r[j]);
    }
#pragma unroll
    for (int j = 0; j < 36; ++j) take<kScalar>(c, y, s, j, g[j], want_scalar(c.seed, s, j, c.t));
  }
}

XS_D void run_routes(const Ctx& c, uint32_t mask, uint32_t* lds, const uint32_t* table, const Contended& fin,
                     Tally (&y)[kNumRoutes]) {
  if (mask & (1u << kGwidth)) run_gwidth(c, y[kGwidth]);
  if (mask & (1u << kBuffer)) run_buffer(c, y[kBuffer]);
  if (mask & (1u << kFlat)) run_flat(c, y[kFlat], lds);
  if (mask & (1u << kAtomic)) run_atomic(c, y[kAtomic], fin);
  if (mask & (1u << kL1)) run_l1(c, y[kL1]);
  if (mask & (1u << kL2)) run_l2(c, y[kL2]);
  if (mask & (1u << kScalar)) run_scalar(c, y[kScalar], table);
}

XS_D Ctx make_ctx(uint8_t* arena, uint32_t seed, uint32_t inj, uint32_t* dump) {
  const uint32_t t = threadIdx.x;
  const size_t first = static_cast<size_t>(blockIdx.x) * kStride + kGuard;
  return Ctx{seed, t, t & 63u, t >> 6, inj, dump, arena + first};
}

__global__ __launch_bounds__(kBlock) void k_mem_sweep(MemRecord* __restrict__ records, uint8_t* arena,
                                                     const uint32_t* __restrict__ table, uint32_t route_mask,
                                                     uint32_t seed, int inject_xcd, int inject_cu,
                                                     uint32_t inject_routes, Expect expect, Contended fin) {
  extern __shared__ uint32_t mem_lds[];
  const uint32_t xcd = xcc_id();
  const uint32_t hw = hw_id();
  const uint32_t cu = cu_key(hw);
  const uint32_t simd = simd_id(hw);
  const bool inject = inject_selected(inject_xcd, inject_cu, xcd, cu);
  const Ctx c = make_ctx(arena, seed, inject ? inject_routes : 0u, nullptr);

  Tally y[kNumRoutes];
  run_routes(c, route_mask, mem_lds, table, fin, y);

  // The markers bound the reduction for tests/test_mem_codeobject.py.
  asm volatile("; mem_sweep reduction begin" ::: "memory");
  reduce_parts<kNumRoutes, 0>(mem_lds, c.t, simd, y, nullptr, route_mask, expect, xcd, cu, &records[blockIdx.x]);
  asm volatile("; mem_sweep reduction end" ::: "memory");
}

// One workgroup; dump holds steps x words x 256 words of route `route`.
__global__ __launch_bounds__(kBlock) void k_mem_probe(uint32_t* __restrict__ dump, uint8_t* arena,
                                                     const uint32_t* __restrict__ table, int route, uint32_t seed,
                                                     Contended fin) {
  extern __shared__ uint32_t mem_lds[];
  const Ctx c = make_ctx(arena, seed, 0u, dump);
  Tally y[kNumRoutes];
  run_routes(c, 1u << route, mem_lds, table, fin, y);
}

// --------------------------------------------------------------------- host
uint32_t want(int r, uint32_t seed, int s, int w, uint32_t t, const Contended& fin) {
  switch (r) {
    case kGwidth: return want_gwidth(seed, s, w, t);
    case kBuffer: return want_buffer(seed, s, w, t);
    case kFlat: return want_flat(seed, s, w, t);
    case kAtomic: return want_atomic(seed, s, w, t, fin);
    case kL1: return want_l1(seed, s, w, t);
    case kL2: return want_l2(seed, s, w, t);
    default: return want_scalar(seed, s, w, t);
  }
}

uint32_t expected_digest(int r, uint32_t seed, const Contended& fin) {
  uint32_t d = 0;
  const Shape sh = kShape[r];
  for (int s = 0; s < sh.steps; ++s)
    for (int w = 0; w < sh.words; ++w)
      for (uint32_t t = 0; t < kBlock; ++t) {
        const uint32_t idx = (static_cast<uint32_t>(s) * sh.words + w) * kBlock + t;
        d += want(r, seed, s, w, t, fin) * (2u * idx + 1u);
      }
  return d;
}

// The node agent sweeps with one seed again and again: keep the last.
void expected(uint32_t route_mask, uint32_t seed, Expect* e, Contended* fin) {
  static std::mutex mu;
  static bool have = false;
  static uint32_t have_seed = 0;
  static uint32_t all[kNumRoutes];
  static Contended have_fin;
  std::lock_guard<std::mutex> g(mu);
  if (!have || have_seed != seed) {
    have_fin = contended_final(seed);
    for (int r = 0; r < kNumRoutes; ++r) all[r] = expected_digest(r, seed, have_fin);
    have = true;
    have_seed = seed;
  }
  for (int r = 0; r < kNumRoutes; ++r) e->digest[r] = (route_mask >> r) & 1u ? all[r] : 0u;
  *fin = have_fin;
}

// The arena of `blocks` slabs, filled with the sentinel, and the scalar table.
// -1003 when the arena cannot be had: nothing is launched.
int prepare_memory(uint32_t seed, size_t blocks, DevMem& arena, DevMem& table) {
  const size_t bytes = blocks * kStride;
  if (hipMalloc(&arena.p, bytes) != hipSuccess) {
    arena.p = nullptr;
    (void)hipGetLastError();
    std::snprintf(g_mem_err, sizeof g_mem_err, "no arena of %zu bytes could be had: nothing was swept", bytes);
    return kUnswept;
  }
  // Every workgroup's 144 KiB holds the same words: a group of them is built once and copied as often as needed.
  const size_t group = std::min(blocks, kHostGroup);
  std::vector<uint32_t> h(group * (kStride / 4));
  for (size_t i = 0; i < h.size(); ++i) h[i] = sentinel(static_cast<uint32_t>(i % (kStride / 4)));
  for (size_t b = 0; b < blocks; b += group)
    XS_CHECK(hipMemcpy(arena.as<uint8_t>() + b * kStride, h.data(), std::min(group, blocks - b) * kStride,
                       hipMemcpyHostToDevice));
  std::vector<uint32_t> tab(kTableWords);
  for (uint32_t i = 0; i < kTableWords; ++i) tab[i] = tilv(seed, kScalar, i);
  XS_CHECK(hipMalloc(&table.p, kTableWords * 4));
  XS_CHECK(hipMemcpy(table.p, tab.data(), kTableWords * 4, hipMemcpyHostToDevice));
  return 0;
}

// Every guard band against the sentinel; -1004 with the first bad address.
int check_guards(const DevMem& arena, size_t blocks) {
  constexpr size_t kGuardWords = kGuard / 4;
  std::vector<uint32_t> h(std::min(blocks, kHostGroup) * 2 * kGuardWords);
  for (size_t first = 0; first < blocks; first += kHostGroup) {
    const size_t n = std::min(kHostGroup, blocks - first);
    const uint8_t* base = arena.as<uint8_t>() + first * kStride;
    // Row b: the band before slab first + b, then the band behind it.
    XS_CHECK(hipMemcpy2D(h.data(), 2 * kGuard, base, kStride, kGuard, n, hipMemcpyDeviceToHost));
    XS_CHECK(hipMemcpy2D(h.data() + kGuardWords, 2 * kGuard, base + kGuard + kSlabBytes, kStride, kGuard, n,
                         hipMemcpyDeviceToHost));
    for (size_t b = 0; b < n; ++b)
      for (size_t half = 0; half < 2; ++half)
        for (size_t i = 0; i < kGuardWords; ++i) {
          const size_t in_stride = half * (kGuard + kSlabBytes) / 4 + i, word = (first + b) * (kStride / 4) + in_stride;
          const uint32_t got = h[(2 * b + half) * kGuardWords + i];
          if (got != sentinel(static_cast<uint32_t>(in_stride))) {
            std::snprintf(g_mem_err, sizeof g_mem_err,
                          "stray store: the guard band %s slab %zu holds 0x%08x at arena byte %zu (address %p), not 0x%08x",
                          half ? "behind" : "before", first + b, got, word * 4,
                          static_cast<const void*>(arena.as<uint8_t>() + word * 4),
                          sentinel(static_cast<uint32_t>(in_stride)));
            return kStrayStore;
          }
        }
  }
  return 0;
}

// The workgroups launch_sweep will launch for `blocks` on `dev`.
int resolve_blocks(int dev, int blocks, size_t* out) {
  if (blocks < 0 || blocks > kMaxBlocks) return kBadArgs;
  int per = 0;
  XS_CHECK(hipSetDevice(dev));
  XS_CHECK(cu_count(dev, &per, 4));
  *out = static_cast<size_t>(blocks ? blocks : per);
  return 0;
}

}  // namespace

extern "C" {

const char* xs_mem_sweep_last_error() { return g_mem_err; }

// Route names, comma-separated, in bit order.
const char* xs_mem_routes() { return kRouteNames; }

// out2 = {steps, words per step}.
int xs_mem_shape(int route, int* out2) {
  if (route < 0 || route >= kNumRoutes || !out2) return kBadArgs;
  out2[0] = kShape[route].steps;
  out2[1] = kShape[route].words;
  return 0;
}

// One workgroup runs `route` and stores every value it received:
// out[step][word][256], n_words = steps x words x 256.
int xs_mem_probe(int dev, int route, uint32_t seed, uint32_t* out, size_t n_words) {
  if (route < 0 || route >= kNumRoutes || !out) return kBadArgs;
  const size_t n = static_cast<size_t>(kShape[route].steps) * kShape[route].words * kBlock;
  if (n_words != n) return kBadArgs;
  const Contended fin = contended_final(seed);
  DevMem arena, table;
  const int rc = launch_probe(
      g_mem_err, dev, reinterpret_cast<const void*>(k_mem_probe), kBlock, kLdsUsed, out, n,
      [&](dim3 grid, dim3 block, size_t smem, void* dump) {
        hipLaunchKernelGGL(k_mem_probe, grid, block, smem, 0, static_cast<uint32_t*>(dump), arena.as<uint8_t>(),
                           table.as<const uint32_t>(), route, seed, fin);
      },
      [&] { return prepare_memory(seed, 1, arena, table); });
  return rc ? rc : check_guards(arena, 1);
}

// Host only. out7[r] = the workgroup digest a healthy CU leaves for route r, 0
// for a route outside route_mask.
int xs_mem_sweep_expected(uint32_t route_mask, uint32_t seed, uint32_t* out7) {
  if (bad_part_mask(route_mask, kAllRoutes) || !out7) return kBadArgs;
  Expect e;
  Contended fin;
  expected(route_mask, seed, &e, &fin);
  for (int r = 0; r < kNumRoutes; ++r) out7[r] = e.digest[r];
  return 0;
}

// What the runtime reports for k_mem_sweep on `dev`: out5 = {registers per
// lane, scratch bytes per lane, dynamic LDS bytes per workgroup, workgroups
// that fit on a CU at once, arena bytes per workgroup}.
int xs_mem_sweep_info(int dev, int* out5) {
  if (int rc = sweep_info(g_mem_err, dev, reinterpret_cast<const void*>(k_mem_sweep), kBlock, true, out5)) return rc;
  out5[4] = static_cast<int>(kStride);
  return 0;
}

// One sweep launch of `blocks` workgroups (0: 4 per CU). Writes `blocks`
// 128-byte records to records_out. Returns 0, -1000 for bad arguments and
// -1003 when the arena could not be allocated (nothing is launched either
// way), -1004 when a guard band was written, or a negative HIP error.
int xs_mem_sweep(int dev, int blocks, uint32_t route_mask, uint32_t seed, int inject_xcd, int inject_cu,
                 uint32_t inject_routes, void* records_out, int* n_records, double* ms) {
  if (bad_part_mask(route_mask, kAllRoutes) || (inject_routes & ~kAllRoutes)) return kBadArgs;
  size_t n = 0;
  if (int rc = resolve_blocks(dev, blocks, &n)) return rc;
  Expect e;
  Contended fin;
  expected(route_mask, seed, &e, &fin);
  DevMem arena, table;
  const int rc = launch_sweep(
      g_mem_err, {dev, blocks, inject_xcd, inject_cu, records_out, n_records, ms},
      reinterpret_cast<const void*>(k_mem_sweep), kBlock, kLdsUsed, sizeof(MemRecord),
      [&](dim3 grid, dim3 block, size_t smem, void* rec) {
        hipLaunchKernelGGL(k_mem_sweep, grid, block, smem, 0, static_cast<MemRecord*>(rec), arena.as<uint8_t>(),
                           table.as<const uint32_t>(), route_mask, seed, inject_xcd, inject_cu, inject_routes, e, fin);
      },
      [&] { return prepare_memory(seed, n, arena, table); });
  if (rc || !arena.p) return rc;
  return check_guards(arena, n);
}

}  // extern "C"
