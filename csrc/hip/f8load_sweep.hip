// FP8 load sweep for gfx950 (MI355X): every CU under load, with a checked
// rowwise-scaled FP8 GEMM whose every tile is written to device memory and
// read back.
//
// The six load sweeps (load_sweep.hip and its siblings) hold a CU at rate with
// a GEMM or an attention pass and compare every result by equality. Two things
// they leave out. FP8 (OCP e4m3), the format most work on this part runs in,
// reaches the f8f6f4 matrix path at 8 bits per element only in
// matrix_sweep.hip: two K-steps, cold, operands built in registers; under load
// that path runs at 4 bits (mxload_sweep.hip). And no sweep runs the epilogue
// every production GEMM has: a dequantising scale, v_cvt_pk_bf16_f32, a
// transpose through LDS and wide vector stores of the result to device memory
// while the next tile's loads and MFMAs are in flight; in five of the six only
// a record leaves the CU, and gradload_sweep.hip pushes its tile out through
// atomics at the L2. k_f8load_sweep is a sweep over named parts (part_sweep.h)
// whose load is Y = bf16((A Bt^T) sa sb): every tile goes to a ring in device
// memory and is read back `slots` laps later by another wave, and everything
// is compared by equality.
//
// The operation and why equality holds. A set s is A_s[128][K] and Bt_s[256][K]
// of e4m3 (B transposed: k is contiguous), K = 64 ksteps. Dword w of panel p
// (0: A, 1: Bt) of set s is fmix32(seed ^ (s << 23 | p << 22 | w)), as in
// mxload_sweep.hip, with every byte h of it made
//     (h & 0x87) | ((6 + ((h >> 3) & 3)) << 3):
// sign and the three mantissa bits are hashed, the exponent field is 6..9
// (four binades), the value +-(8 + m) 2^(E - 10), that is 0.5 to 7.5, never
// zero, NaN or subnormal. An element is at most 120 units of 2^-4, a product
// at most 14,400 units of 2^-8, and any partial sum in any order is one exact
// float while K 14,400 < 2^24: K <= 1,165, so ksteps <= 18 (1,152 x 14,400 =
// 16,588,800); 19 and above are refused with -1000 before anything touches a
// device, and host_sets() re-checks the maximum of sum |a||b| on what it
// generated (-1001). Scales: sa_s[128] and sb_s[256] are f32 powers of two,
// 2^(-2 + (g & 3)) for A's row and 2^(g & 1) for Bt's with
//     g = fmix32(seed ^ (1u << 30 | s << 23 | p << 22 | row)),
// so y = acc sa[i] sb[j] is exact in f32 and the conversion to bf16 is one
// round-to-nearest-even, which the host reproduces in integers; an exact zero
// sum is +0. The host keeps fix = C 2^8 as int32 [set][128][256] and the bf16
// tile as dwords [set][128][128], both from plain integer arithmetic: no float
// is rounded on the host.
//
// Arena. As mxload's without the scale words: a set is `ksteps` blocks of
// 24,576 bytes, block `step` = the 64 bytes of that step of each of the 384
// rows (A's before Bt's), so a step's DMA reads one contiguous block. The
// scales are an array of their own, [set][384] floats.
//
// Work split: the load sweep's. 512 threads, two waves per SIMD,
// exclusive_lds(); a macro tile C[128 x 256] per lap; a wave owns a 64 x 64
// sub-tile (four f32x16 accumulators); sub-tile (w + l) & 7 and set
// set_of(g, l, laps, sets) in lap l (part_sweep.h).
//
// Matrix instruction: v_mfma_f32_32x32x64_f8f6f4 in its unscaled encoding,
// cbsz = blgp = 0 (fp8 on both sides), which the scale builtin selects when
// both scale operands and opsels are literal zeros. One step is 64 elements of
// k: one MFMA per accumulator, four per wave and step. The operand map is the
// one matrix_sweep.hip pins for fp8 in this instruction: element j of lane
// (r, h) is k = k0 + 16 h + (j & 15) + 32 (j >> 4), so a lane's eight operand
// registers are two 128-bit LDS reads of its row, chunks h and 2 + h of the
// step's 64 bytes.
// Operands swapped on purpose: the wave feeds its Bt rows as the MFMA's A and
// its A rows as the MFMA's B. Register q of lane (r, h) is then
// C[row0 + r][col0 + (q & 3) + 8 (q >> 2) + 4 h]: four consecutive registers
// are four consecutive columns of one row, v_cvt_pk_bf16_f32 packs row-major
// dwords and one 64-bit LDS write puts 8 bytes of a row in place.
//
// Staging by LDS DMA: mxload's step geometry. Per step the 384 x 64 operand
// bytes go to LDS in 1,536 chunks of 16 bytes, three global_load_lds_dwordx4
// per thread, into a ring of three stages of 24,576 bytes. The LDS destination
// of one instruction is wave-linear, so rows cannot be padded; the layout is
// XOR-swizzled and the permutation goes into the source address: LDS slot q of
// a stage (16 bytes) holds chunk (q & 3) ^ ((q >> 4) & 3) of row q >> 2. A
// lane reads two chunks of every row here, c = h and c = 2 + h, each with a
// 128-bit read of its own at row 64 + ((c ^ ((row >> 2) & 3)) << 4). The bank
// argument, per read instruction: a 128-bit access is served 16 lanes at a
// time; those are 16 consecutive rows and one c; the group of four banks a
// lane starts in is 4 (row & 3) + (c ^ ((row >> 2) & 3)), which takes 16
// values over 16 consecutive rows whichever c is, so either read is free of
// conflicts, and the two never share a cycle. This is the 64-bank model of the
// public CDNA3 material, assumed for CDNA4: a model, not a measurement.
//
// Pipeline. The DMA of step k + 2 is issued before the MFMAs of step k; one
// barrier per step; a stage is overwritten only after the barrier that follows
// its last read. The vector-memory counter counts DMAs, loads and stores in
// order, so the wait at the end of step k names what may still be outstanding
// behind the DMA of step k + 1: the three DMAs of step k + 2 and, when step
// k - 1 ended a lap or began a read-back, its eight stores or loads in front
// of them (11). Anything else issued in between only makes the wait stricter.
//
// Epilogue, per lap and wave, after the barrier of the lap's last step:
//  1. fix = (int)(acc 256), a mismatch when that loses anything (a NaN too) or
//     differs from the table (part gemm);
//  2. y = acc sa[row] sb[col], two multiplies, and v_cvt_pk_bf16_f32 of two
//     neighbours; the packed dwords are compared with the bf16 table in
//     registers (part round);
//  3. the packed dwords go into the wave's own LDS tile, 64 rows of 128 bytes
//     at a pitch of 144, with sixteen 64-bit writes per lane. Under the model
//     above a 64-bit write is served 32 lanes at a time, 32 rows at one
//     column: 144 bytes are 36 banks, rows r and r + 16 meet (2-way); a pitch
//     that is no multiple of 16 bytes would cure that and break the 128-bit
//     reads of step 4. Not measured;
//  4. the tile is read back as 16-byte row chunks, lane l chunk l & 7 of row
//     e + 8 (l >> 3) in read e: the 16 lanes served together take rows x and
//     x + 8, 288 banks = 32 mod 64 apart, with 32 banks each: no conflict
//     under the model;
//  5. eight global_store_dwordx4 per lane into the workgroup's ring slot, each
//     instruction eight whole 128-byte row segments of Y, whose row pitch is
//     512 bytes. Nothing waits after the stores: the DMAs of the next two
//     steps were issued before them, and they drain under the next steps'
//     MFMAs until the in-order counter reaches them.
// The wave's tile needs no barrier: only its own lanes touch it, and a wave's
// LDS operations complete in order. LDS: 3 x 24,576 + 8 x 9,216 = 147,456
// bytes of the CU's 160 KiB.
//
// The ring and the read-back: the new data path. A workgroup owns `slots`
// slots of 64 KiB ([128][256] bf16) and lap l uses slot l % slots; a launch's
// footprint is blocks x slots x 64 KiB (4 workgroups per CU: slots x 64 MiB;
// the default 8 slots are 512 MiB), allocated and cleared per call and freed
// after it. From lap `slots` on, at the start of lap l, wave w reads back the
// 64 x 64 region (w + 1 + l - slots) & 7 of the slot the lap will reuse, with
// eight global_load_dwordx4 per lane: the region wave (w + 1) & 7 stored in
// lap l - slots. A barrier must stand between those stores and these loads:
// the loads are issued behind the barrier that ends the lap's first step, and
// where a lap is one step (ksteps 1) behind a barrier of their own at its top.
// The words are held in registers through the lap and, before its last
// barrier, compared with the bf16 table of lap l - slots' set (part store).
// The lap's stores follow that barrier, so no region is overwritten before
// its reader has it. After the last lap the slots not yet read (the
// last min(slots, laps) laps) are read back the same way behind a barrier:
// every lap's tile is stored once and read back once. Visibility between the
// storing and the reading wave is a workgroup-scope release fence before a
// barrier and an acquire fence behind it; in the default (non-tgsplit) mode
// the waves of a workgroup share the CU's vector cache and neither fence
// drains the vector-memory counter (profiles/f8load_sweep_defaults.md has the
// disassembly). Which level (L2, Infinity Cache, HBM) served a read-back is
// the hardware's choice and is not observed.
//
// Parts (bit, name). The mask selects what is judged; the pipeline, stores and
// read-back included, always runs: it is the load.
//   0 operand  every dword read from LDS on its way into an MFMA: sum of
//              rotl32(word, i & 31), i the dword's index in the set (logical
//              order, A before Bt). An A dword is read by four waves, a Bt
//              dword by two: 4 sum(A) + 2 sum(Bt) per lap. Not issued when not
//              selected.
//   1 gemm     mismatches against the fix table; the digest is the sum of
//              uint32(fix) (2 (256 row + col) + 1) over the laps.
//   2 round    the packed bf16 dwords in registers against the bf16 table; the
//              digest is the rotate-and-add fold over the dword index
//              128 row + col / 2.
//   3 store    the same fold and compare over what came back from the ring. A
//              healthy CU has store == round; a bad store with a good round
//              names the LDS transpose, the store path or the return path
//              under load.
//
// Record (128 bytes per workgroup), injection and safety rules are the load
// sweep's: part_sweep.h's head with four parts, the reserved word and the
// sub-tile, set and span masks (gemm, round and store feed them). An injected
// part flips bit 0 of one compared word in registers only (operand: the first
// dword thread 0 folds, in the fold only; gemm: fix of thread 0's first
// accumulator of lap 0; round: thread 0's first packed dword of lap 0, in the
// compare and fold only, the stored word is untouched; store: the first dword
// thread 0 reads back). Trip counts come from the kernel arguments only;
// nothing waits on a clock, a flag or another workgroup. No scratch, MODE is
// not written, results leave through vector stores. Bounds: set < sets and
// step < ksteps, so every arena index is below sets ksteps 24,576, every fix
// index below 32,768 sets, every bf16-table index below 16,384 sets, every
// scale index below 384 sets; a ring index is (g slots + slot) 16,384 +
// 128 row + dword with slot < slots, row < 128, dword < 128: below
// blocks slots 16,384; every LDS address below 147,456. laps above 16 x the
// default are refused.
//
// k_f8load_probe is the same device function with a dump: one workgroup at any
// shape stores C of every lap as [lap][128][256] raw f32 bits, behind it the
// dwords each lap's read-back returned as [lap][128][128] and each thread's
// operand fold ([512]).
//
// What the hardware settled: on the first run on an MI355X the probe equalled
// the numpy reference (tests/f8load_sweep_ref.py) at every shape and seed, C,
// read-back and fold; exact zero sums occur and came out as +0. A lap of a
// workgroup takes 21 us at ksteps 16, about 11.6 us of it the epilogue whatever
// ksteps: the launch is bound by the epilogue's table loads, transpose, stores
// and read-back and by the step's DMA and barrier chain, not by the matrix
// cores and not by HBM (the ring moves 1.6 TB/s over the GPU). 512 MiB of ring
// cost nothing measurable against 64 MiB (profiles/f8load_sweep_defaults.md,
// with the disassembly: the compiler pairs the 64-bit tile writes into
// ds_write2_b64).
//
// NOT covered: bf8 and mixed formats; the 16x16x128 shape; fp6; scaled FP8
// (MX: mxload_sweep.hip has the scale path at 4 bits); split-K; xGMI; more
// than one launch; which level of the memory hierarchy held a slot; LDS bank
// conflicts, power, clocks and temperature.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <map>
#include <memory>
#include <mutex>
#include <tuple>
#include <vector>

#include "hip/part_sweep.h"

#define XS_ERR_BUF g_f8_err
#define XS_HD __host__ __device__ __forceinline__
#define XS_D __device__ __forceinline__

namespace {

using namespace xsprobe;

ErrBuf g_f8_err = "";

typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __attribute__((address_space(1))) const void* GlobalPtr;
typedef __attribute__((address_space(3))) void* LdsPtr;

constexpr int kNumParts = 4;
const char kPartNames[] = "operand,gemm,round,store";
constexpr uint32_t kAllParts = (1u << kNumParts) - 1;
constexpr int kOperand = 0, kGemm = 1, kRound = 2, kStore = 3;
constexpr int kBlock = 512;  // 8 waves: two per SIMD
constexpr int kExtra = 3;    // sub-tile, set and span masks
constexpr int kUnswept = -1003;
constexpr int kBoundBroken = -1001;  // the generator left its stated bound (a bug in this file)

// The sweep's fixed shape and defaults: measured in profiles/f8load_sweep_defaults.md.
constexpr uint32_t kF8Ksteps = 16, kF8Sets = 16, kF8Slots = 8;
constexpr uint32_t kF8Laps = 2048;
constexpr uint32_t kMaxLaps = 16 * kF8Laps, kMaxKsteps = 18, kMaxSlots = 16, kMaxSets = 64;

constexpr uint32_t kRowsA = 128, kRowsB = 256, kRows = kRowsA + kRowsB;
constexpr uint32_t kStepBytes = 64;                     // 64 e4m3 of k, per row and step
constexpr uint32_t kStageBytes = kRows * kStepBytes;    // 24,576: a stage, and a step's block of the arena
constexpr uint32_t kStages = 3;
constexpr uint32_t kPitch = 144;                        // a row of a wave's bf16 tile: 128 + 16 bytes
constexpr uint32_t kTileBytes = 64 * kPitch;            // 9,216 per wave
constexpr uint32_t kTilesOff = kStages * kStageBytes;   // 73,728: where the waves' tiles begin
constexpr uint32_t kTileWords = kRowsA * kRowsB;        // C of one set: 128 KiB of fix
constexpr uint32_t kSlotWords = kTileWords / 2;         // Y of one lap: 64 KiB of bf16 pairs, [128][128]
constexpr uint32_t kYRow = kRowsB / 2;                  // dwords in a row of Y
constexpr uint32_t kRedBytes = part_reduction_words<kBlock>(kNumParts, kExtra) * 4;
constexpr uint32_t kLdsUsed = kTilesOff + 8 * kTileBytes;
constexpr int kMaxElem = 120;       // |element| in units of 2^-4
constexpr float kFixScale = 256.f;  // C in units of 2^-8
static_assert(64u * kMaxKsteps * kMaxElem * kMaxElem < (1u << 24), "every partial sum is one exact float");
static_assert(64u * (kMaxKsteps + 1) * kMaxElem * kMaxElem >= (1u << 24), "and the cap is the largest that is");
static_assert(kLdsUsed == 147456 && kLdsUsed >= kRedBytes && kLdsUsed <= kLdsPerCu, "stages and tiles fit a CU's LDS");

// Four e4m3 of a panel: sign and mantissa from the hash, the exponent field 6 + two hashed bits.
XS_HD uint32_t operand_word(uint32_t seed, uint32_t set, uint32_t panel, uint32_t w) {
  const uint32_t h = fmix32(seed ^ (set << 23 | panel << 22 | w));
  return (h & 0x87878787u) | (0x30303030u + (h & 0x18181818u));
}
// The f32 bits of the scale of a row: 2^-2..2^1 for A, 1 or 2 for Bt.
XS_HD uint32_t scale_bits(uint32_t seed, uint32_t set, uint32_t panel, uint32_t row) {
  const uint32_t h = fmix32(seed ^ (1u << 30 | set << 23 | panel << 22 | row));
  return (panel ? 127u + (h & 1u) : 125u + (h & 3u)) << 23;
}

struct F8Record {
  PartRecordHead<kNumParts> head;
  uint32_t reserved;
  uint32_t subtiles, sets, spans;
  uint32_t pad[15];
};
static_assert(sizeof(F8Record) == 128, "one 128-byte record per workgroup");

using Expect = PartExpect<kNumParts>;

struct F8Args {
  const uint8_t* arena;
  const float* scales;   // [set][384]: sa, then sb
  const int32_t* fix;    // [set][128][256]
  const uint32_t* ytab;  // [set][128][128]
  uint32_t* ring;        // [workgroup][slot][128][128]
  uint32_t part_mask, seed, laps, ksteps, sets, slots;
};

// ------------------------------------------------------------------- device
XS_D void lds_dma16(const uint8_t* src, uint8_t* lds_dst) {
  __builtin_amdgcn_global_load_lds((GlobalPtr)src, (LdsPtr)lds_dst, 16, 0, 0);
}

// Ends a step: this lane's LDS reads are done, all but its newest `kLeft`
// vector-memory operations have completed, and so have every other lane's once
// the barrier is passed.
template <int kLeft>
XS_D void land_and_sync() {
  static_assert(kLeft == 0 || kLeft == 3 || kLeft == 11, "a step's DMAs, with a lap's stores in front of them");
  if constexpr (kLeft == 11)
    asm volatile("s_waitcnt vmcnt(11) lgkmcnt(0)\n\ts_barrier" ::: "memory");
  else if constexpr (kLeft == 3)
    asm volatile("s_waitcnt vmcnt(3) lgkmcnt(0)\n\ts_barrier" ::: "memory");
  else
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

XS_D i32x8 join(i32x4 lo, i32x4 hi) { return i32x8{lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w}; }
XS_D uint32_t fold4(i32x4 v, uint32_t s) {
  return rotl(static_cast<uint32_t>(v.x), s) + rotl(static_cast<uint32_t>(v.y), s + 1u) +
         rotl(static_cast<uint32_t>(v.z), s + 2u) + rotl(static_cast<uint32_t>(v.w), s + 3u);
}
XS_D uint32_t fold4(u32x4 v, uint32_t s) {
  return rotl(v.x, s) + rotl(v.y, s + 1u) + rotl(v.z, s + 2u) + rotl(v.w, s + 3u);
}
// min(diff, 1): one VALU instruction the optimiser does not turn back into a compare per element.
XS_D uint32_t differs(uint32_t diff) {
  uint32_t d;
  asm("v_min_u32_e32 %0, 1, %1" : "=v"(d) : "v"(diff));
  return d;
}
// Two floats to a dword of two bf16, round to nearest even; lo in the low half.
XS_D uint32_t pack_bf16(float lo, float hi) {
  uint32_t d;
  asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(d) : "v"(lo), "v"(hi));
  return d;
}

// One workgroup's whole run. g: its ring and its rotation of the sets; inj: the
// parts to inject; dump: kDump only. Leaves the tallies and the three masks.
template <bool kDump>
XS_D void run_f8load(const F8Args& a, uint32_t g, uint32_t inj, uint32_t* dump, uint8_t* lds, Tally (&y)[kNumParts],
                     uint32_t (&extra)[kExtra]) {
  const uint32_t t = threadIdx.x, lane = t & 63u, r = lane & 31u, h = lane >> 5;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const uint32_t ksteps = a.ksteps, laps = a.laps, sets = a.sets, slots = a.slots;
  const bool operand_on = (a.part_mask >> kOperand) & 1u, gemm_on = (a.part_mask >> kGemm) & 1u;
  const bool round_on = (a.part_mask >> kRound) & 1u, store_on = (a.part_mask >> kStore) & 1u;
  uint8_t* const tile = lds + kTilesOff + wave * kTileBytes;
  uint32_t* const ring = a.ring + static_cast<size_t>(g) * slots * kSlotWords;

  // DMA: instruction j of this wave fills slots 64 (8j + wave) + lane, rows
  // 16 (8j + wave) + (lane >> 2); the swizzle is in the source chunk.
  const uint32_t dma_src = wave * 1024u + (lane >> 2) * kStepBytes + (((lane & 3u) ^ ((lane >> 4) & 3u)) << 4);
  const uint32_t dma_dst = wave * 1024u;
  auto issue = [&](uint32_t set, uint32_t step, uint32_t stage) {
    const uint8_t* src = a.arena + static_cast<size_t>(set * ksteps + step) * kStageBytes;
    uint8_t* dst = lds + stage * kStageBytes;
#pragma unroll
    for (uint32_t j = 0; j < 3; ++j) lds_dma16(src + j * 8192u + dma_src, dst + j * 8192u + dma_dst);
  };
  // The issue cursor runs two steps ahead of the compute cursor.
  uint32_t ilap = 0, istep = 0, iset = set_of(g, 0, laps, sets), istage = 0;
  auto issue_next = [&] {
    issue(iset, istep, istage);
    istage = istage == kStages - 1 ? 0u : istage + 1u;
    if (++istep == ksteps) {
      istep = 0;
      ++ilap;
      iset = set_of(g, ilap < laps ? ilap : 0u, laps, sets);
    }
  };

  // The read-back of the tile lap `lp` stored: this wave takes region (wave + 1 + lp) & 7, which wave
  // (wave + 1) & 7 wrote; lane l holds chunk l & 7 (four dwords) of the region's rows e + 8 (l >> 3).
  const uint32_t back_at = 8u * (lane >> 3) * kYRow + 4u * (lane & 7u);
  u32x4 back[8];
  auto region_of = [&](uint32_t lp) {
    const uint32_t rsub = (wave + 1u + lp) & 7u;
    return 64u * (rsub >> 2) * kYRow + 32u * (rsub & 3u) + back_at;
  };
  auto fetch_back = [&](uint32_t lp) {
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    const uint32_t* src = ring + static_cast<size_t>(lp % slots) * kSlotWords + region_of(lp);
#pragma unroll
    for (uint32_t e = 0; e < 8; ++e) back[e] = *reinterpret_cast<const u32x4*>(src + e * kYRow);
  };
  uint32_t store_flip = ((inj >> kStore) & 1u) && t == 0;
  auto judge_back = [&](uint32_t lp, uint32_t span) {
    const uint32_t set = set_of(g, lp, laps, sets), at = region_of(lp);
    const uint32_t* want = a.ytab + static_cast<size_t>(set) * kSlotWords + at;
    uint32_t ne = 0, d = 0;
#pragma unroll
    for (uint32_t e = 0; e < 8; ++e) {
      const u32x4 w = *reinterpret_cast<const u32x4*>(want + e * kYRow);
      u32x4 got = back[e];
      if constexpr (kDump) {
        uint32_t* out = dump + static_cast<size_t>(laps) * kTileWords + static_cast<size_t>(lp) * kSlotWords + at;
        *reinterpret_cast<u32x4*>(out + e * kYRow) = got;
      }
      if (e == 0) got.x ^= store_flip;
      ne += differs(got.x ^ w.x) + differs(got.y ^ w.y) + differs(got.z ^ w.z) + differs(got.w ^ w.w);
      d += fold4(got, 4u * (lane & 7u));  // 128 row + 32 (region & 3) + 4 chunk + word: its low five bits
    }
    store_flip = 0;
    y[kStore].bad += ne;
    y[kStore].digest += d;
    if (ne && store_on) {
      extra[0] |= 1u << ((wave + 1u + lp) & 7u);
      extra[1] |= 1u << (set & 31u);
      extra[2] |= 1u << span;
    }
  };

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int q = 0; q < 16; ++q) acc[i][j][q] = 0.f;

  uint32_t operand_flip = ((inj >> kOperand) & 1u) && t == 0;
  uint32_t lap = 0, step = 0, set = iset, stage = 0, slot = 0;
  uint32_t sub = wave & 7u;  // (wave + lap) & 7
  bool behind = false;       // the step before this one issued eight stores or loads behind its DMAs
  const uint32_t total = laps * ksteps;
  // Where lane (r, h) finds chunk h of its rows (all congruent to r mod 32); chunk 2 + h is 32 bytes off.
  const uint32_t chunk0 = (h ^ ((r >> 2) & 3u)) << 4;

  constexpr uint32_t kAhead = kStages - 1;  // steps the DMA runs ahead of the MFMAs
  for (uint32_t d = 0; d < kAhead && d < total; ++d) issue_next();
  if (total > 1u)
    land_and_sync<3>();
  else
    land_and_sync<0>();

#pragma nounroll
  for (uint32_t gi = 0; gi < total; ++gi) {
    const bool more = gi + kAhead < total;
    if (more) issue_next();
    // A read-back follows a barrier that follows the stores it reads. With one step to a lap that is a barrier of
    // its own; otherwise the one that ends the lap's first step serves.
    const bool fetch = step == 0 && lap >= slots;
    if (fetch && ksteps == 1u) {
      asm volatile("s_barrier" ::: "memory");
      fetch_back(lap - slots);
    }

    const uint32_t sr = sub >> 2, sc = sub & 3u;
    const uint8_t* st = lds + stage * kStageBytes;
    const uint32_t a_row = 64u * sr + r, b_row = kRowsA + 64u * sc + r;
    i32x4 av[2][2], bv[2][2];  // [row block][k half of the lane: chunk h, chunk 2 + h]
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        av[i][c] = *reinterpret_cast<const i32x4*>(st + (a_row + 32u * i) * kStepBytes + (chunk0 ^ (32u * c)));
        bv[i][c] = *reinterpret_cast<const i32x4*>(st + (b_row + 32u * i) * kStepBytes + (chunk0 ^ (32u * c)));
      }
    if (operand_on) {
      // The low bits of the dwords' indices: 16 dwords per row and step; rows 32 apart and A's 128 rows leave them.
      const uint32_t s0 = 16u * ((r * ksteps + step) & 1u) + 4u * h;
      uint32_t f = rotl(static_cast<uint32_t>(av[0][0].x) ^ operand_flip, s0) - rotl(static_cast<uint32_t>(av[0][0].x), s0);
      y[kOperand].bad += operand_flip;
      operand_flip = 0;
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int c = 0; c < 2; ++c) f += fold4(av[i][c], s0 + 8u * c) + fold4(bv[i][c], s0 + 8u * c);
      y[kOperand].digest += f;
    }
    // Bt's rows are the MFMA's A, A's rows its B: a lane's registers run along a row of C.
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(join(bv[j][0], bv[j][1]), join(av[i][0], av[i][1]),
                                                                    acc[i][j], 0, 0, 0, 0, 0, 0);

    const bool last = step + 1u == ksteps;
    // What this lap read back is in registers, and compared, before the barrier its stores follow.
    if (last && lap >= slots) judge_back(lap - slots, 32u * lap / laps);

    // Step gi + 1 has landed; this stage may be overwritten.
    if (!more)
      land_and_sync<0>();
    else if (behind)
      land_and_sync<11>();
    else
      land_and_sync<3>();
    behind = last;
    if (fetch && ksteps != 1u) {
      fetch_back(lap - slots);
      behind = true;
    }

    if (last) {  // the lap is complete
      const int32_t* want = a.fix + static_cast<size_t>(set) * kTileWords;
      const uint32_t* ywant = a.ytab + static_cast<size_t>(set) * kSlotWords;
      const float* scale = a.scales + static_cast<size_t>(set) * kRows;
      uint32_t ne = 0, d = 0, rne = 0, rd = 0;
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const uint32_t row = 64u * sr + 32u * i + r;
        const float sa = scale[row];
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int q4 = 0; q4 < 4; ++q4) {
            const uint32_t col = 64u * sc + 32u * j + 8u * q4 + 4u * h;  // of register 4 q4; the next three follow
            const uint32_t idx = row * kRowsB + col;
            const i32x4 w = *reinterpret_cast<const i32x4*>(want + idx);
            const f32x4 sb = *reinterpret_cast<const f32x4*>(scale + kRowsA + col);
            const u32x2 yw = *reinterpret_cast<const u32x2*>(ywant + idx / 2);
            float yv[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const float c = acc[i][j][4 * q4 + e];
              if constexpr (kDump) dump[static_cast<size_t>(lap) * kTileWords + idx + e] = __float_as_uint(c);
              // (float)fix != v or got != want: v + 0.0f takes -0 to +0 and keeps a NaN a NaN, so the bits differ
              // exactly when the values do.
              const float v = c * kFixScale;
              const int32_t fix = static_cast<int32_t>(v);
              uint32_t got = static_cast<uint32_t>(fix);
              if (i == 0 && j == 0 && q4 == 0 && e == 0 && ((inj >> kGemm) & 1u) && t == 0 && lap == 0) got ^= 1u;
              ne += differs((__float_as_uint(static_cast<float>(fix)) ^ __float_as_uint(v + 0.0f)) |
                            (got ^ static_cast<uint32_t>(w[e])));
              d += got * (2u * (idx + e) + 1u);
              yv[e] = (c + 0.0f) * sa * sb[e];
              acc[i][j][4 * q4 + e] = 0.f;
            }
            const u32x2 pk = u32x2{pack_bf16(yv[0], yv[1]), pack_bf16(yv[2], yv[3])};
            uint32_t first = pk.x;
            if (i == 0 && j == 0 && q4 == 0 && ((inj >> kRound) & 1u) && t == 0 && lap == 0) first ^= 1u;
            rne += differs(first ^ yw.x) + differs(pk.y ^ yw.y);
            const uint32_t s = 16u * j + 4u * q4 + 2u * h;  // 128 row + col / 2: its low five bits
            rd += rotl(first, s) + rotl(pk.y, s + 1u);
            *reinterpret_cast<u32x2*>(tile + (32u * i + r) * kPitch + 64u * j + 16u * q4 + 8u * h) = pk;
          }
      }
      // The wave's tile as row chunks, and out: one instruction is eight whole 128-byte segments of rows of Y.
      uint32_t* out = ring + static_cast<size_t>(slot) * kSlotWords + 64u * sr * kYRow + 32u * sc + back_at;
#pragma unroll
      for (uint32_t e = 0; e < 8; ++e)
        *reinterpret_cast<u32x4*>(out + e * kYRow) =
            *reinterpret_cast<const u32x4*>(tile + (e + 8u * (lane >> 3)) * kPitch + 16u * (lane & 7u));
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
      y[kGemm].bad += ne;
      y[kGemm].digest += d;
      y[kRound].bad += rne;
      y[kRound].digest += rd;
      if ((gemm_on && ne) || (round_on && rne)) {
        extra[0] |= 1u << sub;
        extra[1] |= 1u << (set & 31u);
        extra[2] |= 1u << (32u * lap / laps);
      }
      sub = (sub + 1u) & 7u;
      slot = slot + 1u == slots ? 0u : slot + 1u;
      step = 0;
      ++lap;
      set = set_of(g, lap < laps ? lap : 0u, laps, sets);
    } else {
      ++step;
    }
    stage = stage == kStages - 1 ? 0u : stage + 1u;
  }

  // The laps whose slot no later lap reused: behind a barrier, one after the other.
  __syncthreads();
  for (uint32_t lp = laps > slots ? laps - slots : 0u; lp < laps; ++lp) {
    fetch_back(lp);
    judge_back(lp, 31u);
  }

  if constexpr (kDump) dump[static_cast<size_t>(laps) * (kTileWords + kSlotWords) + t] = y[kOperand].digest;
  // A part that is not selected leaves no tally: its digest in the record is 0.
#pragma unroll
  for (int p = 0; p < kNumParts; ++p)
    if (!((a.part_mask >> p) & 1u)) y[p] = Tally{};
}

__global__ __launch_bounds__(kBlock) void k_f8load_sweep(F8Record* __restrict__ records, F8Args a, int inject_xcd,
                                                        int inject_cu, uint32_t inject_parts, Expect expect) {
  extern __shared__ __attribute__((aligned(16))) uint8_t f8load_lds[];
  const uint32_t xcd = xcc_id();
  const uint32_t hw = hw_id();
  const uint32_t cu = cu_key(hw);
  const uint32_t simd = simd_id(hw);
  const bool inject = inject_selected(inject_xcd, inject_cu, xcd, cu);

  Tally y[kNumParts];
  uint32_t extra[kExtra] = {};
  run_f8load<false>(a, blockIdx.x, inject ? inject_parts & a.part_mask : 0u, nullptr, f8load_lds, y, extra);

  reduce_parts<kNumParts, kExtra, kBlock>(reinterpret_cast<uint32_t*>(f8load_lds), threadIdx.x, simd, y, extra,
                                          a.part_mask, expect, xcd, cu, &records[blockIdx.x]);
}

// One workgroup; dump holds laps x 32,768 words of C, laps x 16,384 of what was read back and 512 folds.
__global__ __launch_bounds__(kBlock) void k_f8load_probe(uint32_t* __restrict__ dump, F8Args a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t f8load_lds[];
  Tally y[kNumParts];
  uint32_t extra[kExtra] = {};
  run_f8load<true>(a, 0u, 0u, dump, f8load_lds, y, extra);
}

// --------------------------------------------------------------------- host
bool bad_shape(uint32_t laps, uint32_t ksteps, uint32_t slots) {
  return laps < 1 || laps > kMaxLaps || ksteps < 1 || ksteps > kMaxKsteps || slots < 1 || slots > kMaxSlots;
}

// One set in the logical order: the panels' dwords (128 and 256 rows of 16
// ksteps) and the scales' f32 bits (128 and 256).
void fill_set(uint32_t seed, uint32_t set, uint32_t ksteps, uint32_t* a_words, uint32_t* bt_words, uint32_t* sa,
              uint32_t* sb) {
  const uint32_t row_dwords = 16u * ksteps;
  for (uint32_t w = 0; w < kRowsA * row_dwords; ++w) a_words[w] = operand_word(seed, set, 0, w);
  for (uint32_t w = 0; w < kRowsB * row_dwords; ++w) bt_words[w] = operand_word(seed, set, 1, w);
  for (uint32_t row = 0; row < kRowsA; ++row) sa[row] = scale_bits(seed, set, 0, row);
  for (uint32_t row = 0; row < kRowsB; ++row) sb[row] = scale_bits(seed, set, 1, row);
}

uint32_t fold_of(const uint32_t* words, size_t first, size_t n) {
  uint32_t f = 0;
  for (size_t i = 0; i < n; ++i) f += rotl(words[i], static_cast<uint32_t>((first + i) & 31u));
  return f;
}

// Every element of a panel in units of 2^-4: +-(8 + m) 2^(E - 6). Returns the
// largest magnitude, or one past the bound for a byte outside the four binades.
int decode_panel(const uint32_t* words, size_t n_bytes, std::vector<int16_t>* out) {
  const uint8_t* bytes = reinterpret_cast<const uint8_t*>(words);
  out->resize(n_bytes);
  int top = 0;
  for (size_t i = 0; i < n_bytes; ++i) {
    const int e = (bytes[i] >> 3) & 15, m = (8 + (bytes[i] & 7)) << (e - 6);
    if (e < 6 || e > 9) return kMaxElem + 1;
    (*out)[i] = static_cast<int16_t>(bytes[i] & 0x80 ? -m : m);
    top = m > top ? m : top;
  }
  return top;
}

// bf16(fix 2^(e - 8)) for |fix| < 2^24, in integers: the f32 is exact, then one round to nearest even.
uint32_t bf16_of(int32_t fix, int e) {
  if (fix == 0) return 0;  // an exact zero sum is +0
  const uint32_t mag = static_cast<uint32_t>(fix < 0 ? -fix : fix);
  int top = 23;
  while (!(mag >> top)) --top;
  const uint32_t bits = (fix < 0 ? 0x80000000u : 0u) | static_cast<uint32_t>(127 + top + e - 8) << 23 |
                        ((mag << (23 - top)) & 0x7fffffu);
  return (bits + 0x7fffu + ((bits >> 16) & 1u)) >> 16;
}

// What the host holds of a (seed, ksteps, sets): the arena's bytes, the scales,
// both tables and, per set, the folds of its panels and the digests of its
// product and of its bf16 tile.
struct HostSets {
  std::vector<uint32_t> arena;   // sets x ksteps x 24,576 bytes
  std::vector<uint32_t> scales;  // sets x 384 f32 bits
  std::vector<int32_t> fix;      // sets x 128 x 256 of C 2^8
  std::vector<uint32_t> ytab;    // sets x 128 x 128 of two bf16
  std::vector<uint32_t> fold_a, fold_bt, gemm, round;
  bool bound_ok = true;
};

struct DeviceSets {
  DevMem arena, scales, fix, ytab;
};

std::mutex g_sets_mu;
std::map<std::tuple<uint32_t, uint32_t, uint32_t>, std::unique_ptr<HostSets>> g_host_sets;
std::map<std::tuple<int, uint32_t, uint32_t, uint32_t>, std::unique_ptr<DeviceSets>> g_device_sets;

// g_sets_mu held.
const HostSets& host_sets(uint32_t seed, uint32_t ksteps, uint32_t sets) {
  auto& slot = g_host_sets[{seed, ksteps, sets}];
  if (slot) return *slot;
  slot = std::make_unique<HostSets>();
  HostSets& hs = *slot;
  const size_t row_dwords = 16u * static_cast<size_t>(ksteps), K = 4 * row_dwords;
  const size_t a_dwords = kRowsA * row_dwords, bt_dwords = kRowsB * row_dwords;
  const size_t set_dwords = static_cast<size_t>(ksteps) * kStageBytes / 4;
  hs.arena.resize(sets * set_dwords);
  hs.scales.resize(static_cast<size_t>(sets) * kRows);
  hs.fix.resize(static_cast<size_t>(sets) * kTileWords);
  hs.ytab.resize(static_cast<size_t>(sets) * kSlotWords);
  std::vector<uint32_t> aw(a_dwords), bw(bt_dwords);
  std::vector<int16_t> A, Bt;
  for (uint32_t s = 0; s < sets; ++s) {
    uint32_t* sa = hs.scales.data() + static_cast<size_t>(s) * kRows;
    uint32_t* sb = sa + kRowsA;
    fill_set(seed, s, ksteps, aw.data(), bw.data(), sa, sb);
    hs.fold_a.push_back(fold_of(aw.data(), 0, a_dwords));
    hs.fold_bt.push_back(fold_of(bw.data(), a_dwords, bt_dwords));
    // The arena's order: per step the 16 dwords of every row.
    for (uint32_t step = 0; step < ksteps; ++step) {
      uint32_t* blk = hs.arena.data() + s * set_dwords + static_cast<size_t>(step) * (kStageBytes / 4);
      for (uint32_t row = 0; row < kRows; ++row) {
        const uint32_t* src = row < kRowsA ? &aw[row * row_dwords] : &bw[(row - kRowsA) * row_dwords];
        for (uint32_t q = 0; q < 16; ++q) blk[row * 16 + q] = src[step * 16 + q];
      }
    }
    if (decode_panel(aw.data(), kRowsA * K, &A) > kMaxElem || decode_panel(bw.data(), kRowsB * K, &Bt) > kMaxElem) {
      hs.bound_ok = false;
      return hs;
    }
    int32_t* C = hs.fix.data() + static_cast<size_t>(s) * kTileWords;
    uint32_t* Y = hs.ytab.data() + static_cast<size_t>(s) * kSlotWords;
    uint32_t d = 0;
    for (uint32_t i = 0; i < kRowsA; ++i)
      for (uint32_t j = 0; j < kRowsB; ++j) {
        int32_t sum = 0, mag = 0;
        for (size_t k = 0; k < K; ++k) {
          const int32_t p = static_cast<int32_t>(A[i * K + k]) * static_cast<int32_t>(Bt[j * K + k]);
          sum += p;
          mag += p < 0 ? -p : p;
        }
        if (mag >= (1 << 24)) hs.bound_ok = false;  // the bound of the header, on what was generated
        C[i * kRowsB + j] = sum;
        d += static_cast<uint32_t>(sum) * (2u * (i * kRowsB + j) + 1u);
        const int e = static_cast<int>(sa[i] >> 23) + static_cast<int>(sb[j] >> 23) - 254;
        const uint32_t half = bf16_of(sum, e);
        if (j & 1u)
          Y[(i * kRowsB + j) / 2] |= half << 16;
        else
          Y[(i * kRowsB + j) / 2] = half;
      }
    hs.gemm.push_back(d);
    hs.round.push_back(fold_of(Y, 0, kSlotWords));
  }
  return hs;
}

// The digests of a healthy workgroup; 0 for a part outside the mask. Every
// lap's tile is read back once, so store is round.
int expected_digests(uint32_t mask, uint32_t seed, uint32_t laps, uint32_t ksteps, uint32_t sets, uint32_t* out) {
  std::lock_guard<std::mutex> g(g_sets_mu);
  const HostSets& hs = host_sets(seed, ksteps, sets);
  if (!hs.bound_ok) {
    std::snprintf(g_f8_err, sizeof g_f8_err, "an operand left the bound that keeps every sum exact");
    return kBoundBroken;
  }
  uint32_t d[kNumParts] = {};
  for (uint32_t l = 0; l < laps; ++l) {
    const uint32_t s = set_of(0, l, laps, sets);
    d[kOperand] += 4u * hs.fold_a[s] + 2u * hs.fold_bt[s];
    d[kGemm] += hs.gemm[s];
    d[kRound] += hs.round[s];
  }
  d[kStore] = d[kRound];
  for (int p = 0; p < kNumParts; ++p) out[p] = (mask >> p) & 1u ? d[p] : 0u;
  return 0;
}

// Arena, scales and tables of (seed, ksteps, sets) on the current device `dev`,
// built and uploaded once, and a ring of blocks x slots slots for this call in
// *ring, cleared. -1003 when any of it cannot be allocated: nothing is launched.
int device_sets(int dev, uint32_t sets, uint32_t blocks, DevMem* ring, F8Args* a) {
  std::lock_guard<std::mutex> g(g_sets_mu);
  auto& slot = g_device_sets[{dev, a->seed, a->ksteps, sets}];
  if (!slot) {
    const HostSets& hs = host_sets(a->seed, a->ksteps, sets);
    if (!hs.bound_ok) return kBoundBroken;
    auto ds = std::make_unique<DeviceSets>();  // what was had is freed with ds
    const std::pair<DevMem*, const std::vector<uint32_t>*> words[] = {
        {&ds->arena, &hs.arena}, {&ds->scales, &hs.scales}, {&ds->ytab, &hs.ytab}};
    bool got = hipMalloc(&ds->fix.p, hs.fix.size() * 4) == hipSuccess;
    for (const auto& [mem, src] : words) got = got && hipMalloc(&mem->p, src->size() * 4) == hipSuccess;
    if (!got) {
      (void)hipGetLastError();
      std::snprintf(g_f8_err, sizeof g_f8_err, "no arena of %zu bytes and its tables could be had: nothing was swept",
                    hs.arena.size() * 4);
      return kUnswept;
    }
    XS_CHECK(hipMemcpy(ds->fix.p, hs.fix.data(), hs.fix.size() * 4, hipMemcpyHostToDevice));
    for (const auto& [mem, src] : words) XS_CHECK(hipMemcpy(mem->p, src->data(), src->size() * 4, hipMemcpyHostToDevice));
    slot = std::move(ds);
  }
  const size_t ring_bytes = static_cast<size_t>(blocks) * a->slots * kSlotWords * 4;
  if (hipMalloc(&ring->p, ring_bytes) != hipSuccess) {
    (void)hipGetLastError();
    ring->p = nullptr;
    std::snprintf(g_f8_err, sizeof g_f8_err, "no ring of %zu bytes could be had: nothing was swept", ring_bytes);
    return kUnswept;
  }
  XS_CHECK(hipMemset(ring->p, 0, ring_bytes));
  a->arena = slot->arena.as<const uint8_t>();
  a->scales = slot->scales.as<const float>();
  a->fix = slot->fix.as<const int32_t>();
  a->ytab = slot->ytab.as<const uint32_t>();
  a->ring = ring->as<uint32_t>();
  a->sets = sets;
  return 0;
}

}  // namespace

extern "C" {

const char* xs_f8load_sweep_last_error() { return g_f8_err; }

// Part names, comma-separated, in bit order.
const char* xs_f8load_parts() { return kPartNames; }

// out2 = {words whatever the laps, words per lap} of a part in the probe's
// dump: gemm has 32,768 per lap, store 16,384, the operand fold one per
// thread; round stays in registers.
int xs_f8load_shape(int part, int* out2) {
  if (part < 0 || part >= kNumParts || !out2) return kBadArgs;
  out2[0] = part == kOperand ? kBlock : 0;
  out2[1] = part == kGemm ? static_cast<int>(kTileWords) : part == kStore ? static_cast<int>(kSlotWords) : 0;
  return 0;
}

// Host only. One set in the logical order, whatever the arena's: the e4m3
// bytes a_out[128][64 ksteps] and bt_out[256][64 ksteps] and the scales as f32
// sa_out[128] and sb_out[256].
int xs_f8load_operands(uint32_t seed, uint32_t set, uint32_t ksteps, void* a_out, void* bt_out, void* sa_out,
                       void* sb_out) {
  if (set >= kMaxSets || ksteps < 1 || ksteps > kMaxKsteps || !a_out || !bt_out || !sa_out || !sb_out) return kBadArgs;
  fill_set(seed, set, ksteps, static_cast<uint32_t*>(a_out), static_cast<uint32_t*>(bt_out),
           static_cast<uint32_t*>(sa_out), static_cast<uint32_t*>(sb_out));
  return 0;
}

// One workgroup at any shape, 16 sets; out = [laps][128][256] raw f32 bits of
// C, then [laps][128][128]: the dwords the read-back of each lap's tile
// returned, then [512]: every thread's operand fold.
// n_words = laps x 49,152 + 512. The mask selects whether the fold is issued.
int xs_f8load_probe(int dev, uint32_t part_mask, uint32_t seed, uint32_t laps, uint32_t ksteps, uint32_t slots,
                    uint32_t* out, size_t n_words) {
  if (bad_part_mask(part_mask, kAllParts) || bad_shape(laps, ksteps, slots) || !out) return kBadArgs;
  const size_t n = static_cast<size_t>(laps) * (kTileWords + kSlotWords) + kBlock;
  if (n_words != n) return kBadArgs;
  F8Args a{nullptr, nullptr, nullptr, nullptr, nullptr, part_mask, seed, laps, ksteps, 0, slots};
  DevMem ring;
  return launch_probe(
      g_f8_err, dev, reinterpret_cast<const void*>(k_f8load_probe), kBlock, kLdsUsed, out, n,
      [&](dim3 grid, dim3 block, size_t smem, void* dump) {
        hipLaunchKernelGGL(k_f8load_probe, grid, block, smem, 0, static_cast<uint32_t*>(dump), a);
      },
      [&] { return device_sets(dev, kF8Sets, 1, &ring, &a); });
}

// Host only. out4[p] = the workgroup digest a healthy CU leaves for part p, 0
// for a part outside part_mask. `slots` does not enter a digest; it is checked.
int xs_f8load_sweep_expected(uint32_t part_mask, uint32_t seed, uint32_t laps, uint32_t ksteps, uint32_t slots,
                             uint32_t* out4) {
  if (bad_part_mask(part_mask, kAllParts) || bad_shape(laps, ksteps, slots) || !out4) return kBadArgs;
  return expected_digests(part_mask, seed, laps, ksteps, kF8Sets, out4);
}

// What the runtime reports for k_f8load_sweep on `dev`: out4 = {registers per
// lane, scratch bytes per lane, dynamic LDS bytes per workgroup, workgroups
// that fit on a CU at once}.
int xs_f8load_sweep_info(int dev, int* out4) {
  return sweep_info(g_f8_err, dev, reinterpret_cast<const void*>(k_f8load_sweep), kBlock, true, out4);
}

// One sweep launch of `blocks` workgroups (0: 4 per CU) of `laps` laps of
// K = 64 ksteps over 16 sets, `slots` ring slots of 64 KiB per workgroup.
// Writes `blocks` 128-byte records to records_out. inject_xcd / inject_cu: -1
// is none / any, values below -1 are refused. Returns 0, -1000 for bad
// arguments (ksteps above 18 among them) and -1003 when arena, tables or ring
// could not be allocated (nothing is launched either way), or a negative HIP
// error. The ring is freed before it returns.
int xs_f8load_sweep(int dev, int blocks, uint32_t part_mask, uint32_t seed, uint32_t laps, uint32_t ksteps,
                    uint32_t slots, int inject_xcd, int inject_cu, uint32_t inject_parts, void* records_out,
                    int* n_records, double* ms) {
  if (bad_part_mask(part_mask, kAllParts) || bad_shape(laps, ksteps, slots) || (inject_parts & ~kAllParts))
    return kBadArgs;
  // launch_sweep refuses these too, but only after the host has built the sets.
  if (!records_out || blocks < 0 || blocks > kMaxBlocks || inject_xcd < -1 || inject_cu < -1 || inject_xcd > 15 ||
      inject_cu > 0xff)
    return kBadArgs;
  if (!blocks) XS_CHECK(cu_count(dev, &blocks, 4));  // the ring is sized by it
  if (blocks <= 0 || blocks > kMaxBlocks) return kBadArgs;
  Expect e;
  if (int rc = expected_digests(part_mask, seed, laps, ksteps, kF8Sets, e.digest)) return rc;
  F8Args a{nullptr, nullptr, nullptr, nullptr, nullptr, part_mask, seed, laps, ksteps, 0, slots};
  DevMem ring;
  return launch_sweep(
      g_f8_err, {dev, blocks, inject_xcd, inject_cu, records_out, n_records, ms},
      reinterpret_cast<const void*>(k_f8load_sweep), kBlock, kLdsUsed, sizeof(F8Record),
      [&](dim3 grid, dim3 block, size_t smem, void* rec) {
        hipLaunchKernelGGL(k_f8load_sweep, grid, block, smem, 0, static_cast<F8Record*>(rec), a, inject_xcd, inject_cu,
                           inject_parts, e);
      },
      [&] { return device_sets(dev, kF8Sets, static_cast<uint32_t>(blocks), &ring, &a); });
}

}  // extern "C"
