// MX load sweep for gfx950 (MI355X): every CU under load, with a checked
// block-scaled FP4 GEMM.
//
// load_sweep.hip holds every CU at rate with v_mfma_i32_32x32x32_i8. The work
// placed on this part mostly runs block-scaled FP4 and FP8 through
// v_mfma_scale_f32_32x32x64_f8f6f4: another data path of the matrix core (a
// mini-float decoder, an E8M0 scale side channel selected by opsel, a float
// adder tree and accumulator), which matrix_sweep.hip touches for two K-steps,
// cold, with operands built in registers. k_mxload_sweep is a sweep over named
// parts (part_sweep.h) whose load is an MXFP4 GEMM pipeline: operands and scale
// bytes come from memory by LDS DMA (global_load_lds_dwordx4, no staging
// registers) into a ring of three LDS stages and from there into the MFMA, two
// waves on every SIMD, for many laps in one launch. All 16 codes of e2m1 are
// finite, so full-entropy hashed bits are valid operands, and with the scale
// ranges below every sum is one exact float: every result of every lap is
// compared on the device by equality, with no tolerance.
//
// Operands. A set s is A_s[128][K] and Bt_s[256][K] of e2m1 (B transposed: k is
// contiguous), K = 128 ksteps. A panel is row-major, K/2 bytes per row; byte b
// of a row holds element 2b in its low nibble and 2b+1 in its high nibble (the
// packing matrix_sweep.hip's header pins for fp4). Dword w of panel p (0: A,
// 1: Bt) of set s is
//     fmix32(seed ^ (s << 23 | p << 22 | w)).
// Scales: one E8M0 byte per row and 32-element k-block, four per row and
// pipeline step (128 elements of k). With
//     h = fmix32(seed ^ (1u << 30 | s << 23 | p << 22 | row ksteps + step))
// the byte of block g (0..3) of that step is 126 + ((h >> 8g) & 3) for A
// (2^-1 .. 2^2) and 127 + ((h >> 8g) & 1) for Bt (1, 2); 255 (NaN) never
// occurs. The four bytes of a row and step are one little-endian scale word;
// a set's scale array is its 384 ksteps words, A's rows before Bt's, word
// row ksteps + step.
// Exactness bound. An element is +-{0, 0.5, 1, 1.5, 2, 3, 4, 6}. A's element
// times its scale is an integer of at most 96 units of 2^-2, Bt's one of at
// most 24 units of 2^-1: every product is a multiple of 2^-3 of at most 2,304
// units (288). Any partial sum in any order is therefore a multiple of 2^-3
// below K 2,304 units, which is under 2^24 for K <= 7,281: ksteps <= 56, larger
// values are refused. host_sets() re-checks the two maxima on what it
// generated. The host computes fix = 8 C in plain int32 and keeps it as a
// table of 128 KiB per set, built once per (seed, ksteps, sets).
//
// Arena. Physical order is not the logical one: a set is `ksteps` blocks of
// 26,112 bytes, block `step` = the 64 bytes of that step of each of the 384
// rows (A's before Bt's), then the 384 scale words of that step. A step's DMA
// therefore reads one contiguous block, and the scale DMA is coalesced. The
// sweep's shape (16 ksteps, 16 sets) is 6.4 MiB, more than one XCD's L2.
//
// Work split: the load sweep's. 512 threads, two waves per SIMD,
// exclusive_lds(); a macro tile C[128 x 256] per lap; a wave owns a 64 x 64
// sub-tile (four f32x16 accumulators); sub-tile (w + l) & 7 and set
// set_of(g, l, laps, sets) in lap l (part_sweep.h).
//
// Staging by LDS DMA. Per step the 384 x 64 operand bytes go to LDS in 1,536
// chunks of 16 bytes, three global_load_lds_dwordx4 per thread. The LDS
// destination of one instruction is wave-linear (base + lane 16: pinned on the
// hardware by the lane sweep's ldsdma path), so rows cannot be padded. The
// layout is XOR-swizzled instead and the permutation goes into the source
// address: LDS slot q of a stage (16 bytes; q = 64 (8j + w) + lane for
// instruction j of wave w) holds chunk (q & 3) ^ ((q >> 4) & 3) of row q >> 2.
// An operand read of lane (r, h) for k-half kh is one 128-bit read at
// row 64 + (((2 kh + h) ^ ((row >> 2) & 3)) << 4). A 128-bit access is served
// 16 lanes at a time; 16 consecutive rows then start in 16 different groups of
// four banks (4 (row & 3) + (chunk ^ ((row >> 2) & 3)) takes 16 values), so
// the reads are free of conflicts under the 64-bank model of the public CDNA3
// material. That model is assumed for CDNA4; no counter was read.
// Scales take a fourth DMA of 4 bytes by waves 0..5: one word per row and step.
// A lane reads its rows' words from LDS and hands them to the MFMA as loaded
// but for one shift by 8 h: the scale of k-block g of an MFMA is taken from
// lane 32 g + r (matrix_sweep.hip's header), so lane (r, h) supplies block
// 2 kh + h, and after the shift k-half kh finds it under opsel 2 kh.
//
// Pipeline. A ring of three stages of 26,112 bytes (78,336 in all). The DMA of
// step k + 2 is issued before the MFMAs of step k; s_waitcnt vmcnt leaves only
// that newest step's DMAs outstanding (4 per lane in waves 0..5, 3 in waves 6
// and 7), so step k + 1 has landed; one barrier per step; a stage is
// overwritten only after the barrier that follows its last read. (The
// compiler is free to let a step's MFMAs, which touch registers only, issue
// behind that barrier, next to the following step's reads; it does.) Per step and
// wave: 8 reads of 128 bits, 4 scale words, 2 k-halves x 4 accumulators = 8
// v_mfma_scale_f32_32x32x64_f8f6f4 with cbsz = blgp = 4; the upper four dwords
// of the operands are zero. After the last step of a lap each lane takes its
// 64 accumulators through fix = (int)(acc 8.0f), counts a mismatch when
// (float)fix != acc 8.0f (NaN and a lost fraction among them) or
// fix != table[idx], folds the digest and clears the accumulators.
//
// Parts (bit, name). The mask selects what is judged; the pipeline always runs.
//   0 operand  every operand dword a wave reads from LDS on its way into an
//              MFMA: sum of rotl(word, i & 31), i the dword's index in its set
//              (logical order, A before Bt). An A dword is read by four waves,
//              a Bt dword by two: 4 sum(A) + 2 sum(Bt) per lap. Covers
//              L2/L1 -> DMA -> LDS -> registers. Not issued when not selected.
//   1 scale    every scale word as read from LDS, before the shift: the same
//              fold over its index in the set's scale array. Both lane halves
//              read a row's word: 8 sum(A) + 4 sum(Bt) per lap. Not issued
//              when not selected.
//   2 gemm     mismatches against the table; the digest is the sum of
//              uint32(fix) (2 (256 row + col) + 1) over the laps.
// A bad gemm with good operand and scale names the f8f6f4 path of the matrix
// core; a bad operand names the route into LDS. There is no stage part (the
// DMA has no register view) and no valu part (load_sweep.hip has it).
//
// Record (128 bytes per workgroup): part_sweep.h's head with three parts, the
// reserved word and the load sweep's three ORed masks: sub-tiles, sets (bit =
// set & 31) and 32 equal spans of the launch's laps that mis-compared.
// Injection: bit 0 of word 0 of the part is flipped in registers (operand,
// scale: word 0 of the first set, in the fold only; gemm: fix of C[0][0] of
// lap 0).
//
// Safety rules. Trip counts come from the kernel arguments only; nothing
// waits on a clock, a flag or another workgroup. No scratch, no vector register
// spilled (the compiler parks some scalars in lanes of a vector register, which
// touches no memory), MODE is not written, results leave through vector stores. Arena and table are never
// written; every index into them is below ksteps sets 26,112 and 32,768 sets
// by construction (set < sets, step < ksteps, row < 384), and every LDS
// address below 3 x 26,112. laps above 16 x the default are refused.
//
// k_mxload_probe is the same device function with a dump: one workgroup at any
// shape stores C of every lap as [lap][128][256] raw f32 bits and behind it
// each thread's operand and scale folds ([2][512]).
//
// NOT covered: fp8, bf8, fp6 and bf6 under load (their hashed bits do not give
// exact sums); mixed formats and the 16x16x128 shape; HBM traffic, and which
// cache level served a DMA; power, clocks and temperature.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <memory>
#include <mutex>
#include <tuple>
#include <vector>

#include "hip/part_sweep.h"

#define XS_ERR_BUF g_mxload_err
#define XS_HD __host__ __device__ __forceinline__
#define XS_D __device__ __forceinline__

namespace {

using namespace xsprobe;

ErrBuf g_mxload_err = "";

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __attribute__((address_space(1))) const void* GlobalPtr;
typedef __attribute__((address_space(3))) void* LdsPtr;

constexpr int kNumParts = 3;
const char kPartNames[] = "operand,scale,gemm";
constexpr uint32_t kAllParts = (1u << kNumParts) - 1;
constexpr int kOperand = 0, kScale = 1, kGemm = 2;
constexpr int kBlock = 512;  // 8 waves: two per SIMD
constexpr int kExtra = 3;    // sub-tile, set and span masks
constexpr int kUnswept = -1003;
constexpr int kBoundBroken = -1001;  // the generator left its stated bound (a bug in this file)

// The sweep's fixed shape and defaults: measured in profiles/mxload_sweep_defaults.md.
constexpr uint32_t kMxKsteps = 16, kMxSets = 16;
constexpr uint32_t kMxLaps = 1024;
constexpr uint32_t kMaxLaps = 16 * kMxLaps, kMaxKsteps = 56, kMaxSets = 64;

constexpr uint32_t kRowsA = 128, kRowsB = 256, kRows = kRowsA + kRowsB;
constexpr uint32_t kStepBytes = 64;                           // 128 e2m1 of k, per row and step
constexpr uint32_t kScaleOff = kRows * kStepBytes;            // 24,576: where a stage's scale words begin
constexpr uint32_t kStageBytes = kScaleOff + kRows * 4;       // 26,112: a stage, and a step's block of the arena
constexpr uint32_t kStages = 3;
constexpr uint32_t kTileWords = kRowsA * kRowsB;              // C of one set: 128 KiB
constexpr uint32_t kFoldWords = 2 * kBlock;                   // the probe's per-thread folds
constexpr uint32_t kRedBytes = part_reduction_words<kBlock>(kNumParts, kExtra) * 4;
constexpr uint32_t kLdsUsed = kStages * kStageBytes > kRedBytes ? kStages * kStageBytes : kRedBytes;
constexpr int kMaxA = 96, kMaxB = 24;  // |element x scale| in units of 2^-2 (A) and 2^-1 (Bt)
static_assert(128u * kMaxKsteps * kMaxA * kMaxB < (1u << 24), "every partial sum is one exact float");

XS_HD uint32_t operand_word(uint32_t seed, uint32_t set, uint32_t panel, uint32_t w) {
  return fmix32(seed ^ (set << 23 | panel << 22 | w));
}
// The four E8M0 bytes of (row, step) of a panel, block g in byte g.
XS_HD uint32_t scale_word(uint32_t seed, uint32_t set, uint32_t panel, uint32_t row_step) {
  const uint32_t h = fmix32(seed ^ (1u << 30 | set << 23 | panel << 22 | row_step));
  return panel ? 0x7f7f7f7fu + (h & 0x01010101u) : 0x7e7e7e7eu + (h & 0x03030303u);
}

struct MxRecord {
  PartRecordHead<kNumParts> head;
  uint32_t reserved;
  uint32_t subtiles, sets, spans;
  uint32_t pad[17];
};
static_assert(sizeof(MxRecord) == 128, "one 128-byte record per workgroup");

using Expect = PartExpect<kNumParts>;

struct MxArgs {
  const uint8_t* arena;
  const int32_t* table;
  uint32_t part_mask, seed, laps, ksteps, sets;
};

// ------------------------------------------------------------------- device
// The sizes are literals: the builtin takes no template parameter.
XS_D void lds_dma16(const uint8_t* src, uint8_t* lds_dst) {
  __builtin_amdgcn_global_load_lds((GlobalPtr)src, (LdsPtr)lds_dst, 16, 0, 0);
}
XS_D void lds_dma4(const uint8_t* src, uint8_t* lds_dst) {
  __builtin_amdgcn_global_load_lds((GlobalPtr)src, (LdsPtr)lds_dst, 4, 0, 0);
}

// Ends a step: this lane's LDS reads are done, all but its newest `kLeft` DMAs
// have landed, and so have every other lane's once the barrier is passed.
template <int kLeft>
XS_D void land_and_sync() {
  static_assert(kLeft == 0 || kLeft == 3 || kLeft == 4, "a step's DMAs per lane");
  if constexpr (kLeft == 4)
    asm volatile("s_waitcnt vmcnt(4) lgkmcnt(0)\n\ts_barrier" ::: "memory");
  else if constexpr (kLeft == 3)
    asm volatile("s_waitcnt vmcnt(3) lgkmcnt(0)\n\ts_barrier" ::: "memory");
  else
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

XS_D i32x8 low_half(i32x4 v) { return i32x8{v.x, v.y, v.z, v.w, 0, 0, 0, 0}; }
XS_D uint32_t fold4(i32x4 v, uint32_t s) {
  return rotl(static_cast<uint32_t>(v.x), s) + rotl(static_cast<uint32_t>(v.y), s + 1u) +
         rotl(static_cast<uint32_t>(v.z), s + 2u) + rotl(static_cast<uint32_t>(v.w), s + 3u);
}

// One workgroup's whole run. g: its rotation of the sets; inj: the parts to
// inject; dump: kDump only. Leaves the tallies and the three masks.
template <bool kDump>
XS_D void run_mxload(const MxArgs& a, uint32_t g, uint32_t inj, uint32_t* dump, uint8_t* lds, Tally (&y)[kNumParts],
                     uint32_t (&extra)[kExtra]) {
  const uint32_t t = threadIdx.x, lane = t & 63u, r = lane & 31u, h = lane >> 5;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const uint32_t ksteps = a.ksteps, laps = a.laps, sets = a.sets;
  const bool operand_on = (a.part_mask >> kOperand) & 1u, scale_on = (a.part_mask >> kScale) & 1u;
  const bool scale_dma = wave < 6u;  // 384 rows: six waves of 64 words

  // DMA: instruction j of this wave fills slots 64 (8j + wave) + lane, rows
  // 16 (8j + wave) + (lane >> 2); the swizzle is in the source chunk.
  const uint32_t dma_src = wave * 1024u + (lane >> 2) * kStepBytes + (((lane & 3u) ^ ((lane >> 4) & 3u)) << 4);
  const uint32_t dma_dst = wave * 1024u;
  auto issue = [&](uint32_t set, uint32_t step, uint32_t stage) {
    const uint8_t* src = a.arena + static_cast<size_t>(set * ksteps + step) * kStageBytes;
    uint8_t* dst = lds + stage * kStageBytes;
#pragma unroll
    for (uint32_t j = 0; j < 3; ++j) lds_dma16(src + j * 8192u + dma_src, dst + j * 8192u + dma_dst);
    if (scale_dma) lds_dma4(src + kScaleOff + wave * 256u + lane * 4u, dst + kScaleOff + wave * 256u);
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
  auto end_step = [&](bool dma_in_flight) {
    if (!dma_in_flight)
      land_and_sync<0>();
    else if (scale_dma)
      land_and_sync<4>();
    else
      land_and_sync<3>();
  };

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int q = 0; q < 16; ++q) acc[i][j][q] = 0.f;

  uint32_t operand_flip = ((inj >> kOperand) & 1u) && t == 0;
  uint32_t scale_flip = ((inj >> kScale) & 1u) && t == 0;
  uint32_t lap = 0, step = 0, set = iset, stage = 0;
  uint32_t sub = wave & 7u;  // (wave + lap) & 7
  const uint32_t total = laps * ksteps;
  // Where lane (r, h) finds chunk h of its rows (all congruent to r mod 32); chunk 2 + h is 32 bytes off.
  const uint32_t chunk0 = (h ^ ((r >> 2) & 3u)) << 4;

  constexpr uint32_t kAhead = kStages - 1;  // steps the DMA runs ahead of the MFMAs
  for (uint32_t d = 0; d < kAhead && d < total; ++d) issue_next();
  end_step(kAhead > 1u && total > 1u);

#pragma nounroll
  for (uint32_t gi = 0; gi < total; ++gi) {
    const bool more = gi + kAhead < total;
    if (more) issue_next();

    const uint32_t sr = sub >> 2, sc = sub & 3u;
    const uint8_t* st = lds + stage * kStageBytes;
    const uint32_t a_row = 64u * sr + r, b_row = kRowsA + 64u * sc + r;
    // The scale words of this lane's four rows; block 2 kh + h comes under opsel 2 kh.
    uint32_t sw[4];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      sw[i] = *reinterpret_cast<const uint32_t*>(st + kScaleOff + (a_row + 32u * i) * 4u);
      sw[2 + i] = *reinterpret_cast<const uint32_t*>(st + kScaleOff + (b_row + 32u * i) * 4u);
    }
    if (scale_on) {
      // Rows 32 apart and the 128 rows of A leave (row ksteps + step) & 31 that of r.
      const uint32_t s = r * ksteps + step;
      y[kScale].digest += rotl(sw[0] ^ scale_flip, s) + rotl(sw[1], s) + rotl(sw[2], s) + rotl(sw[3], s);
      y[kScale].bad += scale_flip;
      scale_flip = 0;
    }
    int sa[2], sb[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      sa[i] = static_cast<int>(sw[i] >> (8u * h));
      sb[i] = static_cast<int>(sw[2 + i] >> (8u * h));
    }
    // The low bits of the operand dwords' indices: as the scale words', by 16 dwords per row and step.
    const uint32_t s0 = 16u * ((r * ksteps + step) & 1u) + 4u * h;
#pragma unroll
    for (int kh = 0; kh < 2; ++kh) {
      const uint32_t off = chunk0 ^ (32u * kh);
      i32x4 av[2], bv[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        av[i] = *reinterpret_cast<const i32x4*>(st + (a_row + 32u * i) * kStepBytes + off);
        bv[i] = *reinterpret_cast<const i32x4*>(st + (b_row + 32u * i) * kStepBytes + off);
      }
      if (operand_on) {
        uint32_t f = 0;
        if (kh == 0) {
          f = rotl(static_cast<uint32_t>(av[0].x) ^ operand_flip, s0) - rotl(static_cast<uint32_t>(av[0].x), s0);
          y[kOperand].bad += operand_flip;
          operand_flip = 0;
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) f += fold4(av[i], s0 + 8u * kh) + fold4(bv[i], s0 + 8u * kh);
        y[kOperand].digest += f;
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          if (kh == 0)
            acc[i][j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(low_half(av[i]), low_half(bv[j]), acc[i][j], 4,
                                                                        4, 0, sa[i], 0, sb[j]);
          else
            acc[i][j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(low_half(av[i]), low_half(bv[j]), acc[i][j], 4,
                                                                        4, 2, sa[i], 2, sb[j]);
        }
    }

    end_step(more && kAhead > 1u);  // step gi + 1 has landed; this stage may be overwritten

    if (step + 1u == ksteps) {  // the lap is complete
      const int32_t* want = a.table + static_cast<size_t>(set) * kTileWords;
      uint32_t ne = 0, d = 0;
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
#pragma unroll
          for (int q = 0; q < 16; ++q) {
            const uint32_t row = 64u * sr + 32u * i + (q & 3) + 8u * (q >> 2) + 4u * h;
            const uint32_t idx = row * kRowsB + 64u * sc + 32u * j + r;
            const float v = acc[i][j][q] * 8.0f;
            const int32_t fix = static_cast<int32_t>(v);
            uint32_t got = static_cast<uint32_t>(fix);
            if (i == 0 && j == 0 && q == 0 && ((inj >> kGemm) & 1u) && t == 0 && lap == 0) got ^= 1u;
            if constexpr (kDump) dump[static_cast<size_t>(lap) * kTileWords + idx] = __float_as_uint(acc[i][j][q]);
            // (float)fix != v or got != want, without a lane mask per element: v + 0.0f takes -0 to +0 and
            // keeps a NaN a NaN, so the bits differ exactly when the values do.
            const uint32_t diff = (__float_as_uint(static_cast<float>(fix)) ^ __float_as_uint(v + 0.0f)) |
                                  (got ^ static_cast<uint32_t>(want[idx]));
            ne += (diff | (0u - diff)) >> 31;
            d += got * (2u * idx + 1u);
            acc[i][j][q] = 0.f;
          }
        }
      y[kGemm].bad += ne;
      y[kGemm].digest += d;
      if (ne) {
        extra[0] |= 1u << sub;
        extra[1] |= 1u << (set & 31u);
        extra[2] |= 1u << (32u * lap / laps);
      }
      sub = (sub + 1u) & 7u;
      step = 0;
      ++lap;
      set = set_of(g, lap < laps ? lap : 0u, laps, sets);
    } else {
      ++step;
    }
    stage = stage == kStages - 1 ? 0u : stage + 1u;
  }

  if constexpr (kDump) {
    uint32_t* folds = dump + static_cast<size_t>(laps) * kTileWords;
    folds[t] = y[kOperand].digest;
    folds[kBlock + t] = y[kScale].digest;
  }
  // A part that is not selected leaves no tally: its digest in the record is 0.
#pragma unroll
  for (int p = 0; p < kNumParts; ++p)
    if (!((a.part_mask >> p) & 1u)) y[p] = Tally{};
  if (!((a.part_mask >> kGemm) & 1u)) extra[0] = extra[1] = extra[2] = 0;
}

__global__ __launch_bounds__(kBlock) void k_mxload_sweep(MxRecord* __restrict__ records, MxArgs a, int inject_xcd,
                                                        int inject_cu, uint32_t inject_parts, Expect expect) {
  extern __shared__ __attribute__((aligned(16))) uint8_t mxload_lds[];
  const uint32_t xcd = xcc_id();
  const uint32_t hw = hw_id();
  const uint32_t cu = cu_key(hw);
  const uint32_t simd = simd_id(hw);
  const bool inject = inject_selected(inject_xcd, inject_cu, xcd, cu);

  Tally y[kNumParts];
  uint32_t extra[kExtra] = {};
  run_mxload<false>(a, blockIdx.x, inject ? inject_parts & a.part_mask : 0u, nullptr, mxload_lds, y, extra);

  reduce_parts<kNumParts, kExtra, kBlock>(reinterpret_cast<uint32_t*>(mxload_lds), threadIdx.x, simd, y, extra,
                                          a.part_mask, expect, xcd, cu, &records[blockIdx.x]);
}

// One workgroup; dump holds laps x 32,768 words of C and 2 x 512 folds.
__global__ __launch_bounds__(kBlock) void k_mxload_probe(uint32_t* __restrict__ dump, MxArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t mxload_lds[];
  Tally y[kNumParts];
  uint32_t extra[kExtra] = {};
  run_mxload<true>(a, 0u, 0u, dump, mxload_lds, y, extra);
}

// --------------------------------------------------------------------- host
bool bad_shape(uint32_t laps, uint32_t ksteps, uint32_t sets) {
  return laps < 1 || laps > kMaxLaps || ksteps < 1 || ksteps > kMaxKsteps || sets < 1 || sets > kMaxSets;
}

// One set in the logical order: the panels' dwords (128 and 256 rows of 16
// ksteps) and the scale words (rows of ksteps).
void fill_set(uint32_t seed, uint32_t set, uint32_t ksteps, uint32_t* a_words, uint32_t* bt_words, uint32_t* a_scales,
              uint32_t* bt_scales) {
  const uint32_t row_dwords = 16u * ksteps;
  for (uint32_t w = 0; w < kRowsA * row_dwords; ++w) a_words[w] = operand_word(seed, set, 0, w);
  for (uint32_t w = 0; w < kRowsB * row_dwords; ++w) bt_words[w] = operand_word(seed, set, 1, w);
  for (uint32_t w = 0; w < kRowsA * ksteps; ++w) a_scales[w] = scale_word(seed, set, 0, w);
  for (uint32_t w = 0; w < kRowsB * ksteps; ++w) bt_scales[w] = scale_word(seed, set, 1, w);
}

uint32_t fold_of(const uint32_t* words, size_t first, size_t n) {
  uint32_t f = 0;
  for (size_t i = 0; i < n; ++i) f += rotl(words[i], static_cast<uint32_t>((first + i) & 31u));
  return f;
}

// Element x scale of every element of a panel as an integer: units of 2^-2
// for A (scale code less 126), of 2^-1 for Bt (less 127). Returns the largest
// magnitude.
int decode_panel(const uint32_t* words, const uint32_t* scales, uint32_t rows, uint32_t ksteps, int scale_lo,
                 std::vector<int16_t>* out) {
  static const int kTwice[8] = {0, 1, 2, 3, 4, 6, 8, 12};  // 2 |e2m1|
  const size_t K = 128u * static_cast<size_t>(ksteps);
  const uint8_t* bytes = reinterpret_cast<const uint8_t*>(words);
  const uint8_t* sc = reinterpret_cast<const uint8_t*>(scales);
  out->resize(rows * K);
  int top = 0;
  for (size_t row = 0; row < rows; ++row)
    for (size_t k = 0; k < K; ++k) {
      const uint32_t code = (bytes[(row * K + k) / 2] >> (4 * (k & 1))) & 15u;
      const int m = kTwice[code & 7u] << (sc[row * (K / 32) + k / 32] - scale_lo);
      (*out)[row * K + k] = static_cast<int16_t>(code & 8u ? -m : m);
      top = m > top ? m : top;
    }
  return top;
}

// What the host holds of a (seed, ksteps, sets): the arena's bytes, the table
// and, per set, the folds of its panels and scales and the digest of its product.
struct HostSets {
  std::vector<uint32_t> arena;  // sets x ksteps x 26,112 bytes
  std::vector<int32_t> table;   // sets x 128 x 256 of fix = 8 C
  std::vector<uint32_t> fold_a, fold_bt, fold_sa, fold_sbt, gemm;
  bool bound_ok = true;
};

struct DeviceSets {
  DevMem arena, table;
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
  const size_t row_dwords = 16u * static_cast<size_t>(ksteps), K = 8 * row_dwords;
  const size_t a_dwords = kRowsA * row_dwords, bt_dwords = kRowsB * row_dwords;
  const size_t set_dwords = static_cast<size_t>(ksteps) * kStageBytes / 4;
  hs.arena.resize(sets * set_dwords);
  hs.table.resize(static_cast<size_t>(sets) * kTileWords);
  std::vector<uint32_t> aw(a_dwords), bw(bt_dwords), as(kRowsA * ksteps), bs(kRowsB * ksteps);
  std::vector<int16_t> A, Bt;
  for (uint32_t s = 0; s < sets; ++s) {
    fill_set(seed, s, ksteps, aw.data(), bw.data(), as.data(), bs.data());
    hs.fold_a.push_back(fold_of(aw.data(), 0, a_dwords));
    hs.fold_bt.push_back(fold_of(bw.data(), a_dwords, bt_dwords));
    hs.fold_sa.push_back(fold_of(as.data(), 0, as.size()));
    hs.fold_sbt.push_back(fold_of(bs.data(), as.size(), bs.size()));
    // The arena's order: per step the 16 dwords of every row, then the scale words.
    for (uint32_t step = 0; step < ksteps; ++step) {
      uint32_t* blk = hs.arena.data() + s * set_dwords + static_cast<size_t>(step) * (kStageBytes / 4);
      for (uint32_t row = 0; row < kRows; ++row) {
        const uint32_t* src = row < kRowsA ? &aw[row * row_dwords] : &bw[(row - kRowsA) * row_dwords];
        for (uint32_t q = 0; q < 16; ++q) blk[row * 16 + q] = src[step * 16 + q];
        blk[kScaleOff / 4 + row] = row < kRowsA ? as[row * ksteps + step] : bs[(row - kRowsA) * ksteps + step];
      }
    }
    // The bound of the header, on what was generated.
    const int top_a = decode_panel(aw.data(), as.data(), kRowsA, ksteps, 126, &A);
    const int top_b = decode_panel(bw.data(), bs.data(), kRowsB, ksteps, 127, &Bt);
    if (top_a > kMaxA || top_b > kMaxB || K * kMaxA * kMaxB >= (1u << 24)) hs.bound_ok = false;
    int32_t* C = hs.table.data() + static_cast<size_t>(s) * kTileWords;
    uint32_t d = 0;
    for (uint32_t i = 0; i < kRowsA; ++i)
      for (uint32_t j = 0; j < kRowsB; ++j) {
        int32_t sum = 0;
        for (size_t k = 0; k < K; ++k) sum += static_cast<int32_t>(A[i * K + k]) * static_cast<int32_t>(Bt[j * K + k]);
        C[i * kRowsB + j] = sum;
        d += static_cast<uint32_t>(sum) * (2u * (i * kRowsB + j) + 1u);
      }
    hs.gemm.push_back(d);
  }
  return hs;
}

// The digests of a healthy workgroup; 0 for a part outside the mask.
int expected_digests(uint32_t mask, uint32_t seed, uint32_t laps, uint32_t ksteps, uint32_t sets, uint32_t* out) {
  std::lock_guard<std::mutex> g(g_sets_mu);
  const HostSets& hs = host_sets(seed, ksteps, sets);
  if (!hs.bound_ok) {
    std::snprintf(g_mxload_err, sizeof g_mxload_err, "an operand left the bound that keeps every sum exact");
    return kBoundBroken;
  }
  uint32_t d[kNumParts] = {};
  for (uint32_t l = 0; l < laps; ++l) {
    const uint32_t s = set_of(0, l, laps, sets);
    d[kOperand] += 4u * hs.fold_a[s] + 2u * hs.fold_bt[s];
    d[kScale] += 8u * hs.fold_sa[s] + 4u * hs.fold_sbt[s];
    d[kGemm] += hs.gemm[s];
  }
  for (int p = 0; p < kNumParts; ++p) out[p] = (mask >> p) & 1u ? d[p] : 0u;
  return 0;
}

// Arena and table of (seed, ksteps, sets) on the current device `dev`, built
// and uploaded once. -1003 when either cannot be allocated: nothing is launched.
int device_sets(int dev, uint32_t seed, uint32_t ksteps, uint32_t sets, MxArgs* a) {
  std::lock_guard<std::mutex> g(g_sets_mu);
  auto& slot = g_device_sets[{dev, seed, ksteps, sets}];
  if (!slot) {
    const HostSets& hs = host_sets(seed, ksteps, sets);
    if (!hs.bound_ok) return kBoundBroken;
    auto ds = std::make_unique<DeviceSets>();
    const size_t arena_bytes = hs.arena.size() * 4, table_bytes = hs.table.size() * 4;
    void *arena = nullptr, *table = nullptr;
    const bool got = hipMalloc(&arena, arena_bytes) == hipSuccess && hipMalloc(&table, table_bytes) == hipSuccess;
    ds->arena.p = arena, ds->table.p = got ? table : nullptr;  // what was had is freed with ds
    if (!got) {
      (void)hipGetLastError();
      std::snprintf(g_mxload_err, sizeof g_mxload_err,
                    "no arena of %zu and table of %zu bytes could be had: nothing was swept", arena_bytes, table_bytes);
      return kUnswept;
    }
    XS_CHECK(hipMemcpy(ds->arena.p, hs.arena.data(), arena_bytes, hipMemcpyHostToDevice));
    XS_CHECK(hipMemcpy(ds->table.p, hs.table.data(), table_bytes, hipMemcpyHostToDevice));
    slot = std::move(ds);
  }
  a->arena = slot->arena.as<const uint8_t>();
  a->table = slot->table.as<const int32_t>();
  return 0;
}

}  // namespace

extern "C" {

const char* xs_mxload_sweep_last_error() { return g_mxload_err; }

// Part names, comma-separated, in bit order.
const char* xs_mxload_parts() { return kPartNames; }

// out2 = {words whatever the laps, words per lap} of a part in the probe's
// dump: gemm has 32,768 per lap, the folds one per thread.
int xs_mxload_shape(int part, int* out2) {
  if (part < 0 || part >= kNumParts || !out2) return kBadArgs;
  out2[0] = part == kGemm ? 0 : kBlock;
  out2[1] = part == kGemm ? static_cast<int>(kTileWords) : 0;
  return 0;
}

// Host only. One set in the logical order, whatever the arena's: the packed
// elements a_out[128][64 ksteps] and bt_out[256][64 ksteps] (two per byte, low
// nibble first) and the E8M0 bytes a_scales[128][4 ksteps] and
// bt_scales[256][4 ksteps], one per 32 elements of k.
int xs_mxload_operands(uint32_t seed, uint32_t set, uint32_t ksteps, void* a_out, void* bt_out, void* a_scales,
                       void* bt_scales) {
  if (set >= kMaxSets || ksteps < 1 || ksteps > kMaxKsteps || !a_out || !bt_out || !a_scales || !bt_scales)
    return kBadArgs;
  fill_set(seed, set, ksteps, static_cast<uint32_t*>(a_out), static_cast<uint32_t*>(bt_out),
           static_cast<uint32_t*>(a_scales), static_cast<uint32_t*>(bt_scales));
  return 0;
}

// One workgroup at any shape; out = [laps][128][256] raw f32 bits of C, then
// [2][512]: every thread's operand fold and scale fold.
// n_words = laps x 32,768 + 1,024. The mask selects which folds are issued.
int xs_mxload_probe(int dev, uint32_t part_mask, uint32_t seed, uint32_t laps, uint32_t ksteps, uint32_t sets,
                    uint32_t* out, size_t n_words) {
  if (bad_part_mask(part_mask, kAllParts) || bad_shape(laps, ksteps, sets) || !out) return kBadArgs;
  const size_t n = static_cast<size_t>(laps) * kTileWords + kFoldWords;
  if (n_words != n) return kBadArgs;
  MxArgs a{nullptr, nullptr, part_mask, seed, laps, ksteps, sets};
  return launch_probe(
      g_mxload_err, dev, reinterpret_cast<const void*>(k_mxload_probe), kBlock, kLdsUsed, out, n,
      [&](dim3 grid, dim3 block, size_t smem, void* dump) {
        hipLaunchKernelGGL(k_mxload_probe, grid, block, smem, 0, static_cast<uint32_t*>(dump), a);
      },
      [&] { return device_sets(dev, seed, ksteps, sets, &a); });
}

// Host only. out3[p] = the workgroup digest a healthy CU leaves for part p at
// the sweep's shape, 0 for a part outside part_mask.
int xs_mxload_sweep_expected(uint32_t part_mask, uint32_t seed, uint32_t laps, uint32_t* out3) {
  if (bad_part_mask(part_mask, kAllParts) || bad_shape(laps, kMxKsteps, kMxSets) || !out3) return kBadArgs;
  return expected_digests(part_mask, seed, laps, kMxKsteps, kMxSets, out3);
}

// What the runtime reports for k_mxload_sweep on `dev`: out4 = {registers per
// lane, scratch bytes per lane, dynamic LDS bytes per workgroup, workgroups
// that fit on a CU at once}.
int xs_mxload_sweep_info(int dev, int* out4) {
  return sweep_info(g_mxload_err, dev, reinterpret_cast<const void*>(k_mxload_sweep), kBlock, true, out4);
}

// One sweep launch of `blocks` workgroups (0: 4 per CU) of `laps` laps at the
// sweep's shape. Writes `blocks` 128-byte records to records_out. inject_xcd /
// inject_cu: -1 is none / any, values below -1 are refused. Returns 0, -1000
// for bad arguments and -1003 when arena or table could not be allocated
// (nothing is launched either way), or a negative HIP error.
int xs_mxload_sweep(int dev, int blocks, uint32_t part_mask, uint32_t seed, uint32_t laps, int inject_xcd,
                    int inject_cu, uint32_t inject_parts, void* records_out, int* n_records, double* ms) {
  if (bad_part_mask(part_mask, kAllParts) || bad_shape(laps, kMxKsteps, kMxSets) || (inject_parts & ~kAllParts))
    return kBadArgs;
  // launch_sweep refuses these too, but only after the host has built the sets.
  if (!records_out || blocks < 0 || blocks > kMaxBlocks || inject_xcd < -1 || inject_cu < -1 || inject_xcd > 15 ||
      inject_cu > 0xff)
    return kBadArgs;
  Expect e;
  if (int rc = expected_digests(part_mask, seed, laps, kMxKsteps, kMxSets, e.digest)) return rc;
  MxArgs a{nullptr, nullptr, part_mask, seed, laps, kMxKsteps, kMxSets};
  return launch_sweep(
      g_mxload_err, {dev, blocks, inject_xcd, inject_cu, records_out, n_records, ms},
      reinterpret_cast<const void*>(k_mxload_sweep), kBlock, kLdsUsed, sizeof(MxRecord),
      [&](dim3 grid, dim3 block, size_t smem, void* rec) {
        hipLaunchKernelGGL(k_mxload_sweep, grid, block, smem, 0, static_cast<MxRecord*>(rec), a, inject_xcd, inject_cu,
                           inject_parts, e);
      },
      [&] { return device_sets(dev, seed, kMxKsteps, kMxSets, &a); });
}

}  // extern "C"
