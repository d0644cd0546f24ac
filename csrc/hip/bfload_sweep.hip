// bf16 load sweep for gfx950 (MI355X): every CU under load, with a checked bf16
// GEMM in the NN layout.
//
// load_sweep.hip holds every CU at rate on v_mfma_i32_32x32x32_i8 and
// mxload_sweep.hip on the block-scaled FP4 MFMA; both store B transposed. The
// format dense training keeps the part busy with is bf16, and its data path is
// otherwise checked cold only: one v_mfma_f32_32x32x16_bf16 on small integers
// in the CU sweep and the health probe. A bf16 GEMM whose B is stored the
// natural way ([K][N], n contiguous) also gets its B operand through
// ds_read_b64_tr_b16, which the lane sweep's `ldstr` path proves cold, on 32
// reads. k_bfload_sweep is a sweep over named parts (part_sweep.h) whose load
// is that GEMM: operands come from memory through L2/L1 into registers, go
// through LDS and, for B, through the transposed LDS read into
// v_mfma_f32_32x32x16_bf16, two waves on every SIMD, many laps in one launch,
// and every result of every lap is compared on the device by equality.
//
// What makes equality possible. An element is x = (h16 & 0x807F) | 0x3F80:
// sign and all seven mantissa bits from the hash, the biased exponent fixed at
// 127, so its value is +-(128 + m) 2^-7, m in 0..127. Every product is a
// multiple of 2^-14 of at most 255^2 = 65,025 units, and any partial sum in
// any order is an exact float while K 65,025 < 2^24: K <= 258. ksteps <= 8
// (K = 256: 16,646,400 < 16,777,216) is the cap. The implicit leading one alone
// costs 2^14 units per product, so a hashed exponent bit would halve K; the
// exponent stays fixed (NOT covered, below). The host re-checks the maximum of
// sum |a||b| on what it generated and refuses (-1001) a set that left the bound.
//
// Operands. A set s is A_s[128][K] and B_s[K][256] of bf16, K = 32 ksteps; A is
// row-major with k contiguous, B row-major with n contiguous (not transposed).
// Dword w of panel p (0: A, 1: B) of set s is
//     fmix32(seed ^ (s << 23 | p << 22 | w))
// with each 16-bit half masked as above, low half first. The panels have 2,048
// ksteps and 4,096 ksteps dwords; B follows A in the arena, so a set is 24,576
// ksteps bytes and its dword i is dword i of A, then of B. The host keeps
// fix = C 2^14 in plain int32 (no float is rounded anywhere on the host) as a
// table of 128 KiB per set. Arena and table are cached per (seed, ksteps, sets)
// and per device for the life of the process; the kernels write neither.
//
// Work split (the load sweep's). A workgroup is 512 threads: 8 waves, two on
// every SIMD, exclusive_lds(), so no two share a CU. Per lap it computes one
// C[128 x 256]; a wave owns a 64 x 64 sub-tile in four 32 x 32 float
// accumulators; sub-tile u covers rows 64 (u >> 2) and columns 64 (u & 3). In
// lap l wave w computes sub-tile (w + l) & 7 and workgroup g reads set
// set_of(g, l, laps, sets) (part_sweep.h).
//
// Pipeline. One K-step is 32 of k: 64 bytes of each of A's 128 rows and 32
// whole rows of B, which are one contiguous block of 16 KiB. That is 1,536
// chunks of 16 bytes, three global_load_dwordx4 per thread: thread t takes
// chunk t & 3 of A's row t >> 2 and chunks t and t + 512 of B's block (row
// chunk >> 5, columns 8 (chunk & 31)..+7). They land in registers and go from
// there into one of two LDS stages. The loads of step k + 1 are in flight while
// the 8 MFMAs of step k (2 k-halves x 4 accumulators) issue from the other
// stage; there is one barrier per step and the global step index runs across
// laps: a stage is written only after the barrier that follows its last read.
// LDS rows are padded: A's pitch is 80 bytes (64 + 16), as in the load sweep;
// B's is 576 (512 + 64). A stage is 128 x 80 + 32 x 576 = 28,672 bytes, two are
// 57,344. The bank model is that of the public CDNA3 material, 64 banks of 4
// bytes, assumed for CDNA4; no counter was read. Under it A's 128-bit reads
// conflict as little as the load sweep's (80 / 16 is odd), and in one
// transposed read a 16-lane group touches four rows of B at 32 consecutive
// bytes each; 576 bytes are 144 banks, 16 mod 64, so the four rows start 16
// banks apart and their 8 banks each do not meet.
//
// Operand reads, for the k-half kh of a step and lane (r = lane & 31,
// h = lane >> 5), as v_mfma_f32_32x32x16_bf16 wants them (matrix_sweep.hip's
// header: A[r][8h..8h+7], B[8h..8h+7][r], C[(q & 3) + 8 (q >> 2) + 4h][r]):
//   A  one 128-bit read gives A[row + r][16 kh + 8 h .. +7].
//   B  two ds_read_b64_tr_b16 per operand, by the lane sweep's map: in a group
//      of 16 lanes, lane 4q + p supplies the address of row q, columns
//      4p..4p+3, and lane i receives column i of the four rows (rows 0, 1 in
//      word 0). Here a row is a k and a column an n: group (lane >> 4) & 1
//      takes columns 16 group, the first read takes k = 16 kh + 8 h + 0..3, the
//      second + 4..7. Together they give the lane B[k..k+7][col + r].
// What the hardware settled: see the end of this header.
//
// Lap epilogue. After the last step of a lap every lane takes its 64
// accumulators through fix = (int)(acc 16384), counts a mismatch when that
// loses anything (a NaN too) or differs from the table, and clears them.
//
// Parts (bit, name). The mask selects what is judged; the pipeline always
// runs, it is the load. The folds of a part that is not selected are not issued.
//   0 stage      every dword a thread received from the arena, before it goes
//                to LDS: sum of rotl32(word, i & 31), i its dword index in the
//                set. The fold commutes and is keyed by i.
//   1 operand    every A dword a wave reads back from LDS, same fold. An A
//                dword is read by four waves: 4 sum(A) per lap.
//   2 transpose  every B dword a lane receives from a transposed read: the word
//                is B[2j][n] | B[2j+1][n] << 16 and its index 256 j + n, same
//                fold. It is read by two waves: 2 sum(B') per lap; the host
//                folds the logical matrix the same way.
//   3 gemm       mismatches against the table are counted; the digest is the
//                sum of uint32(fix) (2 (256 row + col) + 1) over the laps.
// A bad gemm with good operand and transpose names the bf16 path of the matrix
// core; a bad transpose with a good stage names the LDS transpose path under load.
//
// Record (128 bytes per workgroup), injection and safety rules are the load
// sweep's: part_sweep.h's head with four parts, the reserved word and the
// sub-tile, set and span masks; an injected part flips bit 0 of its word 0 in
// registers (stage, operand, transpose: the first dword thread 0 folds, in the
// fold only; gemm: fix of C[0][0] of lap 0). Trip counts come from the kernel
// arguments only; no loop waits on a clock, a flag or another workgroup. No
// scratch, no spill, MODE is not written, results leave through vector stores.
// Every index into the arena is below 24,576 ksteps sets and every index into
// the table below 32,768 sets by construction.
//
// k_bfload_probe is the same device function with a dump: one workgroup at any
// shape stores C of every lap as [lap][128][256] float32 and behind it each
// thread's stage, operand and transpose folds ([3][512]).
//
// What the hardware settled: on the first run on an MI355X the probe equalled
// the numpy reference (tests/bfload_sweep_ref.py) at every shape and seed, C
// and all three folds; the B map above stands as written.
//
// NOT covered: f16, fp8/bf8 and sparse forms under load; varied exponents (the
// accumulator's aligner sees growing sums, but operands of one binade); HBM
// traffic (which cache level served a load is the hardware's choice); more than
// one launch; the 16x16x32 shape; LDS bank conflicts, power, clocks and
// temperature, which are not observed.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <map>
#include <memory>
#include <mutex>
#include <tuple>
#include <vector>

#include "hip/part_sweep.h"

#define XS_ERR_BUF g_bfload_err
#define XS_HD __host__ __device__ __forceinline__
#define XS_D __device__ __forceinline__

namespace {

using namespace xsprobe;

ErrBuf g_bfload_err = "";

typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef short i16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __attribute__((address_space(3))) i16x4* LdsTrPtr;

constexpr int kNumParts = 4;
const char kPartNames[] = "stage,operand,transpose,gemm";
constexpr uint32_t kAllParts = (1u << kNumParts) - 1;
constexpr int kStage = 0, kOperand = 1, kTranspose = 2, kGemm = 3;
constexpr int kBlock = 512;  // 8 waves: two per SIMD
constexpr int kExtra = 3;    // sub-tile, set and span masks
constexpr int kUnswept = -1003;
constexpr int kBoundBroken = -1001;  // the generator left its stated bound (a bug in this file)

// The sweep's fixed shape and defaults: measured in profiles/bfload_sweep_defaults.md.
constexpr uint32_t kBfKsteps = 8, kBfSets = 32;
constexpr uint32_t kBfLaps = 2048;
constexpr uint32_t kMaxLaps = 16 * kBfLaps, kMaxKsteps = 8, kMaxSets = 64;

constexpr uint32_t kRowsA = 128, kColsB = 256;
constexpr uint32_t kStepK = 32;                                  // of k, per K-step
constexpr uint32_t kStepBytesA = 2 * kStepK;                     // 64 of every row of A
constexpr uint32_t kStepBytesB = kStepK * kColsB * 2;            // 16,384: 32 whole rows of B
constexpr uint32_t kPanelBytesA = kRowsA * kStepBytesA;          // per K-step: 8,192
constexpr uint32_t kSetBytes = kPanelBytesA + kStepBytesB;       // per K-step: 24,576
constexpr uint32_t kPitchA = 80;                                 // LDS row of A: 64 + 16 bytes
constexpr uint32_t kPitchB = 576;                                // LDS row of B: 512 + 64 bytes
constexpr uint32_t kStageA = kRowsA * kPitchA;                   // 10,240: where a stage's B rows begin
constexpr uint32_t kStageBytes = kStageA + kStepK * kPitchB;     // 28,672
constexpr uint32_t kTileWords = kRowsA * kColsB;                 // C of one set: 128 KiB
constexpr uint32_t kFoldWords = 3 * kBlock;                      // the probe's per-thread folds
constexpr uint32_t kRedBytes = part_reduction_words<kBlock>(kNumParts, kExtra) * 4;
constexpr uint32_t kLdsUsed = 2 * kStageBytes > kRedBytes ? 2 * kStageBytes : kRedBytes;
constexpr int kMaxElem = 255;        // |element| in units of 2^-7
constexpr float kFixScale = 16384.f;  // C in units of 2^-14
static_assert(kStepK * kMaxKsteps * kMaxElem * kMaxElem < (1u << 24), "every partial sum is one exact float");
static_assert(2 * kStageBytes == 57344 && kStageA % 8 == 0 && kPitchB % 8 == 0, "two stages; 64-bit transposed reads");

// Two bf16 of one binade: sign and mantissa from the hash, the biased exponent 127.
XS_HD uint32_t operand_word(uint32_t seed, uint32_t set, uint32_t panel, uint32_t w) {
  return (fmix32(seed ^ (set << 23 | panel << 22 | w)) & 0x807f807fu) | 0x3f803f80u;
}

struct BfRecord {
  PartRecordHead<kNumParts> head;
  uint32_t reserved;
  uint32_t subtiles, sets, spans;
  uint32_t pad[15];
};
static_assert(sizeof(BfRecord) == 128, "one 128-byte record per workgroup");

using Expect = PartExpect<kNumParts>;

struct BfArgs {
  const uint8_t* arena;
  const int32_t* table;
  uint32_t part_mask, seed, laps, ksteps, sets;
};

// ------------------------------------------------------------------- device
XS_D uint32_t fold4(u32x4 v, uint32_t s) {
  return rotl(v.x, s) + rotl(v.y, s + 1u) + rotl(v.z, s + 2u) + rotl(v.w, s + 3u);
}

// ds_read_b64_tr_b16: the lane's two words of the 4 x 16 block its group addresses.
XS_D u32x2 read_tr16(const uint8_t* p) {
  return __builtin_bit_cast(u32x2, __builtin_amdgcn_ds_read_tr16_b64_v4i16((LdsTrPtr)p));
}

// One workgroup's whole run. g: its rotation of the sets; inj: the parts to
// inject; dump: kDump only. Leaves the tallies and the three masks.
template <bool kDump>
XS_D void run_bfload(const BfArgs& a, uint32_t g, uint32_t inj, float* dump, uint8_t* lds, Tally (&y)[kNumParts],
                     uint32_t (&extra)[kExtra]) {
  const uint32_t t = threadIdx.x, lane = t & 63u, r = lane & 31u, h = lane >> 5;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const uint32_t ksteps = a.ksteps, laps = a.laps, sets = a.sets;
  const bool stage_on = (a.part_mask >> kStage) & 1u, operand_on = (a.part_mask >> kOperand) & 1u;
  const bool transpose_on = (a.part_mask >> kTranspose) & 1u;

  // Staging: chunk cc of the step's four of A's row row0, chunks t and t + 512 of B's block.
  const uint32_t row0 = t >> 2, cc = t & 3u;
  const uint32_t ga_off = row0 * kStepBytesA * ksteps + cc * 16u;                 // in a set, at step 0
  const uint32_t gb_off = kPanelBytesA * ksteps + t * 16u;                         // likewise
  const uint32_t la_off = row0 * kPitchA + cc * 16u;                               // in a stage
  const uint32_t lb_off = kStageA + (t >> 5) * kPitchB + (t & 31u) * 16u;          // chunk t + 512: 16 rows on
  u32x4 stg[3];
  auto issue = [&](uint32_t set, uint32_t step) {
    const uint8_t* p = a.arena + static_cast<size_t>(set) * (kSetBytes * ksteps);
    stg[0] = *reinterpret_cast<const u32x4*>(p + ga_off + step * kStepBytesA);
#pragma unroll
    for (uint32_t j = 0; j < 2; ++j)
      stg[1 + j] = *reinterpret_cast<const u32x4*>(p + gb_off + step * kStepBytesB + j * (kStepBytesB / 2));
  };
  // Folds what `issue` brought for `step` and hands it to a stage. A's panel and
  // a step's block of B are multiples of 32 dwords, so B's indices have the low
  // bits of 4 chunk.
  auto fold_store = [&](uint32_t stage, uint32_t step, uint32_t flip) {
    if (stage_on) {
      const uint32_t sa = 16u * ((row0 * ksteps + step) & 1u) + 4u * cc, sb = 4u * (t & 7u);
      y[kStage].digest += rotl(stg[0].x ^ flip, sa) - rotl(stg[0].x, sa) + fold4(stg[0], sa) + fold4(stg[1], sb) +
                          fold4(stg[2], sb);
      y[kStage].bad += flip;
    }
    uint8_t* st = lds + stage * kStageBytes;
    *reinterpret_cast<u32x4*>(st + la_off) = stg[0];
#pragma unroll
    for (uint32_t j = 0; j < 2; ++j) *reinterpret_cast<u32x4*>(st + lb_off + j * (16u * kPitchB)) = stg[1 + j];
  };

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int q = 0; q < 16; ++q) acc[i][j][q] = 0.f;

  uint32_t operand_flip = ((inj >> kOperand) & 1u) && t == 0;
  uint32_t transpose_flip = ((inj >> kTranspose) & 1u) && t == 0;
  uint32_t lap = 0, step = 0, set = set_of(g, 0, laps, sets);
  uint32_t sub = wave & 7u;  // (wave + lap) & 7
  const uint32_t total = laps * ksteps;
  // The transposed read: lane 4q + p of its group addresses k = 8 h + q, columns 16 group + 4 p.
  const uint32_t tr_off =
      kStageA + (8u * h + ((lane & 15u) >> 2)) * kPitchB + 2u * (16u * ((lane >> 4) & 1u) + 4u * (lane & 3u));

  issue(set, 0);
  fold_store(0, 0, ((inj >> kStage) & 1u) && t == 0);
  __syncthreads();

#pragma nounroll
  for (uint32_t gi = 0; gi < total; ++gi) {
    uint32_t nstep = step + 1u, nlap = lap, nset = set;
    if (nstep == ksteps) {
      nstep = 0;
      nlap = lap + 1u;
      nset = set_of(g, nlap < laps ? nlap : 0u, laps, sets);
    }
    const bool more = gi + 1u < total;
    if (more) issue(nset, nstep);

    const uint32_t sr = sub >> 2, sc = sub & 3u;
    const uint8_t* st = lds + (gi & 1u) * kStageBytes;
    const uint8_t* a_rd = st + (64u * sr + r) * kPitchA + 16u * h;
    const uint8_t* b_rd = st + tr_off + 2u * (64u * sc);
    // Rows 32 apart leave (row ksteps + step) & 1 that of r: 16 dwords per row and step.
    const uint32_t s0 = 16u * ((r * ksteps + step) & 1u) + 4u * h;
#pragma unroll
    for (int kh = 0; kh < 2; ++kh) {
      u32x4 av[2], bv[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        av[i] = *reinterpret_cast<const u32x4*>(a_rd + 32u * i * kPitchA + 32u * kh);
        const u32x2 lo = read_tr16(b_rd + (16u * kh) * kPitchB + 64u * i);
        const u32x2 hi = read_tr16(b_rd + (16u * kh + 4u) * kPitchB + 64u * i);
        bv[i] = u32x4{lo.x, lo.y, hi.x, hi.y};
      }
      if (operand_on) {
        uint32_t f = 0;
        if (kh == 0) {
          f = rotl(av[0].x ^ operand_flip, s0) - rotl(av[0].x, s0);
          y[kOperand].bad += operand_flip;
          operand_flip = 0;
        }
        y[kOperand].digest += f + fold4(av[0], s0 + 8u * kh) + fold4(av[1], s0 + 8u * kh);
      }
      if (transpose_on) {
        // Index 256 j + n of a word: its low five bits are those of n, which are r.
        uint32_t f = 0;
        if (kh == 0) {
          f = rotl(bv[0].x ^ transpose_flip, r) - rotl(bv[0].x, r);
          y[kTranspose].bad += transpose_flip;
          transpose_flip = 0;
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) f += rotl(bv[i].x, r) + rotl(bv[i].y, r) + rotl(bv[i].z, r) + rotl(bv[i].w, r);
        y[kTranspose].digest += f;
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, av[i]),
                                                              __builtin_bit_cast(bf16x8, bv[j]), acc[i][j], 0, 0, 0);
    }

    if (more) fold_store((gi + 1u) & 1u, nstep, 0u);
    __syncthreads();

    if (nstep == 0) {  // the lap is complete
      const int32_t* want = a.table + static_cast<size_t>(set) * kTileWords;
      uint32_t ne = 0, d = 0;
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
#pragma unroll
          for (int q = 0; q < 16; ++q) {
            const uint32_t row = 64u * sr + 32u * i + (q & 3) + 8u * (q >> 2) + 4u * h;
            const uint32_t idx = row * kColsB + 64u * sc + 32u * j + r;
            const float v = acc[i][j][q] * kFixScale;
            const int32_t fix = static_cast<int32_t>(v);
            uint32_t got = static_cast<uint32_t>(fix);
            if (i == 0 && j == 0 && q == 0 && ((inj >> kGemm) & 1u) && t == 0 && lap == 0) got ^= 1u;
            if constexpr (kDump) dump[static_cast<size_t>(lap) * kTileWords + idx] = acc[i][j][q];
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
    }
    step = nstep, lap = nlap, set = nset;
  }

  if constexpr (kDump) {
    uint32_t* folds = reinterpret_cast<uint32_t*>(dump + static_cast<size_t>(laps) * kTileWords);
    folds[t] = y[kStage].digest;
    folds[kBlock + t] = y[kOperand].digest;
    folds[2 * kBlock + t] = y[kTranspose].digest;
  }
  // A part that is not selected leaves no tally: its digest in the record is 0.
#pragma unroll
  for (int p = 0; p < kNumParts; ++p)
    if (!((a.part_mask >> p) & 1u)) y[p] = Tally{};
  if (!((a.part_mask >> kGemm) & 1u)) extra[0] = extra[1] = extra[2] = 0;
}

__global__ __launch_bounds__(kBlock) void k_bfload_sweep(BfRecord* __restrict__ records, BfArgs a, int inject_xcd,
                                                        int inject_cu, uint32_t inject_parts, Expect expect) {
  extern __shared__ __attribute__((aligned(16))) uint8_t bfload_lds[];
  const uint32_t xcd = xcc_id();
  const uint32_t hw = hw_id();
  const uint32_t cu = cu_key(hw);
  const uint32_t simd = simd_id(hw);
  const bool inject = inject_selected(inject_xcd, inject_cu, xcd, cu);

  Tally y[kNumParts];
  uint32_t extra[kExtra] = {};
  run_bfload<false>(a, blockIdx.x, inject ? inject_parts & a.part_mask : 0u, nullptr, bfload_lds, y, extra);

  reduce_parts<kNumParts, kExtra, kBlock>(reinterpret_cast<uint32_t*>(bfload_lds), threadIdx.x, simd, y, extra,
                                          a.part_mask, expect, xcd, cu, &records[blockIdx.x]);
}

// One workgroup; dump holds laps x 32,768 floats of C and 3 x 512 folds.
__global__ __launch_bounds__(kBlock) void k_bfload_probe(float* __restrict__ dump, BfArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t bfload_lds[];
  Tally y[kNumParts];
  uint32_t extra[kExtra] = {};
  run_bfload<true>(a, 0u, 0u, dump, bfload_lds, y, extra);
}

// --------------------------------------------------------------------- host
bool bad_shape(uint32_t laps, uint32_t ksteps, uint32_t sets) {
  return laps < 1 || laps > kMaxLaps || ksteps < 1 || ksteps > kMaxKsteps || sets < 1 || sets > kMaxSets;
}

// One set's dwords: 2,048 ksteps of A[128][K], then 4,096 ksteps of B[K][256].
void fill_set(uint32_t seed, uint32_t set, uint32_t ksteps, uint32_t* a_words, uint32_t* b_words) {
  for (uint32_t w = 0; w < kPanelBytesA / 4 * ksteps; ++w) a_words[w] = operand_word(seed, set, 0, w);
  for (uint32_t w = 0; w < kStepBytesB / 4 * ksteps; ++w) b_words[w] = operand_word(seed, set, 1, w);
}

uint32_t fold_of(const uint32_t* words, size_t first, size_t n) {
  uint32_t f = 0;
  for (size_t i = 0; i < n; ++i) f += rotl(words[i], static_cast<uint32_t>((first + i) & 31u));
  return f;
}

// A bf16 of the fixed binade in units of 2^-7: +-(128 + m).
int element_units(uint16_t x) {
  const int m = 128 + (x & 0x7f);
  return x & 0x8000 ? -m : m;
}

// What the host holds of a (seed, ksteps, sets): the arena's dwords, the table
// and, per set, the folds of its panels, of B as the transposed reads deliver
// it, and the digest of its product.
struct HostSets {
  std::vector<uint32_t> arena;  // sets x 6,144 ksteps dwords
  std::vector<int32_t> table;   // sets x 128 x 256 of fix = C 2^14
  std::vector<uint32_t> fold_a, fold_b, fold_tr, gemm;
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
  const size_t K = static_cast<size_t>(kStepK) * ksteps;
  const size_t a_dwords = kPanelBytesA / 4 * static_cast<size_t>(ksteps);
  const size_t b_dwords = kStepBytesB / 4 * static_cast<size_t>(ksteps);
  const size_t set_dwords = a_dwords + b_dwords;
  hs.arena.resize(sets * set_dwords);
  hs.table.resize(static_cast<size_t>(sets) * kTileWords);
  std::vector<int16_t> A(kRowsA * K), B(K * kColsB);
  std::vector<int32_t> mag(kColsB);
  for (uint32_t s = 0; s < sets; ++s) {
    uint32_t* aw = hs.arena.data() + s * set_dwords;
    uint32_t* bw = aw + a_dwords;
    fill_set(seed, s, ksteps, aw, bw);
    hs.fold_a.push_back(fold_of(aw, 0, a_dwords));
    hs.fold_b.push_back(fold_of(bw, a_dwords, b_dwords));
    const uint16_t* a16 = reinterpret_cast<const uint16_t*>(aw);
    const uint16_t* b16 = reinterpret_cast<const uint16_t*>(bw);
    // B as a transposed read delivers it: word (j, n) = B[2j][n] | B[2j+1][n] << 16, index 256 j + n.
    uint32_t ftr = 0;
    for (size_t j = 0; j < K / 2; ++j)
      for (uint32_t n = 0; n < kColsB; ++n)
        ftr += rotl(b16[2 * j * kColsB + n] | static_cast<uint32_t>(b16[(2 * j + 1) * kColsB + n]) << 16, n & 31u);
    hs.fold_tr.push_back(ftr);
    for (size_t i = 0; i < A.size(); ++i) A[i] = static_cast<int16_t>(element_units(a16[i]));
    for (size_t i = 0; i < B.size(); ++i) B[i] = static_cast<int16_t>(element_units(b16[i]));
    // fix = C 2^14 in plain int32, and the bound of the header on what was generated.
    int32_t* C = hs.table.data() + static_cast<size_t>(s) * kTileWords;
    uint32_t d = 0;
    for (uint32_t i = 0; i < kRowsA; ++i) {
      int32_t* row = C + i * kColsB;
      for (uint32_t j = 0; j < kColsB; ++j) row[j] = mag[j] = 0;
      for (size_t k = 0; k < K; ++k) {
        const int32_t x = A[i * K + k], ax = x < 0 ? -x : x;
        const int16_t* b = &B[k * kColsB];
        for (uint32_t j = 0; j < kColsB; ++j) {
          row[j] += x * b[j];
          mag[j] += ax * (b[j] < 0 ? -b[j] : b[j]);
        }
      }
      for (uint32_t j = 0; j < kColsB; ++j) {
        if (mag[j] >= (1 << 24)) hs.bound_ok = false;
        d += static_cast<uint32_t>(row[j]) * (2u * (i * kColsB + j) + 1u);
      }
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
    std::snprintf(g_bfload_err, sizeof g_bfload_err, "an operand set left the bound that keeps every sum exact");
    return kBoundBroken;
  }
  uint32_t d[kNumParts] = {};
  for (uint32_t l = 0; l < laps; ++l) {
    const uint32_t s = set_of(0, l, laps, sets);
    d[kStage] += hs.fold_a[s] + hs.fold_b[s];
    d[kOperand] += 4u * hs.fold_a[s];
    d[kTranspose] += 2u * hs.fold_tr[s];
    d[kGemm] += hs.gemm[s];
  }
  for (int p = 0; p < kNumParts; ++p) out[p] = (mask >> p) & 1u ? d[p] : 0u;
  return 0;
}

// Arena and table of (seed, ksteps, sets) on the current device `dev`, built
// and uploaded once. -1003 when either cannot be allocated: nothing is launched.
int device_sets(int dev, uint32_t seed, uint32_t ksteps, uint32_t sets, BfArgs* a) {
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
      std::snprintf(g_bfload_err, sizeof g_bfload_err,
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

const char* xs_bfload_sweep_last_error() { return g_bfload_err; }

// Part names, comma-separated, in bit order.
const char* xs_bfload_parts() { return kPartNames; }

// out2 = {words whatever the laps, words per lap} of a part in the probe's
// dump: gemm has 32,768 per lap, the folds one per thread.
int xs_bfload_shape(int part, int* out2) {
  if (part < 0 || part >= kNumParts || !out2) return kBadArgs;
  out2[0] = part == kGemm ? 0 : kBlock;
  out2[1] = part == kGemm ? static_cast<int>(kTileWords) : 0;
  return 0;
}

// Host only. The bf16 bits the arena holds for `set`: a_out[128][32 ksteps],
// b_out[32 ksteps][256].
int xs_bfload_operands(uint32_t seed, uint32_t set, uint32_t ksteps, void* a_out, void* b_out) {
  if (set >= kMaxSets || ksteps < 1 || ksteps > kMaxKsteps || !a_out || !b_out) return kBadArgs;
  fill_set(seed, set, ksteps, static_cast<uint32_t*>(a_out), static_cast<uint32_t*>(b_out));
  return 0;
}

// One workgroup at any shape; out = [laps][128][256] float32 of C, then
// [3][512]: every thread's stage, operand and transpose fold.
// n_words = laps x 32,768 + 1,536. The mask selects which folds are issued.
int xs_bfload_probe(int dev, uint32_t part_mask, uint32_t seed, uint32_t laps, uint32_t ksteps, uint32_t sets,
                    uint32_t* out, size_t n_words) {
  if (bad_part_mask(part_mask, kAllParts) || bad_shape(laps, ksteps, sets) || !out) return kBadArgs;
  const size_t n = static_cast<size_t>(laps) * kTileWords + kFoldWords;
  if (n_words != n) return kBadArgs;
  BfArgs a{nullptr, nullptr, part_mask, seed, laps, ksteps, sets};
  return launch_probe(
      g_bfload_err, dev, reinterpret_cast<const void*>(k_bfload_probe), kBlock, kLdsUsed, out, n,
      [&](dim3 grid, dim3 block, size_t smem, void* dump) {
        hipLaunchKernelGGL(k_bfload_probe, grid, block, smem, 0, static_cast<float*>(dump), a);
      },
      [&] { return device_sets(dev, seed, ksteps, sets, &a); });
}

// Host only. out4[p] = the workgroup digest a healthy CU leaves for part p at
// the sweep's shape, 0 for a part outside part_mask.
int xs_bfload_sweep_expected(uint32_t part_mask, uint32_t seed, uint32_t laps, uint32_t* out4) {
  if (bad_part_mask(part_mask, kAllParts) || bad_shape(laps, kBfKsteps, kBfSets) || !out4) return kBadArgs;
  return expected_digests(part_mask, seed, laps, kBfKsteps, kBfSets, out4);
}

// What the runtime reports for k_bfload_sweep on `dev`: out4 = {registers per
// lane, scratch bytes per lane, dynamic LDS bytes per workgroup, workgroups
// that fit on a CU at once}.
int xs_bfload_sweep_info(int dev, int* out4) {
  return sweep_info(g_bfload_err, dev, reinterpret_cast<const void*>(k_bfload_sweep), kBlock, true, out4);
}

// One sweep launch of `blocks` workgroups (0: 4 per CU) of `laps` laps at the
// sweep's shape. Writes `blocks` 128-byte records to records_out. inject_xcd /
// inject_cu: -1 is none / any, values below -1 are refused. Returns 0, -1000
// for bad arguments and -1003 when arena or table could not be allocated
// (nothing is launched either way), or a negative HIP error.
int xs_bfload_sweep(int dev, int blocks, uint32_t part_mask, uint32_t seed, uint32_t laps, int inject_xcd,
                    int inject_cu, uint32_t inject_parts, void* records_out, int* n_records, double* ms) {
  if (bad_part_mask(part_mask, kAllParts) || bad_shape(laps, kBfKsteps, kBfSets) || (inject_parts & ~kAllParts))
    return kBadArgs;
  // launch_sweep refuses these too, but only after the host has built the sets.
  if (!records_out || blocks < 0 || blocks > kMaxBlocks || inject_xcd < -1 || inject_cu < -1 || inject_xcd > 15 ||
      inject_cu > 0xff)
    return kBadArgs;
  Expect e;
  if (int rc = expected_digests(part_mask, seed, laps, kBfKsteps, kBfSets, e.digest)) return rc;
  BfArgs a{nullptr, nullptr, part_mask, seed, laps, kBfKsteps, kBfSets};
  return launch_sweep(
      g_bfload_err, {dev, blocks, inject_xcd, inject_cu, records_out, n_records, ms},
      reinterpret_cast<const void*>(k_bfload_sweep), kBlock, kLdsUsed, sizeof(BfRecord),
      [&](dim3 grid, dim3 block, size_t smem, void* rec) {
        hipLaunchKernelGGL(k_bfload_sweep, grid, block, smem, 0, static_cast<BfRecord*>(rec), a, inject_xcd, inject_cu,
                           inject_parts, e);
      },
      [&] { return device_sets(dev, seed, kBfKsteps, kBfSets, &a); });
}

}  // extern "C"
