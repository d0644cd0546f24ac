// Attention load sweep for gfx950 (MI355X): every CU under load, with a checked
// attention forward pass.
//
// load_sweep.hip, mxload_sweep.hip and bfload_sweep.hip hold every CU at rate
// with a GEMM whose accumulators go to a comparison and nowhere else. In an
// attention kernel they do not: they pass through the VALU (floor, clamp, max,
// subtract, the transcendental unit's v_exp_f32, v_cvt_pk_bf16_f32), through
// the exchange between a wave's two lane halves (v_permlane32_swap), and go
// straight back into the matrix core as an operand of the second product, with
// a running rescale of the output accumulators in between and V arriving
// through ds_read_b64_tr_b16. k_attnload_sweep is a sweep over named parts
// (part_sweep.h) whose load is that chain, two waves on every SIMD, many laps
// in one launch, every result of every lap compared on the device by equality.
//
// What makes equality possible. One lap is one tile: Q[256][64], K[N][64],
// V[N][64] of bf16, N = 64 kvsteps, no mask, key blocks of 64.
//   K element  (h16 & 0x807F) | 0x3F80: +-(128 + m) 2^-7, all seven mantissa
//              bits and the sign from the hash.
//   Q element  (h16 & 0x807F) | 0x3D80: the same, divided by 16.
//   V element  the integer +-(b & 127) of a hashed byte b (bit 7: the sign),
//              held as bf16, which is exact.
// Scores S = Q K^T: every product is a multiple of 2^-18, |S| < 64 (255/128)^2
// / 16 < 16, so any partial sum in any order is one exact float (22 bits). The
// exponent is e = med3(floor(S), -4, 3): floor and clamp are part of the
// definition, they make every probability a power of two. Online softmax in
// base 2: the running m is the row maximum of e so far (it starts at -4, the
// least e), p = v_exp_f32(e - m) in {2^-7 .. 1}, l <- l 2^(m_old - m) + sum p,
// O <- O 2^(m_old - m) + p V. p is exact in bf16. Relative to the current m
// every term is a multiple of 2^-7 at every moment (e >= -4, m <= 3), |O| <=
// N 127 and l <= N, so all of it is exact while N 127 2^7 < 2^24: N <= 1,032,
// kvsteps <= 16 is the cap. The final division O / l rounds and is left out:
// the results are O (unnormalised), l and m. The host holds fixO = O 128 as
// int32 [256][64], fixL = l 128 [256] and m [256] per set (66 KiB), computed in
// plain integers with no float anywhere, re-checks max |S| < 16 and max over d
// of 128 sum_keys |V| < 2^24 on what it generated and refuses (-1001) a set
// that left the bound.
//
// Operands. Dword w of panel p (0: Q, 1: K, 2: V) of set s is
//     fmix32(seed ^ (s << 23 | p << 21 | w)),
// each 16-bit half (for V: the low byte of each half) taken as above, low half
// first; a panel is row-major with d contiguous: Q has 8,192 dwords, K and V
// 2,048 kvsteps each. In the arena a set is Q (32 KiB), then per key block t
// the block's 64 rows of K (8 KiB) and its 64 rows of V (8 KiB): a block is 16
// KiB, contiguous. A set is 32,768 + 16,384 kvsteps bytes; its dword i is the
// i-th in that order. Arena and table are cached per (seed, kvsteps, sets) and
// per device for the life of the process; the kernels write neither.
//
// Work split. A workgroup is 512 threads: 8 waves, two on every SIMD,
// exclusive_lds(), so no two share a CU. A wave owns 32 query rows: in lap l
// wave w takes query block (w + l) & 7 and workgroup g reads set
// set_of(g, l, laps, sets) (part_sweep.h). Everything per query is per lane.
//
// Lane maps relied on, lane = (r = lane & 31, h = lane >> 5):
//   v_mfma_f32_32x32x16_bf16 (matrix_sweep.hip's header): A[r][8h..8h+7],
//     B[8h..8h+7][r], C[(q & 3) + 8 (q >> 2) + 4h][r] in accumulator register q.
//   S^T = K Q^T, per 32 keys: A = one 128-bit LDS read of K[32 kt + r][16 ks +
//     8h..+7]; B = Q[32 qb + r][16 ks + 8h..+7], read from the arena once per
//     lap into 16 VGPRs. Register q of tile kt then holds query r's score for
//     key 32 kt + 4h + (q & 3) + 8 (q >> 2): a lane holds 32 of a block's 64
//     scores of its query, lane (r, 1 - h) the other 32.
//   v_permlane32_swap v, v (lane_sweep.hip's header: lanes 32-63 of vdst <->
//     lanes 0-31 of src): the two results hold, in either order, the lane's own
//     value and that of lane (r, 1 - h), so their max and their sum are the
//     row's. One swap per statistic and block.
//   O^T[d][i] += V^T P^T: B = P^T straight from the accumulator registers of
//     S^T through v_cvt_pk_bf16_f32: k-step u (16 keys) takes registers 8 (u &
//     1).. + 7 of tile u >> 1, so k-slot (h, jj) of k-step u stands for key
//     16 u + 4h + (jj & 3) + 8 (jj >> 2). A is read to match: two
//     ds_read_b64_tr_b16, of V rows 16 u + 4h + 0..3 and 16 u + 8 + 4h + 0..3,
//     by the map bfload_sweep.hip states: in a group of 16 lanes, lane 4q + p
//     supplies the address of row q, columns 4p..4p+3, and lane i receives
//     column i of the four rows (rows 0, 1 in word 0); group (lane >> 4) & 1
//     takes columns 16 group of the 32 d of tile dt. Summation over keys has no
//     order, so the permutation of k-slots costs nothing. Register q of tile dt
//     holds O[query r][32 dt + (q & 3) + 8 (q >> 2) + 4h].
// Per key block a wave issues 8 MFMAs for S^T and 8 for O^T and holds 32 + 32
// accumulator registers; m, l and the rescale factor are one VGPR each and the
// rescale of O^T is one multiply per accumulator register.
//
// Movement. Thread t brings chunk t (16 bytes) of the block's K and chunk t of
// its V in with two global_load_dwordx4 into staging registers and from there
// into one of two LDS stages; the loads of block t + 1 are in flight while
// block t computes; one barrier per block; the global block index runs across
// laps: a stage is written only after the barrier that follows its last read.
// LDS rows are padded: K to 144 bytes (128 + 16: 144 / 16 is odd, the load
// sweep's rule for 128-bit reads), V to 192 (128 + 64: 48 banks, so the four
// rows of one transposed read start 16 banks apart and their 8 banks each do
// not meet). A stage is 64 x 144 + 64 x 192 = 21,504 bytes, two are 43,008. The
// bank model is that of the public CDNA3 material, 64 banks of 4 bytes, assumed
// for CDNA4; no counter was read.
//
// Lap epilogue. Every lane takes its 32 O^T registers through fix = (int)(acc
// 128), counts a mismatch when that loses anything (a NaN too) or differs from
// the table, and does likewise for l and m.
//
// Parts (bit, name). The mask selects what is judged; the pipeline always
// runs, it is the load. The folds of a part that is not selected are not issued.
//   0 stage      every dword a thread received from the arena (Q, K and V):
//                sum of rotl32(word, i & 31), i its dword index in the set.
//   1 score      sum of (e + 4) (2 (N row + key) + 1) over every clamped
//                exponent: Q K^T, floor and clamp.
//   2 stat       per row, in both lanes that hold it: fixL (2 row + 1) +
//                (m + 4) (2 (256 + row) + 1), so twice the rows' sum: max, exp,
//                sum and the exchange. Mismatches against the table are counted.
//   3 transpose  every word a transposed read delivered: the word is V[2j][n] |
//                V[2j+1][n] << 16 and its index 64 j + n, the stage's fold.
//                Every wave reads all of V: 8 sum(V') per lap.
//   4 out        mismatches against the table are counted; the digest is the
//                sum of uint32(fixO) (2 (64 row + d) + 1) over the laps.
// A bad out with good score, stat and transpose names the second product; a bad
// stat with a good score names the VALU or permlane chain.
//
// Record (128 bytes per workgroup), injection and safety rules are the load
// sweep's: part_sweep.h's head with five parts, the reserved word and the query
// block, set and span masks (of laps whose out or stat mis-compared); an
// injected part flips bit 0 of its word 0 in registers (stage, transpose: the
// first dword thread 0 folds; score: the first e + 4 thread 0 folds, in the
// fold only; stat: fixL of thread 0 in lap 0; out: fix of thread 0's register 0
// in lap 0). Trip counts come from the kernel arguments only; no loop waits on
// a clock, a flag or another workgroup. No scratch, no spill, MODE is not
// written, results leave through vector stores. Every index into the arena is
// below (32,768 + 16,384 kvsteps) sets and every index into the table below
// 16,896 sets by construction.
//
// k_attnload_probe is the same device function with a dump: one workgroup at
// any shape stores O of every lap as [lap][256][64] float32, behind it l as
// [lap][256] float32 and m as [lap][256] int32, and behind those each thread's
// stage, score and transpose folds ([3][512]).
//
// What the hardware settled: on the first run on an MI355X the probe equalled
// the numpy reference (tests/attnload_sweep_ref.py) at every shape and seed, O,
// l, m and all three folds; the lane maps above stand as written, and raw
// v_exp_f32 is exact on the integer arguments -7..0, so v_ldexp_f32 was not
// needed.
//
// NOT covered: masks, head dimensions other than 64, fp8 attention, the final
// division, the backward pass; varied exponents of K and Q (one binade each);
// HBM traffic (which cache level served a load is the hardware's choice); more
// than one launch; LDS bank conflicts, power, clocks and temperature, which are
// not observed.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <map>
#include <memory>
#include <mutex>
#include <tuple>
#include <vector>

#include "hip/part_sweep.h"

#define XS_ERR_BUF g_attnload_err
#define XS_HD __host__ __device__ __forceinline__
#define XS_D __device__ __forceinline__

namespace {

using namespace xsprobe;

ErrBuf g_attnload_err = "";

typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef short i16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __attribute__((address_space(3))) i16x4* LdsTrPtr;

constexpr int kNumParts = 5;
const char kPartNames[] = "stage,score,stat,transpose,out";
constexpr uint32_t kAllParts = (1u << kNumParts) - 1;
constexpr int kStage = 0, kScore = 1, kStat = 2, kTranspose = 3, kOut = 4;
constexpr int kBlock = 512;  // 8 waves: two per SIMD
constexpr int kExtra = 3;    // query block, set and span masks
constexpr int kUnswept = -1003;
constexpr int kBoundBroken = -1001;  // the generator left its stated bound (a bug in this file)

// The sweep's fixed shape and defaults: measured in profiles/attnload_sweep_defaults.md.
constexpr uint32_t kAtKvsteps = 8, kAtSets = 32;
constexpr uint32_t kAtLaps = 1024;
constexpr uint32_t kMaxLaps = 16 * kAtLaps, kMaxKvsteps = 16, kMaxSets = 64;

constexpr uint32_t kRowsQ = 256, kHeadDim = 64, kBlockKeys = 64;
constexpr uint32_t kRowBytes = 2 * kHeadDim;                      // 128: a row of Q, K or V
constexpr uint32_t kBytesQ = kRowsQ * kRowBytes;                  // 32,768
constexpr uint32_t kHalfBlockBytes = kBlockKeys * kRowBytes;      // 8,192: a block's K, or its V
constexpr uint32_t kBlockBytes = 2 * kHalfBlockBytes;             // 16,384: K then V of a key block
constexpr uint32_t kPitchK = 144;                                 // LDS row of K: 128 + 16 bytes
constexpr uint32_t kPitchV = 192;                                 // LDS row of V: 128 + 64 bytes
constexpr uint32_t kStageV = kBlockKeys * kPitchK;                // 9,216: where a stage's V rows begin
constexpr uint32_t kStageBytes = kStageV + kBlockKeys * kPitchV;  // 21,504
constexpr uint32_t kOutWords = kRowsQ * kHeadDim;                 // O of one set: 64 KiB
constexpr uint32_t kSetWords = kOutWords + 2 * kRowsQ;            // fixO, fixL, m: 66 KiB
constexpr uint32_t kFoldWords = 3 * kBlock;                       // the probe's per-thread folds
constexpr uint32_t kRedBytes = part_reduction_words<kBlock>(kNumParts, kExtra) * 4;
constexpr uint32_t kLdsUsed = 2 * kStageBytes > kRedBytes ? 2 * kStageBytes : kRedBytes;
constexpr int kMinE = -4, kMaxE = 3;
constexpr float kFixScale = 128.f;  // O and l in units of 2^-7
static_assert(kBlockKeys * kMaxKvsteps * 127u * (1u << (kMaxE - kMinE)) < (1u << 24), "every partial sum is exact");
static_assert(2 * kStageBytes == 43008 && kStageV % 16 == 0 && kPitchV % 8 == 0, "two stages; 64-bit transposed reads");
static_assert(kMaxSets <= 512 && kBlockBytes / 4 / 2 * kMaxKvsteps < (1u << 21), "the hash's key holds set, panel and w");

XS_HD uint32_t set_bytes(uint32_t kvsteps) { return kBytesQ + kBlockBytes * kvsteps; }

XS_HD uint32_t hash_word(uint32_t seed, uint32_t set, uint32_t panel, uint32_t w) {
  return fmix32(seed ^ (set << 23 | panel << 21 | w));
}
// Two bf16 of one binade: sign and mantissa from the hash, the biased exponent 127 (K) or 123 (Q).
XS_HD uint32_t q_word(uint32_t seed, uint32_t set, uint32_t w) {
  return (hash_word(seed, set, 0, w) & 0x807f807fu) | 0x3d803d80u;
}
XS_HD uint32_t k_word(uint32_t seed, uint32_t set, uint32_t w) {
  return (hash_word(seed, set, 1, w) & 0x807f807fu) | 0x3f803f80u;
}

struct AtRecord {
  PartRecordHead<kNumParts> head;
  uint32_t reserved;
  uint32_t qblocks, sets, spans;
  uint32_t pad[13];
};
static_assert(sizeof(AtRecord) == 128, "one 128-byte record per workgroup");

using Expect = PartExpect<kNumParts>;

struct AtArgs {
  const uint8_t* arena;
  const int32_t* table;
  uint32_t part_mask, seed, laps, kvsteps, sets;
};

// ------------------------------------------------------------------- device
XS_D uint32_t fold4(u32x4 v, uint32_t s) {
  return rotl(v.x, s) + rotl(v.y, s + 1u) + rotl(v.z, s + 2u) + rotl(v.w, s + 3u);
}

// ds_read_b64_tr_b16: the lane's two words of the 4 x 16 block its group addresses.
XS_D u32x2 read_tr16(const uint8_t* p) {
  return __builtin_bit_cast(u32x2, __builtin_amdgcn_ds_read_tr16_b64_v4i16((LdsTrPtr)p));
}

// v_permlane32_swap v, v: the lane's own value and that of lane (r, 1 - h), in either order.
XS_D void both_halves(float x, float& a, float& b) {
  const uint32_t u = __float_as_uint(x);
  const auto s = __builtin_amdgcn_permlane32_swap(u, u, false, false);
  a = __uint_as_float(s[0]);
  b = __uint_as_float(s[1]);
}

// 1 where the float v is not the integer fix, or got is not want (v + 0.0f takes -0 to +0 and keeps a NaN a
// NaN, so the bits differ exactly when the values do).
XS_D uint32_t differs(float v, int32_t fix, uint32_t got, uint32_t want) {
  const uint32_t diff = (__float_as_uint(static_cast<float>(fix)) ^ __float_as_uint(v + 0.0f)) | (got ^ want);
  return (diff | (0u - diff)) >> 31;
}

// One workgroup's whole run. g: its rotation of the sets; inj: the parts to
// inject; dump: kDump only. Leaves the tallies and the three masks.
template <bool kDump>
XS_D void run_attnload(const AtArgs& a, uint32_t g, uint32_t inj, uint32_t* dump, uint8_t* lds, Tally (&y)[kNumParts],
                       uint32_t (&extra)[kExtra]) {
  const uint32_t t = threadIdx.x, lane = t & 63u, r = lane & 31u, h = lane >> 5;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const uint32_t kvsteps = a.kvsteps, laps = a.laps, sets = a.sets, N = kBlockKeys * kvsteps;
  const uint32_t sbytes = set_bytes(kvsteps);
  const bool stage_on = (a.part_mask >> kStage) & 1u, score_on = (a.part_mask >> kScore) & 1u;
  const bool transpose_on = (a.part_mask >> kTranspose) & 1u;

  // Staging: chunk t of the block's K and chunk t of its V; a row is 8 chunks.
  const uint32_t g_off = kBytesQ + t * 16u;  // in a set, at block 0
  const uint32_t lk_off = (t >> 3) * kPitchK + (t & 7u) * 16u;
  const uint32_t lv_off = kStageV + (t >> 3) * kPitchV + (t & 7u) * 16u;
  u32x4 stg[2];
  auto issue = [&](uint32_t set, uint32_t step) {
    const uint8_t* p = a.arena + static_cast<size_t>(set) * sbytes + g_off + step * kBlockBytes;
    stg[0] = *reinterpret_cast<const u32x4*>(p);
    stg[1] = *reinterpret_cast<const u32x4*>(p + kHalfBlockBytes);
  };
  // Folds what `issue` brought and hands it to a stage. Q and every half block
  // are multiples of 32 dwords, so a chunk's index has the low bits of 4 (t & 7).
  auto fold_store = [&](uint32_t stage, uint32_t flip) {
    if (stage_on) {
      const uint32_t s = 4u * (t & 7u);
      y[kStage].digest += rotl(stg[0].x ^ flip, s) - rotl(stg[0].x, s) + fold4(stg[0], s) + fold4(stg[1], s);
      y[kStage].bad += flip;
    }
    uint8_t* st = lds + stage * kStageBytes;
    *reinterpret_cast<u32x4*>(st + lk_off) = stg[0];
    *reinterpret_cast<u32x4*>(st + lv_off) = stg[1];
  };

  u32x4 qv[4];      // Q[32 qb + r][16 ks + 8h .. +7], ks = 0..3
  f32x16 o[2];      // O^T, d tiles 0 and 1
  float m = 0.f, l = 0.f;

  uint32_t score_flip = ((inj >> kScore) & 1u) && t == 0;
  uint32_t transpose_flip = ((inj >> kTranspose) & 1u) && t == 0;
  uint32_t lap = 0, step = 0, set = set_of(g, 0, laps, sets);
  uint32_t qb = wave & 7u;  // (wave + lap) & 7
  const uint32_t total = laps * kvsteps;
  // The transposed read: lane 4q + p of its group addresses key 4h + q, columns 16 group + 4p.
  const uint32_t tr_off =
      kStageV + (4u * h + ((lane & 15u) >> 2)) * kPitchV + 2u * (16u * ((lane >> 4) & 1u) + 4u * (lane & 3u));

  issue(set, 0);
  fold_store(0, ((inj >> kStage) & 1u) && t == 0);
  __syncthreads();

#pragma nounroll
  for (uint32_t gi = 0; gi < total; ++gi) {
    uint32_t nstep = step + 1u, nlap = lap, nset = set;
    if (nstep == kvsteps) {
      nstep = 0;
      nlap = lap + 1u;
      nset = set_of(g, nlap < laps ? nlap : 0u, laps, sets);
    }
    const uint32_t row = 32u * qb + r;  // the lane's query
    if (step == 0) {                    // a lap begins: its Q rows, O = 0, l = 0, m = the least e
      const uint8_t* p = a.arena + static_cast<size_t>(set) * sbytes + row * kRowBytes + 16u * h;
#pragma unroll
      for (uint32_t ks = 0; ks < 4; ++ks) qv[ks] = *reinterpret_cast<const u32x4*>(p + 32u * ks);
      if (stage_on)  // dword 32 row + 8 ks + 4h of the set
#pragma unroll
        for (uint32_t ks = 0; ks < 4; ++ks) y[kStage].digest += fold4(qv[ks], 8u * ks + 4u * h);
#pragma unroll
      for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int q = 0; q < 16; ++q) o[dt][q] = 0.f;
      m = static_cast<float>(kMinE), l = 0.f;
    }
    const bool more = gi + 1u < total;
    if (more) issue(nset, nstep);

    const uint8_t* st = lds + (gi & 1u) * kStageBytes;
    // S^T = K Q^T: two tiles of 32 keys, four k-steps of 16 of d each.
    f32x16 s[2];
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {
#pragma unroll
      for (int q = 0; q < 16; ++q) s[kt][q] = 0.f;
      const uint8_t* k_rd = st + (32u * kt + r) * kPitchK + 16u * h;
#pragma unroll
      for (uint32_t ks = 0; ks < 4; ++ks) {
        const u32x4 kv = *reinterpret_cast<const u32x4*>(k_rd + 32u * ks);
        s[kt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, kv),
                                                        __builtin_bit_cast(bf16x8, qv[ks]), s[kt], 0, 0, 0);
      }
    }
    // e = med3(floor(S), -4, 3) in place, and its maximum over the lane's 32 keys.
    float mx = static_cast<float>(kMinE);
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        s[kt][q] = __builtin_amdgcn_fmed3f(__builtin_floorf(s[kt][q]), static_cast<float>(kMinE),
                                           static_cast<float>(kMaxE));
        mx = __builtin_fmaxf(mx, s[kt][q]);
      }
    if (score_on) {
      // (e + 4) (2 (N row + key) + 1), key = 64 step + 32 kt + 4h + (q & 3) + 8 (q >> 2): the lane's part of
      // the weight once, the register's as a literal.
      uint32_t sum_e = 0, sum_ec = 0;
#pragma unroll
      for (int kt = 0; kt < 2; ++kt)
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          uint32_t e4 = static_cast<uint32_t>(static_cast<int32_t>(s[kt][q]) - kMinE);
          if (kt == 0 && q == 0) {
            e4 ^= score_flip;
            y[kScore].bad += score_flip;
            score_flip = 0;
          }
          sum_e += e4;
          sum_ec += e4 * static_cast<uint32_t>(2 * (32 * kt + (q & 3) + 8 * (q >> 2)));
        }
      y[kScore].digest += sum_e * (2u * (N * row + kBlockKeys * step + 4u * h) + 1u) + sum_ec;
    }
    // The row's maximum, the rescale factor, p = 2^(e - m) in place and the row's sum of p.
    float x0, x1;
    both_halves(mx, x0, x1);
    const float m_new = __builtin_fmaxf(m, __builtin_fmaxf(x0, x1));
    const float scale = __builtin_amdgcn_exp2f(m - m_new);
    m = m_new;
    float ps = 0.f;
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        s[kt][q] = __builtin_amdgcn_exp2f(s[kt][q] - m_new);
        ps += s[kt][q];
      }
    both_halves(ps, x0, x1);
    l = l * scale + (x0 + x1);
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
      for (int q = 0; q < 16; ++q) o[dt][q] *= scale;
    // O^T += V^T P^T: four k-steps of 16 keys, P^T from the registers of S^T.
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      f32x8 pf;
#pragma unroll
      for (int jj = 0; jj < 8; ++jj) pf[jj] = s[u >> 1][8 * (u & 1) + jj];
      const bf16x8 pb = __builtin_convertvector(pf, bf16x8);
      const uint8_t* v_rd = st + tr_off + (16u * u) * kPitchV;
#pragma unroll
      for (int dt = 0; dt < 2; ++dt) {
        const u32x2 lo = read_tr16(v_rd + 64u * dt);
        const u32x2 hi = read_tr16(v_rd + 8u * kPitchV + 64u * dt);
        const u32x4 vv = u32x4{lo.x, lo.y, hi.x, hi.y};
        if (transpose_on) {
          // Index 64 j + n of a word: its low five bits are those of n, which are r.
          uint32_t f = rotl(vv.x, r) + rotl(vv.y, r) + rotl(vv.z, r) + rotl(vv.w, r);
          if (u == 0 && dt == 0) {
            f += rotl(vv.x ^ transpose_flip, r) - rotl(vv.x, r);
            y[kTranspose].bad += transpose_flip;
            transpose_flip = 0;
          }
          y[kTranspose].digest += f;
        }
        o[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, vv), pb, o[dt], 0, 0, 0);
      }
    }

    if (more) fold_store((gi + 1u) & 1u, 0u);
    __syncthreads();

    if (nstep == 0) {  // the lap is complete
      const int32_t* want = a.table + static_cast<size_t>(set) * kSetWords;
      const bool first = t == 0 && lap == 0;
      uint32_t ne = 0, d = 0;
#pragma unroll
      for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4) {
          const uint32_t idx = row * kHeadDim + 32u * dt + 8u * q4 + 4u * h;  // registers 4 q4 .. + 3
          const u32x4 w4 = *reinterpret_cast<const u32x4*>(want + idx);
          const uint32_t w[4] = {w4.x, w4.y, w4.z, w4.w};
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const float acc = o[dt][4 * q4 + i], v = acc * kFixScale;
            const int32_t fix = static_cast<int32_t>(v);
            uint32_t got = static_cast<uint32_t>(fix);
            if (dt == 0 && q4 == 0 && i == 0 && ((inj >> kOut) & 1u) && first) got ^= 1u;
            if constexpr (kDump) dump[static_cast<size_t>(lap) * kOutWords + idx + i] = __float_as_uint(acc);
            ne += differs(v, fix, got, w[i]);
            d += got * (2u * (idx + i) + 1u);
          }
        }
      y[kOut].bad += ne;
      y[kOut].digest += d;
      // l and m, in both lanes that hold the row.
      const float lv = l * kFixScale;
      const int32_t fix_l = static_cast<int32_t>(lv), fix_m = static_cast<int32_t>(m);
      uint32_t got_l = static_cast<uint32_t>(fix_l);
      if (((inj >> kStat) & 1u) && first) got_l ^= 1u;
      const uint32_t ns = differs(lv, fix_l, got_l, static_cast<uint32_t>(want[kOutWords + row])) +
                          differs(m, fix_m, static_cast<uint32_t>(fix_m),
                                  static_cast<uint32_t>(want[kOutWords + kRowsQ + row]));
      y[kStat].bad += ns;
      y[kStat].digest += got_l * (2u * row + 1u) + static_cast<uint32_t>(fix_m - kMinE) * (2u * (kRowsQ + row) + 1u);
      if constexpr (kDump) {
        if (h == 0) {
          uint32_t* stat = dump + static_cast<size_t>(laps) * kOutWords;
          stat[static_cast<size_t>(lap) * kRowsQ + row] = __float_as_uint(l);
          stat[static_cast<size_t>(laps + lap) * kRowsQ + row] = static_cast<uint32_t>(fix_m);
        }
      }
      uint32_t judged = 0;
      if ((a.part_mask >> kOut) & 1u) judged += ne;
      if ((a.part_mask >> kStat) & 1u) judged += ns;
      if (judged) {
        extra[0] |= 1u << qb;
        extra[1] |= 1u << (set & 31u);
        extra[2] |= 1u << (32u * lap / laps);
      }
      qb = (qb + 1u) & 7u;
    }
    step = nstep, lap = nlap, set = nset;
  }

  if constexpr (kDump) {
    uint32_t* folds = dump + static_cast<size_t>(laps) * kSetWords;
    folds[t] = y[kStage].digest;
    folds[kBlock + t] = y[kScore].digest;
    folds[2 * kBlock + t] = y[kTranspose].digest;
  }
  // A part that is not selected leaves no tally: its digest in the record is 0.
#pragma unroll
  for (int p = 0; p < kNumParts; ++p)
    if (!((a.part_mask >> p) & 1u)) y[p] = Tally{};
}

__global__ __launch_bounds__(kBlock) void k_attnload_sweep(AtRecord* __restrict__ records, AtArgs a, int inject_xcd,
                                                          int inject_cu, uint32_t inject_parts, Expect expect) {
  extern __shared__ __attribute__((aligned(16))) uint8_t attnload_lds[];
  const uint32_t xcd = xcc_id();
  const uint32_t hw = hw_id();
  const uint32_t cu = cu_key(hw);
  const uint32_t simd = simd_id(hw);
  const bool inject = inject_selected(inject_xcd, inject_cu, xcd, cu);

  Tally y[kNumParts];
  uint32_t extra[kExtra] = {};
  run_attnload<false>(a, blockIdx.x, inject ? inject_parts & a.part_mask : 0u, nullptr, attnload_lds, y, extra);

  reduce_parts<kNumParts, kExtra, kBlock>(reinterpret_cast<uint32_t*>(attnload_lds), threadIdx.x, simd, y, extra,
                                          a.part_mask, expect, xcd, cu, &records[blockIdx.x]);
}

// One workgroup; dump holds laps x (16,384 + 256 + 256) words of O, l and m and 3 x 512 folds.
__global__ __launch_bounds__(kBlock) void k_attnload_probe(uint32_t* __restrict__ dump, AtArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t attnload_lds[];
  Tally y[kNumParts];
  uint32_t extra[kExtra] = {};
  run_attnload<true>(a, 0u, 0u, dump, attnload_lds, y, extra);
}

// --------------------------------------------------------------------- host
bool bad_shape(uint32_t laps, uint32_t kvsteps, uint32_t sets) {
  return laps < 1 || laps > kMaxLaps || kvsteps < 1 || kvsteps > kMaxKvsteps || sets < 1 || sets > kMaxSets;
}

// The bf16 bits of the integer +-(b & 127), bit 7 of b its sign.
uint16_t v_half(uint32_t b) {
  const uint32_t mag = b & 127u, sign = (b & 128u) << 8;
  if (!mag) return static_cast<uint16_t>(sign);
  uint32_t e = 0;
  while ((mag >> e) > 1u) ++e;
  return static_cast<uint16_t>(sign | (127u + e) << 7 | ((mag << (7u - e)) & 0x7fu));
}
uint32_t v_word(uint32_t seed, uint32_t set, uint32_t w) {
  const uint32_t x = hash_word(seed, set, 2, w);
  return v_half(x & 0xffu) | static_cast<uint32_t>(v_half((x >> 16) & 0xffu)) << 16;
}

// One set's panels in their logical order: 8,192 dwords of Q[256][64], 2,048
// kvsteps each of K[N][64] and V[N][64].
void fill_set(uint32_t seed, uint32_t set, uint32_t kvsteps, uint32_t* q, uint32_t* k, uint32_t* v) {
  for (uint32_t w = 0; w < kBytesQ / 4; ++w) q[w] = q_word(seed, set, w);
  for (uint32_t w = 0; w < kHalfBlockBytes / 4 * kvsteps; ++w) k[w] = k_word(seed, set, w), v[w] = v_word(seed, set, w);
}

// A bf16 of a fixed binade in units of its 2^-7: +-(128 + m).
int element_units(uint16_t x) {
  const int m = 128 + (x & 0x7f);
  return x & 0x8000 ? -m : m;
}
// A V element as the integer it holds.
int v_units(uint16_t x) {
  if (!(x & 0x7fff)) return 0;
  const int e = ((x >> 7) & 0xff) - 127, mag = (128 | (x & 0x7f)) >> (7 - e);
  return x & 0x8000 ? -mag : mag;
}

// What the host holds of a (seed, kvsteps, sets): the arena's dwords, the table
// and, per set, the digests of one lap.
struct HostSets {
  std::vector<uint32_t> arena;  // sets x (8,192 + 4,096 kvsteps) dwords
  std::vector<int32_t> table;   // sets x (fixO[256][64], fixL[256], m[256])
  std::vector<uint32_t> digest[kNumParts];
  bool bound_ok = true;
};

struct DeviceSets {
  DevMem arena, table;
};

std::mutex g_sets_mu;
std::map<std::tuple<uint32_t, uint32_t, uint32_t>, std::unique_ptr<HostSets>> g_host_sets;
std::map<std::tuple<int, uint32_t, uint32_t, uint32_t>, std::unique_ptr<DeviceSets>> g_device_sets;

// g_sets_mu held.
const HostSets& host_sets(uint32_t seed, uint32_t kvsteps, uint32_t sets) {
  auto& slot = g_host_sets[{seed, kvsteps, sets}];
  if (slot) return *slot;
  slot = std::make_unique<HostSets>();
  HostSets& hs = *slot;
  const uint32_t N = kBlockKeys * kvsteps, half = kHalfBlockBytes / 4;  // dwords of a block's K
  const size_t set_dwords = set_bytes(kvsteps) / 4;
  hs.arena.resize(sets * set_dwords);
  hs.table.resize(static_cast<size_t>(sets) * kSetWords);
  std::vector<uint32_t> qw(kBytesQ / 4), kw(static_cast<size_t>(half) * kvsteps), vw(kw.size());
  std::vector<int16_t> Q(kRowsQ * kHeadDim), K(static_cast<size_t>(N) * kHeadDim), V(K.size());
  std::vector<int32_t> e(N);
  for (uint32_t s = 0; s < sets; ++s) {
    fill_set(seed, s, kvsteps, qw.data(), kw.data(), vw.data());
    uint32_t* aw = hs.arena.data() + s * set_dwords;
    std::copy(qw.begin(), qw.end(), aw);
    for (uint32_t t = 0; t < kvsteps; ++t) {
      std::copy(kw.begin() + t * half, kw.begin() + (t + 1) * half, aw + qw.size() + 2 * t * half);
      std::copy(vw.begin() + t * half, vw.begin() + (t + 1) * half, aw + qw.size() + (2 * t + 1) * half);
    }
    uint32_t f = 0;
    for (size_t i = 0; i < set_dwords; ++i) f += rotl(aw[i], static_cast<uint32_t>(i & 31u));
    hs.digest[kStage].push_back(f);
    const uint16_t* q16 = reinterpret_cast<const uint16_t*>(qw.data());
    const uint16_t* k16 = reinterpret_cast<const uint16_t*>(kw.data());
    const uint16_t* v16 = reinterpret_cast<const uint16_t*>(vw.data());
    // V as a transposed read delivers it: word (j, n) = V[2j][n] | V[2j+1][n] << 16, index 64 j + n; 8 waves.
    f = 0;
    for (uint32_t j = 0; j < N / 2; ++j)
      for (uint32_t n = 0; n < kHeadDim; ++n)
        f += rotl(v16[2 * j * kHeadDim + n] | static_cast<uint32_t>(v16[(2 * j + 1) * kHeadDim + n]) << 16, n & 31u);
    hs.digest[kTranspose].push_back(8u * f);
    for (size_t i = 0; i < Q.size(); ++i) Q[i] = static_cast<int16_t>(element_units(q16[i]));
    for (size_t i = 0; i < K.size(); ++i) K[i] = static_cast<int16_t>(element_units(k16[i]));
    for (size_t i = 0; i < V.size(); ++i) V[i] = static_cast<int16_t>(v_units(v16[i]));
    // The second bound of the header: 128 sum_keys |V| per d, what O can reach in units of 2^-7 with every p = 1.
    for (uint32_t d = 0; d < kHeadDim; ++d) {
      int64_t mag = 0;
      for (uint32_t k = 0; k < N; ++k) mag += V[k * kHeadDim + d] < 0 ? -V[k * kHeadDim + d] : V[k * kHeadDim + d];
      if (mag * 128 >= (1 << 24)) hs.bound_ok = false;
    }
    // In plain integers: S in units of 2^-18, floor is the arithmetic shift, p 128 = 1 << (e - m + 7).
    int32_t* fix_o = hs.table.data() + static_cast<size_t>(s) * kSetWords;
    int32_t *fix_l = fix_o + kOutWords, *row_m = fix_l + kRowsQ;
    uint32_t d_score = 0, d_stat = 0, d_out = 0;
    for (uint32_t i = 0; i < kRowsQ; ++i) {
      int32_t mrow = kMinE;
      for (uint32_t k = 0; k < N; ++k) {
        int32_t su = 0;
        for (uint32_t d = 0; d < kHeadDim; ++d) su += Q[i * kHeadDim + d] * K[k * kHeadDim + d];
        if (su >= (16 << 18) || su <= -(16 << 18)) hs.bound_ok = false;
        const int32_t fl = su >> 18;
        e[k] = fl < kMinE ? kMinE : fl > kMaxE ? kMaxE : fl;
        mrow = e[k] > mrow ? e[k] : mrow;
        d_score += static_cast<uint32_t>(e[k] - kMinE) * (2u * (N * i + k) + 1u);
      }
      int32_t* orow = fix_o + i * kHeadDim;
      for (uint32_t d = 0; d < kHeadDim; ++d) orow[d] = 0;
      int32_t lsum = 0;
      for (uint32_t k = 0; k < N; ++k) {
        const int32_t p = 1 << (e[k] - mrow + 7);
        lsum += p;
        for (uint32_t d = 0; d < kHeadDim; ++d) orow[d] += p * V[k * kHeadDim + d];
      }
      fix_l[i] = lsum, row_m[i] = mrow;
      d_stat += static_cast<uint32_t>(lsum) * (2u * i + 1u) + static_cast<uint32_t>(mrow - kMinE) * (2u * (kRowsQ + i) + 1u);
      for (uint32_t d = 0; d < kHeadDim; ++d) d_out += static_cast<uint32_t>(orow[d]) * (2u * (i * kHeadDim + d) + 1u);
    }
    hs.digest[kScore].push_back(d_score);
    hs.digest[kStat].push_back(2u * d_stat);  // both lanes of a row
    hs.digest[kOut].push_back(d_out);
  }
  return hs;
}

// The digests of a healthy workgroup; 0 for a part outside the mask.
int expected_digests(uint32_t mask, uint32_t seed, uint32_t laps, uint32_t kvsteps, uint32_t sets, uint32_t* out) {
  std::lock_guard<std::mutex> g(g_sets_mu);
  const HostSets& hs = host_sets(seed, kvsteps, sets);
  if (!hs.bound_ok) {
    std::snprintf(g_attnload_err, sizeof g_attnload_err, "an operand set left the bound that keeps every sum exact");
    return kBoundBroken;
  }
  uint32_t d[kNumParts] = {};
  for (uint32_t l = 0; l < laps; ++l)
    for (int p = 0; p < kNumParts; ++p) d[p] += hs.digest[p][set_of(0, l, laps, sets)];
  for (int p = 0; p < kNumParts; ++p) out[p] = (mask >> p) & 1u ? d[p] : 0u;
  return 0;
}

// Arena and table of (seed, kvsteps, sets) on the current device `dev`, built
// and uploaded once. -1003 when either cannot be allocated: nothing is launched.
int device_sets(int dev, uint32_t seed, uint32_t kvsteps, uint32_t sets, AtArgs* a) {
  std::lock_guard<std::mutex> g(g_sets_mu);
  auto& slot = g_device_sets[{dev, seed, kvsteps, sets}];
  if (!slot) {
    const HostSets& hs = host_sets(seed, kvsteps, sets);
    if (!hs.bound_ok) return kBoundBroken;
    auto ds = std::make_unique<DeviceSets>();
    const size_t arena_bytes = hs.arena.size() * 4, table_bytes = hs.table.size() * 4;
    void *arena = nullptr, *table = nullptr;
    const bool got = hipMalloc(&arena, arena_bytes) == hipSuccess && hipMalloc(&table, table_bytes) == hipSuccess;
    ds->arena.p = arena, ds->table.p = got ? table : nullptr;  // what was had is freed with ds
    if (!got) {
      (void)hipGetLastError();
      std::snprintf(g_attnload_err, sizeof g_attnload_err,
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

const char* xs_attnload_sweep_last_error() { return g_attnload_err; }

// Part names, comma-separated, in bit order.
const char* xs_attnload_parts() { return kPartNames; }

// out2 = {words whatever the laps, words per lap} of a part in the probe's
// dump: out has 16,384 per lap, stat 512 (l, then m), the folds one per thread.
int xs_attnload_shape(int part, int* out2) {
  if (part < 0 || part >= kNumParts || !out2) return kBadArgs;
  const bool fold = part == kStage || part == kScore || part == kTranspose;
  out2[0] = fold ? kBlock : 0;
  out2[1] = fold ? 0 : part == kOut ? static_cast<int>(kOutWords) : 2 * static_cast<int>(kRowsQ);
  return 0;
}

// Host only. The bf16 bits of `set` in their logical order: q_out[256][64],
// k_out[64 kvsteps][64], v_out[64 kvsteps][64].
int xs_attnload_operands(uint32_t seed, uint32_t set, uint32_t kvsteps, void* q_out, void* k_out, void* v_out) {
  if (set >= kMaxSets || kvsteps < 1 || kvsteps > kMaxKvsteps || !q_out || !k_out || !v_out) return kBadArgs;
  fill_set(seed, set, kvsteps, static_cast<uint32_t*>(q_out), static_cast<uint32_t*>(k_out),
           static_cast<uint32_t*>(v_out));
  return 0;
}

// One workgroup at any shape; out = [laps][256][64] float32 of O, [laps][256]
// float32 of l, [laps][256] int32 of m, then [3][512]: every thread's stage,
// score and transpose fold. n_words = laps x 16,896 + 1,536. The mask selects
// which folds are issued.
int xs_attnload_probe(int dev, uint32_t part_mask, uint32_t seed, uint32_t laps, uint32_t kvsteps, uint32_t sets,
                      uint32_t* out, size_t n_words) {
  if (bad_part_mask(part_mask, kAllParts) || bad_shape(laps, kvsteps, sets) || !out) return kBadArgs;
  const size_t n = static_cast<size_t>(laps) * kSetWords + kFoldWords;
  if (n_words != n) return kBadArgs;
  AtArgs a{nullptr, nullptr, part_mask, seed, laps, kvsteps, sets};
  return launch_probe(
      g_attnload_err, dev, reinterpret_cast<const void*>(k_attnload_probe), kBlock, kLdsUsed, out, n,
      [&](dim3 grid, dim3 block, size_t smem, void* dump) {
        hipLaunchKernelGGL(k_attnload_probe, grid, block, smem, 0, static_cast<uint32_t*>(dump), a);
      },
      [&] { return device_sets(dev, seed, kvsteps, sets, &a); });
}

// Host only. out5[p] = the workgroup digest a healthy CU leaves for part p at
// the sweep's shape, 0 for a part outside part_mask.
int xs_attnload_sweep_expected(uint32_t part_mask, uint32_t seed, uint32_t laps, uint32_t* out5) {
  if (bad_part_mask(part_mask, kAllParts) || bad_shape(laps, kAtKvsteps, kAtSets) || !out5) return kBadArgs;
  return expected_digests(part_mask, seed, laps, kAtKvsteps, kAtSets, out5);
}

// What the runtime reports for k_attnload_sweep on `dev`: out4 = {registers per
// lane, scratch bytes per lane, dynamic LDS bytes per workgroup, workgroups
// that fit on a CU at once}.
int xs_attnload_sweep_info(int dev, int* out4) {
  return sweep_info(g_attnload_err, dev, reinterpret_cast<const void*>(k_attnload_sweep), kBlock, true, out4);
}

// One sweep launch of `blocks` workgroups (0: 4 per CU) of `laps` laps at the
// sweep's shape. Writes `blocks` 128-byte records to records_out. inject_xcd /
// inject_cu: -1 is none / any, values below -1 are refused. Returns 0, -1000
// for bad arguments and -1003 when arena or table could not be allocated
// (nothing is launched either way), or a negative HIP error.
int xs_attnload_sweep(int dev, int blocks, uint32_t part_mask, uint32_t seed, uint32_t laps, int inject_xcd,
                      int inject_cu, uint32_t inject_parts, void* records_out, int* n_records, double* ms) {
  if (bad_part_mask(part_mask, kAllParts) || bad_shape(laps, kAtKvsteps, kAtSets) || (inject_parts & ~kAllParts))
    return kBadArgs;
  // launch_sweep refuses these too, but only after the host has built the sets.
  if (!records_out || blocks < 0 || blocks > kMaxBlocks || inject_xcd < -1 || inject_cu < -1 || inject_xcd > 15 ||
      inject_cu > 0xff)
    return kBadArgs;
  Expect e;
  if (int rc = expected_digests(part_mask, seed, laps, kAtKvsteps, kAtSets, e.digest)) return rc;
  AtArgs a{nullptr, nullptr, part_mask, seed, laps, kAtKvsteps, kAtSets};
  return launch_sweep(
      g_attnload_err, {dev, blocks, inject_xcd, inject_cu, records_out, n_records, ms},
      reinterpret_cast<const void*>(k_attnload_sweep), kBlock, kLdsUsed, sizeof(AtRecord),
      [&](dim3 grid, dim3 block, size_t smem, void* rec) {
        hipLaunchKernelGGL(k_attnload_sweep, grid, block, smem, 0, static_cast<AtRecord*>(rec), a, inject_xcd,
                           inject_cu, inject_parts, e);
      },
      [&] { return device_sets(dev, seed, kAtKvsteps, kAtSets, &a); });
}

}  // extern "C"
