// Gradient load sweep for gfx950 (MI355X): every CU under load, with a checked
// bf16 weight-gradient GEMM in the TN layout, split-K through float atomics.
//
// The five load sweeps (load_sweep.hip and its siblings) keep a CU busy with
// work shaped like a forward pass: operands are read, products stay in
// registers and only a record leaves the CU. A training step spends most of
// its matrix time in backward GEMMs, and the weight gradient dW = X^T dY
// differs from all of them in three ways: both operands are stored token-major,
// so both MFMA operands come through the transposed LDS read
// (ds_read_b64_tr_b16; bfload_sweep.hip does that for B only); several waves
// hold partial sums of the same output element and combine them with
// global_atomic_add_f32, executed at the L2 (mem_sweep.hip proves those cold,
// a few per CU, with the matrix cores idle); and every lap pushes its whole
// output tile out of the CU through the vector-memory atomic path while the
// loads, LDS traffic and MFMAs of the next lap are in flight. k_gradload_sweep
// is a sweep over named parts (part_sweep.h) whose load is that GEMM, and every
// register partial and every accumulated sum is compared on the device by
// equality.
//
// The operation. Per lap dW[i][j] += sum_t X[t][i] dY[t][j], i, j in 0..127, t
// over K = 32 ksteps tokens. What accumulates in one memory location before it
// is read back and cleared is one epoch of `epoch` laps.
//
// What makes equality possible. X is bfload's element, x = (h16 & 0x807F) |
// 0x3F80: +-(128 + m) 2^-7, m in 0..127. dY is a signed integer +-(1..8): the
// sign is bit 15 of the hash's half and the magnitude 1 + (h16 & 7), exact in
// bf16. A product is a multiple of 2^-7 of at most 255 x 8 = 2,040 units, and
// any partial sum in any order, the order the atomics arrive in included, is an
// exact float while tokens x 2,040 < 2^24. The tokens of an epoch are
// 32 ksteps epoch, so the cap is epoch ksteps <= 257 (32 x 257 x 2,040 =
// 16,776,960 < 16,777,216; 258 breaks it). The host refuses anything above it
// with -1000 before launch and re-checks the maximum of sum |x||dy| over an
// epoch on what it generated (-1001). Tables are fix = dW 2^7 in plain int32;
// no float is rounded on the host.
//
// Operands. A set s is X_s[K][128] and dY_s[K][128] of bf16, both row-major
// with the token as the row: i and j are contiguous, k is not. Dword w of
// panel p (0: X, 1: dY) of set s comes from fmix32(seed ^ (s << 22 | p << 21 |
// w)), each 16-bit half made an element as above, low half first. A panel has
// 2,048 ksteps dwords; dY follows X in the arena, so a set is 16,384 ksteps
// bytes and its dword i is dword i of X, then of dY. Sets come in `groups`
// groups of `epoch` sets: set = group epoch + (lap in its epoch).
// groups = max(1, 32 / epoch), so the sweep's default shape has 32 sets.
//
// Work split. A workgroup is 512 threads: 8 waves, two on every SIMD,
// exclusive_lds(), so no two share a CU. The 128 x 128 tile is four 64 x 64
// sub-tiles; sub-tile u covers rows 64 (u >> 1) and columns 64 (u & 1). In lap
// l wave w owns sub-tile (w + l) & 3 and k-half w >> 2 of every 32-token step:
// one v_mfma_f32_32x32x16_bf16 per step for each of its four 32 x 32
// accumulators. Waves w and w + 4, which the hardware places on different
// SIMDs, hold the two halves of every output element: that is the split-K.
//
// Pipeline. One step is 32 rows of X and 32 of dY, each one contiguous block of
// 8 KiB: 1,024 chunks of 16 bytes, two global_load_dwordx4 per thread (chunk t
// of either block: row t >> 4, columns 8 (t & 15)..+7). The route is the
// register one of bfload_sweep.hip, not mxload_sweep.hip's LDS DMA: the
// `stage` part needs a register view of every dword as it arrived, which a DMA
// into LDS does not have, and the padded rows below need a store whose LDS
// address the lane chooses. A ring of two LDS stages: the loads of step k + 1
// are in flight while the 4 MFMAs of step k issue from the other stage; one
// barrier per step, and the step index runs across laps, so a stage is written
// only after the barrier that follows its last read. An LDS row is padded to a
// pitch of 320 bytes (256 + 64); a stage is 2 x 32 x 320 = 20,480 bytes, two
// are 40,960. The bank model is that of the public CDNA3 material, 64 banks of
// 4 bytes, assumed for CDNA4; no counter was read. Under it, in one transposed
// read a 16-lane group touches four rows at 32 consecutive bytes each; 320
// bytes are 80 banks, 16 mod 64, so the four rows start 16 banks apart and
// their 8 banks each do not meet.
//
// Operand reads, for lane (r = lane & 31, h = lane >> 5) of a wave with k-half
// kq, as v_mfma_f32_32x32x16_bf16 wants them (matrix_sweep.hip's header:
// A[r][8h..8h+7], B[8h..8h+7][r], C[(q & 3) + 8 (q >> 2) + 4h][r]). Both are
// the read bfload's header documents for B: in a group of 16 lanes, lane
// 4q + p supplies the address of row q, columns 4p..4p+3, and lane i receives
// column i of the four rows (rows 0, 1 in word 0). A row is a token k and a
// column an i (X, the A operand: A[i][k] = X[k][i]) or a j (dY, the B operand):
// group (lane >> 4) & 1 takes columns 16 group, the first read takes
// k = 16 kq + 8 h + 0..3, the second + 4..7; two reads give the lane
// X[k..k+7][row0 + r] or dY[k..k+7][col0 + r].
//
// Lap epilogue. After the last step of a lap every lane takes its 64
// accumulators through fix = (int)(acc 128), counts a mismatch when that loses
// anything (a NaN too) or differs from the per-set, per-k-half table
// [set][2][128][128] (part gemm), then adds each accumulator into the
// workgroup's slab with one no-return global_atomic_add_f32 at agent scope and
// clears it. A slab is 128 x 128 floats, 64 KiB of device memory, kept in the
// order the accumulators have: word ((4 u + 2 i + j) 16 + q) 64 + lane is
// element (64 (u >> 1) + 32 i + (q & 3) + 8 (q >> 2) + 4 h, 64 (u & 1) + 32 j +
// r) of accumulator (i, j) of sub-tile u, so one atomic instruction covers 256
// contiguous bytes. Nothing waits after the adds: the next lap's first loads
// were issued before them and its MFMAs follow at once. The vector memory
// counter counts in order, so the wait for the operands of the step after that
// is also a wait for the adds; they have one step's MFMAs to drain.
//
// Epoch end. After the last lap of an epoch, and after the last lap of the
// launch even if its epoch is partial, every wave releases its atomics with an
// agent-scope fence, the workgroup meets at a barrier, and the slab is read
// back and cleared in one operation per element, a returning
// global_atomic_swap of 0. Wave w reads accumulators (w >> 2, 0..1) of
// sub-tile (w + l + 2) & 3: neither of the two waves that added to an element
// in lap l reads it back. The value goes through fix and is compared with the
// epoch table [group][128][128] (part accum); a partial last epoch has a table
// of its own behind those. A wave has compared what its swaps returned before
// it leaves the epoch end, and the barrier of the next step stands between
// that and the next add to the same word.
//
// Slabs and sets. A workgroup has `slabs` slabs and uses slab e % slabs in
// epoch e; the footprint of a launch is blocks x slabs x 64 KiB, allocated and
// zeroed per call and freed after it. While lap l is below the last multiple
// of epoch x groups that fits in `laps`, workgroup g takes group
// (e + g 40503 % groups) % groups in epoch e, behind it group e % groups (the
// load sweep's documented departure): over `groups` epochs every workgroup
// sees every group once, so a healthy CU's digests do not depend on g.
//
// Parts (bit, name). The mask selects what is judged; the pipeline, atomics and
// read-back included, always runs: it is the load. The folds of a part that is
// not selected are not issued.
//   0 stage      every operand dword as it arrived from memory, before it goes
//                to LDS: sum of rotl32(word, i & 31), i its dword index in the
//                set.
//   1 transpose  every dword a lane receives from a transposed read, X and dY:
//                the word is M[2j][n] | M[2j+1][n] << 16 and its index
//                128 j + n, same fold. Either is read by two waves:
//                2 (sum(X') + sum(dY')) per lap.
//   2 gemm       mismatches of the register partials against the set table; the
//                digest is the sum of uint32(fix) (2 (128 row + col) + 1) over
//                both k-halves and the laps.
//   3 accum      mismatches of the slab as read back against the epoch table,
//                same digest over the epochs.
// A bad accum with a good gemm names the atomic or write path, or the return
// path, under load; a bad gemm with a good transpose names the matrix core; a
// bad transpose with a good stage names the transposed LDS read.
//
// Record (128 bytes per workgroup), injection and safety rules are the load
// sweep's: part_sweep.h's head with four parts, the reserved word and the
// sub-tile, set and span masks; an injected part flips bit 0 of one compared
// word in registers (stage, transpose: the first dword thread 0 folds, in the
// fold only; gemm: fix of thread 0's first accumulator of lap 0; accum: fix of
// the first word thread 0 reads back). Trip counts come from the kernel
// arguments only; no loop waits on a clock, a flag or another workgroup. No
// scratch, no spill, MODE is not written, results leave through vector stores
// and vector atomics only. Bounds: set < groups epoch and step < ksteps, so
// every arena index is below 16,384 ksteps sets; every table index below
// 32,768 sets (k-half < 2, element < 16,384); every epoch-table index below
// 16,384 (groups + 1); every slab index below 16,384 slabs blocks (slot <
// slabs, the word formula above is at most 16,383); every LDS address below
// 40,960 (row <= 31, column bytes <= 248 + 8).
//
// k_gradload_probe is the same device function with a dump: one workgroup at
// any legal shape stores the register partials as [lap][2][128][128] float32,
// behind them the slab as read back as [epoch][128][128] float32 and each
// thread's stage and transpose folds ([2][512]).
//
// What the hardware settled: on the first run on an MI355X the probe equalled
// the numpy reference (tests/gradload_sweep_ref.py) at every shape and seed,
// partials, slabs and both folds; the transposed read's map stands as written
// for A as for B. The launch is bound by the lap epilogue's atomics and table
// loads at every ksteps, not by the matrix cores
// (profiles/gradload_sweep_defaults.md, with the disassembly of the atomic).
//
// NOT covered: global_atomic_pk_add_bf16 accumulation; fp8 gradients; the
// activation gradient dX = dY W^T; split-K across workgroups (it would lose
// the attribution of a fault to one CU); xGMI traffic; more than one launch;
// varied exponents. Which level of the memory hierarchy held a slab is the
// hardware's choice and is not observed; LDS bank conflicts, power, clocks and
// temperature are not observed.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <map>
#include <memory>
#include <mutex>
#include <tuple>
#include <vector>

#include "hip/part_sweep.h"

#define XS_ERR_BUF g_grad_err
#define XS_HD __host__ __device__ __forceinline__
#define XS_D __device__ __forceinline__

namespace {

using namespace xsprobe;

ErrBuf g_grad_err = "";

typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef short i16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __attribute__((address_space(3))) i16x4* LdsTrPtr;
typedef __attribute__((address_space(1))) float* GlobalFloatPtr;

constexpr int kNumParts = 4;
const char kPartNames[] = "stage,transpose,gemm,accum";
constexpr uint32_t kAllParts = (1u << kNumParts) - 1;
constexpr int kStage = 0, kTranspose = 1, kGemm = 2, kAccum = 3;
constexpr int kBlock = 512;  // 8 waves: two per SIMD
constexpr int kExtra = 3;    // sub-tile, set and span masks
constexpr int kUnswept = -1003;
constexpr int kBoundBroken = -1001;  // the generator left its stated bound (a bug in this file)

// The sweep's defaults: measured in profiles/gradload_sweep_defaults.md.
constexpr uint32_t kGradKsteps = 8, kGradEpoch = 32, kGradSlabs = 8, kGradSets = 32;
constexpr uint32_t kGradLaps = 2048;
constexpr uint32_t kMaxLaps = 16 * kGradLaps, kMaxKsteps = 8, kMaxSlabs = 16;
constexpr uint32_t kMaxEpochSteps = 257;  // epoch x ksteps: 32 x 257 x 2,040 < 2^24

constexpr uint32_t kTile = 128;
constexpr uint32_t kStepK = 32;                          // tokens per step
constexpr uint32_t kStepBytes = kStepK * kTile * 2;      // 8,192: 32 whole rows of either operand
constexpr uint32_t kSetBytes = 2 * kStepBytes;           // per step: 16,384
constexpr uint32_t kPitch = 320;                         // LDS row: 256 + 64 bytes
constexpr uint32_t kOperandStage = kStepK * kPitch;      // 10,240: where a stage's dY rows begin
constexpr uint32_t kStageBytes = 2 * kOperandStage;      // 20,480
constexpr uint32_t kTileWords = kTile * kTile;           // dW of one lap: 64 KiB
constexpr uint32_t kFoldWords = 2 * kBlock;              // the probe's per-thread folds
constexpr uint32_t kSpread = 40503u;
constexpr uint32_t kRedBytes = part_reduction_words<kBlock>(kNumParts, kExtra) * 4;
constexpr uint32_t kLdsUsed = 2 * kStageBytes > kRedBytes ? 2 * kStageBytes : kRedBytes;
constexpr int kMaxProduct = 255 * 8;  // |x||dy| in units of 2^-7
constexpr float kFixScale = 128.f;    // dW in units of 2^-7
static_assert(kStepK * kMaxEpochSteps * kMaxProduct < (1u << 24), "every partial sum of an epoch is one exact float");
static_assert(kStepK * (kMaxEpochSteps + 1) * kMaxProduct >= (1u << 24), "and the cap is the largest that is");
static_assert(2 * kStageBytes == 40960 && kOperandStage % 8 == 0 && kPitch % 8 == 0, "two stages; 64-bit reads");

// Two bf16 of X: sign and mantissa from the hash, the biased exponent 127.
XS_HD uint32_t x_word(uint32_t seed, uint32_t set, uint32_t w) {
  return (fmix32(seed ^ (set << 22 | w)) & 0x807f807fu) | 0x3f803f80u;
}

struct GradRecord {
  PartRecordHead<kNumParts> head;
  uint32_t reserved;
  uint32_t subtiles, sets, spans;
  uint32_t pad[15];
};
static_assert(sizeof(GradRecord) == 128, "one 128-byte record per workgroup");

using Expect = PartExpect<kNumParts>;

struct GradArgs {
  const uint8_t* arena;
  const int32_t* table;   // [set][2][128][128]
  const int32_t* etable;  // [groups + 1][128][128]: the last is the partial epoch's
  float* slabs;           // [workgroup][slab][16,384], in accumulator order
  uint32_t part_mask, seed, laps, ksteps, epoch, nslabs, groups;
};

XS_HD uint32_t groups_of(uint32_t epoch) { return epoch < kGradSets ? kGradSets / epoch : 1u; }

// ------------------------------------------------------------------- device
XS_D uint32_t fold4(u32x4 v, uint32_t s) {
  return rotl(v.x, s) + rotl(v.y, s + 1u) + rotl(v.z, s + 2u) + rotl(v.w, s + 3u);
}

// ds_read_b64_tr_b16: the lane's two words of the 4 x 16 block its group addresses.
XS_D u32x2 read_tr16(const uint8_t* p) {
  return __builtin_bit_cast(u32x2, __builtin_amdgcn_ds_read_tr16_b64_v4i16((LdsTrPtr)p));
}

// global_atomic_add_f32 without return, at agent scope: the result is not used, so no register comes back.
XS_D void slab_add(float* p, float v) { (void)__builtin_amdgcn_global_atomic_fadd_f32((GlobalFloatPtr)p, v); }

// global_atomic_swap with return: what the word held, which is then 0.
XS_D float slab_take(float* p) {
  return __uint_as_float(
      __hip_atomic_exchange(reinterpret_cast<uint32_t*>(p), 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}

// fix of acc against want into (ne, d). (float)fix != v or got != want, without a lane mask per element:
// v + 0.0f takes -0 to +0 and keeps a NaN a NaN, so the bits differ exactly when the values do, and
// min(diff, 1) is one VALU instruction the optimiser does not turn back into 64 compares.
XS_D void judge(float acc, uint32_t flip, int32_t want, uint32_t idx, uint32_t& ne, uint32_t& d) {
  const float v = acc * kFixScale;
  const int32_t fix = static_cast<int32_t>(v);
  const uint32_t got = static_cast<uint32_t>(fix) ^ flip;
  const uint32_t diff =
      (__float_as_uint(static_cast<float>(fix)) ^ __float_as_uint(v + 0.0f)) | (got ^ static_cast<uint32_t>(want));
  uint32_t differs;
  asm("v_min_u32_e32 %0, 1, %1" : "=v"(differs) : "v"(diff));
  ne += differs;
  d += got * (2u * idx + 1u);
}

// One workgroup's whole run. g: its slabs and its rotation of the groups; inj:
// the parts to inject; dump: kDump only. Leaves the tallies and the three masks.
template <bool kDump>
XS_D void run_gradload(const GradArgs& a, uint32_t g, uint32_t inj, float* dump, uint8_t* lds, Tally (&y)[kNumParts],
                       uint32_t (&extra)[kExtra]) {
  const uint32_t t = threadIdx.x, lane = t & 63u, r = lane & 31u, h = lane >> 5;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(t >> 6), kq = wave >> 2;
  const uint32_t ksteps = a.ksteps, laps = a.laps, epoch = a.epoch, groups = a.groups, nslabs = a.nslabs;
  const uint32_t full = laps - laps % (epoch * groups);
  const bool stage_on = (a.part_mask >> kStage) & 1u, transpose_on = (a.part_mask >> kTranspose) & 1u;
  const bool gemm_on = (a.part_mask >> kGemm) & 1u, accum_on = (a.part_mask >> kAccum) & 1u;
  float* const slab0 = a.slabs + static_cast<size_t>(g) * nslabs * kTileWords;

  // Staging: chunk t of the step's block of X and of dY: row t >> 4, chunk t & 15 of the row.
  const uint32_t l_off = (t >> 4) * kPitch + (t & 15u) * 16u;
  u32x4 stg[2];
  auto issue = [&](uint32_t set, uint32_t step) {
    const uint8_t* p = a.arena + static_cast<size_t>(set) * (kSetBytes * ksteps) + step * kStepBytes + t * 16u;
    stg[0] = *reinterpret_cast<const u32x4*>(p);
    stg[1] = *reinterpret_cast<const u32x4*>(p + kStepBytes * ksteps);
  };
  // Folds what `issue` brought and hands it to a stage. A panel and a step's block are multiples of 32 dwords,
  // so a dword's index in the set has the low bits of 4 t + its place in the chunk.
  auto fold_store = [&](uint32_t stage, uint32_t flip) {
    if (stage_on) {
      const uint32_t s = 4u * (t & 7u);
      y[kStage].digest += rotl(stg[0].x ^ flip, s) - rotl(stg[0].x, s) + fold4(stg[0], s) + fold4(stg[1], s);
      y[kStage].bad += flip;
    }
    uint8_t* st = lds + stage * kStageBytes + l_off;
    *reinterpret_cast<u32x4*>(st) = stg[0];
    *reinterpret_cast<u32x4*>(st + kOperandStage) = stg[1];
  };

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int q = 0; q < 16; ++q) acc[i][j][q] = 0.f;

  uint32_t transpose_flip = ((inj >> kTranspose) & 1u) && t == 0;
  uint32_t accum_flip = ((inj >> kAccum) & 1u) && t == 0;
  // lap = epoch ep + at; the workgroup reads set group epoch + at and adds into slab `slot` = ep % nslabs.
  uint32_t lap = 0, step = 0, at = 0, slot = 0;
  uint32_t group = full ? static_cast<uint32_t>(static_cast<uint64_t>(g) * kSpread % groups) : 0u;
  uint32_t sub = wave & 3u;  // (wave + lap) & 3
  const uint32_t total = laps * ksteps;
  // The transposed read: lane 4q + p of its group addresses k = 16 kq + 8 h + q, columns 16 group + 4 p.
  const uint32_t tr_off =
      (16u * kq + 8u * h + ((lane & 15u) >> 2)) * kPitch + 2u * (16u * ((lane >> 4) & 1u) + 4u * (lane & 3u));

  issue(group * epoch, 0);
  fold_store(0, ((inj >> kStage) & 1u) && t == 0);
  __syncthreads();

#pragma nounroll
  for (uint32_t gi = 0; gi < total; ++gi) {
    uint32_t nstep = step + 1u, nlap = lap, nat = at, ngroup = group;
    if (nstep == ksteps) {
      nstep = 0;
      nlap = lap + 1u;
      if (++nat == epoch) {
        nat = 0;
        ngroup = group + 1u == groups ? 0u : group + 1u;
        if (nlap == full) ngroup = 0;  // full is a multiple of epoch groups: e % groups from here on
      }
    }
    const bool more = gi + 1u < total;
    if (more) issue(ngroup * epoch + nat, nstep);

    const uint32_t sr = sub >> 1, sc = sub & 1u;
    const uint8_t* st = lds + (gi & 1u) * kStageBytes + tr_off;
    const uint8_t* x_rd = st + 2u * (64u * sr);
    const uint8_t* d_rd = st + kOperandStage + 2u * (64u * sc);
    u32x4 av[2], bv[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const u32x2 xl = read_tr16(x_rd + 64u * i), xh = read_tr16(x_rd + 4u * kPitch + 64u * i);
      const u32x2 dl = read_tr16(d_rd + 64u * i), dh = read_tr16(d_rd + 4u * kPitch + 64u * i);
      av[i] = u32x4{xl.x, xl.y, xh.x, xh.y};
      bv[i] = u32x4{dl.x, dl.y, dh.x, dh.y};
    }
    if (transpose_on) {
      // Index 128 j + n of a word: its low five bits are those of n, which are r.
      uint32_t f = rotl(av[0].x ^ transpose_flip, r) - rotl(av[0].x, r);
      y[kTranspose].bad += transpose_flip;
      transpose_flip = 0;
#pragma unroll
      for (int i = 0; i < 2; ++i)
        f += rotl(av[i].x, r) + rotl(av[i].y, r) + rotl(av[i].z, r) + rotl(av[i].w, r) + rotl(bv[i].x, r) +
             rotl(bv[i].y, r) + rotl(bv[i].z, r) + rotl(bv[i].w, r);
      y[kTranspose].digest += f;
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, av[i]),
                                                            __builtin_bit_cast(bf16x8, bv[j]), acc[i][j], 0, 0, 0);

    if (more) fold_store((gi + 1u) & 1u, 0u);
    __syncthreads();

    if (nstep == 0) {  // the lap is complete
      const uint32_t set = group * epoch + at;
      const int32_t* want = a.table + (static_cast<size_t>(set) * 2u + kq) * kTileWords;
      float* slab = slab0 + static_cast<size_t>(slot) * kTileWords;
      const uint32_t row0 = 64u * sr + 4u * h, col0 = 64u * sc + r;
      uint32_t ne = 0, d = 0;
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int q = 0; q < 16; ++q) {
            const uint32_t idx = (row0 + 32u * i + (q & 3) + 8u * (q >> 2)) * kTile + col0 + 32u * j;
            const uint32_t flip = i == 0 && j == 0 && q == 0 && ((inj >> kGemm) & 1u) && t == 0 && lap == 0;
            if constexpr (kDump) dump[(static_cast<size_t>(lap) * 2u + kq) * kTileWords + idx] = acc[i][j][q];
            judge(acc[i][j][q], flip, want[idx], idx, ne, d);
          }
      // The split-K: both k-halves' waves add into the same words; 256 contiguous bytes per instruction.
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int q = 0; q < 16; ++q) {
            slab_add(slab + ((4u * sub + 2u * i + j) * 16u + q) * 64u + lane, acc[i][j][q]);
            acc[i][j][q] = 0.f;
          }
      y[kGemm].bad += ne;
      y[kGemm].digest += d;
      if (ne && gemm_on) {
        extra[0] |= 1u << sub;
        extra[1] |= 1u << (set & 31u);
        extra[2] |= 1u << (32u * lap / laps);
      }

      if (nat == 0 || nlap == laps) {  // the epoch is complete, or the launch is
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        __syncthreads();
        // Sub-tile (w + l + 2) & 3, accumulators (kq, 0..1): written in this lap by waves (w + 2) & 3 and + 4.
        const uint32_t rsub = (sub + 2u) & 3u;
        const int32_t* ewant = a.etable + static_cast<size_t>(nat == 0 ? group : groups) * kTileWords;
        const uint32_t erow0 = 64u * (rsub >> 1) + 32u * kq + 4u * h, ecol0 = 64u * (rsub & 1u) + r;
        const uint32_t ep = lap / epoch;
        float back[2][16];
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int q = 0; q < 16; ++q) back[j][q] = slab_take(slab + ((4u * rsub + 2u * kq + j) * 16u + q) * 64u + lane);
        uint32_t ene = 0, ed = 0;
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int q = 0; q < 16; ++q) {
            const uint32_t idx = (erow0 + (q & 3) + 8u * (q >> 2)) * kTile + ecol0 + 32u * j;
            if constexpr (kDump) dump[static_cast<size_t>(laps) * 2u * kTileWords + ep * kTileWords + idx] = back[j][q];
            judge(back[j][q], j == 0 && q == 0 ? accum_flip : 0u, ewant[idx], idx, ene, ed);
          }
        accum_flip = 0;
        y[kAccum].bad += ene;
        y[kAccum].digest += ed;
        if (ene && accum_on) {
          extra[0] |= 1u << rsub;
          extra[1] |= 1u << (set & 31u);
          extra[2] |= 1u << (32u * lap / laps);
        }
        slot = slot + 1u == nslabs ? 0u : slot + 1u;
      }
      sub = (sub + 1u) & 3u;
    }
    step = nstep, lap = nlap, at = nat, group = ngroup;
  }

  if constexpr (kDump) {
    const uint32_t epochs = (laps + epoch - 1u) / epoch;
    uint32_t* folds = reinterpret_cast<uint32_t*>(dump + (static_cast<size_t>(laps) * 2u + epochs) * kTileWords);
    folds[t] = y[kStage].digest;
    folds[kBlock + t] = y[kTranspose].digest;
  }
  // A part that is not selected leaves no tally: its digest in the record is 0.
#pragma unroll
  for (int p = 0; p < kNumParts; ++p)
    if (!((a.part_mask >> p) & 1u)) y[p] = Tally{};
}

__global__ __launch_bounds__(kBlock) void k_gradload_sweep(GradRecord* __restrict__ records, GradArgs a, int inject_xcd,
                                                          int inject_cu, uint32_t inject_parts, Expect expect) {
  extern __shared__ __attribute__((aligned(16))) uint8_t gradload_lds[];
  const uint32_t xcd = xcc_id();
  const uint32_t hw = hw_id();
  const uint32_t cu = cu_key(hw);
  const uint32_t simd = simd_id(hw);
  const bool inject = inject_selected(inject_xcd, inject_cu, xcd, cu);

  Tally y[kNumParts];
  uint32_t extra[kExtra] = {};
  run_gradload<false>(a, blockIdx.x, inject ? inject_parts & a.part_mask : 0u, nullptr, gradload_lds, y, extra);

  reduce_parts<kNumParts, kExtra, kBlock>(reinterpret_cast<uint32_t*>(gradload_lds), threadIdx.x, simd, y, extra,
                                          a.part_mask, expect, xcd, cu, &records[blockIdx.x]);
}

// One workgroup; dump holds laps x 32,768 floats of partials, 16,384 per epoch of the slab and 2 x 512 folds.
__global__ __launch_bounds__(kBlock) void k_gradload_probe(float* __restrict__ dump, GradArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t gradload_lds[];
  Tally y[kNumParts];
  uint32_t extra[kExtra] = {};
  run_gradload<true>(a, 0u, 0u, dump, gradload_lds, y, extra);
}

// --------------------------------------------------------------------- host
bool bad_shape(uint32_t laps, uint32_t ksteps, uint32_t epoch, uint32_t slabs) {
  return laps < 1 || laps > kMaxLaps || ksteps < 1 || ksteps > kMaxKsteps || epoch < 1 || epoch > kMaxEpochSteps ||
         epoch * ksteps > kMaxEpochSteps || slabs < 1 || slabs > kMaxSlabs;
}

// The bf16 of a dY element: +-(1..8) from a half of the hash.
uint16_t dy_half(uint32_t h16) {
  static const uint16_t kInt[8] = {0x3f80, 0x4000, 0x4040, 0x4080, 0x40a0, 0x40c0, 0x40e0, 0x4100};
  return static_cast<uint16_t>((h16 & 0x8000u) | kInt[h16 & 7u]);
}

// One set's dwords: 2,048 ksteps of X[K][128], then as many of dY[K][128].
void fill_set(uint32_t seed, uint32_t set, uint32_t ksteps, uint32_t* x_words, uint32_t* dy_words) {
  const uint32_t n = kStepBytes / 4 * ksteps;
  for (uint32_t w = 0; w < n; ++w) {
    x_words[w] = x_word(seed, set, w);
    const uint32_t hh = fmix32(seed ^ (set << 22 | 1u << 21 | w));
    dy_words[w] = dy_half(hh & 0xffffu) | static_cast<uint32_t>(dy_half(hh >> 16)) << 16;
  }
}

uint32_t fold_of(const uint32_t* words, size_t first, size_t n) {
  uint32_t f = 0;
  for (size_t i = 0; i < n; ++i) f += rotl(words[i], static_cast<uint32_t>((first + i) & 31u));
  return f;
}

// An X element in units of 2^-7, +-(128 + m), and a dY element, +-(1..8).
int x_units(uint16_t v) {
  const int m = 128 + (v & 0x7f);
  return v & 0x8000 ? -m : m;
}
int dy_units(uint16_t v) {
  const uint32_t e = (v >> 7) & 0xffu, frac = v & 0x7fu;  // 1.frac x 2^(e - 127), an integer here
  const int mag = static_cast<int>(((128u + frac) << (e - 127u)) >> 7);
  return v & 0x8000 ? -mag : mag;
}

uint32_t digest_of(const int32_t* fix) {
  uint32_t d = 0;
  for (uint32_t i = 0; i < kTileWords; ++i) d += static_cast<uint32_t>(fix[i]) * (2u * i + 1u);
  return d;
}

// What the host holds of a (seed, ksteps, epoch): the arena's dwords, the set
// table, the table of the full epochs and, per set, the folds of its panels
// as they lie and as the transposed reads deliver them, and its digest.
struct HostSets {
  uint32_t groups = 0;
  std::vector<uint32_t> arena;  // sets x 4,096 ksteps dwords
  std::vector<int32_t> table;   // sets x 2 x 128 x 128 of fix = dW 2^7 of a k-half
  std::vector<int32_t> etable;  // groups x 128 x 128: the sum over a group's sets
  std::vector<uint32_t> fold, fold_tr, gemm, accum;
  bool bound_ok = true;
};

std::mutex g_sets_mu;
std::map<std::tuple<uint32_t, uint32_t, uint32_t>, std::unique_ptr<HostSets>> g_host_sets;

// g_sets_mu held.
const HostSets& host_sets(uint32_t seed, uint32_t ksteps, uint32_t epoch) {
  auto& slot = g_host_sets[{seed, ksteps, epoch}];
  if (slot) return *slot;
  slot = std::make_unique<HostSets>();
  HostSets& hs = *slot;
  hs.groups = groups_of(epoch);
  const uint32_t sets = hs.groups * epoch;
  const size_t K = static_cast<size_t>(kStepK) * ksteps;
  const size_t panel = kStepBytes / 4 * static_cast<size_t>(ksteps);
  hs.arena.resize(sets * 2 * panel);
  hs.table.resize(static_cast<size_t>(sets) * 2 * kTileWords);
  hs.etable.assign(static_cast<size_t>(hs.groups) * kTileWords, 0);
  std::vector<int16_t> X(K * kTile), D(K * kTile);
  std::vector<int32_t> mag(static_cast<size_t>(hs.groups) * kTileWords, 0);
  for (uint32_t s = 0; s < sets; ++s) {
    uint32_t* xw = hs.arena.data() + s * 2 * panel;
    uint32_t* dw = xw + panel;
    fill_set(seed, s, ksteps, xw, dw);
    hs.fold.push_back(fold_of(xw, 0, 2 * panel));
    const uint16_t* x16 = reinterpret_cast<const uint16_t*>(xw);
    const uint16_t* d16 = reinterpret_cast<const uint16_t*>(dw);
    // As a transposed read delivers them: word (j, n) = M[2j][n] | M[2j+1][n] << 16, index 128 j + n.
    uint32_t ftr = 0;
    for (size_t j = 0; j < K / 2; ++j)
      for (uint32_t n = 0; n < kTile; ++n)
        ftr += rotl(x16[2 * j * kTile + n] | static_cast<uint32_t>(x16[(2 * j + 1) * kTile + n]) << 16, n & 31u) +
               rotl(d16[2 * j * kTile + n] | static_cast<uint32_t>(d16[(2 * j + 1) * kTile + n]) << 16, n & 31u);
    hs.fold_tr.push_back(ftr);
    for (size_t i = 0; i < X.size(); ++i) X[i] = static_cast<int16_t>(x_units(x16[i]));
    for (size_t i = 0; i < D.size(); ++i) D[i] = static_cast<int16_t>(dy_units(d16[i]));
    // fix = dW 2^7 of either k-half in plain int32, the epoch's sum, and the bound of the header on what was
    // generated: token k of a step belongs to k-half (k >> 4) & 1.
    int32_t* C = hs.table.data() + static_cast<size_t>(s) * 2 * kTileWords;
    int32_t* E = hs.etable.data() + static_cast<size_t>(s / epoch) * kTileWords;
    int32_t* M = mag.data() + static_cast<size_t>(s / epoch) * kTileWords;
    for (size_t i = 0; i < 2 * kTileWords; ++i) C[i] = 0;
    for (size_t k = 0; k < K; ++k) {
      int32_t* half = C + ((k >> 4) & 1u) * kTileWords;
      const int16_t* xr = &X[k * kTile];
      const int16_t* dr = &D[k * kTile];
      for (uint32_t i = 0; i < kTile; ++i) {
        const int32_t x = xr[i], ax = x < 0 ? -x : x;
        for (uint32_t j = 0; j < kTile; ++j) {
          half[i * kTile + j] += x * dr[j];
          M[i * kTile + j] += ax * (dr[j] < 0 ? -dr[j] : dr[j]);
        }
      }
    }
    for (uint32_t i = 0; i < kTileWords; ++i) E[i] += C[i] + C[kTileWords + i];
    hs.gemm.push_back(digest_of(C) + digest_of(C + kTileWords));
  }
  for (int32_t m : mag)
    if (m >= (1 << 24)) hs.bound_ok = false;
  for (uint32_t gr = 0; gr < hs.groups; ++gr)
    hs.accum.push_back(digest_of(hs.etable.data() + static_cast<size_t>(gr) * kTileWords));
  return hs;
}

// g_sets_mu held. The sums of a partial last epoch of `laps`: the first laps % epoch sets of its group.
void partial_epoch(const HostSets& hs, uint32_t laps, uint32_t epoch, std::vector<int32_t>* out) {
  out->assign(kTileWords, 0);
  const uint32_t group = laps / epoch % hs.groups;
  for (uint32_t at = 0; at < laps % epoch; ++at) {
    const int32_t* C = hs.table.data() + static_cast<size_t>(group * epoch + at) * 2 * kTileWords;
    for (uint32_t i = 0; i < kTileWords; ++i) (*out)[i] += C[i] + C[kTileWords + i];
  }
}

// The digests of a healthy workgroup (workgroup 0: group e % groups in every epoch); 0 for a part outside the mask.
int expected_digests(uint32_t mask, uint32_t seed, uint32_t laps, uint32_t ksteps, uint32_t epoch, uint32_t* out) {
  std::lock_guard<std::mutex> g(g_sets_mu);
  const HostSets& hs = host_sets(seed, ksteps, epoch);
  if (!hs.bound_ok) {
    std::snprintf(g_grad_err, sizeof g_grad_err, "an operand set left the bound that keeps every sum exact");
    return kBoundBroken;
  }
  uint32_t d[kNumParts] = {};
  for (uint32_t l = 0; l < laps; ++l) {
    const uint32_t group = l / epoch % hs.groups, s = group * epoch + l % epoch;
    d[kStage] += hs.fold[s];
    d[kTranspose] += 2u * hs.fold_tr[s];
    d[kGemm] += hs.gemm[s];
    if (l % epoch == epoch - 1u) d[kAccum] += hs.accum[group];
  }
  if (laps % epoch) {
    std::vector<int32_t> tail;
    partial_epoch(hs, laps, epoch, &tail);
    d[kAccum] += digest_of(tail.data());
  }
  for (int p = 0; p < kNumParts; ++p) out[p] = (mask >> p) & 1u ? d[p] : 0u;
  return 0;
}

// What one call holds on the device; freed with it.
struct DeviceArea {
  DevMem arena, table, etable, slabs;
};

// Allocates and fills *da for a launch of `blocks` workgroups and points *a at
// it: arena, tables and the zeroed slabs. -1003 when any of it cannot be had:
// nothing is launched.
int device_area(DeviceArea* da, uint32_t blocks, GradArgs* a) {
  std::lock_guard<std::mutex> g(g_sets_mu);
  const HostSets& hs = host_sets(a->seed, a->ksteps, a->epoch);
  if (!hs.bound_ok) return kBoundBroken;
  std::vector<int32_t> tail;
  partial_epoch(hs, a->laps, a->epoch, &tail);
  const size_t arena_bytes = hs.arena.size() * 4, table_bytes = hs.table.size() * 4;
  const size_t etable_bytes = hs.etable.size() * 4, tail_bytes = tail.size() * 4;
  const size_t slab_bytes = static_cast<size_t>(blocks) * a->nslabs * kTileWords * 4;
  const bool got = hipMalloc(&da->arena.p, arena_bytes) == hipSuccess &&
                   hipMalloc(&da->table.p, table_bytes) == hipSuccess &&
                   hipMalloc(&da->etable.p, etable_bytes + tail_bytes) == hipSuccess &&
                   hipMalloc(&da->slabs.p, slab_bytes) == hipSuccess;
  if (!got) {
    (void)hipGetLastError();
    std::snprintf(g_grad_err, sizeof g_grad_err,
                  "no arena of %zu, tables of %zu and slabs of %zu bytes could be had: nothing was swept", arena_bytes,
                  table_bytes + etable_bytes + tail_bytes, slab_bytes);
    return kUnswept;
  }
  XS_CHECK(hipMemcpy(da->arena.p, hs.arena.data(), arena_bytes, hipMemcpyHostToDevice));
  XS_CHECK(hipMemcpy(da->table.p, hs.table.data(), table_bytes, hipMemcpyHostToDevice));
  XS_CHECK(hipMemcpy(da->etable.p, hs.etable.data(), etable_bytes, hipMemcpyHostToDevice));
  XS_CHECK(hipMemcpy(da->etable.as<uint8_t>() + etable_bytes, tail.data(), tail_bytes, hipMemcpyHostToDevice));
  XS_CHECK(hipMemset(da->slabs.p, 0, slab_bytes));
  a->arena = da->arena.as<const uint8_t>();
  a->table = da->table.as<const int32_t>();
  a->etable = da->etable.as<const int32_t>();
  a->slabs = da->slabs.as<float>();
  a->groups = hs.groups;
  return 0;
}

}  // namespace

extern "C" {

const char* xs_gradload_sweep_last_error() { return g_grad_err; }

// Part names, comma-separated, in bit order.
const char* xs_gradload_parts() { return kPartNames; }

// out2 = {words whatever the laps, words per lap (accum: per epoch)} of a part
// in the probe's dump: gemm has 32,768 per lap, accum 16,384 per epoch, the
// folds one per thread.
int xs_gradload_shape(int part, int* out2) {
  if (part < 0 || part >= kNumParts || !out2) return kBadArgs;
  out2[0] = part == kGemm || part == kAccum ? 0 : kBlock;
  out2[1] = part == kGemm ? static_cast<int>(2 * kTileWords) : part == kAccum ? static_cast<int>(kTileWords) : 0;
  return 0;
}

// Host only. The bf16 bits the arena holds for `set`: x_out[32 ksteps][128],
// dy_out[32 ksteps][128].
int xs_gradload_operands(uint32_t seed, uint32_t set, uint32_t ksteps, void* x_out, void* dy_out) {
  if (set >= (1u << 10) || ksteps < 1 || ksteps > kMaxKsteps || !x_out || !dy_out) return kBadArgs;
  fill_set(seed, set, ksteps, static_cast<uint32_t*>(x_out), static_cast<uint32_t*>(dy_out));
  return 0;
}

// One workgroup at any legal shape; out = [laps][2][128][128] float32 of the
// register partials, then [epochs][128][128] float32 of the slab as read back
// (epochs = ceil(laps / epoch)), then [2][512]: every thread's stage and
// transpose fold. The mask selects which folds are issued.
int xs_gradload_probe(int dev, uint32_t part_mask, uint32_t seed, uint32_t laps, uint32_t ksteps, uint32_t epoch,
                      uint32_t slabs, uint32_t* out, size_t n_words) {
  if (bad_part_mask(part_mask, kAllParts) || bad_shape(laps, ksteps, epoch, slabs) || !out) return kBadArgs;
  const size_t epochs = (laps + epoch - 1) / epoch;
  const size_t n = (static_cast<size_t>(laps) * 2 + epochs) * kTileWords + kFoldWords;
  if (n_words != n) return kBadArgs;
  GradArgs a{nullptr, nullptr, nullptr, nullptr, part_mask, seed, laps, ksteps, epoch, slabs, 0};
  DeviceArea da;
  return launch_probe(
      g_grad_err, dev, reinterpret_cast<const void*>(k_gradload_probe), kBlock, kLdsUsed, out, n,
      [&](dim3 grid, dim3 block, size_t smem, void* dump) {
        hipLaunchKernelGGL(k_gradload_probe, grid, block, smem, 0, static_cast<float*>(dump), a);
      },
      [&] { return device_area(&da, 1, &a); });
}

// Host only. out4[p] = the workgroup digest a healthy CU leaves for part p, 0
// for a part outside part_mask. `slabs` does not enter a digest; it is checked.
int xs_gradload_sweep_expected(uint32_t part_mask, uint32_t seed, uint32_t laps, uint32_t ksteps, uint32_t epoch,
                               uint32_t slabs, uint32_t* out4) {
  if (bad_part_mask(part_mask, kAllParts) || bad_shape(laps, ksteps, epoch, slabs) || !out4) return kBadArgs;
  return expected_digests(part_mask, seed, laps, ksteps, epoch, out4);
}

// What the runtime reports for k_gradload_sweep on `dev`: out4 = {registers per
// lane, scratch bytes per lane, dynamic LDS bytes per workgroup, workgroups
// that fit on a CU at once}.
int xs_gradload_sweep_info(int dev, int* out4) {
  return sweep_info(g_grad_err, dev, reinterpret_cast<const void*>(k_gradload_sweep), kBlock, true, out4);
}

// One sweep launch of `blocks` workgroups (0: 4 per CU) of `laps` laps of
// K = 32 ksteps, `epoch` laps to an epoch, `slabs` slabs per workgroup. Writes
// `blocks` 128-byte records to records_out. inject_xcd / inject_cu: -1 is none
// / any, values below -1 are refused. Returns 0, -1000 for bad arguments
// (epoch ksteps above 257 among them) and -1003 when arena, tables or slabs
// could not be allocated (nothing is launched either way), or a negative HIP
// error. What it allocated on the device is freed before it returns.
int xs_gradload_sweep(int dev, int blocks, uint32_t part_mask, uint32_t seed, uint32_t laps, uint32_t ksteps,
                      uint32_t epoch, uint32_t slabs, int inject_xcd, int inject_cu, uint32_t inject_parts,
                      void* records_out, int* n_records, double* ms) {
  if (bad_part_mask(part_mask, kAllParts) || bad_shape(laps, ksteps, epoch, slabs) || (inject_parts & ~kAllParts))
    return kBadArgs;
  // launch_sweep refuses these too, but only after the host has built the sets.
  if (!records_out || blocks < 0 || blocks > kMaxBlocks || inject_xcd < -1 || inject_cu < -1 || inject_xcd > 15 ||
      inject_cu > 0xff)
    return kBadArgs;
  if (!blocks) XS_CHECK(cu_count(dev, &blocks, 4));  // the slabs are sized by it
  if (blocks <= 0 || blocks > kMaxBlocks) return kBadArgs;
  Expect e;
  if (int rc = expected_digests(part_mask, seed, laps, ksteps, epoch, e.digest)) return rc;
  GradArgs a{nullptr, nullptr, nullptr, nullptr, part_mask, seed, laps, ksteps, epoch, slabs, 0};
  DeviceArea da;
  return launch_sweep(
      g_grad_err, {dev, blocks, inject_xcd, inject_cu, records_out, n_records, ms},
      reinterpret_cast<const void*>(k_gradload_sweep), kBlock, kLdsUsed, sizeof(GradRecord),
      [&](dim3 grid, dim3 block, size_t smem, void* rec) {
        hipLaunchKernelGGL(k_gradload_sweep, grid, block, smem, 0, static_cast<GradRecord*>(rec), a, inject_xcd,
                           inject_cu, inject_parts, e);
      },
      [&] { return device_area(&da, static_cast<uint32_t>(blocks), &a); });
}

}  // extern "C"
