// Load sweep for gfx950 (MI355X): every CU under load, with a checked int8 GEMM.
//
// The other per-CU sweeps run one unit at a time, cold and short. A defect
// that shows only when the matrix cores, the LDS, the VALU and the path from
// memory are busy at once, or only after some tens of milliseconds at full
// rate, passes them all. k_load_sweep is a sweep over named parts
// (part_sweep.h) whose load is a real GEMM pipeline: full-entropy int8 operands
// come from memory through L2/L1 into registers, go through LDS into
// v_mfma_i32_32x32x32_i8, two waves on every SIMD, an integer chain on the VALU
// between the MFMAs, for many laps in one launch. Every product of int8 is one
// exact int32 whatever the bits are, so every result of every lap is compared
// on the device by integer equality.
//
// Operands. A set s is A_s[128][K] and Bt_s[256][K] (B transposed: k is
// contiguous, a lane's 16 operand bytes are one 128-bit read), K = 64 ksteps.
// The two panels stand one behind the other, so a set is one matrix of 384
// rows of K bytes (rows 0..127: A, rows 128..383: Bt) and its dword i is
// dword i of that matrix. Byte b of panel p (0: A, 1: Bt) of set s is byte
// b & 3, little-endian, of
//     fmix32(key),  key = seed ^ (s << 23 | p << 22 | b >> 2)
// (fmix32: part_sweep.h; a panel has at most 2^22 dwords, sets are below 64).
// -128 occurs. |C| <= K 2^14, so ksteps <= 1024 keeps C inside int32. The host
// generates the sets, uploads them into one read-only arena (384 K bytes per
// set) and C_s = A_s Bt_s^T, computed in plain int32, as a table of 128 KiB
// per set; both are cached per (seed, ksteps, sets) for the life of the
// process and the kernels never write either.
//
// Work split. A workgroup is 512 threads: 8 waves, two on every SIMD. It asks
// for exclusive_lds(), so no two share a CU. Per lap it computes one macro
// tile C[128 x 256]; a wave owns a 64 x 64 sub-tile (four 32 x 32
// accumulators, 64 registers); sub-tile u covers rows 64 (u >> 2) and columns
// 64 (u & 3). In lap l wave w computes sub-tile (w + l) & 7, and workgroup g
// uses set (g + l) % sets while l is below the last multiple of `sets` that
// fits in `laps`, and set l % sets in the laps behind it: the workgroup digest
// a healthy CU leaves is then the same for every g, which the record's
// comparison with one host digest per part needs. With `laps` a multiple of
// `sets` every lap is rotated by g.
//
// Pipeline. One K-step is 64 bytes of k of all 384 rows: 1,536 chunks of 16
// bytes, three global_load_dwordx4 per thread (thread t: rows t >> 2,
// 128 + (t >> 2) and 256 + (t >> 2), chunk t & 3). They land in registers and
// go from there into one of two LDS stages. The loads of step k + 1 are in
// flight while the 8 MFMAs of step k (2 k-halves x 4 accumulators) issue from
// the other stage; there is one barrier per step: a stage is written only
// after the barrier that follows its last read.
// LDS rows have a pitch of 80 bytes (64 + 16). An operand read is 128 bits
// per lane, lanes 0..31 on 32 consecutive rows at one column and lanes 32..63
// 16 bytes further. With 64 banks of 4 bytes a 128-bit access is served 16
// lanes at a time, 256 bytes; 80 / 16 = 5 is odd, so 16 consecutive rows start
// in 16 different groups of four banks: no conflict. (The staging writes, four
// chunks of each of 4 rows per 16 lanes, conflict two ways on 3 of 16 groups;
// there are 3 of them per thread and step against 8 reads.) The bank model is
// public CDNA3 material, assumed for CDNA4; no counter was read.
// Operand and C/D lane maps are those matrix_sweep.hip's header gives for i8.
// After the last step of a lap each lane loads its 64 expected words from the
// table, compares, folds the lap into the tallies and clears its accumulators.
//
// Parts (bit, name). The mask selects what is judged; the pipeline always
// runs, it is the load.
//   0 stage  every dword a thread received from the arena, before it goes to
//            LDS: sum of rotl32(word, i & 31), i the dword's index in its set.
//            The fold commutes and is keyed by i, so its expected value does
//            not depend on which thread moved what.
//   1 lds    every operand dword a wave reads back from LDS on its way into an
//            MFMA, same fold. An A dword is read by four waves, a Bt dword by
//            two: 4 sum(A) + 2 sum(Bt) per lap.
//   2 gemm   the accumulators: mismatches against the table are counted; the
//            digest is the sum of got (2 (256 row + col) + 1) over the laps.
//   3 valu   an integer chain per thread between the MFMAs: it starts at
//            fmix32(seed ^ 0x80000000 ^ thread) and per K-step runs
//            kLoadValuRounds times s = fmix32(s ^ (lap ksteps + step)); the
//            digest is the sum of s_final (2 t + 1). Not issued when the part
//            is not selected.
// A healthy gemm with a bad lds names the LDS; a bad gemm with good stage and
// lds names the matrix core.
//
// Record (128 bytes per workgroup): part_sweep.h's head with four parts, the
// reserved word and three ORed words: the sub-tiles that mis-compared (bit =
// sub-tile), the sets that did (bit = set & 31) and a mask over 32 equal spans
// of the launch's laps (bit = 32 lap / laps) in which a mismatch occurred: a
// fault that appears only late in a launch is what this sweep exists for.
// Injection: as in the other part sweeps, bit 0 of word 0 of the part is
// flipped in registers (stage, lds: dword 0 of the first set, in the fold
// only; gemm: C[0][0] of lap 0; valu: thread 0's s_final).
//
// Safety rules. Trip counts come from the kernel arguments only; no loop waits
// on a clock, a flag or another workgroup. No scratch, no spill, MODE is not
// written, results leave through vector stores. Arena and table are read-only;
// every index into them is below 384 K sets and 32,768 sets by construction.
//
// k_load_probe is the same device function with a dump: one workgroup at any
// shape stores C of every lap as [lap][128][256] int32 and behind it each
// thread's stage, lds and valu folds ([3][512]).
//
// NOT covered: formats other than i8 under load; HBM traffic (which cache
// level served a load is the hardware's choice); more than one launch; power,
// clocks and temperature, which are not observed.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <map>
#include <memory>
#include <mutex>
#include <tuple>
#include <vector>

#include "hip/part_sweep.h"

#define XS_ERR_BUF g_load_err
#define XS_HD __host__ __device__ __forceinline__
#define XS_D __device__ __forceinline__

namespace {

using namespace xsprobe;

ErrBuf g_load_err = "";

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));

constexpr int kNumParts = 4;
const char kPartNames[] = "stage,lds,gemm,valu";
constexpr uint32_t kAllParts = (1u << kNumParts) - 1;
constexpr int kStage = 0, kLds = 1, kGemm = 2, kValu = 3;
constexpr int kBlock = 512;  // 8 waves: two per SIMD
constexpr int kExtra = 3;    // sub-tile, set and span masks
constexpr int kUnswept = -1003;

// The sweep's fixed shape and defaults: measured in profiles/load_sweep_defaults.md.
constexpr uint32_t kLoadKsteps = 32, kLoadSets = 8;
constexpr uint32_t kLoadLaps = 1024;
constexpr uint32_t kLoadValuRounds = 2;
constexpr uint32_t kMaxLaps = 16 * kLoadLaps, kMaxKsteps = 1024, kMaxSets = 64;

constexpr uint32_t kRowsA = 128, kRowsB = 256, kRows = kRowsA + kRowsB;
constexpr uint32_t kStepBytes = 64;                  // of k, per row and K-step
constexpr uint32_t kPitch = 80;                      // LDS row: 64 + 16 bytes
constexpr uint32_t kStageBytes = kRows * kPitch;     // 30,720
constexpr uint32_t kTileWords = kRowsA * kRowsB;     // C of one set: 128 KiB
constexpr uint32_t kFoldWords = 3 * kBlock;          // the probe's per-thread folds
constexpr uint32_t kRedBytes = part_reduction_words<kBlock>(kNumParts, kExtra) * 4;
constexpr uint32_t kLdsUsed = 2 * kStageBytes > kRedBytes ? 2 * kStageBytes : kRedBytes;

XS_HD uint32_t operand_word(uint32_t seed, uint32_t set, uint32_t panel, uint32_t w) {
  return fmix32(seed ^ (set << 23 | panel << 22 | w));
}
XS_HD uint32_t chain_start(uint32_t seed, uint32_t t) { return fmix32(seed ^ 0x80000000u ^ t); }

struct LoadRecord {
  PartRecordHead<kNumParts> head;
  uint32_t reserved;
  uint32_t subtiles, sets, spans;
  uint32_t pad[15];
};
static_assert(sizeof(LoadRecord) == 128, "one 128-byte record per workgroup");

using Expect = PartExpect<kNumParts>;

struct LoadArgs {
  const uint8_t* arena;
  const int32_t* table;
  uint32_t part_mask, seed, laps, ksteps, sets;
};

// ------------------------------------------------------------------- device
// One workgroup's whole run. g: its rotation of the sets; inj: the parts to
// inject; dump: kDump only. Leaves the tallies and the three masks.
template <bool kDump>
XS_D void run_load(const LoadArgs& a, uint32_t g, uint32_t inj, int32_t* dump, uint8_t* lds, Tally (&y)[kNumParts],
                   uint32_t (&extra)[kExtra]) {
  const uint32_t t = threadIdx.x, lane = t & 63u, r = lane & 31u, h = lane >> 5;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const uint32_t ksteps = a.ksteps, laps = a.laps, sets = a.sets;
  const size_t K = static_cast<size_t>(kStepBytes) * ksteps;
  const uint32_t row_dwords = 16u * ksteps;
  const bool valu_on = (a.part_mask >> kValu) & 1u;

  // Staging: rows row0, row0 + 128, row0 + 256, chunk cc of the step's four.
  const uint32_t row0 = t >> 2, cc = t & 3u;
  const size_t g_off = row0 * K + cc * 16u;           // in a set, at step 0
  const uint32_t l_off = row0 * kPitch + cc * 16u;    // in a stage
  u32x4 stg[3];
  auto issue = [&](uint32_t set, uint32_t step) {
    const uint8_t* p = a.arena + set * (kRows * K) + g_off + step * kStepBytes;
#pragma unroll
    for (int j = 0; j < 3; ++j) stg[j] = *reinterpret_cast<const u32x4*>(p + j * (128u * K));
  };
  // Folds what `issue` brought for `step` and hands it to a stage. The three
  // rows are 128 apart, so their dword indices agree in the low five bits.
  auto fold_store = [&](uint32_t stage, uint32_t step, uint32_t flip) {
    const uint32_t s0 = 16u * ((row0 * ksteps + step) & 1u) + 4u * cc;
    uint32_t f = rotl(stg[0].x ^ flip, s0) - rotl(stg[0].x, s0);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      f += rotl(stg[j].x, s0) + rotl(stg[j].y, s0 + 1u) + rotl(stg[j].z, s0 + 2u) + rotl(stg[j].w, s0 + 3u);
      *reinterpret_cast<u32x4*>(lds + stage * kStageBytes + l_off + j * (128u * kPitch)) = stg[j];
    }
    y[kStage].digest += f;
    y[kStage].bad += flip;
  };

  i32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int q = 0; q < 16; ++q) acc[i][j][q] = 0;

  uint32_t chain = chain_start(a.seed, t);
  uint32_t lds_flip = ((inj >> kLds) & 1u) && t == 0;
  uint32_t lap = 0, step = 0, set = set_of(g, 0, laps, sets);
  uint32_t sub = wave & 7u;  // (wave + lap) & 7
  const uint32_t total = laps * ksteps;

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

    // Operand rows of this lap's sub-tile and the low bits of their dword indices.
    const uint32_t sr = sub >> 2, sc = sub & 3u;
    const uint8_t* st = lds + (gi & 1u) * kStageBytes + 16u * h;
    const uint32_t a_row = 64u * sr + r, b_row = kRowsA + 64u * sc + r;
    // Rows 32 apart and the A / Bt offset of 128 rows leave (row ksteps + step) & 1 that of r.
    const uint32_t s0 = 16u * ((r * ksteps + step) & 1u) + 4u * h;
    uint32_t f = 0;
#pragma unroll
    for (int kh = 0; kh < 2; ++kh) {
      i32x4 av[2], bv[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        av[i] = *reinterpret_cast<const i32x4*>(st + (a_row + 32u * i) * kPitch + 32u * kh);
        bv[i] = *reinterpret_cast<const i32x4*>(st + (b_row + 32u * i) * kPitch + 32u * kh);
      }
      if (kh == 0) {
        f += rotl(static_cast<uint32_t>(av[0].x) ^ lds_flip, s0) - rotl(static_cast<uint32_t>(av[0].x), s0);
        y[kLds].bad += lds_flip;
        lds_flip = 0;
      }
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const uint32_t s = s0 + 8u * kh;
        f += rotl(av[i].x, s) + rotl(av[i].y, s + 1u) + rotl(av[i].z, s + 2u) + rotl(av[i].w, s + 3u);
        f += rotl(bv[i].x, s) + rotl(bv[i].y, s + 1u) + rotl(bv[i].z, s + 2u) + rotl(bv[i].w, s + 3u);
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(av[i], bv[j], acc[i][j], 0, 0, 0);
      if (kh == 0 && valu_on) {
#pragma unroll
        for (uint32_t q = 0; q < kLoadValuRounds; ++q) chain = fmix32(chain ^ gi);
      }
    }
    y[kLds].digest += f;

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
            const uint32_t idx = row * kRowsB + 64u * sc + 32u * j + r;
            uint32_t got = static_cast<uint32_t>(acc[i][j][q]);
            if (i == 0 && j == 0 && q == 0 && ((inj >> kGemm) & 1u) && t == 0 && lap == 0) got ^= 1u;
            if constexpr (kDump) dump[static_cast<size_t>(lap) * kTileWords + idx] = static_cast<int32_t>(got);
            ne += got != static_cast<uint32_t>(want[idx]);
            d += got * (2u * idx + 1u);
            acc[i][j][q] = 0;
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

  if (((inj >> kValu) & 1u) && t == 0) chain ^= 1u, y[kValu].bad += 1u;
  if constexpr (kDump) {
    int32_t* folds = dump + static_cast<size_t>(laps) * kTileWords;
    folds[t] = static_cast<int32_t>(y[kStage].digest);
    folds[kBlock + t] = static_cast<int32_t>(y[kLds].digest);
    folds[2 * kBlock + t] = static_cast<int32_t>(chain);
  }
  y[kValu].digest = chain * (2u * t + 1u);
  // A part that is not selected leaves no tally: its digest in the record is 0.
#pragma unroll
  for (int p = 0; p < kNumParts; ++p)
    if (!((a.part_mask >> p) & 1u)) y[p] = Tally{};
  if (!((a.part_mask >> kGemm) & 1u)) extra[0] = extra[1] = extra[2] = 0;
}

__global__ __launch_bounds__(kBlock) void k_load_sweep(LoadRecord* __restrict__ records, LoadArgs a, int inject_xcd,
                                                      int inject_cu, uint32_t inject_parts, Expect expect) {
  extern __shared__ __attribute__((aligned(16))) uint8_t load_lds[];
  const uint32_t xcd = xcc_id();
  const uint32_t hw = hw_id();
  const uint32_t cu = cu_key(hw);
  const uint32_t simd = simd_id(hw);
  const bool inject = inject_selected(inject_xcd, inject_cu, xcd, cu);

  Tally y[kNumParts];
  uint32_t extra[kExtra] = {};
  run_load<false>(a, blockIdx.x, inject ? inject_parts & a.part_mask : 0u, nullptr, load_lds, y, extra);

  reduce_parts<kNumParts, kExtra, kBlock>(reinterpret_cast<uint32_t*>(load_lds), threadIdx.x, simd, y, extra,
                                          a.part_mask, expect, xcd, cu, &records[blockIdx.x]);
}

// One workgroup; dump holds laps x 32,768 words of C and 3 x 512 folds.
__global__ __launch_bounds__(kBlock) void k_load_probe(int32_t* __restrict__ dump, LoadArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t load_lds[];
  Tally y[kNumParts];
  uint32_t extra[kExtra] = {};
  run_load<true>(a, 0u, 0u, dump, load_lds, y, extra);
}

// --------------------------------------------------------------------- host
bool bad_shape(uint32_t laps, uint32_t ksteps, uint32_t sets) {
  return laps < 1 || laps > kMaxLaps || ksteps < 1 || ksteps > kMaxKsteps || sets < 1 || sets > kMaxSets;
}

// One set's bytes: 128 K of A, then 256 K of Bt.
void fill_set(uint32_t seed, uint32_t set, uint32_t ksteps, uint32_t* a_words, uint32_t* bt_words) {
  const uint32_t row_dwords = 16u * ksteps;
  for (uint32_t w = 0; w < kRowsA * row_dwords; ++w) a_words[w] = operand_word(seed, set, 0, w);
  for (uint32_t w = 0; w < kRowsB * row_dwords; ++w) bt_words[w] = operand_word(seed, set, 1, w);
}

uint32_t fold_of(const uint32_t* words, size_t first, size_t n) {
  uint32_t f = 0;
  for (size_t i = 0; i < n; ++i) f += rotl(words[i], static_cast<uint32_t>((first + i) & 31u));
  return f;
}

// What the host holds of a (seed, ksteps, sets): the arena's bytes, the table
// and, per set, the folds of its panels and the digest of its product.
struct HostSets {
  std::vector<uint32_t> arena;  // sets x 384 x 16 ksteps dwords
  std::vector<int32_t> table;   // sets x 128 x 256
  std::vector<uint32_t> fold_a, fold_bt, gemm;
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
  const size_t row_dwords = 16u * static_cast<size_t>(ksteps), K = 4 * row_dwords;
  const size_t a_dwords = kRowsA * row_dwords, set_dwords = kRows * row_dwords;
  hs.arena.resize(sets * set_dwords);
  hs.table.resize(static_cast<size_t>(sets) * kTileWords);
  for (uint32_t s = 0; s < sets; ++s) {
    uint32_t* aw = hs.arena.data() + s * set_dwords;
    uint32_t* bw = aw + a_dwords;
    fill_set(seed, s, ksteps, aw, bw);
    hs.fold_a.push_back(fold_of(aw, 0, a_dwords));
    hs.fold_bt.push_back(fold_of(bw, a_dwords, set_dwords - a_dwords));
    const int8_t* A = reinterpret_cast<const int8_t*>(aw);
    const int8_t* Bt = reinterpret_cast<const int8_t*>(bw);
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

// g_sets_mu held. The node agent sweeps with one seed and lap count again and again: the digests are kept.
uint32_t valu_digest(uint32_t seed, uint32_t laps, uint32_t ksteps) {
  static std::map<std::tuple<uint32_t, uint32_t, uint32_t>, uint32_t> known;
  const auto it = known.find({seed, laps, ksteps});
  if (it != known.end()) return it->second;
  uint32_t d = 0;
  for (uint32_t t = 0; t < kBlock; ++t) {
    uint32_t s = chain_start(seed, t);
    for (uint32_t gi = 0; gi < laps * ksteps; ++gi)
      for (uint32_t q = 0; q < kLoadValuRounds; ++q) s = fmix32(s ^ gi);
    d += s * (2u * t + 1u);
  }
  known[{seed, laps, ksteps}] = d;
  return d;
}

// The digests of a healthy workgroup; 0 for a part outside the mask.
void expected_digests(uint32_t mask, uint32_t seed, uint32_t laps, uint32_t ksteps, uint32_t sets, uint32_t* out) {
  std::lock_guard<std::mutex> g(g_sets_mu);
  const HostSets& hs = host_sets(seed, ksteps, sets);
  uint32_t d[kNumParts] = {};
  for (uint32_t l = 0; l < laps; ++l) {
    const uint32_t s = set_of(0, l, laps, sets);
    d[kStage] += hs.fold_a[s] + hs.fold_bt[s];
    d[kLds] += 4u * hs.fold_a[s] + 2u * hs.fold_bt[s];
    d[kGemm] += hs.gemm[s];
  }
  if ((mask >> kValu) & 1u) d[kValu] = valu_digest(seed, laps, ksteps);
  for (int p = 0; p < kNumParts; ++p) out[p] = (mask >> p) & 1u ? d[p] : 0u;
}

// Arena and table of (seed, ksteps, sets) on the current device `dev`, built
// and uploaded once. -1003 when either cannot be allocated: nothing is launched.
int device_sets(int dev, uint32_t seed, uint32_t ksteps, uint32_t sets, LoadArgs* a) {
  std::lock_guard<std::mutex> g(g_sets_mu);
  auto& slot = g_device_sets[{dev, seed, ksteps, sets}];
  if (!slot) {
    const HostSets& hs = host_sets(seed, ksteps, sets);
    auto ds = std::make_unique<DeviceSets>();
    const size_t arena_bytes = hs.arena.size() * 4, table_bytes = hs.table.size() * 4;
    void *arena = nullptr, *table = nullptr;
    const bool got = hipMalloc(&arena, arena_bytes) == hipSuccess && hipMalloc(&table, table_bytes) == hipSuccess;
    ds->arena.p = arena, ds->table.p = got ? table : nullptr;  // what was had is freed with ds
    if (!got) {
      (void)hipGetLastError();
      std::snprintf(g_load_err, sizeof g_load_err, "no arena of %zu and table of %zu bytes could be had: nothing was swept",
                    arena_bytes, table_bytes);
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

const char* xs_load_sweep_last_error() { return g_load_err; }

// Part names, comma-separated, in bit order.
const char* xs_load_parts() { return kPartNames; }

// out2 = {words whatever the laps, words per lap} of a part in the probe's
// dump: gemm has 32,768 per lap, the folds one per thread.
int xs_load_shape(int part, int* out2) {
  if (part < 0 || part >= kNumParts || !out2) return kBadArgs;
  out2[0] = part == kGemm ? 0 : kBlock;
  out2[1] = part == kGemm ? static_cast<int>(kTileWords) : 0;
  return 0;
}

// Host only. The bytes the arena holds for `set`: a_out[128][64 ksteps],
// bt_out[256][64 ksteps].
int xs_load_operands(uint32_t seed, uint32_t set, uint32_t ksteps, void* a_out, void* bt_out) {
  if (set >= kMaxSets || ksteps < 1 || ksteps > kMaxKsteps || !a_out || !bt_out) return kBadArgs;
  fill_set(seed, set, ksteps, static_cast<uint32_t*>(a_out), static_cast<uint32_t*>(bt_out));
  return 0;
}

// One workgroup at any shape; out = [laps][128][256] int32 of C, then
// [3][512]: every thread's stage fold, lds fold and final chain value.
// n_words = laps x 32,768 + 1,536. The mask selects whether the chain runs.
int xs_load_probe(int dev, uint32_t part_mask, uint32_t seed, uint32_t laps, uint32_t ksteps, uint32_t sets,
                  uint32_t* out, size_t n_words) {
  if (bad_part_mask(part_mask, kAllParts) || bad_shape(laps, ksteps, sets) || !out) return kBadArgs;
  const size_t n = static_cast<size_t>(laps) * kTileWords + kFoldWords;
  if (n_words != n) return kBadArgs;
  LoadArgs a{nullptr, nullptr, part_mask, seed, laps, ksteps, sets};
  return launch_probe(
      g_load_err, dev, reinterpret_cast<const void*>(k_load_probe), kBlock, kLdsUsed, out, n,
      [&](dim3 grid, dim3 block, size_t smem, void* dump) {
        hipLaunchKernelGGL(k_load_probe, grid, block, smem, 0, static_cast<int32_t*>(dump), a);
      },
      [&] { return device_sets(dev, seed, ksteps, sets, &a); });
}

// Host only. out4[p] = the workgroup digest a healthy CU leaves for part p at
// the sweep's shape, 0 for a part outside part_mask.
int xs_load_sweep_expected(uint32_t part_mask, uint32_t seed, uint32_t laps, uint32_t* out4) {
  if (bad_part_mask(part_mask, kAllParts) || bad_shape(laps, kLoadKsteps, kLoadSets) || !out4) return kBadArgs;
  expected_digests(part_mask, seed, laps, kLoadKsteps, kLoadSets, out4);
  return 0;
}

// What the runtime reports for k_load_sweep on `dev`: out4 = {registers per
// lane, scratch bytes per lane, dynamic LDS bytes per workgroup, workgroups
// that fit on a CU at once}.
int xs_load_sweep_info(int dev, int* out4) {
  return sweep_info(g_load_err, dev, reinterpret_cast<const void*>(k_load_sweep), kBlock, true, out4);
}

// One sweep launch of `blocks` workgroups (0: 4 per CU) of `laps` laps at the
// sweep's shape. Writes `blocks` 128-byte records to records_out. inject_xcd /
// inject_cu: -1 is none / any, values below -1 are refused. Returns 0, -1000
// for bad arguments and -1003 when arena or table could not be allocated
// (nothing is launched either way), or a negative HIP error.
int xs_load_sweep(int dev, int blocks, uint32_t part_mask, uint32_t seed, uint32_t laps, int inject_xcd, int inject_cu,
                  uint32_t inject_parts, void* records_out, int* n_records, double* ms) {
  if (bad_part_mask(part_mask, kAllParts) || bad_shape(laps, kLoadKsteps, kLoadSets) || (inject_parts & ~kAllParts))
    return kBadArgs;
  // launch_sweep refuses these too, but only after the host has built the sets.
  if (!records_out || blocks < 0 || blocks > kMaxBlocks || inject_xcd < -1 || inject_cu < -1 || inject_xcd > 15 ||
      inject_cu > 0xff)
    return kBadArgs;
  Expect e;
  expected_digests(part_mask, seed, laps, kLoadKsteps, kLoadSets, e.digest);
  LoadArgs a{nullptr, nullptr, part_mask, seed, laps, kLoadKsteps, kLoadSets};
  return launch_sweep(
      g_load_err, {dev, blocks, inject_xcd, inject_cu, records_out, n_records, ms},
      reinterpret_cast<const void*>(k_load_sweep), kBlock, kLdsUsed, sizeof(LoadRecord),
      [&](dim3 grid, dim3 block, size_t smem, void* rec) {
        hipLaunchKernelGGL(k_load_sweep, grid, block, smem, 0, static_cast<LoadRecord*>(rec), a, inject_xcd, inject_cu,
                           inject_parts, e);
      },
      [&] { return device_sets(dev, seed, kLoadKsteps, kLoadSets, &a); });
}

}  // extern "C"
