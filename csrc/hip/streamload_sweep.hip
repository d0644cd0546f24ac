// Stream load sweep for gfx950 (MI355X): every CU under load, with a checked
// int8 GEMM whose weights stream from memory straight into the matrix core.
//
// The other load sweeps (load_sweep.hip and its three siblings) hold every CU
// at rate on arenas of 5 to 6.4 MiB, far inside the 256 MiB Infinity Cache:
// under their load nothing draws on the HBM channels, the fabric between the
// XCDs and the memory dies, or a deep queue of outstanding vector loads. The
// HBM sweep reads DRAM at rate, with the matrix cores and the LDS idle.
// k_streamload_sweep is the state in between, that of inference decode: a
// skinny GEMM of 16 tokens whose every weight byte comes from a large arena,
// goes from the load's registers into v_mfma_i32_16x16x64_i8 and is not seen
// again by that wave. Int8 products are exact whatever the bits are, so every
// result of every lap is compared on the device by integer equality: the first
// 16x16 matrix form held to an exact value, and under load.
//
// The operation. Ct[n][m] = sum_k Wt[n][k] X[m][k], int8 operands, int32
// accumulators, 16 tokens m, K = 64 ksteps (ksteps 1..64, the sweep's default
// 64), |Ct| <= K 2^14 < 2^26. The weights are the A operand (16 rows n by 64 of
// k), the activations the B operand (64 of k by 16 tokens). With r = lane & 15
// and g = lane >> 4 a lane supplies 16 bytes of weight row r and 16 bytes of
// token r, both from k-slot g of the step. Slot g of A and slot g of B stand
// for the same k by the instruction's definition and the sum over k has no
// order, so which 16 of the step's 64 k a slot holds does not matter as long
// as A and B agree; no k-slot map is stated or needed. The C/D map is the
// 16x16 one of the ISA text: lane (c = lane & 15, g = lane >> 4), register i
// holds D[4 g + i][c], weight row 4 g + i and token c. k_streamload_probe's
// test pins it.
//
// Layout. A panel is 16 weight rows by K, 16 K bytes; the arena holds `panels`
// of them (a multiple of 8, at least 8, at most 2^28 dwords in all), pre-tiled
// so that one wave-step is one contiguous KiB:
//   byte of Wt[n][k]: ((n >> 4) ksteps + (k >> 6)) 1024 + ((k >> 4) & 3) 256
//                     + (n & 15) 16 + (k & 15)
// Lane L reads bytes 16 L .. 16 L + 15 of the step's KiB with one
// global_load_dwordx4, and what arrives is the MFMA's A operand: the weights
// never touch LDS. X[16][K] is tiled the same way, (k >> 6) 1024 +
// ((k >> 4) & 3) 256 + m 16 + (k & 15). Dword w of the arena is
// fmix32(seed ^ w), dword w of X is fmix32(seed ^ 0x40000000 ^ w) (fmix32:
// part_sweep.h); -128 occurs; there is one X per launch.
//
// Work split and pipeline. A workgroup is 512 threads, two waves on every
// SIMD, and asks for exclusive_lds(), so no two share a CU. It brings X (at
// most 64 KiB) into LDS once, tiled; every later LDS read is lane-linear, a
// ds_read_b128 at step 1024 + lane 16, free of bank conflicts under any bank
// model. Per lap wave w owns one panel and streams it. Each wave runs a
// register ring of kDepth outstanding global_load_dwordx4 on a global step
// index that runs across lap boundaries: the loads of the first steps of lap
// l + 1 are in flight while the last steps of lap l issue their MFMAs, and
// with ksteps < kDepth the ring reaches more than one lap ahead. The ring is
// plain C++ whose indices are compile-time (the loop is unrolled kDepth
// times), consumed oldest first with nothing else on the vector memory
// counter, so the compiler releases a slot with s_waitcnt vmcnt(kDepth - 1).
// To keep it so, the 256 expected words of a lap's panel ride the ring as its
// step number `ksteps`: a lap is ksteps weight steps and one table step, all
// of one KiB per wave, and no load is ever issued under a condition. The slots
// issued past the last lap re-read the arena's first KiB and are not consumed.
// A weight step is one LDS read, one MFMA and the folds; at the table step
// each lane compares its 4 accumulators with the slot by integer equality and
// clears them. After the X load there is no barrier until the record is
// reduced, no split-K, and no wave waits on another workgroup.
//
// Which panel when. R = panels / 8 laps make a round. While lap l is below the
// last multiple of R that fits in `laps`, workgroup g takes panel group
// (l + off(g)) % R with off(g) = (g 40503) % R, in the laps behind that group
// l % R; wave w takes panel 8 group + w. Over a full round every workgroup
// reads the whole arena once, so a healthy CU's digests do not depend on g,
// which the record's comparison with one host digest per part needs (the same
// departure for a partial tail as load_sweep.hip's). The multiplier is meant
// to spread concurrent workgroups over the arena; how well it does is not
// observed.
//
// Parts (bit, name). The mask selects what is judged; the pipeline always
// runs, and the folds of a part that is not selected are not issued.
//   0 stage  every weight dword as it arrived in registers: sum of
//            rotl32(word, i & 31), i its dword index in the arena. HBM,
//            fabric, L2, L1, VGPR.
//   1 act    every X dword a wave reads from LDS on its way into the MFMA,
//            same fold by X index: 8 sum(X) per lap.
//   2 gemm   mismatches against the table are counted; the digest is the sum
//            of uint32(got) (2 (256 panel + 16 n + m) + 1).
// A bad gemm with good stage and act names the 16x16 int8 path of the matrix
// core; a bad stage names the path from memory.
//
// Record (128 bytes per workgroup): part_sweep.h's head with three parts, the
// reserved word and the load sweep's three ORed words: the waves that
// mis-compared (bit = wave), the panels that did (bit = panel & 31) and the 32
// equal spans of the launch's laps in which one did. Injection: bit 0 of word
// 0 of the part is flipped in registers (stage, act: thread 0's first dword,
// in the fold only; gemm: wave 0's Ct[0][0] of lap 0).
//
// Safety rules. Trip counts come from the kernel arguments only; no loop waits
// on a clock, a flag or another workgroup. No scratch, no spill, MODE is not
// written, results leave through vector stores. Arena, X and table are
// read-only; every arena index is below panels 16 K and every table index
// below 1,024 panels by construction (group < R, wave < 8, step < ksteps).
//
// Host. The arena is large (STREAMLOAD_PANELS in profiles/
// streamload_sweep_defaults.md), so the host never holds it: it is generated
// chunk by chunk on at most 16 threads and uploaded through one pinned staging
// buffer, and while a panel's bytes are at hand its 16x16 block of Ct (plain
// int32) and its fold are taken. The table (1 KiB per panel, in the order the
// lanes hold it: word 4 lane + i) and the per-panel digests are cached per
// (seed, ksteps, panels) for the life of the process; arena, X and table on
// the device are allocated per call and freed after it: the agent does not sit
// on a GiB of a tenant's HBM between sweeps.
//
// k_streamload_probe is the same device function with a dump: one workgroup at
// any legal shape stores Ct of every lap as [lap][128][16] int32, wave w's
// panel at rows 16 w .., and behind it each thread's stage and act folds
// ([2][512]).
//
// NOT covered: token counts other than 16; fp8 or MX weights on this path;
// split-K; writes to HBM under load; xGMI traffic; more than one launch. Which
// level of the memory hierarchy served a load is the hardware's choice and is
// not observed; power, clocks and temperature are not observed.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <map>
#include <memory>
#include <mutex>
#include <thread>
#include <tuple>
#include <vector>

#include "hip/part_sweep.h"

#define XS_ERR_BUF g_stream_err
#define XS_HD __host__ __device__ __forceinline__
#define XS_D __device__ __forceinline__

// The ring's depth and whether its loads are nontemporal: measured in
// profiles/streamload_sweep_defaults.md (16 gains 0.5% for 31 registers; nt is
// 1.7% slower on a DRAM-sized arena and 8% on a cache-sized one, because other
// workgroups re-read what a wave streams); a build may override them to
// measure again.
#ifndef XS_STREAMLOAD_DEPTH
#define XS_STREAMLOAD_DEPTH 8
#endif
#ifndef XS_STREAMLOAD_NT
#define XS_STREAMLOAD_NT 0
#endif

namespace {

using namespace xsprobe;

ErrBuf g_stream_err = "";

typedef int i32x4 __attribute__((ext_vector_type(4)));

constexpr int kNumParts = 3;
const char kPartNames[] = "stage,act,gemm";
constexpr uint32_t kAllParts = (1u << kNumParts) - 1;
constexpr int kStage = 0, kAct = 1, kGemm = 2;
constexpr int kBlock = 512;  // 8 waves: two per SIMD
constexpr int kWaves = kBlock / 64;
constexpr int kExtra = 3;  // wave, panel and span masks
constexpr int kUnswept = -1003;
constexpr int kDepth = XS_STREAMLOAD_DEPTH;
constexpr bool kNontemporal = XS_STREAMLOAD_NT != 0;

// The sweep's defaults: measured in profiles/streamload_sweep_defaults.md.
constexpr uint32_t kStreamKsteps = 64, kStreamPanels = 16384;  // K = 4,096; 1 GiB
constexpr uint32_t kStreamLaps = kStreamPanels / kWaves;      // one round
constexpr uint32_t kMaxLaps = 16 * kStreamLaps, kMaxKsteps = 64;
constexpr size_t kMaxArenaDwords = size_t{1} << 28;  // the hash's key is 28 bits of index

constexpr uint32_t kTokens = 16, kPanelRows = 16;
constexpr uint32_t kStepBytes = 1024, kStepDwords = 256;   // one wave-step: 16 rows x 64 of k
constexpr uint32_t kTileWords = kPanelRows * kTokens;      // Ct of one panel: 1 KiB
constexpr uint32_t kLapWords = kWaves * kTileWords;        // the probe's [128][16] per lap
constexpr uint32_t kFoldWords = 2 * kBlock;                // the probe's per-thread folds
constexpr uint32_t kXKey = 0x40000000u;
constexpr uint32_t kSpread = 40503u;
constexpr size_t kChunkBytes = size_t{32} << 20;  // the staging buffer
constexpr uint32_t kRedBytes = part_reduction_words<kBlock>(kNumParts, kExtra) * 4;
constexpr uint32_t kLdsUsed = kMaxKsteps * kStepBytes > kRedBytes ? kMaxKsteps * kStepBytes : kRedBytes;

struct StreamRecord {
  PartRecordHead<kNumParts> head;
  uint32_t reserved;
  uint32_t waves, panels, spans;
  uint32_t pad[17];
};
static_assert(sizeof(StreamRecord) == 128, "one 128-byte record per workgroup");

using Expect = PartExpect<kNumParts>;

struct StreamArgs {
  const uint8_t* arena;
  const uint8_t* x;
  const uint8_t* table;
  uint32_t part_mask, seed, laps, ksteps, panels;
};

// The panel group workgroup g starts with, and where a wave stands in its stream.
XS_HD uint32_t group_offset(uint32_t g, uint32_t rounds_len) {
  return static_cast<uint32_t>(static_cast<uint64_t>(g) * kSpread % rounds_len);
}
struct Cursor {
  uint32_t lap, step, group;  // step == ksteps: the lap's table step
};

// ------------------------------------------------------------------- device
XS_D u32x4 ring_load(const uint8_t* p) {
  const u32x4* q = reinterpret_cast<const u32x4*>(p);
  if constexpr (kNontemporal) return __builtin_nontemporal_load(q);
  return *q;
}

XS_D uint32_t fold4(const u32x4& v, uint32_t s0) {
  return rotl(v.x, s0) + rotl(v.y, s0 + 1u) + rotl(v.z, s0 + 2u) + rotl(v.w, s0 + 3u);
}

// One workgroup's whole run. g: its rotation of the panel groups; inj: the
// parts to inject; dump: kDump only. Leaves the tallies and the three masks.
template <bool kDump>
XS_D void run_stream(const StreamArgs& a, uint32_t g, uint32_t inj, int32_t* dump, uint8_t* lds, Tally (&y)[kNumParts],
                     uint32_t (&extra)[kExtra]) {
  const uint32_t t = threadIdx.x, lane = t & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const uint32_t ksteps = a.ksteps, laps = a.laps;
  const uint32_t R = a.panels / kWaves, full = laps - laps % R;
  const bool stage_on = (a.part_mask >> kStage) & 1u, act_on = (a.part_mask >> kAct) & 1u;

  // X into LDS, once, as it lies in memory.
  for (uint32_t v = t; v < 64u * ksteps; v += kBlock)
    reinterpret_cast<u32x4*>(lds)[v] = reinterpret_cast<const u32x4*>(a.x)[v];
  __syncthreads();

  const uint32_t lane_off = 16u * lane;
  const uint32_t s0 = (4u * lane) & 31u;  // a step is 256 dwords: the index's low five bits are the lane's
  auto advance = [&](Cursor& c) {
    if (++c.step > ksteps) {
      c.step = 0;
      ++c.lap;
      c.group = c.group + 1u == R ? 0u : c.group + 1u;
      if (c.lap == full) c.group = 0;  // full is a multiple of R: l % R from here on
    }
  };
  auto address = [&](const Cursor& c) -> const uint8_t* {
    const size_t panel = static_cast<size_t>(kWaves) * c.group + wave;
    size_t off = 0;  // past the last lap: the arena's first KiB, not consumed
    const uint8_t* base = a.arena;
    if (c.lap < laps) {
      if (c.step < ksteps) {
        off = (panel * ksteps + c.step) * kStepBytes;
      } else {
        base = a.table;
        off = panel * (kTileWords * 4u);
      }
    }
    return base + off + lane_off;
  };

  Cursor ic{0u, 0u, full ? group_offset(g, R) : 0u};
  Cursor cc = ic;
  u32x4 ring[kDepth];
#pragma unroll
  for (int j = 0; j < kDepth; ++j) {
    ring[j] = ring_load(address(ic));
    advance(ic);
  }

  i32x4 acc = {0, 0, 0, 0};
  uint32_t stage_flip = ((inj >> kStage) & 1u) && t == 0;
  uint32_t act_flip = ((inj >> kAct) & 1u) && t == 0;
  const uint32_t total = laps * (ksteps + 1u);

#pragma nounroll
  for (uint32_t base = 0; base < total; base += kDepth) {
#pragma unroll
    for (int j = 0; j < kDepth; ++j) {
      const u32x4 v = ring[j];
      if (cc.lap < laps) {
        if (cc.step < ksteps) {
          const i32x4 xv = *reinterpret_cast<const i32x4*>(lds + cc.step * kStepBytes + lane_off);
          if (stage_on) {
            y[kStage].digest += fold4(v, s0) + rotl(v.x ^ stage_flip, s0) - rotl(v.x, s0);
            y[kStage].bad += stage_flip;
            stage_flip = 0;
          }
          if (act_on) {
            const u32x4 xu = {static_cast<uint32_t>(xv.x), static_cast<uint32_t>(xv.y), static_cast<uint32_t>(xv.z),
                              static_cast<uint32_t>(xv.w)};
            y[kAct].digest += fold4(xu, s0) + rotl(xu.x ^ act_flip, s0) - rotl(xu.x, s0);
            y[kAct].bad += act_flip;
            act_flip = 0;
          }
          const i32x4 wv = {static_cast<int>(v.x), static_cast<int>(v.y), static_cast<int>(v.z),
                            static_cast<int>(v.w)};
          acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(wv, xv, acc, 0, 0, 0);
        } else {  // the lap is complete: v holds the lane's four expected words
          const uint32_t panel = kWaves * cc.group + wave;
          const uint32_t c = lane & 15u, n0 = 4u * (lane >> 4);
          uint32_t ne = 0, d = 0;
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            uint32_t got = static_cast<uint32_t>(acc[i]);
            if (i == 0 && ((inj >> kGemm) & 1u) && t == 0 && cc.lap == 0) got ^= 1u;
            const uint32_t idx = kTokens * (n0 + i) + c;
            if constexpr (kDump)
              dump[static_cast<size_t>(cc.lap) * kLapWords + wave * kTileWords + idx] = static_cast<int32_t>(got);
            ne += got != v[i];
            d += got * (2u * (kTileWords * panel + idx) + 1u);
            acc[i] = 0;
          }
          y[kGemm].bad += ne;
          y[kGemm].digest += d;
          if (ne) {
            extra[0] |= 1u << wave;
            extra[1] |= 1u << (panel & 31u);
            extra[2] |= 1u << (32u * cc.lap / laps);
          }
        }
      }
      advance(cc);
      ring[j] = ring_load(address(ic));
      advance(ic);
    }
  }

  if constexpr (kDump) {
    int32_t* folds = dump + static_cast<size_t>(laps) * kLapWords;
    folds[t] = static_cast<int32_t>(y[kStage].digest);
    folds[kBlock + t] = static_cast<int32_t>(y[kAct].digest);
  }
  // A part that is not selected leaves no tally: its digest in the record is 0.
#pragma unroll
  for (int p = 0; p < kNumParts; ++p)
    if (!((a.part_mask >> p) & 1u)) y[p] = Tally{};
  if (!((a.part_mask >> kGemm) & 1u)) extra[0] = extra[1] = extra[2] = 0;
}

__global__ __launch_bounds__(kBlock) void k_streamload_sweep(StreamRecord* __restrict__ records, StreamArgs a,
                                                            int inject_xcd, int inject_cu, uint32_t inject_parts,
                                                            Expect expect) {
  extern __shared__ __attribute__((aligned(16))) uint8_t stream_lds[];
  const uint32_t xcd = xcc_id();
  const uint32_t hw = hw_id();
  const uint32_t cu = cu_key(hw);
  const uint32_t simd = simd_id(hw);
  const bool inject = inject_selected(inject_xcd, inject_cu, xcd, cu);

  Tally y[kNumParts];
  uint32_t extra[kExtra] = {};
  run_stream<false>(a, blockIdx.x, inject ? inject_parts & a.part_mask : 0u, nullptr, stream_lds, y, extra);

  reduce_parts<kNumParts, kExtra, kBlock>(reinterpret_cast<uint32_t*>(stream_lds), threadIdx.x, simd, y, extra,
                                          a.part_mask, expect, xcd, cu, &records[blockIdx.x]);
}

// One workgroup; dump holds laps x 2,048 words of Ct and 2 x 512 folds.
__global__ __launch_bounds__(kBlock) void k_streamload_probe(int32_t* __restrict__ dump, StreamArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t stream_lds[];
  Tally y[kNumParts];
  uint32_t extra[kExtra] = {};
  run_stream<true>(a, 0u, 0u, dump, stream_lds, y, extra);
}

// --------------------------------------------------------------------- host
bool bad_shape(uint32_t laps, uint32_t ksteps, uint32_t panels) {
  return laps < 1 || laps > kMaxLaps || ksteps < 1 || ksteps > kMaxKsteps || panels < kWaves || panels % kWaves ||
         static_cast<size_t>(panels) * ksteps * kStepDwords > kMaxArenaDwords;
}

// fn(i) for i in [0, n) on at most 16 threads.
template <typename F>
void on_threads(size_t n, F&& fn) {
  const size_t hw = std::max(1u, std::thread::hardware_concurrency());
  const size_t nt = std::min<size_t>({16, hw, n});
  if (nt <= 1) {
    for (size_t i = 0; i < n; ++i) fn(i);
    return;
  }
  std::vector<std::thread> pool;
  for (size_t k = 0; k < nt; ++k)
    pool.emplace_back([&, k] {
      for (size_t i = n * k / nt; i < n * (k + 1) / nt; ++i) fn(i);
    });
  for (auto& th : pool) th.join();
}

void fill_words(uint32_t key, size_t first, size_t n, uint32_t* out) {
  for (size_t i = 0; i < n; ++i) out[i] = fmix32(key ^ static_cast<uint32_t>(first + i));
}

uint32_t fold_of(const uint32_t* words, size_t first, size_t n) {
  uint32_t f = 0;
  for (size_t i = 0; i < n; ++i) f += rotl(words[i], static_cast<uint32_t>((first + i) & 31u));
  return f;
}

// What the host keeps of a (seed, ksteps, panels): X, the table and, per
// panel, the fold of its bytes and the digest of its block of Ct.
struct HostTable {
  std::vector<uint32_t> x;     // 256 ksteps dwords, tiled
  std::vector<int32_t> table;  // panels x 256, word 4 lane + i
  std::vector<uint32_t> fold, gemm;
  uint32_t fold_x = 0;
};

// The 16x16 block of Ct of one tiled panel against the tiled X, in plain
// int32, into `row` (lane order) with its digest.
void tabulate_panel(const uint32_t* words, const HostTable& ht, uint32_t ksteps, uint32_t panel, int32_t* row,
                    uint32_t* digest) {
  const int8_t* w = reinterpret_cast<const int8_t*>(words);
  const int8_t* x = reinterpret_cast<const int8_t*>(ht.x.data());
  int32_t c[kPanelRows][kTokens] = {};
  for (uint32_t slot = 0; slot < 4u * ksteps; ++slot) {  // 16 of k of all rows and tokens: 256 bytes of each
    const int8_t* ws = w + 256u * slot;
    const int8_t* xs = x + 256u * slot;
    for (uint32_t n = 0; n < kPanelRows; ++n)
      for (uint32_t m = 0; m < kTokens; ++m) {
        int32_t s = 0;
        for (uint32_t k = 0; k < 16; ++k) s += static_cast<int32_t>(ws[16 * n + k]) * static_cast<int32_t>(xs[16 * m + k]);
        c[n][m] += s;
      }
  }
  uint32_t d = 0;
  for (uint32_t n = 0; n < kPanelRows; ++n)
    for (uint32_t m = 0; m < kTokens; ++m) {
      const uint32_t lane = 16u * (n >> 2) + m;
      row[4u * lane + (n & 3u)] = c[n][m];
      d += static_cast<uint32_t>(c[n][m]) * (2u * (kTileWords * panel + kTokens * n + m) + 1u);
    }
  *digest = d;
}

void start_table(HostTable* ht, uint32_t seed, uint32_t ksteps, uint32_t panels) {
  ht->x.resize(static_cast<size_t>(kStepDwords) * ksteps);
  fill_words(seed ^ kXKey, 0, ht->x.size(), ht->x.data());
  ht->fold_x = fold_of(ht->x.data(), 0, ht->x.size());
  ht->table.resize(static_cast<size_t>(panels) * kTileWords);
  ht->fold.resize(panels);
  ht->gemm.resize(panels);
}

// The arena chunk by chunk through `stage` (room for `chunk_panels` panels):
// every chunk is generated on the threads, tabulated into *tab unless that is
// null, and handed to sink(first dword, dwords), whose error ends the walk.
template <typename Sink>
int walk_arena(uint32_t seed, uint32_t ksteps, uint32_t panels, uint32_t* stage, size_t chunk_panels, HostTable* tab,
               Sink&& sink) {
  const size_t panel_dwords = static_cast<size_t>(kStepDwords) * ksteps;
  for (size_t first = 0; first < panels; first += chunk_panels) {
    const size_t n = std::min<size_t>(chunk_panels, panels - first);
    on_threads(n, [&](size_t i) {
      const size_t p = first + i;
      uint32_t* words = stage + i * panel_dwords;
      fill_words(seed, p * panel_dwords, panel_dwords, words);
      if (!tab) return;
      tab->fold[p] = fold_of(words, p * panel_dwords, panel_dwords);
      tabulate_panel(words, *tab, ksteps, static_cast<uint32_t>(p), tab->table.data() + p * kTileWords, &tab->gemm[p]);
    });
    if (int rc = sink(first * panel_dwords, n * panel_dwords)) return rc;
  }
  return 0;
}

size_t chunk_panels_of(uint32_t ksteps, uint32_t panels) {
  return std::min<size_t>(panels, kChunkBytes / (static_cast<size_t>(kStepBytes) * ksteps));
}

std::mutex g_tables_mu;
std::map<std::tuple<uint32_t, uint32_t, uint32_t>, std::unique_ptr<HostTable>> g_tables;

// g_tables_mu held. The table of (seed, ksteps, panels), built without a device when it is not known yet.
const HostTable& host_table(uint32_t seed, uint32_t ksteps, uint32_t panels) {
  auto& slot = g_tables[{seed, ksteps, panels}];
  if (slot) return *slot;
  auto ht = std::make_unique<HostTable>();
  start_table(ht.get(), seed, ksteps, panels);
  const size_t chunk = chunk_panels_of(ksteps, panels);
  std::vector<uint32_t> stage(chunk * kStepDwords * ksteps);
  walk_arena(seed, ksteps, panels, stage.data(), chunk, ht.get(), [](size_t, size_t) { return 0; });
  slot = std::move(ht);
  return *slot;
}

// g_tables_mu held. The digests of a healthy workgroup; 0 for a part outside the mask.
void expected_digests(const HostTable& ht, uint32_t mask, uint32_t laps, uint32_t panels, uint32_t* out) {
  const uint32_t R = panels / kWaves;
  uint32_t d[kNumParts] = {};
  for (uint32_t l = 0; l < laps; ++l)  // workgroup 0: group l % R in every lap
    for (uint32_t w = 0; w < kWaves; ++w) {
      d[kStage] += ht.fold[kWaves * (l % R) + w];
      d[kGemm] += ht.gemm[kWaves * (l % R) + w];
    }
  d[kAct] = laps * kWaves * ht.fold_x;
  for (int p = 0; p < kNumParts; ++p) out[p] = (mask >> p) & 1u ? d[p] : 0u;
}

struct PinnedMem {
  void* p = nullptr;
  PinnedMem() = default;
  PinnedMem(const PinnedMem&) = delete;
  PinnedMem& operator=(const PinnedMem&) = delete;
  ~PinnedMem() {
    if (p) (void)hipHostFree(p);
  }
};

// Arena, X and table of one call on the current device; freed with it.
struct DeviceArena {
  DevMem arena, x, table;
};

// Allocates and fills *da for (seed, ksteps, panels), points *a at it and
// leaves the digests of `mask` at `laps` in *e. The first call of a (seed,
// ksteps, panels) builds the table while the chunks go by. -1003 when arena,
// table or staging cannot be had: nothing is launched.
int device_arena(DeviceArena* da, uint32_t seed, uint32_t ksteps, uint32_t panels, uint32_t mask, uint32_t laps,
                 StreamArgs* a, Expect* e) {
  std::lock_guard<std::mutex> g(g_tables_mu);
  const size_t panel_dwords = static_cast<size_t>(kStepDwords) * ksteps;
  const size_t arena_bytes = panels * panel_dwords * 4, x_bytes = panel_dwords * 4;
  const size_t table_bytes = static_cast<size_t>(panels) * kTileWords * 4;
  const size_t chunk = chunk_panels_of(ksteps, panels);
  PinnedMem stage;
  const bool got = hipMalloc(&da->arena.p, arena_bytes) == hipSuccess && hipMalloc(&da->x.p, x_bytes) == hipSuccess &&
                   hipMalloc(&da->table.p, table_bytes) == hipSuccess &&
                   hipHostMalloc(&stage.p, chunk * panel_dwords * 4, hipHostMallocDefault) == hipSuccess;
  if (!got) {
    (void)hipGetLastError();
    std::snprintf(g_stream_err, sizeof g_stream_err,
                  "no arena of %zu and table of %zu bytes could be had: nothing was swept", arena_bytes, table_bytes);
    return kUnswept;
  }
  auto& slot = g_tables[{seed, ksteps, panels}];
  std::unique_ptr<HostTable> fresh;
  if (!slot) {
    fresh = std::make_unique<HostTable>();
    start_table(fresh.get(), seed, ksteps, panels);
  }
  uint8_t* dst = da->arena.as<uint8_t>();
  const uint32_t* src = static_cast<const uint32_t*>(stage.p);
  if (int rc = walk_arena(seed, ksteps, panels, static_cast<uint32_t*>(stage.p), chunk, fresh.get(),
                          [&](size_t first_dword, size_t dwords) {
                            XS_CHECK(hipMemcpy(dst + first_dword * 4, src, dwords * 4, hipMemcpyHostToDevice));
                            return 0;
                          }))
    return rc;
  if (fresh) slot = std::move(fresh);
  XS_CHECK(hipMemcpy(da->x.p, slot->x.data(), x_bytes, hipMemcpyHostToDevice));
  XS_CHECK(hipMemcpy(da->table.p, slot->table.data(), table_bytes, hipMemcpyHostToDevice));
  a->arena = da->arena.as<const uint8_t>();
  a->x = da->x.as<const uint8_t>();
  a->table = da->table.as<const uint8_t>();
  expected_digests(*slot, mask, laps, panels, e->digest);
  return 0;
}

}  // namespace

extern "C" {

const char* xs_streamload_sweep_last_error() { return g_stream_err; }

// Part names, comma-separated, in bit order.
const char* xs_streamload_parts() { return kPartNames; }

// out2 = {words whatever the laps, words per lap} of a part in the probe's
// dump: gemm has 2,048 per lap, the folds one per thread.
int xs_streamload_shape(int part, int* out2) {
  if (part < 0 || part >= kNumParts || !out2) return kBadArgs;
  out2[0] = part == kGemm ? 0 : kBlock;
  out2[1] = part == kGemm ? static_cast<int>(kLapWords) : 0;
  return 0;
}

// Host only. The bytes the arena holds for `panel` and those of X, untiled:
// wt_out[16][64 ksteps], x_out[16][64 ksteps].
int xs_streamload_operands(uint32_t seed, uint32_t panel, uint32_t ksteps, void* wt_out, void* x_out) {
  if (ksteps < 1 || ksteps > kMaxKsteps || !wt_out || !x_out) return kBadArgs;
  const size_t panel_dwords = static_cast<size_t>(kStepDwords) * ksteps, K = 64u * static_cast<size_t>(ksteps);
  if ((static_cast<size_t>(panel) + 1) * panel_dwords > kMaxArenaDwords) return kBadArgs;
  std::vector<uint32_t> w(panel_dwords), x(panel_dwords);
  fill_words(seed, panel * panel_dwords, panel_dwords, w.data());
  fill_words(seed ^ kXKey, 0, panel_dwords, x.data());
  const uint8_t* wb = reinterpret_cast<const uint8_t*>(w.data());
  const uint8_t* xb = reinterpret_cast<const uint8_t*>(x.data());
  for (size_t r = 0; r < kPanelRows; ++r)
    for (size_t k = 0; k < K; ++k) {
      const size_t at = (k >> 6) * kStepBytes + ((k >> 4) & 3u) * 256u + r * 16u + (k & 15u);
      static_cast<uint8_t*>(wt_out)[r * K + k] = wb[at];
      static_cast<uint8_t*>(x_out)[r * K + k] = xb[at];
    }
  return 0;
}

// One workgroup at any legal shape on an arena of its own; out = [laps][128][16]
// int32 of Ct, wave w's panel at rows 16 w .., then [2][512]: every thread's
// stage and act fold. n_words = laps x 2,048 + 1,024. The mask selects which
// folds are issued.
int xs_streamload_probe(int dev, uint32_t part_mask, uint32_t seed, uint32_t laps, uint32_t ksteps, uint32_t panels,
                        uint32_t* out, size_t n_words) {
  if (bad_part_mask(part_mask, kAllParts) || bad_shape(laps, ksteps, panels) || !out) return kBadArgs;
  const size_t n = static_cast<size_t>(laps) * kLapWords + kFoldWords;
  if (n_words != n) return kBadArgs;
  StreamArgs a{nullptr, nullptr, nullptr, part_mask, seed, laps, ksteps, panels};
  DeviceArena da;
  Expect e;
  return launch_probe(
      g_stream_err, dev, reinterpret_cast<const void*>(k_streamload_probe), kBlock, kLdsUsed, out, n,
      [&](dim3 grid, dim3 block, size_t smem, void* dump) {
        hipLaunchKernelGGL(k_streamload_probe, grid, block, smem, 0, static_cast<int32_t*>(dump), a);
      },
      [&] { return device_arena(&da, seed, ksteps, panels, part_mask, laps, &a, &e); });
}

// Host only. out3[p] = the workgroup digest a healthy CU leaves for part p, 0
// for a part outside part_mask. The first call of a (seed, ksteps, panels)
// generates the whole arena once, chunk by chunk.
int xs_streamload_sweep_expected(uint32_t part_mask, uint32_t seed, uint32_t laps, uint32_t ksteps, uint32_t panels,
                                 uint32_t* out3) {
  if (bad_part_mask(part_mask, kAllParts) || bad_shape(laps, ksteps, panels) || !out3) return kBadArgs;
  std::lock_guard<std::mutex> g(g_tables_mu);
  expected_digests(host_table(seed, ksteps, panels), part_mask, laps, panels, out3);
  return 0;
}

// What the runtime reports for k_streamload_sweep on `dev`: out4 = {registers
// per lane, scratch bytes per lane, dynamic LDS bytes per workgroup,
// workgroups that fit on a CU at once}.
int xs_streamload_sweep_info(int dev, int* out4) {
  return sweep_info(g_stream_err, dev, reinterpret_cast<const void*>(k_streamload_sweep), kBlock, true, out4);
}

// One sweep launch of `blocks` workgroups (0: 4 per CU) of `laps` laps over an
// arena of `panels` panels of K = 64 ksteps (the sweep's: 64 and
// STREAMLOAD_PANELS; smaller ones are for tests). Writes `blocks` 128-byte
// records to records_out. inject_xcd / inject_cu: -1 is none / any, values
// below -1 are refused. Returns 0, -1000 for bad arguments and -1003 when
// arena or table could not be allocated (nothing is launched either way), or a
// negative HIP error. What it allocated on the device is freed before it returns.
int xs_streamload_sweep(int dev, int blocks, uint32_t part_mask, uint32_t seed, uint32_t laps, uint32_t ksteps,
                        uint32_t panels, int inject_xcd, int inject_cu, uint32_t inject_parts, void* records_out,
                        int* n_records, double* ms) {
  if (bad_part_mask(part_mask, kAllParts) || bad_shape(laps, ksteps, panels) || (inject_parts & ~kAllParts))
    return kBadArgs;
  // launch_sweep refuses these too, but only after the host has built the arena.
  if (!records_out || blocks < 0 || blocks > kMaxBlocks || inject_xcd < -1 || inject_cu < -1 || inject_xcd > 15 ||
      inject_cu > 0xff)
    return kBadArgs;
  StreamArgs a{nullptr, nullptr, nullptr, part_mask, seed, laps, ksteps, panels};
  DeviceArena da;
  Expect e;
  return launch_sweep(
      g_stream_err, {dev, blocks, inject_xcd, inject_cu, records_out, n_records, ms},
      reinterpret_cast<const void*>(k_streamload_sweep), kBlock, kLdsUsed, sizeof(StreamRecord),
      [&](dim3 grid, dim3 block, size_t smem, void* rec) {
        hipLaunchKernelGGL(k_streamload_sweep, grid, block, smem, 0, static_cast<StreamRecord*>(rec), a, inject_xcd,
                           inject_cu, inject_parts, e);
      },
      [&] { return device_arena(&da, seed, ksteps, panels, part_mask, laps, &a, &e); });
}

}  // extern "C"
