// CU sweep for gfx950 (MI355X): the node agent's per-CU compute check.
//
// xs_mfma_check runs one wave on one CU and xs_health_check does not record
// where its workgroups ran, so a bad matrix core, VALU or LDS bank on any
// other CU goes unseen. k_cu_sweep is one launch of 256-thread workgroups
// (4 waves: one per SIMD) that each hold more than half of a CU's 160 KiB LDS,
// so two of them never share a CU and a grid of 4 x CUs reaches every CU of an
// idle device. Every workgroup is self-contained (no waiting on another
// workgroup, no spinning on memory, no inter-workgroup atomics), records where
// it ran and checks three engines on the device:
//
//  * VALU  lane t = 64*wave + lane runs kSweepChain steps of
//            x = x*1664525 + 1013904223;  x ^= x >> 15;  x = rotl(x, 7)
//          from x = (t + 1) * 0x9e3779b9 (all mod 2^32). Digest
//          sum_t x_t * (2t + 1); compared with the host's value.
//  * MFMA  every wave computes C[32x32] = A[32xK]·B[Kx32] with
//          v_mfma_f32_32x32x16_bf16 from the integers of xs_mfma_check,
//            A[i][k] = (3i + 7k) % 17 - 8,  B[k][j] = (5k + 11j + (j > k ? 3 : 0)) % 13 - 6,
//          built in registers, and compares each of its 16 outputs per lane
//          with an int32 VALU dot product. Wave digest
//          D = sum_ij uint32(C[i][j]) * (2(32i + j) + 1); workgroup digest
//          sum_w D_w << w (15 D on a healthy CU).
//  * LDS   the first lds_bytes of the allocation, as n = lds_bytes/4 words.
//          Pass s (0, 1): lane t writes p_s(i) = (i*2654435761 ^ 0xa5a5a5a5)
//          ^ (s ? 0xffffffff : 0) to words i = t, t + 256, ...; after a
//          barrier lane t reads back words [t*n/256, (t+1)*n/256) and counts
//          mismatches. Pass digest D_s = sum_i v(i) * (2i + 1); workgroup
//          digest D_0 ^ rotl(D_1, 16).
//
// Operand maps (cdna_hip_programming.md §3, gfx950): lane l, r = l&31,
// h = l>>5 holds A[r][k0+8h+j] and B[k0+8h+j][r] (j = 0..7); accumulator
// register q holds C[(q&3) + 8(q>>2) + 4h][r].
//
// HW_REG_HW_ID (GFX9/CDNA ISA, hardware register 4): WAVE_ID [3:0],
// SIMD_ID [5:4], PIPE_ID [7:6], CU_ID [11:8], SH_ID [12], SE_ID [15:13],
// TG_ID [19:16], VM_ID [23:20], QUEUE_ID [26:24], STATE_ID [29:27],
// ME_ID [31:30]. The CU key of a record is bits [15:8]: SE, SH and CU id.
//
// Injection (testing the comparator and the localisation on a healthy GPU): a
// workgroup on inject_xcd whose CU key is inject_cu (or any, with -1) flips
// one bit of the value it computed for each engine in inject_engines before
// comparing. Registers only: no access changes.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>

#include "hip/sweep_common.h"

#define XS_ERR_BUF g_sweep_err

namespace {

xsprobe::ErrBuf g_sweep_err;

using namespace xsprobe;

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kSweepBlock = 256;    // 4 waves: one per SIMD
constexpr int kSweepChain = 32768;  // hash-chain steps per lane

enum : uint32_t { kFailMfma = 1, kFailValu = 2, kFailLds = 4 };

struct SweepRecord {
  uint32_t xcd, cu, simd_mask, fail;
  uint32_t mfma, valu, lds, reserved;
};
static_assert(sizeof(SweepRecord) == 32, "one 32-byte record per workgroup");

__host__ __device__ __forceinline__ uint32_t chain_step(uint32_t x) {
  x = x * 1664525u + 1013904223u;
  x ^= x >> 15;
  return rotl32(x, 7);
}
__host__ __device__ __forceinline__ int a_elem(int i, int k) { return (i * 3 + k * 7) % 17 - 8; }
__host__ __device__ __forceinline__ int b_elem(int k, int j) { return (k * 5 + j * 11 + (j > k ? 3 : 0)) % 13 - 6; }
__host__ __device__ __forceinline__ uint32_t lds_pattern(uint32_t i, int pass) {
  return (i * 2654435761u ^ 0xa5a5a5a5u) ^ (pass ? 0xffffffffu : 0u);
}

__global__ __launch_bounds__(kSweepBlock) void k_cu_sweep(SweepRecord* __restrict__ records, int K, uint32_t lds_words,
                                                         int inject_xcd, int inject_cu, uint32_t inject_engines,
                                                         uint32_t expect_valu) {
  extern __shared__ uint32_t sweep_lds[];
  const uint32_t t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const uint32_t xcd = xcc_id();
  const uint32_t hw = hw_id();
  const uint32_t cu = cu_key(hw);
  const uint32_t simd = simd_id(hw);
  const bool inject = inject_selected(inject_xcd, inject_cu, xcd, cu);
  const uint32_t inj = inject ? inject_engines : 0u;
  uint32_t fail = 0;

  // VALU: the long engine first, so every CU is still busy while the
  // dispatcher hands out the first CUs' worth of workgroups.
  uint32_t x = (t + 1u) * 0x9e3779b9u;
  for (int n = 0; n < kSweepChain; ++n) x = chain_step(x);
  if ((inj & kFailValu) && t == 0) x ^= 1u;
  const uint32_t valu_wave = wave_sum(x * (2u * t + 1u));

  // MFMA against an int32 VALU dot product of the same integers.
  const int r = lane & 31, h = lane >> 5;
  f32x16 acc = {};
  for (int k0 = 0; k0 < K; k0 += 16) {
    bf16x8 a, b;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      a[j] = static_cast<__bf16>(static_cast<float>(a_elem(r, k0 + 8 * h + j)));
      b[j] = static_cast<__bf16>(static_cast<float>(b_elem(k0 + 8 * h + j, r)));
    }
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc, 0, 0, 0);
  }
  uint32_t mfma_part = 0, mfma_bad = 0;
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const int i = (q & 3) + 8 * (q >> 2) + 4 * h;
    int got = static_cast<int>(acc[q]);
    if ((inj & kFailMfma) && t == 0 && q == 0) got ^= 1;
    int ref = 0;
    for (int k = 0; k < K; ++k) ref += a_elem(i, k) * b_elem(k, r);
    mfma_bad |= got != ref || acc[q] != static_cast<float>(static_cast<int>(acc[q]));
    mfma_part += static_cast<uint32_t>(got) * (2u * static_cast<uint32_t>(i * 32 + r) + 1u);
  }
  const uint32_t mfma_wave = wave_sum(mfma_part);
  if (mfma_bad) fail |= kFailMfma;

  // LDS: write strided, read back in contiguous per-lane chunks, then the complement.
  const uint32_t chunk = lds_words / kSweepBlock;
  uint32_t lds_digest[2];
  uint32_t lds_bad = 0;
#pragma unroll
  for (int pass = 0; pass < 2; ++pass) {
    for (uint32_t i = t; i < lds_words; i += kSweepBlock) sweep_lds[i] = lds_pattern(i, pass);
    __syncthreads();
    uint32_t d = 0;
    for (uint32_t i = t * chunk; i < (t + 1u) * chunk; ++i) {
      uint32_t v = sweep_lds[i];
      if ((inj & kFailLds) && pass == 0 && i == 0) v ^= 1u;
      lds_bad += v != lds_pattern(i, pass);
      d += v * (2u * i + 1u);
    }
    lds_digest[pass] = wave_sum(d);
    __syncthreads();
  }
  if (lds_bad) fail |= kFailLds;
  const uint32_t fail_wave = wave_or(fail);

  // Combine the four waves through the first words of the (now idle) allocation.
  if (lane == 0) {
    uint32_t* s = sweep_lds + wave * 8;
    s[0] = valu_wave;
    s[1] = mfma_wave;
    s[2] = lds_digest[0];
    s[3] = lds_digest[1];
    s[4] = fail_wave;
    s[5] = 1u << simd;
  }
  __syncthreads();
  if (t == 0) {
    uint32_t valu = 0, mfma = 0, l0 = 0, l1 = 0, f = 0, simds = 0;
    for (int w = 0; w < kSweepBlock / 64; ++w) {
      const uint32_t* s = sweep_lds + w * 8;
      valu += s[0];
      mfma += s[1] << w;
      l0 += s[2];
      l1 += s[3];
      f |= s[4];
      simds |= s[5];
    }
    if (valu != expect_valu) f |= kFailValu;
    u32x4* out = reinterpret_cast<u32x4*>(&records[blockIdx.x]);
    out[0] = u32x4{xcd, cu, simds, f};
    out[1] = u32x4{mfma, valu, l0 ^ rotl32(l1, 16), 0u};
  }
}

uint32_t expected_valu() {
  uint32_t d = 0;
  for (uint32_t t = 0; t < kSweepBlock; ++t) {
    uint32_t x = (t + 1u) * 0x9e3779b9u;
    for (int n = 0; n < kSweepChain; ++n) x = chain_step(x);
    d += x * (2u * t + 1u);
  }
  return d;
}

uint32_t expected_mfma(int K) {
  uint32_t d = 0;
  for (int i = 0; i < 32; ++i)
    for (int j = 0; j < 32; ++j) {
      int c = 0;
      for (int k = 0; k < K; ++k) c += a_elem(i, k) * b_elem(k, j);
      d += static_cast<uint32_t>(c) * (2u * static_cast<uint32_t>(i * 32 + j) + 1u);
    }
  uint32_t out = 0;
  for (int w = 0; w < kSweepBlock / 64; ++w) out += d << w;
  return out;
}

uint32_t expected_lds(size_t lds_bytes) {
  const uint32_t n = static_cast<uint32_t>(lds_bytes / 4);
  uint32_t d[2] = {0, 0};
  for (int pass = 0; pass < 2; ++pass)
    for (uint32_t i = 0; i < n; ++i) d[pass] += lds_pattern(i, pass) * (2u * i + 1u);
  return d[0] ^ rotl32(d[1], 16);
}

}  // namespace

extern "C" {

const char* xs_cu_sweep_last_error() { return g_sweep_err; }

// Bytes of LDS the sweep can cover on `dev` (0 on error).
size_t xs_cu_sweep_max_lds(int dev) {
  size_t m = 0;
  return max_workgroup_lds(g_sweep_err, dev, &m) == 0 ? m : 0;
}

// Host-side digests from the same formulas: out3 = {mfma, valu, lds}.
int xs_cu_sweep_expected(int k, size_t lds_bytes, uint32_t* out3) {
  if ((k != 16 && k != 64) || lds_bytes < 1024 || lds_bytes % 1024 || lds_bytes > kLdsPerCu || !out3) return kBadArgs;
  out3[0] = expected_mfma(k);
  out3[1] = expected_valu();
  out3[2] = expected_lds(lds_bytes);
  return 0;
}

// One sweep launch of `blocks` workgroups (0: 4 per CU). Writes `blocks`
// 32-byte records to records_out (the caller's buffer holds at least that
// many; with blocks == 0, 4 x computeUnits). Any negative inject_xcd selects
// no workgroup and any negative inject_cu every CU. Returns 0, -1000 for bad
// arguments (nothing is launched), or a negative HIP error.
int xs_cu_sweep(int dev, int blocks, int k, size_t lds_bytes, int inject_xcd, int inject_cu, int inject_engines,
                void* records_out, int* n_records, double* ms) {
  if ((k != 16 && k != 64) || lds_bytes < 1024 || lds_bytes % 1024) return kBadArgs;
  if (inject_engines < 0 || inject_engines > 7) return kBadArgs;
  SweepCall call{dev, blocks, inject_xcd, inject_cu, records_out, n_records, ms};
  call.negative_inject_ok = true;
  const uint32_t expect_valu = expected_valu();
  // The first lds_bytes of the allocation are tested, whatever its size.
  return launch_sweep(g_sweep_err, call, reinterpret_cast<const void*>(k_cu_sweep), kSweepBlock, lds_bytes,
                      sizeof(SweepRecord), [&](dim3 grid, dim3 block, size_t smem, void* rec) {
                        hipLaunchKernelGGL(k_cu_sweep, grid, block, smem, 0, static_cast<SweepRecord*>(rec), k,
                                           static_cast<uint32_t>(lds_bytes / 4), inject_xcd, inject_cu,
                                           static_cast<uint32_t>(inject_engines), expect_valu);
                      });
}

}  // extern "C"
