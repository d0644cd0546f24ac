// Matrix-core probes for gfx950 (MI355X): the node agent's compute check.
//
//  * xs_mfma_check   one wave computes C[32x32] = A[32xK]·B[Kx32] with
//                    v_mfma_f32_32x32x16_bf16 from exact small-integer bf16
//                    inputs (asymmetric B); the host compares bit-exactly
//                    against an integer reference. A GPU whose matrix cores
//                    mis-compute fails health even when HBM checksums pass.
//  * xs_mfma_peak    back-to-back bf16 MFMA issue, 2 waves per SIMD and 4
//                    independent 32x32 accumulators per wave (hides the
//                    MFMA dependency latency), optionally restricted to the
//                    XCDs of a mask (blocks read HW_REG_XCC_ID and the others
//                    exit), so a CPX/QPX/DPX partition's matrix throughput can
//                    be measured directly. Dense bf16 only (no sparsity). One
//                    counter per XCD says where the counted workgroups ran; a
//                    launch in which a selected XCD ran none fails with -1002
//                    instead of a rate.
//  * xs_mfma_tile_op, xs_mfma_peak_op  one launch of the same kernels on the
//                    caller's operands / with every accumulator and every
//                    workgroup's XCD stored, for the GPU tests; xs_mfma_inputs
//                    and xs_mfma_compare are the check's host halves.
//
// What is pinned, and where: tests/test_gpu_mfma_probe.py holds k_mfma_tile to
// an int64 / float64 numpy product of operands the test chose (identities that
// name a wrong lane map, full significands, 2^-60..2^60, Inf and NaN, a
// float64 rounding bound), every accumulator of k_mfma_peak to iters x the
// reference tile, the workgroups counted to those that recorded a selected
// XCD, and the flop count to its formula; tests/test_mfma_health.py holds the
// comparator to numpy on the CPU. The reference is tests/mfma_probe_ref.py.
//
// Operand maps (cdna_hip_programming.md §3, gfx950): lane l, r = l&31,
// h = l>>5 holds A[r][k0+8h+j] and B[k0+8h+j][r] (j = 0..7); accumulator
// register q holds C[(q&3) + 8(q>>2) + 4h][r].
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define XS_ERR_RC(e) (-1)  // this file's ABI: every HIP error is -1
#include "hip/sweep_common.h"

#define XS_ERR_BUF g_mfma_err

namespace {

xsprobe::ErrBuf g_mfma_err;

using xsprobe::kBadArgs;
using xsprobe::kCounterStride;
using xsprobe::kMaxXcds;
using xsprobe::xcc_id;

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kPeakBlock = 256;  // 4 waves: one per SIMD
constexpr int kAcc = 4;          // independent accumulators per wave

__global__ __launch_bounds__(64) void k_mfma_tile(const __bf16* __restrict__ A, const __bf16* __restrict__ B,
                                                  float* __restrict__ C, int K) {
  const int l = threadIdx.x, r = l & 31, h = l >> 5;
  f32x16 acc = {};
  for (int k0 = 0; k0 < K; k0 += 16) {
    bf16x8 a, b;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      a[j] = A[r * K + k0 + 8 * h + j];
      b[j] = B[(k0 + 8 * h + j) * 32 + r];
    }
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc, 0, 0, 0);
  }
#pragma unroll
  for (int q = 0; q < 16; ++q) C[((q & 3) + 8 * (q >> 2) + 4 * h) * 32 + r] = acc[q];
}

constexpr int kMaxTileK = 4096;             // xs_mfma_tile_op: A and B of 256 KiB each
constexpr int kMaxCheckedBlocks = 4096;     // xs_mfma_peak_op: 64 KiB of accumulators per workgroup
constexpr uint32_t kDidNotRun = 0x80000000u;  // xcd_of_block flag of a workgroup that exited
constexpr int kIdleXcd = -1002;

// One counter per XCD (thread 0 of a workgroup that runs adds 1 to its XCD's),
// so the host sees where the counted workgroups ran. CHECK = true is the
// tests' instantiation of the same loop: every workgroup records its XCD in
// xcd_of_block (with kDidNotRun when it exited) and every lane of a workgroup
// that ran stores its kAcc x 16 accumulator values to
// acc_out[((block * kPeakBlock + thread) * kAcc + n) * 16 + q]. The timed
// instantiation keeps its never-taken store.
template <bool CHECK>
__global__ __launch_bounds__(kPeakBlock) void k_mfma_peak(int iters, uint32_t xcd_mask, unsigned* __restrict__ active,
                                                           float* __restrict__ sink, float* __restrict__ acc_out,
                                                           uint32_t* __restrict__ xcd_of_block) {
  const uint32_t x = xcc_id();
  const bool run = x < kMaxXcds && ((xcd_mask >> x) & 1u);
  if constexpr (CHECK) {
    if (threadIdx.x == 0) xcd_of_block[blockIdx.x] = x | (run ? 0u : kDidNotRun);
  }
  if (!run) return;
  if (threadIdx.x == 0) atomicAdd(active + x * kCounterStride, 1u);
  bf16x8 a, b;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    a[j] = static_cast<__bf16>(0.125f * static_cast<float>((threadIdx.x + j) & 7));
    b[j] = static_cast<__bf16>(0.0625f * static_cast<float>((threadIdx.x * 3 + j) & 15));
  }
  f32x16 acc[kAcc];
#pragma unroll
  for (int n = 0; n < kAcc; ++n) acc[n] = f32x16{};
  for (int i = 0; i < iters; ++i) {
#pragma unroll
    for (int n = 0; n < kAcc; ++n) acc[n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc[n], 0, 0, 0);
  }
  if constexpr (CHECK) {
    float* out = acc_out + (static_cast<size_t>(blockIdx.x) * kPeakBlock + threadIdx.x) * (kAcc * 16);
#pragma unroll
    for (int n = 0; n < kAcc; ++n)
#pragma unroll
      for (int q = 0; q < 16; ++q) out[n * 16 + q] = acc[n][q];
  } else {
    float s = 0.f;
#pragma unroll
    for (int n = 0; n < kAcc; ++n)
#pragma unroll
      for (int q = 0; q < 16; ++q) s += acc[n][q];
    // Data-dependent store: the accumulators stay live, the store almost never runs.
    if (s == -1.0f) sink[blockIdx.x] = s;
  }
}

inline uint16_t bf16_bits(float f) {
  const __bf16 v = static_cast<__bf16>(f);
  uint16_t u;
  std::memcpy(&u, &v, sizeof u);
  return u;
}

inline bool tile_k_ok(int K) { return K > 0 && K % 16 == 0 && K <= kMaxTileK; }

// The check's integers: A[32xK] in [-8, 8], B[Kx32] in [-6, 6], B asymmetric.
inline int a_int(int i, int k) { return (i * 3 + k * 7) % 17 - 8; }
inline int b_int(int k, int j) { return (k * 5 + j * 11 + (j > k ? 3 : 0)) % 13 - 6; }

// Flops of one k_mfma_peak dispatch in which `active` workgroups ran.
inline double peak_flops(unsigned active, int iters) {
  const double flop_per_mfma = 2.0 * 32 * 32 * 16;
  return static_cast<double>(active) * (kPeakBlock / 64) * kAcc * static_cast<double>(iters) * flop_per_mfma;
}

inline bool mask_ok(uint32_t xcd_mask) { return xcd_mask != 0 && !(xcd_mask & ~0xffu); }

}  // namespace

extern "C" {

const char* xs_mfma_last_error() { return g_mfma_err; }

// Largest K xs_mfma_tile_op, xs_mfma_inputs, xs_mfma_compare and xs_mfma_check take.
int xs_mfma_max_k() { return kMaxTileK; }

// k_mfma_tile as xs_mfma_check launches it (one wave), on the caller's
// operands: a_bits / b_bits are the host bf16 bit patterns of A[32xK] and
// B[Kx32], row-major; c_out receives C[32x32] as fp32 (host). K must be a
// positive multiple of 16, at most kMaxTileK (4096): -1000 otherwise, no
// value is substituted. -1001 for a null pointer.
int xs_mfma_tile_op(int dev, const uint16_t* a_bits, const uint16_t* b_bits, int K, float* c_out) {
  if (!tile_k_ok(K)) return kBadArgs;
  if (!a_bits || !b_bits || !c_out) return -1001;
  XS_CHECK(hipSetDevice(dev));
  const size_t ab = static_cast<size_t>(32) * K * sizeof(uint16_t);
  xsprobe::DevMem da, db, dc;
  XS_CHECK(hipMalloc(&da.p, ab));
  XS_CHECK(hipMalloc(&db.p, ab));
  XS_CHECK(hipMalloc(&dc.p, 32 * 32 * sizeof(float)));
  XS_CHECK(hipMemcpy(da.p, a_bits, ab, hipMemcpyHostToDevice));
  XS_CHECK(hipMemcpy(db.p, b_bits, ab, hipMemcpyHostToDevice));
  XS_CHECK(hipMemset(dc.p, 0xff, 32 * 32 * sizeof(float)));
  hipLaunchKernelGGL(k_mfma_tile, dim3(1), dim3(64), 0, 0, da.as<const __bf16>(), db.as<const __bf16>(),
                     dc.as<float>(), K);
  XS_CHECK(hipGetLastError());
  XS_CHECK(hipMemcpy(c_out, dc.p, 32 * 32 * sizeof(float), hipMemcpyDeviceToHost));
  return 0;
}

// The check's operands as integers: a_out[32xK], b_out[Kx32]. Host only.
int xs_mfma_inputs(int K, int* a_out, int* b_out) {
  if (!tile_k_ok(K) || !a_out || !b_out) return kBadArgs;
  for (int i = 0; i < 32; ++i)
    for (int k = 0; k < K; ++k) a_out[i * K + k] = a_int(i, k);
  for (int k = 0; k < K; ++k)
    for (int j = 0; j < 32; ++j) b_out[k * 32 + j] = b_int(k, j);
  return 0;
}

// The check's comparator over a caller's C[32x32] (host): the number of
// elements that differ from the integer product of xs_mfma_inputs(K), and the
// indices (32 * row + col) of the first `cap` of them in bad_index_out. Host only.
int xs_mfma_compare(int K, const float* c, int* bad_index_out, int cap) {
  if (!tile_k_ok(K) || !c || cap < 0 || (cap > 0 && !bad_index_out)) return kBadArgs;
  int bad = 0;
  for (int i = 0; i < 32; ++i)
    for (int j = 0; j < 32; ++j) {
      long ref = 0;
      for (int k = 0; k < K; ++k) ref += static_cast<long>(a_int(i, k)) * b_int(k, j);
      if (c[i * 32 + j] != static_cast<float>(ref)) {
        if (bad < cap) bad_index_out[bad] = i * 32 + j;
        ++bad;
      }
    }
  return bad;
}

// Exact-integer MFMA tile check: xs_mfma_inputs -> xs_mfma_tile_op ->
// xs_mfma_compare. Returns the number of mismatching elements of the 32x32
// result (0 = pass), -1000 for a K that is not a positive multiple of 16 up
// to kMaxTileK, or another value <0 on a HIP error.
int xs_mfma_check(int dev, int K) {
  if (!tile_k_ok(K)) return kBadArgs;
  std::vector<int> ai(32 * K), bi(K * 32);
  if (int rc = xs_mfma_inputs(K, ai.data(), bi.data())) return rc;
  std::vector<uint16_t> a(ai.size()), b(bi.size());
  for (size_t i = 0; i < ai.size(); ++i) a[i] = bf16_bits(static_cast<float>(ai[i]));
  for (size_t i = 0; i < bi.size(); ++i) b[i] = bf16_bits(static_cast<float>(bi[i]));
  std::vector<float> c(32 * 32);
  if (int rc = xs_mfma_tile_op(dev, a.data(), b.data(), K, c.data())) return rc;
  return xs_mfma_compare(K, c.data(), nullptr, 0);
}

// One launch of the checked instantiation of k_mfma_peak, no warm-up, at the
// production block size: `blocks` workgroups (0: 8 per CU; at most 4096),
// iters > 0, xcd_mask as xs_mfma_peak (-1000 otherwise). Host outputs:
// acc_out[blocks x 256 x kAcc x 16] fp32, the accumulators of every lane
// (all-ones bit patterns where a workgroup did not run); xcd_of_block_out
// [blocks], the XCD each workgroup ran on, with bit 31 set when it exited;
// active_per_xcd_out[8], the kernel's own counters. A selected XCD that got
// no workgroup is reported through the counters, not as an error.
int xs_mfma_peak_op(int dev, int iters, uint32_t xcd_mask, int blocks, float* acc_out, uint32_t* xcd_of_block_out,
                    unsigned* active_per_xcd_out) {
  if (!mask_ok(xcd_mask) || iters <= 0 || blocks < 0 || blocks > kMaxCheckedBlocks) return kBadArgs;
  if (!acc_out || !xcd_of_block_out || !active_per_xcd_out) return -1001;
  XS_CHECK(hipSetDevice(dev));
  if (blocks == 0) XS_CHECK(xsprobe::cu_count(dev, &blocks, 8));
  if (blocks > kMaxCheckedBlocks) return kBadArgs;
  const size_t acc_bytes = static_cast<size_t>(blocks) * kPeakBlock * kAcc * 16 * sizeof(float);
  const size_t xcd_bytes = static_cast<size_t>(blocks) * sizeof(uint32_t);
  xsprobe::XcdCounters active;
  XS_CHECK(active.init());
  xsprobe::DevMem acc_mem, xcd_mem;
  XS_CHECK(hipMalloc(&acc_mem.p, acc_bytes));
  XS_CHECK(hipMalloc(&xcd_mem.p, xcd_bytes));
  XS_CHECK(hipMemset(acc_mem.p, 0xff, acc_bytes));
  XS_CHECK(hipMemset(xcd_mem.p, 0xff, xcd_bytes));
  hipLaunchKernelGGL(k_mfma_peak<true>, dim3(blocks), dim3(kPeakBlock), 0, 0, iters, xcd_mask, active.of(0),
                     static_cast<float*>(nullptr), acc_mem.as<float>(), xcd_mem.as<uint32_t>());
  XS_CHECK(hipGetLastError());
  XS_CHECK(hipDeviceSynchronize());
  XS_CHECK(hipMemcpy(acc_out, acc_mem.p, acc_bytes, hipMemcpyDeviceToHost));
  XS_CHECK(hipMemcpy(xcd_of_block_out, xcd_mem.p, xcd_bytes, hipMemcpyDeviceToHost));
  XS_CHECK(active.fetch(active_per_xcd_out));
  return 0;
}

// Dense bf16 MFMA throughput on the XCDs of `xcd_mask` (0xff = whole GPU;
// 0 and bits above the 8 XCDs are refused with -1000 before anything is
// launched). `blocks` = launch size (0: 8 per CU = 8 waves per SIMD). With
// the clock ramped by the warm-up, 2-8 waves per SIMD all issue at 98-99% of
// the 2.5 PF rate (profiles/r4z_mfma_sweep.jsonl); the earlier 79% reading was a
// clock still ramping under a short warm-up (r4x/r4y sweeps: rate rising with
// launch size and length only because each point ran hotter). Returns 0 and TFLOP/s, ms, the
// number of workgroups that ran on the selected XCDs, that number per XCD
// (active_per_xcd[8], may be null) and the flops credited to the timed
// dispatch (flops_out, may be null). -1002 when a selected XCD ran no
// workgroup in the timed launch (xs_mfma_last_error names it): the rate of a
// partition that did not all work is not reported.
int xs_mfma_peak(int dev, int iters, uint32_t xcd_mask, int blocks, double* tflops, double* ms_out,
                 int* active_blocks, unsigned* active_per_xcd, double* flops_out) {
  if (!mask_ok(xcd_mask)) return kBadArgs;
  XS_CHECK(hipSetDevice(dev));
  if (blocks <= 0) XS_CHECK(xsprobe::cu_count(dev, &blocks, 8));
  if (iters <= 0) iters = 4096;
  xsprobe::XcdCounters counters;  // [0] the warm-up launches', [1] the timed launch's
  XS_CHECK(counters.init(2));
  xsprobe::DevMem sink_mem;
  XS_CHECK(hipMalloc(&sink_mem.p, blocks * sizeof(float)));
  xsprobe::Stream stream;
  XS_CHECK(hipStreamCreate(&stream.s));
  auto go = [&](int timed) {
    hipLaunchKernelGGL(k_mfma_peak<false>, dim3(blocks), dim3(kPeakBlock), 0, stream.s, iters, xcd_mask,
                       counters.of(timed), sink_mem.as<float>(), static_cast<float*>(nullptr),
                       static_cast<uint32_t*>(nullptr));
  };
  // Warm-up: code resident, then about 20 ms of the same load so the clock has
  // ramped before the timed launch: 2.11 -> 2.40-2.41 PF/s in a fresh process
  // (profiles/r4za_probe_warm_ab.jsonl). The HBM probes are memory-bound and
  // read the same with or without it (same file), so they keep their short one.
  double t[3];
  if (int rc = xsprobe::time_launches(g_mfma_err, stream.s, 1, [&](int) { go(0); }, t)) return rc;
  const float warm_ms = static_cast<float>(t[0]);
  const char* env = std::getenv("XS_PROBE_WARM_MS");  // only this probe reads it; 0 = one launch
  const float target = env ? static_cast<float>(std::atof(env)) : 20.f;
  const int warm = target <= 0.f ? 0 : warm_ms > 0.f ? std::min(64, static_cast<int>(target / warm_ms) + 1) : 4;
  for (int w = 0; w < warm; ++w) go(0);
  if (int rc = xsprobe::time_launches(g_mfma_err, stream.s, 1, [&](int) { go(1); }, t)) return rc;
  const double ms = t[0];
  unsigned both[2 * kMaxXcds];
  XS_CHECK(counters.fetch(both));
  const unsigned* per_xcd = both + kMaxXcds;
  unsigned active = 0;
  uint32_t idle = 0;
  for (int x = 0; x < kMaxXcds; ++x) {
    active += per_xcd[x];
    if (((xcd_mask >> x) & 1u) && per_xcd[x] == 0) idle |= 1u << x;
  }
  if (active_per_xcd)
    for (int x = 0; x < kMaxXcds; ++x) active_per_xcd[x] = per_xcd[x];
  *active_blocks = static_cast<int>(active);
  if (idle) {
    std::snprintf(g_mfma_err, sizeof g_mfma_err,
                  "k_mfma_peak: no workgroup ran on XCD(s) %s of xcd_mask 0x%x (%d workgroups launched, %u ran)",
                  xsprobe::XcdList(idle).text, xcd_mask, blocks, active);
    return kIdleXcd;
  }
  const double flops = peak_flops(active, iters);
  *tflops = ms > 0 ? flops / (ms * 1e-3) / 1e12 : 0.0;
  *ms_out = ms;
  if (flops_out) *flops_out = flops;
  return 0;
}

}  // extern "C"
