// What the probe and sweep files share: where a wave runs, the wave
// reductions, the error check, the probes' CU count, launch timing and per-XCD
// counters, and the host side of a per-CU sweep launch.
//
// A per-CU sweep (cu_sweep.hip, matrix_sweep.hip, regfile_sweep.hip,
// lane_sweep.hip, valu_sweep.hip) is one launch of 256-thread workgroups of
// which no two fit on a CU, 4 per CU by default, each leaving one record whose
// first four words are {xcd, cu key, simd mask, fail bits}. The kernels
// differ; how such a launch is validated, sized, timed and read back is
// launch_sweep() below.
//
// Two things a new sweep decides on purpose when it fills a SweepCall, because
// the existing ones differ and their callers rely on it:
//  * blocks == 0 means "4 per CU" to launch_sweep. xs_matrix_sweep refuses 0
//    itself before it calls; the other three pass it through.
//  * inject_xcd / inject_cu below -1 are refused, -1 meaning "none" / "any".
//    xs_cu_sweep sets negative_inject_ok and takes any negative value as -1.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "hip/device_raii.h"

// Returns from the enclosing function on a HIP error, with "call: reason" in
// XS_ERR_BUF, which the including file defines as the name of its own
// char[512] (what its xs_*_last_error returns). The value returned is
// -(HIP error) - 1; mfma_probe.hip, whose ABI is -1 for every HIP error,
// defines its own XS_ERR_RC before it includes this file.
#ifndef XS_ERR_RC
#define XS_ERR_RC(e) (-static_cast<int>(e) - 1)
#endif
#define XS_CHECK(x)                                                                      \
  do {                                                                                   \
    hipError_t e_ = (x);                                                                 \
    if (e_ != hipSuccess) {                                                              \
      std::snprintf(XS_ERR_BUF, sizeof XS_ERR_BUF, "%s: %s", #x, hipGetErrorString(e_)); \
      return XS_ERR_RC(e_);                                                              \
    }                                                                                    \
  } while (0)

namespace xsprobe {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// ------------------------------------------------------------------- device
// HW_REG_XCC_ID: the XCD the wave runs on.
__device__ __forceinline__ uint32_t xcc_id() {
  uint32_t v;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(v));
  return v & 0xf;
}
// HW_REG_HW_ID (GFX9/CDNA ISA, hardware register 4): WAVE_ID [3:0],
// SIMD_ID [5:4], PIPE_ID [7:6], CU_ID [11:8], SH_ID [12], SE_ID [15:13], ...
__device__ __forceinline__ uint32_t hw_id() {
  uint32_t v;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(v));
  return v;
}
// The CU key of a record: SE, SH and CU id of hw_id().
__device__ __forceinline__ uint32_t cu_key(uint32_t hw) { return (hw >> 8) & 0xffu; }
__device__ __forceinline__ uint32_t simd_id(uint32_t hw) { return (hw >> 4) & 0x3u; }

// Whether the workgroup on (xcd, cu) is the one an injection names: on
// inject_xcd (negative: none) and with CU key inject_cu (negative: any).
__device__ __forceinline__ bool inject_selected(int inject_xcd, int inject_cu, uint32_t xcd, uint32_t cu) {
  return inject_xcd >= 0 && xcd == static_cast<uint32_t>(inject_xcd) &&
         (inject_cu < 0 || cu == static_cast<uint32_t>(inject_cu));
}

__host__ __device__ __forceinline__ uint32_t rotl32(uint32_t x, int s) {
  s &= 31;
  return s ? (x << s) | (x >> (32 - s)) : x;
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ uint32_t wave_or(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v |= __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ uint32_t wave_min(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, static_cast<uint32_t>(__shfl_xor(v, o, 64)));
  return v;
}

// --------------------------------------------------------------------- host
using ErrBuf = char[512];

constexpr int kBadArgs = -1000;
constexpr int kMaxBlocks = 1 << 20;
constexpr size_t kLdsPerCu = 160u << 10;     // LDS of one gfx950 CU
constexpr size_t kLdsExclusive = 96u << 10;  // > half a CU's LDS: one sweep workgroup per CU

#define XS_ERR_BUF err

// out = per_cu x the compute units of `dev`: a grid of per_cu workgroups per
// CU. Like XcdCounters it returns the HIP error for the caller's XS_CHECK: one
// body then serves files whose XS_ERR_RC differs.
inline hipError_t cu_count(int dev, int* out, int per_cu = 1) {
  hipDeviceProp_t p;
  const hipError_t e = hipGetDeviceProperties(&p, dev);
  if (e == hipSuccess) *out = per_cu * p.multiProcessorCount;
  return e;
}

// Per-launch timing: `launch(i)` enqueues launch i; every launch sits
// between its own event pair on `s`. out: [median ms, min ms, batch ms per
// launch (first start to last end / iters)]. Events are created once.
template <typename F>
int time_launches(ErrBuf& err, hipStream_t s, int iters, F&& launch, double out[3]) {
  std::vector<Event> ev(2 * static_cast<size_t>(iters));
  for (auto& e : ev) XS_CHECK(hipEventCreate(&e.e));
  for (int i = 0; i < iters; ++i) {
    XS_CHECK(hipEventRecord(ev[2 * i].e, s));
    launch(i);
    XS_CHECK(hipEventRecord(ev[2 * i + 1].e, s));
  }
  XS_CHECK(hipEventSynchronize(ev.back().e));
  XS_CHECK(hipGetLastError());
  std::vector<double> per(iters);
  for (int i = 0; i < iters; ++i) {
    float ms = 0;
    XS_CHECK(hipEventElapsedTime(&ms, ev[2 * i].e, ev[2 * i + 1].e));
    per[i] = ms;
  }
  float total = 0;
  XS_CHECK(hipEventElapsedTime(&total, ev.front().e, ev.back().e));
  std::vector<double> sorted = per;
  std::sort(sorted.begin(), sorted.end());
  out[0] = sorted[sorted.size() / 2];
  out[1] = sorted.front();
  out[2] = static_cast<double>(total) / iters;
  return 0;
}

// One counter per XCD and launch, each on its own 128-B line: k_pinned hands
// out an XCD's chunks from it, k_mfma_peak counts the workgroups that ran
// there, and the host reads which selected XCDs took part in a launch.
constexpr int kMaxXcds = 8;
constexpr int kCounterStride = 32;  // unsigned per XCD counter (128 B)

struct XcdCounters {
  DevMem d;
  int launches = 0;
  // Zeroed counters for `n` launches.
  hipError_t init(int n = 1) {
    launches = n;
    const hipError_t e = hipMalloc(&d.p, sizeof(unsigned) * kMaxXcds * kCounterStride * n);
    return e != hipSuccess ? e : hipMemset(d.p, 0, sizeof(unsigned) * kMaxXcds * kCounterStride * n);
  }
  unsigned* of(int launch) const { return d.as<unsigned>() + static_cast<size_t>(launch) * kMaxXcds * kCounterStride; }
  // The eight counters of every launch, all completed, in one copy: per_xcd[launch * kMaxXcds + xcd].
  hipError_t fetch(unsigned* per_xcd) const {
    std::vector<unsigned> h(static_cast<size_t>(launches) * kMaxXcds * kCounterStride);
    const hipError_t e = hipMemcpy(h.data(), d.p, sizeof(unsigned) * h.size(), hipMemcpyDeviceToHost);
    for (int i = 0; i < launches * kMaxXcds; ++i) per_xcd[i] = h[static_cast<size_t>(i) * kCounterStride];
    return e;
  }
};

// The XCDs of `mask` as "0,3,5", for an error text.
struct XcdList {
  char text[32] = "";
  explicit XcdList(uint32_t mask) {
    for (int x = 0, k = 0; x < kMaxXcds; ++x)
      if ((mask >> x) & 1u) k += std::snprintf(text + k, sizeof text - k, "%s%d", k ? "," : "", x);
  }
};

// Largest dynamic LDS one workgroup may ask for on `dev`, in whole KiB.
inline int max_workgroup_lds(ErrBuf& err, int dev, size_t* out) {
  hipDeviceProp_t p;
  XS_CHECK(hipGetDeviceProperties(&p, dev));
  const size_t m = std::max<size_t>(p.sharedMemPerBlock, p.maxSharedMemoryPerMultiProcessor);
  *out = std::min(m, kLdsPerCu) & ~static_cast<size_t>(1023);
  return 0;
}

// The dynamic LDS a sweep workgroup that touches `used` bytes asks for: always
// more than half a CU's LDS, whatever part of it is used, so sweep workgroups
// never share a CU. kBadArgs when the device cannot give `used`.
inline int exclusive_lds(ErrBuf& err, int dev, size_t used, size_t* out) {
  size_t lds_max = 0;
  if (int rc = max_workgroup_lds(err, dev, &lds_max)) return rc;
  if (used > lds_max) return kBadArgs;
  *out = std::max(used, std::min(kLdsExclusive, lds_max));
  return 0;
}

// What the runtime reports for `kernel` launched with `block` threads and
// `smem` bytes of dynamic LDS on the current device: out = {registers per lane,
// scratch bytes per lane, [smem, when not 0,] workgroups that fit on a CU}.
inline int kernel_info(ErrBuf& err, const void* kernel, int block, size_t smem, int* out) {
  if (smem) XS_CHECK(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(smem)));
  hipFuncAttributes a;
  XS_CHECK(hipFuncGetAttributes(&a, kernel));
  int per_cu = 0;
  XS_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, block, smem));
  *out++ = a.numRegs;
  *out++ = static_cast<int>(a.localSizeBytes);
  if (smem) *out++ = static_cast<int>(smem);
  *out = per_cu;
  return 0;
}

// An xs_*_sweep_info: kernel_info() of a sweep kernel on `dev`, launched with
// exclusive_lds() when `exclusive` is set and with no dynamic LDS otherwise.
inline int sweep_info(ErrBuf& err, int dev, const void* kernel, int threads, bool exclusive, int* out) {
  if (!out) return kBadArgs;
  XS_CHECK(hipSetDevice(dev));
  size_t smem = 0;
  if (exclusive)
    if (int rc = exclusive_lds(err, dev, 0, &smem)) return rc;
  return kernel_info(err, kernel, threads, smem, out);
}

// The arguments every xs_*_sweep takes.
struct SweepCall {
  int dev, blocks;  // blocks 0: 4 per CU
  int inject_xcd, inject_cu;
  void* records_out;  // at least `blocks` records (with blocks == 0, 4 x computeUnits)
  int* n_records;
  double* ms;
  bool negative_inject_ok = false;
};

struct NoPrepare {
  int operator()() const { return 0; }
};

// One sweep launch: `threads` per workgroup, `lds_used` bytes of dynamic LDS
// touched by `kernel` (0: it has none; otherwise the launch asks for
// exclusive_lds()), one record of `record_bytes` per workgroup, poisoned with
// 0xff before the launch. launch(grid, block, smem, records on the device)
// does the hipLaunchKernelGGL and nothing else: it alone is timed. prepare() runs
// on the device after validation and before anything is allocated, for what
// the kernel reads. Returns 0, kBadArgs (nothing is launched) or a negative
// HIP error.
template <typename Launch, typename Prepare = NoPrepare>
int launch_sweep(ErrBuf& err, const SweepCall& c, const void* kernel, int threads, size_t lds_used,
                 size_t record_bytes, Launch&& launch, Prepare&& prepare = Prepare{}) {
  if (!c.records_out || c.blocks < 0 || c.blocks > kMaxBlocks) return kBadArgs;
  if (c.inject_xcd > 15 || c.inject_cu > 0xff) return kBadArgs;
  if (!c.negative_inject_ok && (c.inject_xcd < -1 || c.inject_cu < -1)) return kBadArgs;
  XS_CHECK(hipSetDevice(c.dev));
  hipDeviceProp_t p;
  XS_CHECK(hipGetDeviceProperties(&p, c.dev));
  const int blocks = c.blocks ? c.blocks : 4 * p.multiProcessorCount;
  if (blocks <= 0 || blocks > kMaxBlocks) return kBadArgs;
  size_t smem = 0;
  if (lds_used) {
    if (int rc = exclusive_lds(err, c.dev, lds_used, &smem)) return rc;
    XS_CHECK(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(smem)));
  }
  if (int rc = prepare()) return rc;
  DevMem rec;
  const size_t bytes = static_cast<size_t>(blocks) * record_bytes;
  XS_CHECK(hipMalloc(&rec.p, bytes));
  XS_CHECK(hipMemset(rec.p, 0xff, bytes));
  Event e0, e1;
  XS_CHECK(hipEventCreate(&e0.e));
  XS_CHECK(hipEventCreate(&e1.e));
  XS_CHECK(hipEventRecord(e0.e, 0));
  launch(dim3(blocks), dim3(threads), smem, rec.p);
  XS_CHECK(hipGetLastError());
  XS_CHECK(hipEventRecord(e1.e, 0));
  XS_CHECK(hipEventSynchronize(e1.e));
  float t = 0.f;
  XS_CHECK(hipEventElapsedTime(&t, e0.e, e1.e));
  XS_CHECK(hipMemcpy(c.records_out, rec.p, bytes, hipMemcpyDeviceToHost));
  if (c.n_records) *c.n_records = blocks;
  if (c.ms) *c.ms = t;
  return 0;
}

// One workgroup of a sweep's probe kernel, which stores every word it
// received: a sweep launch of one workgroup whose record is the dump of
// `n_words`, copied to `out`.
template <typename Launch, typename Prepare = NoPrepare>
int launch_probe(ErrBuf& err, int dev, const void* kernel, int threads, size_t lds_used, uint32_t* out,
                 size_t n_words, Launch&& launch, Prepare&& prepare = Prepare{}) {
  return launch_sweep(err, {dev, 1, -1, -1, out, nullptr, nullptr}, kernel, threads, lds_used, n_words * 4, launch,
                      prepare);
}

#undef XS_ERR_BUF

}  // namespace xsprobe
