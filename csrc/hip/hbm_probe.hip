// MI355X (gfx950) device probes used by the node agent and the benchmarks.
//
// There is no GPU code in the reference: the scheduler only
// counts extended resources. An MI355X-native scheduler must validate what it
// promises, so the node agent runs these probes on the box:
//
//  * xs_hbm_bandwidth   streaming read / write / copy / triad over N bytes with
//                       16-byte lanes (global_load/store_dwordx4). Variants:
//                       unroll 1/4/8 (independent 16 B accesses in flight per
//                       lane), non-temporal vs default cache policy, 4/8/16
//                       persistent workgroups of 256 threads per CU or a
//                       one-shot grid (one workgroup per 4 KiB, no loop);
//                       probe_bench sweeps them and the node agent keeps the
//                       fastest (profiles/r5*_stream_sweep.md). HBM3E peak
//                       is 8 TB/s. Each launch is timed by its own event pair
//                       and the median is reported (the back-to-back batch
//                       rate, launch gaps included, is kept as a second
//                       figure); working sets default to 1 GiB, 4x the 256 MB
//                       Infinity Cache, so the rate is HBM's and not the
//                       cache's (profiles/r4*_pmc_probe_summary.md checks the
//                       median against rocprofv3's dispatch times and bytes).
//  * xs_hbm_bandwidth_xcd  the same traffic executed only by workgroups that
//                       land on the XCDs in `xcd_mask` (work handed out by an
//                       atomic chunk counter, so every launched workgroup
//                       exits): the HBM bandwidth one CPX partition (one XCD,
//                       32 CUs) or a QPX/DPX partition can pull, measured on
//                       an SPX device. A launch in which a selected XCD got
//                       no workgroup fails with -1002 instead of a rate.
//  * xs_stream_op, xs_pinned_op, xs_segment_op, xs_checksum_op  one
//                       launch of the same kernels over caller-owned buffers,
//                       for the GPU tests; the read paths run as checked
//                       instantiations (k_*_fold) that report the XOR of the
//                       words read and the number of 16-B loads issued.
//  * xs_xcd_census      every workgroup records s_getreg(HW_REG_XCC_ID):
//                       counts XCDs visible to this device — verifies the
//                       compute-partition mode the node advertises (SPX -> 8
//                       XCDs, CPX -> 1).
//  * xs_health_check    deterministic integer checksum over a pattern buffer
//                       (catches a dead/ECC-faulting device before the node is
//                       advertised schedulable): allocate, xs_pattern_op,
//                       xs_health_verify; the two halves also run on a
//                       caller-owned buffer, so the GPU tests hold the pattern
//                       to numpy and see the verdict fail on a flipped bit.
//
// Exposed as a C ABI (loaded with ctypes from flex_gpu_scheduler_amd/ops).
// Every entry point checks its arguments before it touches the device: -1000
// for bad arguments, -1001 for a null or mis-aligned buffer, nothing launched.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <type_traits>
#include <vector>

#include "hip/sweep_common.h"

#define XS_ERR_BUF g_err

namespace {

xsprobe::ErrBuf g_err;

using xsprobe::DevMem;
using xsprobe::Stream;
using xsprobe::XcdCounters;
using xsprobe::hw_id;
using xsprobe::kBadArgs;
using xsprobe::kCounterStride;
using xsprobe::kMaxXcds;
using xsprobe::xcc_id;

constexpr int kBlock = 256;  // 4 waves of 64 lanes

typedef uint32_t vec4 __attribute__((ext_vector_type(4)));  // 16 B/lane
typedef float f32x4 __attribute__((ext_vector_type(4)));

template <bool NT, typename T>
__device__ __forceinline__ T ld(const T* p) {
  if constexpr (NT) return __builtin_nontemporal_load(p);
  else return *p;
}
template <bool NT, typename T>
__device__ __forceinline__ void st(T v, T* p) {
  if constexpr (NT) __builtin_nontemporal_store(v, p);
  else *p = v;
}

// Checked instantiations (FOLD) make a read path observable: the XOR of every
// lane's acc goes to fold[0] and the number of 16-B loads issued to fold[1],
// reduced per wave first, then one atomic each from the wave's first lane.
// Every lane of the wave must arrive. The timed kernels instantiate the same
// loop source with FOLD = false and keep their DCE sink.
__device__ __forceinline__ void fold_wave(uint32_t acc, unsigned long long loads, unsigned long long* __restrict__ fold) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    acc ^= __shfl_down(acc, off, 64);
    loads += __shfl_down(loads, off, 64);
  }
  if ((threadIdx.x & 63) == 0 && loads != 0) {
    atomicXor(&fold[0], static_cast<unsigned long long>(acc));
    atomicAdd(&fold[1], loads);
  }
}

// Grid-stride walk in rows of U*grid lanes: one wave-instruction touches
// 1 KiB contiguous, U independent 16-B accesses per lane in flight.
template <int U, bool NT, bool FOLD>
__device__ __forceinline__ void read_lanes(const vec4* __restrict__ src, size_t n, uint32_t* __restrict__ sink,
                                           unsigned long long* __restrict__ fold) {
  const size_t stride = static_cast<size_t>(gridDim.x) * kBlock;
  size_t i = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  uint32_t acc = 0;
  [[maybe_unused]] unsigned long long loads = 0;
  for (; i + (U - 1) * stride < n; i += U * stride) {
    vec4 v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) v[u] = ld<NT>(&src[i + u * stride]);
#pragma unroll
    for (int u = 0; u < U; ++u) acc ^= v[u].x ^ v[u].y ^ v[u].z ^ v[u].w;
    if constexpr (FOLD) loads += U;
  }
  for (; i < n; i += stride) {
    vec4 v = ld<NT>(&src[i]);
    acc ^= v.x ^ v.y ^ v.z ^ v.w;
    if constexpr (FOLD) ++loads;
  }
  if constexpr (FOLD) fold_wave(acc, loads, fold);
  else if (acc == 0x9e3779b9u) sink[0] = acc;  // defeats DCE without a store per lane
}

template <int U, bool NT>
__global__ __launch_bounds__(kBlock) void k_read(const vec4* __restrict__ src, size_t n, uint32_t* __restrict__ sink) {
  read_lanes<U, NT, false>(src, n, sink, nullptr);
}

template <int U, bool NT>
__global__ __launch_bounds__(kBlock) void k_read_fold(const vec4* __restrict__ src, size_t n,
                                                      unsigned long long* __restrict__ fold) {
  read_lanes<U, NT, true>(src, n, nullptr, fold);
}

template <int U, bool NT>
__global__ __launch_bounds__(kBlock) void k_write(vec4* __restrict__ dst, size_t n, uint32_t seed) {
  const size_t stride = static_cast<size_t>(gridDim.x) * kBlock;
  vec4 v = {seed, seed ^ 0x55555555u, seed + 1, ~seed};
  size_t i = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  for (; i + (U - 1) * stride < n; i += U * stride) {
#pragma unroll
    for (int u = 0; u < U; ++u) st<NT>(v, &dst[i + u * stride]);
  }
  for (; i < n; i += stride) st<NT>(v, &dst[i]);
}

template <int U, bool NT>
__global__ __launch_bounds__(kBlock) void k_copy(const vec4* __restrict__ src, vec4* __restrict__ dst, size_t n) {
  const size_t stride = static_cast<size_t>(gridDim.x) * kBlock;
  size_t i = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  for (; i + (U - 1) * stride < n; i += U * stride) {
    vec4 v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) v[u] = ld<NT>(&src[i + u * stride]);
#pragma unroll
    for (int u = 0; u < U; ++u) st<NT>(v[u], &dst[i + u * stride]);
  }
  for (; i < n; i += stride) st<NT>(ld<NT>(&src[i]), &dst[i]);
}

// STREAM triad a = b + s*c on float4 lanes.
template <int U, bool NT>
__global__ __launch_bounds__(kBlock) void k_triad(f32x4* __restrict__ a, const f32x4* __restrict__ b,
                                                  const f32x4* __restrict__ c, float s, size_t n) {
  const size_t stride = static_cast<size_t>(gridDim.x) * kBlock;
  size_t i = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  for (; i + (U - 1) * stride < n; i += U * stride) {
    f32x4 x[U], y[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      x[u] = ld<NT>(&b[i + u * stride]);
      y[u] = ld<NT>(&c[i + u * stride]);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) st<NT>(x[u] + s * y[u], &a[i + u * stride]);
  }
  for (; i < n; i += stride) st<NT>(ld<NT>(&b[i]) + s * ld<NT>(&c[i]), &a[i]);
}

// XCD-pinned streaming: workgroups off the selected XCDs exit at once. The
// selected XCDs split the buffer into equal contiguous slices (by their rank
// in xcd_mask) and the workgroups of each XCD pull 256 KiB chunks of their
// slice from that XCD's own counter, so the launch always ends and no
// atomic is shared across XCDs (one counter per 128-B line: a single
// device-wide counter serialized the 8-XCD case at ~2 TB/s, round-3 pmc
// run). mode 0 read, 1 write, 2 copy. Where workgroups land is the
// dispatcher's choice: a selected XCD that gets none leaves its slice
// untouched, which the host detects from that XCD's counter (check_drained)
// and reports as an error, never as a rate.
constexpr size_t kChunk = 16384;  // vec4s = 256 KiB

struct Slice {
  size_t c0, c1;
};
// The chunks [c0, c1) that XCD x of the selected set `sel` owns of a buffer of
// n vec4s: the kernel's split and the host's check of it.
__host__ __device__ __forceinline__ Slice xcd_slice(size_t n, uint32_t sel, uint32_t x) {
  const size_t nsel = static_cast<size_t>(__builtin_popcount(sel));
  const size_t rank = static_cast<size_t>(__builtin_popcount(sel & ((1u << x) - 1u)));
  const size_t nchunks = (n + kChunk - 1) / kChunk;
  return {nchunks * rank / nsel, nchunks * (rank + 1) / nsel};
}

template <bool FOLD>
__device__ __forceinline__ void pinned_lanes(const vec4* __restrict__ src, vec4* __restrict__ dst, size_t n,
                                             uint32_t xcd_mask, unsigned* __restrict__ counters, int mode,
                                             uint32_t* __restrict__ sink, unsigned long long* __restrict__ fold) {
  const uint32_t x = xcc_id();
  if (x >= kMaxXcds || !((xcd_mask >> x) & 1u)) return;
  const auto [c0, c1] = xcd_slice(n, xcd_mask & 0xffu, x);
  unsigned* ctr = counters + x * kCounterStride;
  __shared__ unsigned chunk;
  uint32_t acc = 0;
  [[maybe_unused]] unsigned long long loads = 0;
  const vec4 fill = {1u, 2u, 3u, 4u};
  for (;;) {
    if (threadIdx.x == 0) chunk = atomicAdd(ctr, 1u);
    __syncthreads();
    const size_t c = c0 + chunk;
    __syncthreads();
    if (c >= c1) break;
    size_t base = c * kChunk;
    size_t end = base + kChunk < n ? base + kChunk : n;
    size_t i = base + threadIdx.x;
    for (; i + 3 * kBlock < end; i += 4 * kBlock) {
      if (mode == 1) {
#pragma unroll
        for (int u = 0; u < 4; ++u) __builtin_nontemporal_store(fill, &dst[i + u * kBlock]);
      } else {
        vec4 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = __builtin_nontemporal_load(&src[i + u * kBlock]);
        if (mode == 2) {
#pragma unroll
          for (int u = 0; u < 4; ++u) __builtin_nontemporal_store(v[u], &dst[i + u * kBlock]);
        } else {
#pragma unroll
          for (int u = 0; u < 4; ++u) acc ^= v[u].x ^ v[u].y ^ v[u].z ^ v[u].w;
          if constexpr (FOLD) loads += 4;
        }
      }
    }
    for (; i < end; i += kBlock) {
      if (mode == 1) {
        __builtin_nontemporal_store(fill, &dst[i]);
      } else {
        vec4 v = __builtin_nontemporal_load(&src[i]);
        if (mode == 2) __builtin_nontemporal_store(v, &dst[i]);
        else {
          acc ^= v.x ^ v.y ^ v.z ^ v.w;
          if constexpr (FOLD) ++loads;
        }
      }
    }
  }
  if constexpr (FOLD) fold_wave(acc, loads, fold);  // a workgroup leaves the loop as one
  else if (acc == 0x9e3779b9u) sink[0] = acc;
}

__global__ __launch_bounds__(kBlock) void k_pinned(const vec4* __restrict__ src, vec4* __restrict__ dst, size_t n,
                                                   uint32_t xcd_mask, unsigned* __restrict__ counters, int mode,
                                                   uint32_t* __restrict__ sink) {
  pinned_lanes<false>(src, dst, n, xcd_mask, counters, mode, sink, nullptr);
}

__global__ __launch_bounds__(kBlock) void k_pinned_fold(const vec4* __restrict__ src, size_t n, uint32_t xcd_mask,
                                                        unsigned* __restrict__ counters,
                                                        unsigned long long* __restrict__ fold) {
  pinned_lanes<true>(src, nullptr, n, xcd_mask, counters, 0, nullptr, fold);
}

__global__ __launch_bounds__(64) void k_census(uint32_t* __restrict__ xcd_of_block, uint32_t* __restrict__ hwid_of_block) {
  if (threadIdx.x == 0) {
    xcd_of_block[blockIdx.x] = xcc_id();
    hwid_of_block[blockIdx.x] = hw_id();
  }
}

__global__ __launch_bounds__(kBlock) void k_pattern(uint32_t* __restrict__ buf, size_t n) {
  const size_t stride = static_cast<size_t>(gridDim.x) * kBlock;
  for (size_t i = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x; i < n; i += stride)
    buf[i] = static_cast<uint32_t>(i * 2654435761u) ^ 0xa5a5a5a5u;
}

// Block-level sum of the pattern (wave64 shuffles, then LDS across 4 waves).
__global__ __launch_bounds__(kBlock) void k_checksum(const uint32_t* __restrict__ buf, size_t n,
                                                     unsigned long long* __restrict__ out) {
  const size_t stride = static_cast<size_t>(gridDim.x) * kBlock;
  unsigned long long acc = 0;
  for (size_t i = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x; i < n; i += stride) acc += buf[i];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
  __shared__ unsigned long long part[kBlock / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) part[wave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long s = 0;
#pragma unroll
    for (int w = 0; w < kBlock / 64; ++w) s += part[w];
    atomicAdd(out, s);
  }
}

// Counter calibration (xs_segment_access): every wave touches segments of
// `seg_lanes` x 16 B, each at the start of its own `stride_vec`-vec4 slot, so
// a dispatch moves a known number of bytes in a known number of 128-B lines
// (touches x ceil(seg/128)); rocprofv3's L2 memory-side request counters are
// read against that count (scripts/pmc_calibrate.sh). Lanes >= seg_lanes
// idle; mode 0 reads, 1 writes.
template <int MODE, bool NT, bool FOLD>
__device__ __forceinline__ void segment_lanes(vec4* __restrict__ buf, size_t touches, size_t stride_vec, int seg_lanes,
                                              uint32_t* __restrict__ sink, unsigned long long* __restrict__ fold) {
  const size_t wave = (static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x) >> 6;
  const size_t nwaves = (static_cast<size_t>(gridDim.x) * kBlock) >> 6;
  const int lane = threadIdx.x & 63;
  uint32_t acc = 0;
  [[maybe_unused]] unsigned long long loads = 0;
  const vec4 fill = {5u, 6u, 7u, 8u};
  if (lane < seg_lanes) {
    for (size_t t = wave; t < touches; t += nwaves) {
      vec4* p = buf + t * stride_vec + lane;
      if constexpr (MODE == 0) {
        vec4 v = ld<NT>(p);
        acc ^= v.x ^ v.y ^ v.z ^ v.w;
        if constexpr (FOLD) ++loads;
      } else {
        st<NT>(fill, p);
      }
    }
  }
  if constexpr (FOLD) fold_wave(acc, loads, fold);
  else if (acc == 0x9e3779b9u) sink[0] = acc;
}

template <int MODE, bool NT>
__global__ __launch_bounds__(kBlock) void k_segments(vec4* __restrict__ buf, size_t touches, size_t stride_vec,
                                                     int seg_lanes, uint32_t* __restrict__ sink) {
  segment_lanes<MODE, NT, false>(buf, touches, stride_vec, seg_lanes, sink, nullptr);
}

template <bool NT>
__global__ __launch_bounds__(kBlock) void k_segments_fold(vec4* __restrict__ buf, size_t touches, size_t stride_vec,
                                                          int seg_lanes, unsigned long long* __restrict__ fold) {
  segment_lanes<0, NT, true>(buf, touches, stride_vec, seg_lanes, nullptr, fold);
}

constexpr int kBadBuffer = -1001;
constexpr int kUndrained = -1002;
constexpr int kBlocksPerCu = 8;  // the persistent grid of everything but a variant

// A caller's buffer that is null though `needed`, or not aligned to `align` (a power of two).
bool bad_buffer(const void* p, size_t align, bool needed = true) {
  return (!p && needed) || (reinterpret_cast<uintptr_t>(p) & (align - 1));
}

// What a timed probe reports: `moved` bytes per launch over time_launches' t.
void report_rate(double moved, const double t[3], double* gbps, double* ms_per_iter, double* detail) {
  if (gbps) *gbps = moved / (t[0] * 1e-3) / 1e9;
  if (ms_per_iter) *ms_per_iter = t[0];
  if (detail) {
    detail[0] = moved / (t[1] * 1e-3) / 1e9;
    detail[1] = moved / (t[2] * 1e-3) / 1e9;
    detail[2] = t[2];
  }
}

// variant = unroll(1|4|8) | (nt ? 0x100 : 0) | (one_shot ? 0x200 : 0) |
// (blocks_per_cu << 16); 0 = default.
struct Variant {
  int unroll = 4;
  bool nt = true;
  int bpc = 8;
  bool one_shot = false;  // grid = one workgroup per 256 x 16 B x unroll (bpc unused)
};
Variant decode(int v) {
  Variant o;
  if (v == 0) return o;
  int u = v & 0xff;
  o.unroll = (u == 1 || u == 4 || u == 8) ? u : 4;
  o.nt = (v & 0x100) != 0;
  o.one_shot = (v & 0x200) != 0;
  int b = (v >> 16) & 0xff;
  o.bpc = (b == 4 || b == 8 || b == 16) ? b : 8;
  return o;
}

// Workgroups of a launch over n vec4s: the persistent grid (CUs x bpc), or
// for a one-shot variant enough workgroups that each lane does `unroll`
// accesses and exits (capped at 2^22 workgroups, where the kernels' grid
// stride takes over: past 16 GiB per array).
int grid_for(const Variant& v, size_t n, int cus) {
  if (!v.one_shot) return cus * v.bpc;
  const size_t per = static_cast<size_t>(kBlock) * v.unroll;
  return static_cast<int>(std::min<size_t>((n + per - 1) / per, size_t{1} << 22));
}

constexpr uint32_t kWriteSeed = 7;
constexpr float kTriadScale = 3.0f;

// f(U, NT) with variant v's unroll and cache policy as compile-time constants
// (std::integral_constant<int, U>, std::bool_constant<NT>).
template <typename F>
void with_variant(const Variant& v, F&& f) {
  auto with_unroll = [&](auto nt) {
    if (v.unroll == 1) f(std::integral_constant<int, 1>{}, nt);
    else if (v.unroll == 8) f(std::integral_constant<int, 8>{}, nt);
    else f(std::integral_constant<int, 4>{}, nt);
  };
  if (v.nt) with_unroll(std::true_type{});
  else with_unroll(std::false_type{});
}

// mode 0 read(a), 1 write(a <- pattern(seed)), 2 copy(b <- a), 3 triad(a <- b + scale*c).
void launch(const Variant& v, int mode, int grid, hipStream_t s, void* a, void* b, void* c, size_t n, uint32_t* sink,
            uint32_t seed = kWriteSeed, float scale = kTriadScale) {
  with_variant(v, [&](auto u, auto nt) {
    constexpr int U = decltype(u)::value;
    constexpr bool NT = decltype(nt)::value;
    switch (mode) {
      case 0: k_read<U, NT><<<grid, kBlock, 0, s>>>(static_cast<const vec4*>(a), n, sink); break;
      case 1: k_write<U, NT><<<grid, kBlock, 0, s>>>(static_cast<vec4*>(a), n, seed); break;
      case 2: k_copy<U, NT><<<grid, kBlock, 0, s>>>(static_cast<const vec4*>(a), static_cast<vec4*>(b), n); break;
      default:
        k_triad<U, NT><<<grid, kBlock, 0, s>>>(static_cast<f32x4*>(a), static_cast<const f32x4*>(b),
                                              static_cast<const f32x4*>(c), scale, n);
    }
  });
}

// One k_segments launch: the checked read when `fold` is given, otherwise
// mode 0 reads into the DCE sink and mode 1 writes the fill.
void launch_segments(int mode, bool nt, int grid, hipStream_t s, vec4* buf, size_t touches, size_t stride_vec,
                     int seg_lanes, uint32_t* sink, unsigned long long* fold) {
  auto with_policy = [&](auto policy) {
    constexpr bool NT = decltype(policy)::value;
    if (fold) k_segments_fold<NT><<<grid, kBlock, 0, s>>>(buf, touches, stride_vec, seg_lanes, fold);
    else if (mode == 0) k_segments<0, NT><<<grid, kBlock, 0, s>>>(buf, touches, stride_vec, seg_lanes, sink);
    else k_segments<1, NT><<<grid, kBlock, 0, s>>>(buf, touches, stride_vec, seg_lanes, sink);
  };
  if (nt) with_policy(std::true_type{});
  else with_policy(std::false_type{});
}

// What xs_segment_access and xs_segment_op both require of a segment layout.
bool segment_args_ok(int mode, int seg_bytes, size_t stride_bytes, size_t touches) {
  return mode >= 0 && mode <= 1 && seg_bytes >= 16 && seg_bytes <= 1024 && seg_bytes % 16 == 0 &&
         stride_bytes % 128 == 0 && stride_bytes >= static_cast<size_t>(seg_bytes) && touches != 0;
}

constexpr int kMaxGrid = 1 << 22;  // grid_for's cap; an explicit grid obeys it too

// Device-side fold of a checked read: [0] XOR of every lane's acc, [1] 16-B
// loads issued. Zeroed here, copied to the caller's two words after the launch.
struct Fold {
  DevMem d;
  int init() {
    XS_CHECK(hipMalloc(&d.p, 2 * sizeof(unsigned long long)));
    XS_CHECK(hipMemset(d.p, 0, 2 * sizeof(unsigned long long)));
    return 0;
  }
  int fetch(unsigned long long* out) {
    XS_CHECK(hipMemcpy(out, d.p, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return 0;
  }
};

// Both k_pinned callers: some of the 8 XCDs, chunk indices that fit its 32-bit counters.
bool pinned_args_ok(int mode, uint32_t xcd_mask, size_t n) {
  return mode >= 0 && mode <= 2 && xcd_mask != 0 && !(xcd_mask & ~0xffu) && n != 0 && n / kChunk < 0xffffff00ull;
}

// Checks k_pinned's counters of every launch, all completed. A workgroup on a
// selected XCD takes chunks from that XCD's counter until its slice is done, so
// a selected XCD with a slice and a counter still 0 received no workgroup and
// its slice was never processed: the first such launch fails with kUndrained.
int check_drained(const XcdCounters& counters, size_t n, uint32_t xcd_mask) {
  std::vector<unsigned> ctr(static_cast<size_t>(counters.launches) * kMaxXcds);
  XS_CHECK(counters.fetch(ctr.data()));
  for (int launch = 0; launch < counters.launches; ++launch) {
    uint32_t missed = 0;
    for (uint32_t x = 0; x < kMaxXcds; ++x) {
      if (!((xcd_mask >> x) & 1u)) continue;
      const auto [c0, c1] = xcd_slice(n, xcd_mask & 0xffu, x);
      if (c1 > c0 && ctr[launch * kMaxXcds + x] == 0) missed |= 1u << x;
    }
    if (!missed) continue;
    std::snprintf(g_err, sizeof g_err,
                  "k_pinned: no workgroup ran on XCD(s) %s of xcd_mask 0x%x (launch %d); their slices were not processed",
                  xsprobe::XcdList(missed).text, xcd_mask, launch);
    return kUndrained;
  }
  return 0;
}

Variant default_variant(int mode) {
  // Measured optimum per mode on MI355X at the 2 GiB working set
  // (profiles/r5_stream_sweep.md, 648 layouts x unroll x policy x grid):
  // read: a persistent grid of 8 workgroups per CU, one non-temporal 16-B
  // load per lane per iteration (~7.0 TB/s, 88%). Write and copy: a one-shot
  // grid, one workgroup per 4 KiB and no loop (write 6.83 TB/s plain, copy
  // 6.48 TB/s non-temporal, vs 5.7 / 5.95 for the best persistent grid):
  // freshly dispatched workgroups keep more stores in flight than a
  // persistent loop whose waves stall on their own store queue.
  Variant v;
  v.unroll = 1;
  v.nt = mode != 1;
  v.bpc = 8;
  v.one_shot = mode != 0;
  return v;
}

}  // namespace

extern "C" {

const char* xs_last_error() { return g_err; }

int xs_device_count() {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

// JSON description of device `dev` into out (len bytes). Returns bytes written or <0.
int xs_device_props(int dev, char* out, int len) {
  hipDeviceProp_t p;
  XS_CHECK(hipGetDeviceProperties(&p, dev));
  size_t free_b = 0, total_b = 0;
  XS_CHECK(hipSetDevice(dev));
  XS_CHECK(hipMemGetInfo(&free_b, &total_b));
  int n = std::snprintf(out, len,
                        "{\"name\":\"%s\",\"gcnArchName\":\"%s\",\"computeUnits\":%d,\"totalGlobalMem\":%zu,"
                        "\"freeMem\":%zu,\"clockRateKHz\":%d,\"memoryClockRateKHz\":%d,\"memoryBusWidth\":%d,"
                        "\"l2CacheSize\":%d,\"pciBusID\":%d,\"pciDeviceID\":%d,\"pciDomainID\":%d,"
                        "\"maxSharedMemoryPerMultiProcessor\":%zu,\"warpSize\":%d}",
                        p.name, p.gcnArchName, p.multiProcessorCount, p.totalGlobalMem, free_b, p.clockRate,
                        p.memoryClockRate, p.memoryBusWidth, p.l2CacheSize, p.pciBusID, p.pciDeviceID, p.pciDomainID,
                        p.maxSharedMemoryPerMultiProcessor, p.warpSize);
  return n;
}

// mode: 0 read, 1 write, 2 copy, 3 triad. bytes = working set per array.
// cu_limit > 0 caps the grid at cu_limit * blocks_per_cu workgroups.
// detail (optional, 3 doubles): min-launch GB/s, batch GB/s, batch ms/launch.
int xs_hbm_bandwidth(int dev, size_t bytes, int iters, int cu_limit, int mode, int variant, double* gbps,
                     double* ms_per_iter, double* detail) {
  const size_t n = bytes / sizeof(vec4);
  if (n == 0 || mode < 0 || mode > 3) return kBadArgs;
  XS_CHECK(hipSetDevice(dev));
  if (iters <= 0) iters = 10;
  bytes = n * sizeof(vec4);
  Variant v = variant == 0 ? default_variant(mode) : decode(variant);
  DevMem a, b, c, sink;
  XS_CHECK(hipMalloc(&a.p, bytes));
  XS_CHECK(hipMalloc(&b.p, bytes));
  if (mode == 3) XS_CHECK(hipMalloc(&c.p, bytes));
  XS_CHECK(hipMalloc(&sink.p, sizeof(uint32_t)));
  int cus = 0;
  XS_CHECK(xsprobe::cu_count(dev, &cus));
  if (cu_limit > 0 && cu_limit < cus) {
    cus = cu_limit;
    v.one_shot = false;  // a CU budget needs the persistent grid
  }
  int grid = grid_for(v, n, cus);
  Stream s;
  XS_CHECK(hipStreamCreateWithFlags(&s.s, hipStreamNonBlocking));
  // Page everything in and warm the launch path.
  launch(Variant{}, 1, grid, s.s, a.p, nullptr, nullptr, n, sink.as<uint32_t>());
  launch(Variant{}, 1, grid, s.s, b.p, nullptr, nullptr, n, sink.as<uint32_t>());
  if (c.p) launch(Variant{}, 1, grid, s.s, c.p, nullptr, nullptr, n, sink.as<uint32_t>());
  XS_CHECK(hipGetLastError());
  launch(v, mode, grid, s.s, a.p, b.p, c.p, n, sink.as<uint32_t>());
  XS_CHECK(hipStreamSynchronize(s.s));
  double t[3];
  auto timed = [&](int) { launch(v, mode, grid, s.s, a.p, b.p, c.p, n, sink.as<uint32_t>()); };
  if (int rc = xsprobe::time_launches(g_err, s.s, iters, timed, t)) return rc;
  report_rate(static_cast<double>(bytes) * (mode == 2 ? 2.0 : mode == 3 ? 3.0 : 1.0), t, gbps, ms_per_iter, detail);
  return 0;
}

// One streaming kernel over caller-owned device buffers (e.g. torch tensors),
// run to completion: the GPU tier checks the kernels' results against exact
// references (a float64 bound for triad; subnormal operands and results are
// kept, the library is built without a flush-to-zero flag). mode 1: a <- pattern(seed); 2: b <- a; 3: a <- b +
// scale*c (float4 lanes). bytes must be a multiple of 16 and every pointer
// 16-byte aligned. variant as in xs_hbm_bandwidth (0 = the tuned default).
// grid > 0 launches that many workgroups instead of the variant's own grid
// (the tests reach the unrolled bodies and the grid-stride path with small
// buffers that way). mode 0 (read a) needs `fold`, two host words: the
// checked read kernel's XOR of all 32-bit words and its count of 16-B loads.
int xs_stream_op(int dev, int mode, void* a, void* b, void* c, size_t bytes, uint32_t seed, float scale, int variant,
                 int grid, unsigned long long* fold) {
  if (mode < 0 || mode > 3 || (mode == 0) != (fold != nullptr) || bytes == 0 || bytes % sizeof(vec4) != 0 ||
      grid < 0 || grid > kMaxGrid)
    return kBadArgs;
  if (bad_buffer(a, sizeof(vec4)) || bad_buffer(b, sizeof(vec4), mode >= 2) || bad_buffer(c, sizeof(vec4), mode == 3))
    return kBadBuffer;
  XS_CHECK(hipSetDevice(dev));
  Variant v = variant == 0 ? default_variant(mode) : decode(variant);
  const size_t n = bytes / sizeof(vec4);
  if (grid == 0) {
    int cus = 0;
    XS_CHECK(xsprobe::cu_count(dev, &cus));
    grid = grid_for(v, n, cus);
  }
  Fold f;
  if (mode == 0) {
    if (int rc = f.init()) return rc;
    with_variant(v, [&](auto u, auto nt) {  // the checked read of variant v: same unroll and cache policy
      k_read_fold<decltype(u)::value, decltype(nt)::value><<<grid, kBlock>>>(static_cast<const vec4*>(a), n,
                                                                             f.d.as<unsigned long long>());
    });
  } else {
    launch(v, mode, grid, nullptr, a, b, c, n, nullptr, seed, scale);
  }
  XS_CHECK(hipGetLastError());
  XS_CHECK(hipDeviceSynchronize());
  return mode == 0 ? f.fetch(fold) : 0;
}

// XCD-pinned streaming over caller-owned buffers (mode 1 write dst, 2 copy
// src -> dst): only workgroups on the XCDs in xcd_mask do the work. Which XCD
// a workgroup lands on is the dispatcher's choice, so the per-XCD counters are
// read back after the launch: -1002 when a selected XCD with a non-empty slice
// received no workgroup (xs_last_error names it); what the other XCDs wrote
// stays. xcd_mask bits above the 8 XCDs are refused. grid > 0 launches that
// many workgroups instead of 8 per CU. mode 0 (read src) needs `fold`, two
// host words as in xs_stream_op.
int xs_pinned_op(int dev, int mode, const void* src, void* dst, size_t bytes, uint32_t xcd_mask, int grid,
                 unsigned long long* fold) {
  const size_t n = bytes / sizeof(vec4);
  if (!pinned_args_ok(mode, xcd_mask, n) || (mode == 0) != (fold != nullptr) || bytes % sizeof(vec4) != 0 ||
      grid < 0 || grid > kMaxGrid)
    return kBadArgs;
  if (bad_buffer(dst, sizeof(vec4), mode != 0) || bad_buffer(src, sizeof(vec4), mode != 1)) return kBadBuffer;
  XS_CHECK(hipSetDevice(dev));
  XcdCounters counters;
  XS_CHECK(counters.init());
  DevMem sink;
  XS_CHECK(hipMalloc(&sink.p, sizeof(uint32_t)));
  if (grid == 0) XS_CHECK(xsprobe::cu_count(dev, &grid, kBlocksPerCu));
  Fold f;
  if (mode == 0) {
    if (int rc = f.init()) return rc;
    k_pinned_fold<<<grid, kBlock>>>(static_cast<const vec4*>(src), n, xcd_mask, counters.of(0),
                                    f.d.as<unsigned long long>());
  } else {
    k_pinned<<<grid, kBlock>>>(static_cast<const vec4*>(src), static_cast<vec4*>(dst), n, xcd_mask, counters.of(0),
                               mode, sink.as<uint32_t>());
  }
  XS_CHECK(hipGetLastError());
  XS_CHECK(hipDeviceSynchronize());
  if (int rc = check_drained(counters, n, xcd_mask)) return rc;
  return mode == 0 ? f.fetch(fold) : 0;
}

// Bandwidth pulled by the workgroups resident on the XCDs in xcd_mask
// (mode 0 read, 1 write, 2 copy). detail as in xs_hbm_bandwidth.
int xs_hbm_bandwidth_xcd(int dev, size_t bytes, int iters, uint32_t xcd_mask, int mode, double* gbps,
                         double* ms_per_iter, double* detail) {
  const size_t n = bytes / sizeof(vec4);
  if (!pinned_args_ok(mode, xcd_mask, n)) return kBadArgs;
  XS_CHECK(hipSetDevice(dev));
  if (iters <= 0) iters = 10;
  bytes = n * sizeof(vec4);
  DevMem a, b, sink;
  XS_CHECK(hipMalloc(&a.p, bytes));
  XS_CHECK(hipMalloc(&b.p, bytes));
  XS_CHECK(hipMalloc(&sink.p, sizeof(uint32_t)));
  XcdCounters counters;  // fresh ones per launch; the warm-up is launch `iters`
  XS_CHECK(counters.init(iters + 1));
  int grid = 0;  // every CU gets 8 workgroups; only masked XCDs work
  XS_CHECK(xsprobe::cu_count(dev, &grid, kBlocksPerCu));
  Stream s;
  XS_CHECK(hipStreamCreateWithFlags(&s.s, hipStreamNonBlocking));
  auto pinned = [&](int i) {
    k_pinned<<<grid, kBlock, 0, s.s>>>(a.as<const vec4>(), b.as<vec4>(), n, xcd_mask, counters.of(i), mode,
                                       sink.as<uint32_t>());
  };
  k_write<4, true><<<grid, kBlock, 0, s.s>>>(a.as<vec4>(), n, 1);
  pinned(iters);
  XS_CHECK(hipGetLastError());
  XS_CHECK(hipStreamSynchronize(s.s));
  double t[3];
  if (int rc = xsprobe::time_launches(g_err, s.s, iters, pinned, t)) return rc;
  // No rate for bytes that were not moved: every launch must have had a
  // workgroup on each selected XCD.
  if (int rc = check_drained(counters, n, xcd_mask)) return rc;
  report_rate(static_cast<double>(bytes) * (mode == 2 ? 2.0 : 1.0), t, gbps, ms_per_iter, detail);
  return 0;
}

// Counter calibration: `touches` segments of `seg_bytes` (16..1024, a
// multiple of 16), one per `stride_bytes` slot (a multiple of 128, >=
// seg_bytes), read (mode 0) or written (mode 1), default or non-temporal
// policy; `iters` timed launches after one warm-up. out: [median ms, bytes
// per dispatch, 128-B lines per dispatch].
int xs_segment_access(int dev, int mode, int nt, int seg_bytes, size_t stride_bytes, size_t touches, int iters,
                      double* out) {
  if (!segment_args_ok(mode, seg_bytes, stride_bytes, touches)) return kBadArgs;
  XS_CHECK(hipSetDevice(dev));
  if (iters <= 0) iters = 10;
  const size_t bytes = stride_bytes * touches;
  const size_t n = bytes / sizeof(vec4);
  DevMem buf, sink;
  XS_CHECK(hipMalloc(&buf.p, bytes));
  XS_CHECK(hipMalloc(&sink.p, sizeof(uint32_t)));
  int grid = 0;
  XS_CHECK(xsprobe::cu_count(dev, &grid, kBlocksPerCu));
  Stream s;
  XS_CHECK(hipStreamCreateWithFlags(&s.s, hipStreamNonBlocking));
  k_write<4, true><<<grid, kBlock, 0, s.s>>>(buf.as<vec4>(), n, 1);  // page in
  auto go = [&](int) {
    launch_segments(mode, nt, grid, s.s, buf.as<vec4>(), touches, stride_bytes / sizeof(vec4), seg_bytes / 16,
                    sink.as<uint32_t>(), nullptr);
  };
  go(0);
  XS_CHECK(hipGetLastError());
  XS_CHECK(hipStreamSynchronize(s.s));
  double t[3];
  if (int rc = xsprobe::time_launches(g_err, s.s, iters, go, t)) return rc;
  out[0] = t[0];
  out[1] = static_cast<double>(touches) * seg_bytes;
  out[2] = static_cast<double>(touches) * ((seg_bytes + 127) / 128);
  return 0;
}

// One k_segments launch (arguments as xs_segment_access) over a caller-owned
// device buffer of stride_bytes x touches bytes, run to completion, so a test
// sees what the kernel touched. mode 1 writes the fill (5, 6, 7, 8); mode 0
// needs `fold`, two host words: XOR of the 32-bit words read, 16-B loads issued.
int xs_segment_op(int dev, int mode, int nt, int seg_bytes, size_t stride_bytes, size_t touches, void* buf,
                  unsigned long long* fold) {
  if (!segment_args_ok(mode, seg_bytes, stride_bytes, touches) || (mode == 0) != (fold != nullptr)) return kBadArgs;
  if (bad_buffer(buf, sizeof(vec4))) return kBadBuffer;
  XS_CHECK(hipSetDevice(dev));
  int grid = 0;
  XS_CHECK(xsprobe::cu_count(dev, &grid, kBlocksPerCu));
  Fold f;
  if (mode == 0) {  // and only then is `fold` given: launch_segments runs the checked read
    if (int rc = f.init()) return rc;
  }
  launch_segments(mode, nt, grid, nullptr, static_cast<vec4*>(buf), touches, stride_bytes / sizeof(vec4),
                  seg_bytes / 16, nullptr, f.d.as<unsigned long long>());
  XS_CHECK(hipGetLastError());
  XS_CHECK(hipDeviceSynchronize());
  return mode == 0 ? f.fetch(fold) : 0;
}

// Launches `blocks` single-wave workgroups; returns the number of distinct
// XCDs observed and writes a 8-entry histogram of blocks per XCD.
int xs_xcd_census(int dev, int blocks, int* xcd_hist8, int* distinct_cus) {
  XS_CHECK(hipSetDevice(dev));
  if (blocks <= 0) blocks = 2048;
  DevMem dx, dh;
  XS_CHECK(hipMalloc(&dx.p, blocks * sizeof(uint32_t)));
  XS_CHECK(hipMalloc(&dh.p, blocks * sizeof(uint32_t)));
  k_census<<<blocks, 64>>>(dx.as<uint32_t>(), dh.as<uint32_t>());
  XS_CHECK(hipGetLastError());
  XS_CHECK(hipDeviceSynchronize());
  std::vector<uint32_t> hx(blocks), hh(blocks);
  XS_CHECK(hipMemcpy(hx.data(), dx.p, blocks * sizeof(uint32_t), hipMemcpyDeviceToHost));
  XS_CHECK(hipMemcpy(hh.data(), dh.p, blocks * sizeof(uint32_t), hipMemcpyDeviceToHost));
  int hist[16] = {0};
  for (int i = 0; i < blocks; ++i) hist[hx[i] & 0xf]++;
  int distinct = 0;
  for (int i = 0; i < 16; ++i) distinct += hist[i] > 0;
  if (xcd_hist8)
    for (int i = 0; i < 8; ++i) xcd_hist8[i] = hist[i];
  if (distinct_cus) {
    // Unique (xcd, HW_ID CU/SE bits) pairs approximate distinct CUs touched.
    int uniq = 0;
    for (int i = 0; i < blocks; ++i) {
      uint32_t key = ((hx[i] & 0xf) << 16) | (hh[i] & 0xfff0);
      bool seen = false;
      for (int j = 0; j < i && !seen; ++j) seen = ((((hx[j] & 0xf) << 16) | (hh[j] & 0xfff0)) == key);
      uniq += !seen;
    }
    *distinct_cus = uniq;
  }
  return distinct;
}

// k_pattern, launched as xs_health_check launches it, over a caller-owned
// device buffer of `bytes` (a multiple of 4, 4-byte aligned): word i <-
// uint32(i * 2654435761) ^ 0xa5a5a5a5.
int xs_pattern_op(int dev, void* buf, size_t bytes) {
  if (bytes == 0 || bytes % sizeof(uint32_t) != 0) return kBadArgs;
  if (bad_buffer(buf, sizeof(uint32_t))) return kBadBuffer;
  XS_CHECK(hipSetDevice(dev));
  int grid = 0;
  XS_CHECK(xsprobe::cu_count(dev, &grid, kBlocksPerCu));
  k_pattern<<<grid, kBlock>>>(static_cast<uint32_t*>(buf), bytes / sizeof(uint32_t));
  XS_CHECK(hipGetLastError());
  XS_CHECK(hipDeviceSynchronize());
  return 0;
}

// k_checksum, launched as xs_health_check launches it, over a caller-owned
// device buffer of `bytes` (a multiple of 4, 4-byte aligned): out_sum <- the
// sum of its 32-bit words.
int xs_checksum_op(int dev, const void* buf, size_t bytes, unsigned long long* out_sum) {
  if (bytes == 0 || bytes % sizeof(uint32_t) != 0 || !out_sum) return kBadArgs;
  if (bad_buffer(buf, sizeof(uint32_t))) return kBadBuffer;
  XS_CHECK(hipSetDevice(dev));
  int grid = 0;
  XS_CHECK(xsprobe::cu_count(dev, &grid, kBlocksPerCu));
  DevMem out;
  XS_CHECK(hipMalloc(&out.p, sizeof(unsigned long long)));
  XS_CHECK(hipMemset(out.p, 0, sizeof(unsigned long long)));
  k_checksum<<<grid, kBlock>>>(static_cast<const uint32_t*>(buf), bytes / sizeof(uint32_t),
                              out.as<unsigned long long>());
  XS_CHECK(hipGetLastError());
  XS_CHECK(hipMemcpy(out_sum, out.p, sizeof *out_sum, hipMemcpyDeviceToHost));
  return 0;
}

// The health check's verdict over a caller-owned device buffer (as
// xs_pattern_op): k_checksum's sum of its words against the host's sum of the
// pattern for that many words. Returns 0 when they agree, 1 when they differ,
// <0 on bad arguments or HIP errors.
int xs_health_verify(int dev, const void* buf, size_t bytes, unsigned long long* device_sum,
                     unsigned long long* host_sum) {
  unsigned long long d = 0;
  if (int rc = xs_checksum_op(dev, buf, bytes, &d)) return rc;
  const size_t n = bytes / sizeof(uint32_t);
  unsigned long long h = 0;
  for (size_t i = 0; i < n; ++i) h += static_cast<uint32_t>(static_cast<uint32_t>(i * 2654435761u) ^ 0xa5a5a5a5u);
  if (device_sum) *device_sum = d;
  if (host_sum) *host_sum = h;
  return d == h ? 0 : 1;
}

// Writes a pattern over `bytes` and verifies its checksum on the host:
// allocate -> xs_pattern_op -> xs_health_verify. Returns 0 when healthy, 1 on
// mismatch, <0 on HIP errors.
int xs_health_check(int dev, size_t bytes, unsigned long long* device_sum, unsigned long long* host_sum) {
  XS_CHECK(hipSetDevice(dev));
  size_t n = bytes / sizeof(uint32_t);
  if (n == 0) n = 1 << 20;
  DevMem buf;
  XS_CHECK(hipMalloc(&buf.p, n * sizeof(uint32_t)));
  if (int rc = xs_pattern_op(dev, buf.p, n * sizeof(uint32_t))) return rc;
  return xs_health_verify(dev, buf.p, n * sizeof(uint32_t), device_sum, host_sum);
}

}  // extern "C"
