// HBM sweep for gfx950 (MI355X): the node agent's memory check.
//
// xs_health_check writes 64 MiB and sums it straight back: a quarter of the
// 256 MiB Infinity Cache, so most likely no DRAM cell is read, and the verdict
// is one sum with no address in it. xs_hbm_sweep is the memory counterpart of
// the CU sweep and the matrix-format sweep: it takes all free HBM, writes an
// address-keyed pattern, reads it back from DRAM in both polarities and says
// which vector, which bits and which direction failed.
//
// Pattern. The unit is one 16-byte vector with a 64-bit index v that runs
// across the whole sweep (not per chunk). With lo = uint32(v),
// hi = uint32(v >> 32) and a 32-bit seed, all arithmetic mod 2^32:
//
//   mix32(x):  x ^= x >> 16;  x *= 0x7feb352d;  x ^= x >> 15;  x *= 0x846ca68b;  x ^= x >> 16
//   word_j(v) = mix32(lo + 0x9E3779B9 * (j + 1)) ^ mix32(hi ^ seed)        j = 0..3
//
// word_j is the j-th little-endian 32-bit word of the vector; the inverted
// pattern is the bitwise complement. mix32 is a bijection, so two vectors whose
// indices differ in any one bit differ (in all four words when the bit is in
// lo or in hi): a stuck or shorted address line reads back another vector's
// data. Every one of the 128 bits takes both values inside any aligned 4 KiB.
// hbm_pattern() below is the one generator, shared by the kernels and the host.
//
// Passes (moving inversions):
//   0 fill             writes the pattern
//   1 verify + invert  reads and checks the pattern, writes the complement of
//                      the EXPECTED value (never of what was read, so an error
//                      does not propagate into pass 2)
//   2 verify           reads and checks the complement
// xs_hbm_sweep runs pass 0 over all chunks, then pass 1 over all chunks, then
// pass 2: every other vector of the sweep is written between a vector's write
// and its read, so from 1 GiB upwards (4x the Infinity Cache, the rule of
// hbm_probe.hip) the reads come from HBM.
//
// Kernel shape: hbm_probe.hip's streaming shape. 256-thread workgroups, a
// persistent grid of 8 per CU, a grid-stride walk in rows, U = 4 independent
// non-temporal 16-byte loads in flight per lane plus a remainder loop, vector
// stores only. The compare is one OR of expected ^ actual over the four
// words; the mismatch path is a rare branch.
//
// Result of one verify launch (HbmSweepResult, device memory zeroed by the
// host): vectors_read; fold = XOR over all vectors read of
// (w0 ^ w2) | (w1 ^ w3) << 32, i.e. of the vector's two little-endian 64-bit
// halves, reduced per wave with shuffles and added with one atomic each per
// wave (with vectors_read it shows every vector was visited once; a vector and
// its complement fold to the same value, so a clean pass 1 and pass 2 agree).
// The waves spread these atomics over 16 stripes of the result, one 128-byte
// line each, and the host adds the stripes up: with all 16,384 atomics of a
// launch on one line they took 0.19 ms, as long as reading 1 GiB
// (profiles/hbm_sweep_defaults.md). Then bad_vectors; bad_bits (popcount of
// expected ^ actual); one_to_zero / zero_to_one bit counts (expected 1 read
// 0 / expected 0 read 1); flip_or[j] = OR of
// expected ^ actual of word j; reader_xcd_mask = OR of 1 << HW_REG_XCC_ID of
// the waves that saw a mismatch (the reader, not the memory channel); and a
// log of at most 32 entries {v, expected[4], actual[4], xcd, pass}, slots
// claimed with an atomicAdd (log_claims counts every claim; faults beyond the
// cap are counted, not logged).
//
// Injection (testing the comparator and the localisation on healthy memory):
// xs_hbm_sweep flips the bits of inject_mask in word inject_word of global
// vector inject_vec after pass 0 or after pass 1, from the host, with an
// 8-byte read-xor-write hipMemcpy into a chunk the sweep owns. The kernels know
// nothing of it and no access leaves the sweep's own buffers.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "hip/sweep_common.h"

#define XS_ERR_BUF g_hbm_err

namespace {

xsprobe::ErrBuf g_hbm_err;

using xsprobe::DevMem;
using xsprobe::Event;
using xsprobe::Stream;
using xsprobe::kBadArgs;
using xsprobe::xcc_id;

typedef uint32_t vec4 __attribute__((ext_vector_type(4)));  // 16 B/lane

constexpr int kBlock = 256;           // 4 waves of 64 lanes
constexpr int kUnroll = 4;            // independent 16-B loads in flight per lane
constexpr int kBlocksPerCu = 8;       // persistent grid
constexpr int kMaxGrid = 1 << 22;
constexpr uint32_t kLogCap = 32;
constexpr int kStripes = 16;          // lines the waves' fold atomics are spread over
constexpr int kMaxBadChunks = 64;     // per-chunk counts reported (sparse); the rest are only summed
constexpr size_t kMaxChunks = 1 << 16;
constexpr size_t kDefaultChunk = size_t{1} << 30;
constexpr size_t kReserve = size_t{2} << 30;  // left free when the budget is "all free HBM"
constexpr int kBadBuffer = -1001;
constexpr int kUnswept = -1003;       // no chunk could be allocated: nothing was tested
constexpr uint64_t kNoInject = ~uint64_t{0};

struct HbmLogEntry {
  uint64_t v;
  uint32_t expected[4];
  uint32_t actual[4];
  uint32_t xcd, pass;
};
static_assert(sizeof(HbmLogEntry) == 48, "fixed layout (ops/hip_probe.py mirrors it)");

struct HbmStripe {  // one 128-byte line
  unsigned long long vectors_read, fold, reserved[14];
};

struct alignas(128) HbmSweepResult {
  HbmStripe stripe[kStripes];  // vectors_read is their sum, the fold their XOR
  unsigned long long bad_vectors, bad_bits, one_to_zero, zero_to_one;
  uint32_t flip_or[4];
  uint32_t reader_xcd_mask, log_claims;
  HbmLogEntry log[kLogCap];
};
static_assert(sizeof(HbmStripe) == 128 && sizeof(HbmSweepResult) == 3712 && offsetof(HbmSweepResult, log) == 2104,
              "fixed layout (ops/hip_probe.py mirrors it)");

struct HbmBadChunk {
  uint64_t chunk, bad_vectors;
};

struct HbmSweepSummary {
  uint64_t bytes_requested, bytes_tested, chunk_bytes;
  uint32_t chunks, short_;
  unsigned long long vectors_read, fold[2], bad_vectors, bad_bits, one_to_zero, zero_to_one;  // fold per verify pass
  uint32_t flip_or[4];
  uint32_t reader_xcd_mask, log_entries;
  double ms[3];
  uint32_t bad_chunks, reserved;  // chunks with a bad vector; the first kMaxBadChunks follow
  HbmBadChunk bad_chunk[kMaxBadChunks];
};
static_assert(sizeof(HbmSweepSummary) == 144 + 16 * kMaxBadChunks, "fixed layout (ops/hip_probe.py mirrors it)");

__host__ __device__ __forceinline__ uint32_t mix32(uint32_t x) {
  x ^= x >> 16;
  x *= 0x7feb352du;
  x ^= x >> 15;
  x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}

// The high-index term of a vector: constant over 2^32 vectors (64 GiB).
__host__ __device__ __forceinline__ uint32_t hbm_hi_term(uint64_t v, uint32_t seed) {
  return mix32(static_cast<uint32_t>(v >> 32) ^ seed);
}

// The pattern of vector v given its high-index term; inv is 0 or ~0.
__host__ __device__ __forceinline__ vec4 hbm_pattern_lo(uint32_t lo, uint32_t hterm, uint32_t inv) {
  const uint32_t m = hterm ^ inv;
  vec4 w;
  w.x = mix32(lo + 0x9E3779B9u * 1u) ^ m;
  w.y = mix32(lo + 0x9E3779B9u * 2u) ^ m;
  w.z = mix32(lo + 0x9E3779B9u * 3u) ^ m;
  w.w = mix32(lo + 0x9E3779B9u * 4u) ^ m;
  return w;
}

__host__ __device__ __forceinline__ vec4 hbm_pattern(uint64_t v, uint32_t seed, uint32_t inv) {
  return hbm_pattern_lo(static_cast<uint32_t>(v), hbm_hi_term(v, seed), inv);
}

// A lane's pattern generator: the high term is recomputed only when the
// lane's walk crosses a multiple of 2^32 vectors, so a vector costs the eight
// multiplies of its four low-index words.
struct LanePattern {
  uint32_t seed, inv, hi, hterm;
  __device__ __forceinline__ LanePattern(uint64_t v0, uint32_t seed_, uint32_t inv_)
      : seed(seed_), inv(inv_), hi(static_cast<uint32_t>(v0 >> 32)), hterm(hbm_hi_term(v0, seed_)) {}
  __device__ __forceinline__ vec4 at(uint64_t v) {
    const uint32_t h = static_cast<uint32_t>(v >> 32);
    if (h != hi) {
      hi = h;
      hterm = mix32(h ^ seed);
    }
    return hbm_pattern_lo(static_cast<uint32_t>(v), hterm, inv);
  }
};

__global__ __launch_bounds__(kBlock) void k_hbm_fill(vec4* __restrict__ buf, size_t n, uint64_t first_vec,
                                                     uint32_t seed) {
  const size_t stride = static_cast<size_t>(gridDim.x) * kBlock;
  size_t i = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  LanePattern pat(first_vec + i, seed, 0u);
  for (; i + (kUnroll - 1) * stride < n; i += kUnroll * stride) {
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) __builtin_nontemporal_store(pat.at(first_vec + i + u * stride), &buf[i + u * stride]);
  }
  for (; i < n; i += stride) __builtin_nontemporal_store(pat.at(first_vec + i), &buf[i]);
}

// The rare path: one lane found expected != actual.
__device__ __forceinline__ void hbm_report(HbmSweepResult* __restrict__ r, uint64_t v, vec4 e, vec4 a, uint32_t pass) {
  const vec4 d = e ^ a;
  const uint32_t down = __popc(d.x & e.x) + __popc(d.y & e.y) + __popc(d.z & e.z) + __popc(d.w & e.w);
  const uint32_t up = __popc(d.x & ~e.x) + __popc(d.y & ~e.y) + __popc(d.z & ~e.z) + __popc(d.w & ~e.w);
  const uint32_t xcd = xcc_id();
  atomicAdd(&r->bad_vectors, 1ull);
  atomicAdd(&r->bad_bits, static_cast<unsigned long long>(down + up));
  atomicAdd(&r->one_to_zero, static_cast<unsigned long long>(down));
  atomicAdd(&r->zero_to_one, static_cast<unsigned long long>(up));
  if (d.x) atomicOr(&r->flip_or[0], d.x);
  if (d.y) atomicOr(&r->flip_or[1], d.y);
  if (d.z) atomicOr(&r->flip_or[2], d.z);
  if (d.w) atomicOr(&r->flip_or[3], d.w);
  atomicOr(&r->reader_xcd_mask, 1u << xcd);
  const uint32_t slot = atomicAdd(&r->log_claims, 1u);
  if (slot < kLogCap) {
    HbmLogEntry* g = &r->log[slot];
    g->v = v;
    g->expected[0] = e.x, g->expected[1] = e.y, g->expected[2] = e.z, g->expected[3] = e.w;
    g->actual[0] = a.x, g->actual[1] = a.y, g->actual[2] = a.z, g->actual[3] = a.w;
    g->xcd = xcd;
    g->pass = pass;
  }
}

// Pass 1 (INVERT: expects the pattern, writes the complement of the expected
// value) and pass 2 (expects the complement, writes nothing). inv is the
// polarity of what is expected: 0 or ~0.
template <bool INVERT>
__global__ __launch_bounds__(kBlock) void k_hbm_verify(vec4* __restrict__ buf, size_t n, uint64_t first_vec,
                                                       uint32_t seed, uint32_t inv, uint32_t pass,
                                                       HbmSweepResult* __restrict__ res) {
  const size_t stride = static_cast<size_t>(gridDim.x) * kBlock;
  size_t i = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  LanePattern pat(first_vec + i, seed, inv);
  uint32_t f0 = 0, f1 = 0;
  unsigned long long loads = 0;
  for (; i + (kUnroll - 1) * stride < n; i += kUnroll * stride) {
    vec4 a[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) a[u] = __builtin_nontemporal_load(&buf[i + u * stride]);
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const uint64_t v = first_vec + i + u * stride;
      const vec4 e = pat.at(v);
      const vec4 d = e ^ a[u];
      f0 ^= a[u].x ^ a[u].z;
      f1 ^= a[u].y ^ a[u].w;
      if (d.x | d.y | d.z | d.w) hbm_report(res, v, e, a[u], pass);
      if constexpr (INVERT) __builtin_nontemporal_store(~e, &buf[i + u * stride]);
    }
    loads += kUnroll;
  }
  for (; i < n; i += stride) {
    const vec4 a = __builtin_nontemporal_load(&buf[i]);
    const uint64_t v = first_vec + i;
    const vec4 e = pat.at(v);
    const vec4 d = e ^ a;
    f0 ^= a.x ^ a.z;
    f1 ^= a.y ^ a.w;
    if (d.x | d.y | d.z | d.w) hbm_report(res, v, e, a, pass);
    if constexpr (INVERT) __builtin_nontemporal_store(~e, &buf[i]);
    ++loads;
  }
  // Every lane of the wave arrives here: reduce, then one atomic each per wave.
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    f0 ^= __shfl_down(f0, off, 64);
    f1 ^= __shfl_down(f1, off, 64);
    loads += __shfl_down(loads, off, 64);
  }
  if ((threadIdx.x & 63) == 0 && loads != 0) {
    HbmStripe* st = &res->stripe[(blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6)) % kStripes];
    atomicXor(&st->fold, static_cast<unsigned long long>(f0) | static_cast<unsigned long long>(f1) << 32);
    atomicAdd(&st->vectors_read, loads);
  }
}

hipError_t production_grid(int dev, int* grid) { return xsprobe::cu_count(dev, grid, kBlocksPerCu); }

void launch_pass(int pass, int grid, hipStream_t s, void* buf, size_t n, uint64_t first_vec, uint32_t seed,
                 HbmSweepResult* res) {
  vec4* p = static_cast<vec4*>(buf);
  if (pass == 0) k_hbm_fill<<<grid, kBlock, 0, s>>>(p, n, first_vec, seed);
  else if (pass == 1) k_hbm_verify<true><<<grid, kBlock, 0, s>>>(p, n, first_vec, seed, 0u, 1u, res);
  else k_hbm_verify<false><<<grid, kBlock, 0, s>>>(p, n, first_vec, seed, ~0u, 2u, res);
}

}  // namespace

extern "C" {

const char* xs_hbm_sweep_last_error() { return g_hbm_err; }

// Host only: out_words <- the 4 x nvec words of vectors [first_vec, first_vec + nvec).
int xs_hbm_sweep_pattern(uint64_t first_vec, size_t nvec, uint32_t seed, int inverted, uint32_t* out_words) {
  if (!out_words) return kBadArgs;
  const uint32_t inv = inverted ? ~0u : 0u;
  for (size_t i = 0; i < nvec; ++i) {
    const vec4 w = hbm_pattern(first_vec + i, seed, inv);
    out_words[4 * i + 0] = w.x;
    out_words[4 * i + 1] = w.y;
    out_words[4 * i + 2] = w.z;
    out_words[4 * i + 3] = w.w;
  }
  return 0;
}

// One pass (0 fill, 1 verify + invert, 2 verify) over a caller-owned device
// buffer whose first vector has global index first_vec, run to completion.
// grid 0: the production grid (8 workgroups per CU). result (host, one
// HbmSweepResult) is written for passes 1 and 2 and may be null for pass 0.
// -1000: bytes == 0, bytes % 16, unknown pass, bad grid, pass 1/2 without
// result; -1001: null or mis-aligned buffer. Nothing is launched then.
int xs_hbm_sweep_op(int dev, int pass, void* buf, size_t bytes, uint64_t first_vec, uint32_t seed, int grid,
                    void* result) {
  if (pass < 0 || pass > 2 || bytes == 0 || bytes % sizeof(vec4) != 0 || grid < 0 || grid > kMaxGrid ||
      (pass != 0 && !result))
    return kBadArgs;
  if (!buf || (reinterpret_cast<uintptr_t>(buf) & (sizeof(vec4) - 1))) return kBadBuffer;
  XS_CHECK(hipSetDevice(dev));
  if (grid == 0) XS_CHECK(production_grid(dev, &grid));
  DevMem res;
  if (pass != 0) {
    XS_CHECK(hipMalloc(&res.p, sizeof(HbmSweepResult)));
    XS_CHECK(hipMemset(res.p, 0, sizeof(HbmSweepResult)));
  }
  launch_pass(pass, grid, nullptr, buf, bytes / sizeof(vec4), first_vec, seed, res.as<HbmSweepResult>());
  XS_CHECK(hipGetLastError());
  XS_CHECK(hipDeviceSynchronize());
  if (pass != 0) XS_CHECK(hipMemcpy(result, res.p, sizeof(HbmSweepResult), hipMemcpyDeviceToHost));
  return 0;
}

// The whole sweep of `bytes` of HBM (0: hipMemGetInfo's free minus a 2 GiB
// reserve), rounded down to 16 B, taken with hipMalloc in chunks of
// chunk_bytes (0: 1 GiB; the last chunk is shorter). All chunks are held until
// pass 2 is done: freeing one and allocating the next would hand back the same
// pages. An allocation that fails part-way means another tenant took the
// memory: what was obtained is swept and summary->short_ = 1. When not even
// the first chunk could be had, nothing is tested and the return is -1003: the
// caller reports the GPU as unswept, never as failed.
// inject_vec != ~0: see the header. summary: one HbmSweepSummary; log: room
// for 32 HbmLogEntry (summary->log_entries are filled, in chunk then pass
// order). Returns 0 when the sweep ran (faults are in the summary), -1000 for
// bad arguments, -1003 unswept, or a negative HIP error.
int xs_hbm_sweep(int dev, size_t bytes, size_t chunk_bytes, uint32_t seed, uint64_t inject_vec, int inject_word,
                 uint32_t inject_mask, int inject_after_pass, void* summary, void* log) {
  if (!summary || !log) return kBadArgs;
  if (chunk_bytes == 0) chunk_bytes = kDefaultChunk;
  if (chunk_bytes % sizeof(vec4) != 0) return kBadArgs;
  const bool inject = inject_vec != kNoInject;
  if (inject && (inject_word < 0 || inject_word > 3 || inject_after_pass < 0 || inject_after_pass > 1)) return kBadArgs;
  XS_CHECK(hipSetDevice(dev));
  if (bytes == 0) {
    size_t free_b = 0, total_b = 0;
    XS_CHECK(hipMemGetInfo(&free_b, &total_b));
    if (free_b <= kReserve + sizeof(vec4)) {
      std::snprintf(g_hbm_err, sizeof g_hbm_err, "unswept: %zu bytes free, the reserve is %zu", free_b, kReserve);
      return kUnswept;
    }
    bytes = free_b - kReserve;
  }
  bytes &= ~(sizeof(vec4) - 1);
  if (bytes == 0) return kBadArgs;
  const size_t want = (bytes + chunk_bytes - 1) / chunk_bytes;
  if (want > kMaxChunks) return kBadArgs;
  const size_t chunk_vecs = chunk_bytes / sizeof(vec4);

  std::vector<DevMem> chunk(want);
  std::vector<size_t> nvec(want, 0);
  size_t got = 0, tested = 0;
  for (; got < want; ++got) {
    const size_t sz = std::min(chunk_bytes, bytes - got * chunk_bytes);
    if (hipMalloc(&chunk[got].p, sz) != hipSuccess) {
      chunk[got].p = nullptr;
      (void)hipGetLastError();  // the failed allocation is an answer, not an error of the sweep
      break;
    }
    nvec[got] = sz / sizeof(vec4);
    tested += sz;
  }
  if (got == 0) {
    std::snprintf(g_hbm_err, sizeof g_hbm_err, "unswept: could not allocate the first chunk of %zu bytes",
                  std::min(chunk_bytes, bytes));
    return kUnswept;
  }
  size_t inj_chunk = 0, inj_off = 0;
  if (inject) {
    inj_chunk = inject_vec / chunk_vecs;
    inj_off = inject_vec % chunk_vecs;
    if (inj_chunk >= got || inj_off >= nvec[inj_chunk]) return kBadArgs;
  }

  // One result per (chunk, verify pass): [2c] pass 1, [2c + 1] pass 2.
  DevMem res;
  const size_t res_bytes = 2 * got * sizeof(HbmSweepResult);
  XS_CHECK(hipMalloc(&res.p, res_bytes));
  XS_CHECK(hipMemset(res.p, 0, res_bytes));
  int grid = 0;
  XS_CHECK(production_grid(dev, &grid));
  Stream s;
  XS_CHECK(hipStreamCreateWithFlags(&s.s, hipStreamNonBlocking));
  Event ev[6];
  for (auto& e : ev) XS_CHECK(hipEventCreate(&e.e));
  XS_CHECK(hipDeviceSynchronize());  // the memset above, before work on a non-blocking stream
  for (int pass = 0; pass < 3; ++pass) {
    XS_CHECK(hipEventRecord(ev[2 * pass].e, s.s));
    for (size_t c = 0; c < got; ++c) {
      HbmSweepResult* r = pass == 0 ? nullptr : res.as<HbmSweepResult>() + 2 * c + (pass - 1);
      launch_pass(pass, grid, s.s, chunk[c].p, nvec[c], c * chunk_vecs, seed, r);
    }
    XS_CHECK(hipGetLastError());
    XS_CHECK(hipEventRecord(ev[2 * pass + 1].e, s.s));
    XS_CHECK(hipEventSynchronize(ev[2 * pass + 1].e));
    if (inject && pass == inject_after_pass) {
      // The 8 aligned bytes that hold the word: read, flip, write back.
      char* at = chunk[inj_chunk].as<char>() + inj_off * sizeof(vec4) + (inject_word & ~1) * sizeof(uint32_t);
      uint32_t pair[2];
      XS_CHECK(hipMemcpy(pair, at, sizeof pair, hipMemcpyDeviceToHost));
      pair[inject_word & 1] ^= inject_mask;
      XS_CHECK(hipMemcpy(at, pair, sizeof pair, hipMemcpyHostToDevice));
    }
  }

  std::vector<HbmSweepResult> h(2 * got);
  XS_CHECK(hipMemcpy(h.data(), res.p, res_bytes, hipMemcpyDeviceToHost));
  HbmSweepSummary out;
  std::memset(&out, 0, sizeof out);
  out.bytes_requested = bytes;
  out.bytes_tested = tested;
  out.chunk_bytes = chunk_bytes;
  out.chunks = static_cast<uint32_t>(got);
  out.short_ = got < want ? 1u : 0u;
  HbmLogEntry* lg = static_cast<HbmLogEntry*>(log);
  for (size_t c = 0; c < got; ++c) {
    unsigned long long bad_here = 0;
    for (int k = 0; k < 2; ++k) {
      const HbmSweepResult& r = h[2 * c + k];
      for (const HbmStripe& st : r.stripe) {
        out.vectors_read += st.vectors_read;
        out.fold[k] ^= st.fold;
      }
      out.bad_vectors += r.bad_vectors;
      out.bad_bits += r.bad_bits;
      out.one_to_zero += r.one_to_zero;
      out.zero_to_one += r.zero_to_one;
      for (int j = 0; j < 4; ++j) out.flip_or[j] |= r.flip_or[j];
      out.reader_xcd_mask |= r.reader_xcd_mask;
      bad_here += r.bad_vectors;
      const uint32_t logged = std::min(r.log_claims, kLogCap);
      for (uint32_t e = 0; e < logged && out.log_entries < kLogCap; ++e) lg[out.log_entries++] = r.log[e];
    }
    if (bad_here) {
      if (out.bad_chunks < static_cast<uint32_t>(kMaxBadChunks)) out.bad_chunk[out.bad_chunks] = {c, bad_here};
      ++out.bad_chunks;
    }
  }
  for (int pass = 0; pass < 3; ++pass) {
    float ms = 0.f;
    XS_CHECK(hipEventElapsedTime(&ms, ev[2 * pass].e, ev[2 * pass + 1].e));
    out.ms[pass] = ms;
  }
  std::memcpy(summary, &out, sizeof out);
  return 0;
}

}  // extern "C"
