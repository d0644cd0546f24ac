// What the sweeps over named parts share (paths in lane_sweep.hip, units in
// valu_sweep.hip, formats in matrix_sweep.hip): a bit mask selects the parts, a
// workgroup's record carries fail bits that are part bits and one digest per
// part. The lane and VALU sweeps also share how a received word enters a
// part's tally and how a workgroup's 256 tallies become its 128-byte record;
// k_matrix_sweep reduces with wave shuffles and shares the mask check alone.
#pragma once

#include "hip/sweep_common.h"

namespace xsprobe {

constexpr int kPartBlock = 256;  // 4 waves: one per SIMD

// A selection of parts: at least one, none beyond `all`.
inline bool bad_part_mask(uint32_t mask, uint32_t all) { return mask == 0 || (mask & ~all); }

// The murmur3 finaliser, a bijection of 32 bits: what the operands are hashed with.
__host__ __device__ __forceinline__ uint32_t fmix32(uint32_t h) {
  h ^= h >> 16;
  h *= 0x85ebca6bu;
  h ^= h >> 13;
  h *= 0xc2b2ae35u;
  h ^= h >> 16;
  return h;
}

// One thread's mismatches and digest of one part.
struct Tally {
  uint32_t bad = 0, digest = 0;
};

// The workgroup digest a healthy CU leaves per part; 0 for a part not selected.
template <int N>
struct PartExpect {
  uint32_t digest[N];
};

// How a record of N parts begins; a reserved word and the sweep's own tail follow.
template <int N>
struct PartRecordHead {
  uint32_t xcd, cu, simd_mask, fail;  // fail: bit = part
  uint32_t bad[N];
  uint32_t digest[N];  // 0 for a part not selected
  uint32_t bad_simds;  // SIMD ids whose wave mis-compared
};

// Takes the word a thread received at flat index `idx` of a part into the
// part's tally. An injected part flips bit 0 of word 0 first (registers only);
// a probe stores the word to `dump` (a sweep: nullptr). Returns got != want.
__device__ __forceinline__ uint32_t take_word(Tally& y, uint32_t* dump, uint32_t idx, uint32_t got, uint32_t want,
                                              bool injected) {
  if (injected && idx == 0) got ^= 1u;
  if (dump) dump[idx] = got;
  const uint32_t ne = got != want;
  y.bad += ne;
  y.digest += got * (2u * idx + 1u);
  return ne;
}

// LDS words the reduction below uses, from the start of the allocation.
template <int B = kPartBlock>
constexpr uint32_t part_reduction_words(int n, int extra) {
  return (2 * n + 2 + extra) * B;
}

// The B threads' tallies (256 unless the sweep says otherwise) and `extra` (X words a thread ORs in, written
// behind the reserved word) become the workgroup's record: every thread stores
// its words to `lds` as [quantity][thread]; after a barrier thread 0 sums the
// counts and digests, ORs the rest, fails a selected part that counted a
// mismatch or whose digest is not the host's, and writes the record with
// vector stores. No shuffle, DPP or permute: lane_sweep.hip tests those.
// A block above 256 threads sums in two stages: lane 0 of every wave folds its
// wave's 64 words of each quantity into its own, and after another barrier
// thread 0 sums one word per wave.
template <int N, int X, int B = kPartBlock, typename Record>
__device__ __forceinline__ void reduce_parts(uint32_t* lds, uint32_t t, uint32_t simd, const Tally (&y)[N],
                                             const uint32_t* extra, uint32_t part_mask, const PartExpect<N>& expect,
                                             uint32_t xcd, uint32_t cu, Record* record) {
  constexpr uint32_t kBadSimds = 2 * N, kSimds = 2 * N + 1, kWords = 2 * N + 2 + X;
  constexpr uint32_t kHead = sizeof(PartRecordHead<N>) / 4, kRecord = sizeof(Record) / 4;
  static_assert(sizeof(Record) == 128 && kHead + 1 + X <= kRecord, "the record holds the head and the extra words");
  __syncthreads();
  uint32_t any = 0;
#pragma unroll
  for (int p = 0; p < N; ++p) {
    lds[p * B + t] = y[p].bad;
    lds[(N + p) * B + t] = y[p].digest;
    any |= y[p].bad;
  }
  lds[kBadSimds * B + t] = any ? 1u << simd : 0u;
  lds[kSimds * B + t] = 1u << simd;
#pragma unroll
  for (int q = 0; q < X; ++q) lds[(kSimds + 1 + q) * B + t] = extra[q];
  __syncthreads();
  constexpr int kStride = B > kPartBlock ? 64 : 1;  // thread 0 reads every kStride-th word
  if constexpr (kStride > 1) {
    if ((t & 63u) == 0) {
      uint32_t part[kWords] = {};
      for (int j = 0; j < 64; ++j) {
#pragma unroll
        for (uint32_t q = 0; q < 2 * N; ++q) part[q] += lds[q * B + t + j];
#pragma unroll
        for (uint32_t q = 2 * N; q < kWords; ++q) part[q] |= lds[q * B + t + j];
      }
#pragma unroll
      for (uint32_t q = 0; q < kWords; ++q) lds[q * B + t] = part[q];
    }
    __syncthreads();
  }
  if (t == 0) {
    uint32_t sum[kWords] = {};
    for (int u = 0; u < B; u += kStride) {
#pragma unroll
      for (uint32_t q = 0; q < 2 * N; ++q) sum[q] += lds[q * B + u];
#pragma unroll
      for (uint32_t q = 2 * N; q < kWords; ++q) sum[q] |= lds[q * B + u];
    }
    uint32_t fail = 0;
#pragma unroll
    for (int p = 0; p < N; ++p)
      if (((part_mask >> p) & 1u) && (sum[p] || sum[N + p] != expect.digest[p])) fail |= 1u << p;
    uint32_t w[kRecord] = {xcd, cu, sum[kSimds], fail};
#pragma unroll
    for (uint32_t q = 0; q < 2 * N; ++q) w[4 + q] = sum[q];
    w[kHead - 1] = sum[kBadSimds];
#pragma unroll
    for (uint32_t q = 0; q < X; ++q) w[kHead + 1 + q] = sum[kSimds + 1 + q];
    u32x4* out = reinterpret_cast<u32x4*>(record);
#pragma unroll
    for (uint32_t q = 0; q < kRecord / 4; ++q) out[q] = u32x4{w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]};
  }
}

}  // namespace xsprobe
