// Matrix-format sweep for gfx950 (MI355X): every data path through the matrix
// cores, checked on every CU.
//
// k_cu_sweep runs one matrix instruction (v_mfma_f32_32x32x16_bf16). The
// matrix cores have other decoders and data paths, and a CU whose fp8 decoder,
// block-scale path or f64 path mis-computes passes that check. k_matrix_sweep
// is the same kind of launch (256-thread workgroups that each hold more than
// half of a CU's LDS, 4 x CUs of them, every workgroup self-contained) and
// runs, on each of the four waves of a workgroup, one exact product per format:
//
//   bit name   instruction                               K/step  operand per lane
//    0  f16    v_mfma_f32_32x32x16_f16                     16    8 x f16
//    1  f32    v_mfma_f32_32x32x2_f32                       2    1 x f32
//    2  f64    v_mfma_f64_16x16x4_f64 (16x16 tile)          4    1 x f64
//    3  fp8    v_mfma_f32_32x32x16_fp8_fp8  (OCP e4m3fn)   16    8 bytes
//    4  bf8    v_mfma_f32_32x32x16_bf8_bf8  (OCP e5m2)     16    8 bytes
//    5  i8     v_mfma_i32_32x32x32_i8                      32    16 bytes
//    6  mxfp8  v_mfma_scale_f32_32x32x64_f8f6f4 cbsz=blgp=0  64  32 x e4m3 in 8 VGPRs + E8M0 scale
//    7  mxbf8    "                              cbsz=blgp=1  64  32 x e5m2 in 8 VGPRs + scale
//    8  mxfp6    "                              cbsz=blgp=2  64  32 x e2m3 in 6 VGPRs + scale
//    9  mxbf6    "                              cbsz=blgp=3  64  32 x e3m2 in 6 VGPRs + scale
//   10  mxfp4    "                              cbsz=blgp=4  64  32 x e2m1 in 4 VGPRs + scale
//
// Each row runs two K-steps into one accumulator. bf16 stays with k_cu_sweep.
//
// Inputs are encodings produced by a_code<F>(row, k) / b_code<F>(k, col) (and
// a_scale / b_scale for the MX rows), __host__ __device__ functions shared by
// the kernels and the host reference. The kernels assemble them into operand
// registers with integer shifts: nothing is loaded from memory and no
// conversion instruction produces an operand, so the host decodes the very
// bits the MFMA saw. The value ranges keep every partial sum, in any order,
// an exact multiple of 2^-frac below 2^24 units (2^31 for f64 and i8); the
// bound stands next to each generator and expected_tile() re-checks it. The
// result is therefore one exact number per element, with no tolerance.
//
// Operand maps the sweep relies on (lane l; pinned by the tile test of
// tests/test_gpu_matrix_sweep.py against an independent numpy decode):
//   f16        r = l&31, h = l>>5: element j is A[r][k0+8h+j], B[k0+8h+j][r]
//   f32        A[l&31][k0 + (l>>5)], B[k0 + (l>>5)][l&31]
//   f64        A[l&15][k0 + (l>>4)], B[k0 + (l>>4)][l&15]
//   fp8, bf8   byte j (little-endian in the 64-bit operand) is k = k0+8h+j
//   i8         byte j of the 128-bit operand is k = k0+16h+j
//   f8f6f4     32 elements per lane, packed densely little-endian: bits
//              [w*j, w*j+w) of the register stream, w = 8, 6 or 4 (fp4: low
//              nibble first; fp6: one 192-bit stream).
//              fp6, fp4: element j is k = k0+32h+j.
//              fp8, bf8: element j is k = k0+16h+(j&15)+32(j>>4): a lane holds
//              16 elements of each of the two 32-element k-blocks.
//              Scales go by k-block, not by lane: the elements of k-block
//              (k-k0)>>5 = g of row (column) r take the scale byte of lane
//              32g+r. For fp6/fp4 that is the lane's own 32 elements; for
//              fp8/bf8 a lane's bytes 16..31 take the scale of the lane 32
//              above or below (laying fp8 out like fp4 mis-scales half of K:
//              1006 of 1024 results were wrong). Lane 32g+r therefore holds
//              the A scale of (row r, block k0/32+g) and the B scale of (that
//              block, column r). The byte of the scale register is chosen by
//              opsel (0..3 = byte 0..3). A product pins which element of A
//              meets which element of B and which scale each takes; an order
//              of the elements inside a k-block that A and B share (the
//              nibble order of fp4, say) cancels out of every product. What
//              is pinned there is that A and B agree: reversing the nibbles
//              of A alone fails the tile test.
//   C/D        32x32: register q is C[(q&3) + 8(q>>2) + 4h][r];
//              f64 16x16: register q is C[(l>>4) + 4q][l&15].
//
// Digest of one wave's tile: D = sum_ij uint32(fix[i][j]) * (2(tile*i + j) + 1)
// with fix = C * 2^frac as an integer (a swapped pair of unequal elements
// changes it); the wave also checks that every accumulator converts to that
// integer without loss. Workgroup digest: sum_w D_w << w (15 D when healthy).
//
// One 64-byte record per workgroup: {xcd, cu key, simd mask, format fail mask,
// 11 workgroup digests (0 for a format not selected), 0}. XCC id and the CU key
// (bits 15:8 of HW_REG_HW_ID) are read as in cu_sweep.hip.
//
// Injection: a workgroup on inject_xcd whose CU key is inject_cu (or any, with
// -1) flips the low bit of fix[.] of lane 0, register 0 of wave 0 for each
// format in inject_formats before the digest. Registers only.
//
// k_matrix_tile<F> runs the same mfma_tile<F>() on one wave and stores the
// whole result tile: the checked instantiation of what the sweep digests.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <type_traits>
#include <vector>

#include "hip/part_sweep.h"

#define XS_ERR_BUF g_matrix_err
#define XS_HD __host__ __device__ __forceinline__

namespace {

xsprobe::ErrBuf g_matrix_err;

using namespace xsprobe;

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef uint16_t u16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef double f64x4 __attribute__((ext_vector_type(4)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef int i32x16 __attribute__((ext_vector_type(16)));

enum Fmt : int { kF16, kF32, kF64, kFp8, kBf8, kI8, kMxFp8, kMxBf8, kMxFp6, kMxBf6, kMxFp4, kNumFmt };
const char kFmtNames[] = "f16,f32,f64,fp8,bf8,i8,mxfp8,mxbf8,mxfp6,mxbf6,mxfp4";
constexpr uint32_t kAllFormats = (1u << kNumFmt) - 1;

enum Kind : int { kPlain, kByte, kInt8, kMx };
enum AccKind : int { kAccF32, kAccF64, kAccI32 };

// Operands are mini-floats of `ebits` exponent and `mbits` mantissa bits with
// bias 2^(ebits-1) - 1 (f16, f32, f64, e4m3, e5m2, e2m3, e3m2 and e2m1 all are).
struct Desc {
  int kind, acc;
  int ebits, mbits;
  int tile;   // the result is tile x tile
  int kstep;  // K of one instruction; every format runs two
  int frac;   // every result is a multiple of 2^-frac
  int mu;     // kPlain: mantissa bits the generators use
  int eb0;    // kByte: lowest exponent field of B
  int amax, bmax, cap;  // kMx: largest magnitude code of A and of B; A capped by its scale
};

constexpr Desc kDesc[kNumFmt] = {
    /* f16   */ {kPlain, kAccF32, 5, 10, 32, 16, 9, 3, 0, 0, 0, 0},
    /* f32   */ {kPlain, kAccF32, 8, 23, 32, 2, 15, 6, 0, 0, 0, 0},
    /* f64   */ {kPlain, kAccF64, 11, 52, 16, 4, 21, 9, 0, 0, 0, 0},
    /* fp8   */ {kByte, kAccF32, 4, 3, 32, 16, 11, 0, 8, 0, 0, 0},
    /* bf8   */ {kByte, kAccF32, 5, 2, 32, 16, 19, 0, 14, 0, 0, 0},
    /* i8    */ {kInt8, kAccI32, 0, 0, 32, 32, 0, 0, 0, 0, 0, 0},
    /* mxfp8 */ {kMx, kAccF32, 4, 3, 32, 64, 22, 0, 0, 55, 15, 1},
    /* mxbf8 */ {kMx, kAccF32, 5, 2, 32, 64, 36, 0, 0, 31, 11, 1},
    /* mxfp6 */ {kMx, kAccF32, 2, 3, 32, 64, 10, 0, 0, 31, 31, 1},
    /* mxbf6 */ {kMx, kAccF32, 3, 2, 32, 64, 12, 0, 0, 31, 11, 1},
    /* mxfp4 */ {kMx, kAccF32, 2, 1, 32, 64, 6, 0, 0, 7, 7, 0},
};

constexpr int kScaleLo = 125, kScaleSpan = 5;  // E8M0 codes 125..129: 2^-2 .. 2^2
// The scale byte sits in a different byte of the scale register for A than
// for B; the other bytes hold decoys (kDecoy + byte index: 2^-7 .. 2^-4), so a
// wrong byte select or an A/B swap changes the result.
constexpr int kOpselA = 2, kOpselB = 1, kDecoy = 120;

constexpr int kBlock = 256;          // 4 waves: one per SIMD
constexpr size_t kLdsUsed = 64 * 4;  // the four waves combine through 16 words each
constexpr int kBoundBroken = -1001;  // a generator left its stated bound (a bug in this file)

struct MatrixRecord {
  uint32_t xcd, cu, simd_mask, fail;
  uint32_t digest[kNumFmt];
  uint32_t reserved;
};
static_assert(sizeof(MatrixRecord) == 64, "one 64-byte record per workgroup");

struct Expect {
  uint32_t wave[kNumFmt];  // digest of one healthy wave
};

// ---------------------------------------------------------------- generators
XS_HD uint32_t mix(uint32_t x, uint32_t y, uint32_t salt) {
  uint32_t v = (x + 1u) * 0x9e3779b1u ^ (y + 1u) * 0x85ebca6bu ^ (salt + 1u) * 0xc2b2ae35u;
  v ^= v >> 15;
  v *= 0x2c1b3c6du;
  v ^= v >> 13;
  return v;
}
// Bits 8..23 of a hash mapped onto [0, n).
XS_HD uint32_t pick(uint32_t v, uint32_t n) { return (((v >> 8) & 0xffffu) * n) >> 16; }

// A magnitude code (the encoding without its sign bit) as an integer count of
// the format's subnormal unit 2^(1 - bias - M): monotone in the code.
XS_HD uint32_t mag_n(uint32_t c, int M) {
  const uint32_t E = c >> M, m = c & ((1u << M) - 1u);
  return E ? ((1u << M) + m) << (E - 1u) : m;
}
// The largest magnitude code whose mag_n is <= N.
XS_HD uint32_t cap_code(uint32_t N, int M) {
  if (N < (2u << M)) return N;
  int top = 0;
  while (N >> (top + 1)) ++top;
  const uint32_t E = static_cast<uint32_t>(top - M + 1);
  return (E << M) | ((N >> (E - 1u)) & ((1u << M) - 1u));
}

// E8M0 scale codes of the MX rows: A per (row, 32-element k-block), B per
// (k-block, column). Hashed, so they differ between rows, columns and blocks
// and take every value of 2^-2 .. 2^2.
template <int F>
XS_HD uint32_t a_scale(int i, int kb) {
  return kScaleLo + pick(mix(i, kb, 4 * F + 2), kScaleSpan);
}
template <int F>
XS_HD uint32_t b_scale(int kb, int j) {
  return kScaleLo + pick(mix(kb, j, 4 * F + 3), kScaleSpan);
}

// A[i][k] as an encoding. With u = the unit named per kind:
//  kPlain  sign | exponent field bias-1 .. bias+2 | top `mu` mantissa bits:
//          |A| = n * 2^(-1-mu), n < 2^(mu+4). With B (below) every product is
//          a multiple of 2^-(3+2mu) = 2^-frac and |sum| < 2K * 2^(2mu+8) units:
//          f16 2^19, f32 2^22 (< 2^24, exact in f32), f64 2^29 (< 2^31).
//  kByte   sign | magnitude code with exponent field 0..3 (subnormals
//          included): |A| = n * 2^(1-bias-M), n <= 60 (e4m3) or 28 (e5m2).
//          With B, |sum| <= 32 * 60 * 60 = 115200 units of 2^-frac.
//  kInt8   any byte; -128 and 127 occur. |sum| <= 64 * 2^14 = 2^20 in i32.
//  kMx     sign | magnitude code 0 .. cap, every code where amax is the
//          format's last (fp6, bf6, fp4). With `cap` the block's scale 2^s
//          limits the code to mag_n <= mag_n(amax) >> (s + 2), so that
//          |A * scale| <= mag_n(amax) units of u_a * 2^-2. B is not capped:
//          |B * scale| <= 16 mag_n(bmax) units of u_b * 2^-2. Every product
//          is a multiple of u_a u_b 2^-4 = 2^-frac and
//          |sum| <= 128 * mag_n(amax) * 16 mag_n(bmax) units:
//            mxfp8 128*480*240 = 14.7M   mxbf8 128*448*224 = 12.8M
//            mxfp6 128*60*960  =  7.4M   mxbf6 128*448*224 = 12.8M
//            mxfp4 (no cap) 128*192*192 = 4.7M          all < 2^24 = 16.8M.
template <int F>
XS_HD uint64_t a_code(int i, int k) {
  constexpr Desc d = kDesc[F];
  const uint32_t v = mix(i, k, 4 * F);
  const uint64_t sign = v & 1u;
  if constexpr (d.kind == kPlain) {
    const uint64_t E = (1u << (d.ebits - 1)) - 2u + ((v >> 1) & 3u);
    const uint64_t m = (v >> 3) & ((1u << d.mu) - 1u);
    return sign << (d.ebits + d.mbits) | E << d.mbits | m << (d.mbits - d.mu);
  } else if constexpr (d.kind == kByte) {
    return sign << 7 | pick(v, 4u << d.mbits);
  } else if constexpr (d.kind == kInt8) {
    return (v >> 8) & 0xffu;
  } else {
    uint32_t N = mag_n(d.amax, d.mbits);
    if (d.cap) N >>= a_scale<F>(i, k / 32) - kScaleLo;
    return sign << (d.ebits + d.mbits) | pick(v, cap_code(N, d.mbits) + 1u);
  }
}

// B[k][j] as an encoding; another hash than A's, and not symmetric in (k, j).
//  kPlain  exponent field bias-2 .. bias+1: |B| = n * 2^(-2-mu), n < 2^(mu+4).
//  kByte   exponent field eb0 .. eb0+3 (normals): |B| = n * 2^(eb0-bias-M),
//          n <= 60 (e4m3, values 2 .. 30) or 28 (e5m2, values 0.5 .. 7).
//  kInt8   any byte.
//  kMx     magnitude code 0 .. bmax whatever the scale (bound: see a_code).
template <int F>
XS_HD uint64_t b_code(int k, int j) {
  constexpr Desc d = kDesc[F];
  const uint32_t v = mix(k, j, 4 * F + 1);
  const uint64_t sign = v & 1u;
  if constexpr (d.kind == kPlain) {
    const uint64_t E = (1u << (d.ebits - 1)) - 3u + ((v >> 1) & 3u);
    const uint64_t m = (v >> 3) & ((1u << d.mu) - 1u);
    return sign << (d.ebits + d.mbits) | E << d.mbits | m << (d.mbits - d.mu);
  } else if constexpr (d.kind == kByte) {
    return sign << 7 | ((static_cast<uint32_t>(d.eb0) << d.mbits) + pick(v, 4u << d.mbits));
  } else if constexpr (d.kind == kInt8) {
    return (v >> 8) & 0xffu;
  } else {
    return sign << (d.ebits + d.mbits) | pick(v, d.bmax + 1u);
  }
}

// The scale register of a lane: the true code in byte `sel`, decoys elsewhere.
XS_HD uint32_t scale_reg(uint32_t code, int sel) {
  uint32_t r = 0;
  for (int p = 0; p < 4; ++p) r |= (p == sel ? code : static_cast<uint32_t>(kDecoy + p)) << (8 * p);
  return r;
}

// ------------------------------------------------------------------- device
template <int F>
struct Acc {
  using type = std::conditional_t<kDesc[F].acc == kAccF64, f64x4, std::conditional_t<kDesc[F].acc == kAccI32, i32x16, f32x16>>;
  static constexpr int regs = kDesc[F].acc == kAccF64 ? 4 : 16;
};

// Element j (w bits) of a dense little-endian register stream.
template <int W>
__device__ __forceinline__ void put(uint32_t (&r)[8], int j, uint32_t code) {
  const int bit = j * W;
  r[bit >> 5] |= code << (bit & 31);
  if ((bit & 31) + W > 32) r[(bit >> 5) + 1] |= code >> (32 - (bit & 31));
}

__device__ __forceinline__ i32x8 as_i32x8(const uint32_t (&r)[8]) {
  i32x8 v;
#pragma unroll
  for (int q = 0; q < 8; ++q) v[q] = static_cast<int>(r[q]);
  return v;
}

// One wave's product for format F: two K-steps into one accumulator.
template <int F>
__device__ __forceinline__ typename Acc<F>::type mfma_tile(int lane) {
  constexpr Desc d = kDesc[F];
  typename Acc<F>::type acc = {};
  const int r = lane & 31, h = lane >> 5;
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const int k0 = s * d.kstep;
    if constexpr (F == kF16) {
      u16x8 a, b;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        a[j] = static_cast<uint16_t>(a_code<F>(r, k0 + 8 * h + j));
        b[j] = static_cast<uint16_t>(b_code<F>(k0 + 8 * h + j, r));
      }
      acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), acc, 0,
                                                   0, 0);
    } else if constexpr (F == kF32) {
      const float a = __builtin_bit_cast(float, static_cast<uint32_t>(a_code<F>(r, k0 + h)));
      const float b = __builtin_bit_cast(float, static_cast<uint32_t>(b_code<F>(k0 + h, r)));
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
    } else if constexpr (F == kF64) {
      const int r16 = lane & 15, k = k0 + (lane >> 4);
      const double a = __builtin_bit_cast(double, a_code<F>(r16, k));
      const double b = __builtin_bit_cast(double, b_code<F>(k, r16));
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
    } else if constexpr (d.kind == kByte) {
      uint64_t a = 0, b = 0;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        a |= a_code<F>(r, k0 + 8 * h + j) << (8 * j);
        b |= b_code<F>(k0 + 8 * h + j, r) << (8 * j);
      }
      if constexpr (F == kFp8)
        acc = __builtin_amdgcn_mfma_f32_32x32x16_fp8_fp8(static_cast<long>(a), static_cast<long>(b), acc, 0, 0, 0);
      else
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf8_bf8(static_cast<long>(a), static_cast<long>(b), acc, 0, 0, 0);
    } else if constexpr (F == kI8) {
      uint32_t a[4] = {}, b[4] = {};
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        a[j >> 2] |= static_cast<uint32_t>(a_code<F>(r, k0 + 16 * h + j)) << (8 * (j & 3));
        b[j >> 2] |= static_cast<uint32_t>(b_code<F>(k0 + 16 * h + j, r)) << (8 * (j & 3));
      }
      const i32x4 av = {static_cast<int>(a[0]), static_cast<int>(a[1]), static_cast<int>(a[2]), static_cast<int>(a[3])};
      const i32x4 bv = {static_cast<int>(b[0]), static_cast<int>(b[1]), static_cast<int>(b[2]), static_cast<int>(b[3])};
      acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(av, bv, acc, 0, 0, 0);
    } else {
      constexpr int W = d.ebits + d.mbits + 1;
      constexpr int fmt = F - kMxFp8;  // cbsz = blgp: 0 fp8, 1 bf8, 2 fp6, 3 bf6, 4 fp4
      uint32_t a[8] = {}, b[8] = {};
#pragma unroll
      for (int j = 0; j < 32; ++j) {
        const int k = k0 + (W == 8 ? 16 * h + (j & 15) + 32 * (j >> 4) : 32 * h + j);
        put<W>(a, j, static_cast<uint32_t>(a_code<F>(r, k)));
        put<W>(b, j, static_cast<uint32_t>(b_code<F>(k, r)));
      }
      const int kb = k0 / 32 + h;
      const int sa = static_cast<int>(scale_reg(a_scale<F>(r, kb), kOpselA));
      const int sb = static_cast<int>(scale_reg(b_scale<F>(kb, r), kOpselB));
      acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(as_i32x8(a), as_i32x8(b), acc, fmt, fmt, kOpselA, sa,
                                                            kOpselB, sb);
    }
  }
  return acc;
}

// Where accumulator register q of `lane` sits in the result tile.
template <int F>
__device__ __forceinline__ int tile_pos(int lane, int q) {
  if constexpr (kDesc[F].acc == kAccF64)
    return ((lane >> 4) + 4 * q) * 16 + (lane & 15);
  else
    return ((q & 3) + 8 * (q >> 2) + 4 * (lane >> 5)) * 32 + (lane & 31);
}

// The accumulator in units of 2^-frac; `lossy` is set when it is no such integer.
template <int F, typename T>
__device__ __forceinline__ int32_t to_fixed(T x, uint32_t& lossy) {
  if constexpr (kDesc[F].acc == kAccI32) {
    return x;
  } else {
    const T s = x * static_cast<T>(1ull << kDesc[F].frac);
    const int32_t f = static_cast<int32_t>(s);
    lossy |= !(static_cast<T>(f) == s);
    return f;
  }
}

template <int F>
__device__ __forceinline__ void sweep_formats(uint32_t mask, uint32_t inj, int lane, const Expect& expect,
                                              uint32_t (&digest)[kNumFmt], uint32_t& fail) {
  if constexpr (F < kNumFmt) {
    digest[F] = 0;
    if ((mask >> F) & 1u) {
      const auto acc = mfma_tile<F>(lane);
      uint32_t part = 0, lossy = 0;
#pragma unroll
      for (int q = 0; q < Acc<F>::regs; ++q) {
        int32_t f = to_fixed<F>(acc[q], lossy);
        if (((inj >> F) & 1u) && lane == 0 && q == 0) f ^= 1;
        part += static_cast<uint32_t>(f) * (2u * static_cast<uint32_t>(tile_pos<F>(lane, q)) + 1u);
      }
      digest[F] = wave_sum(part);
      if (wave_or(lossy) || digest[F] != expect.wave[F]) fail |= 1u << F;
    }
    sweep_formats<F + 1>(mask, inj, lane, expect, digest, fail);
  }
}

__global__ __launch_bounds__(kBlock) void k_matrix_sweep(MatrixRecord* __restrict__ records, uint32_t format_mask,
                                                        int inject_xcd, int inject_cu, uint32_t inject_formats,
                                                        Expect expect) {
  extern __shared__ uint32_t matrix_lds[];
  const uint32_t t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const uint32_t xcd = xcc_id();
  const uint32_t hw = hw_id();
  const uint32_t cu = cu_key(hw);
  const uint32_t simd = simd_id(hw);
  const bool inject = inject_selected(inject_xcd, inject_cu, xcd, cu);
  const uint32_t inj = inject && wave == 0 ? inject_formats : 0u;

  uint32_t digest[kNumFmt];
  uint32_t fail = 0;
  sweep_formats<0>(format_mask, inj, static_cast<int>(lane), expect, digest, fail);

  // Combine the four waves through the first words of the allocation.
  if (lane == 0) {
    uint32_t* s = matrix_lds + wave * 16;
#pragma unroll
    for (int f = 0; f < kNumFmt; ++f) s[f] = digest[f];
    s[kNumFmt] = fail;
    s[kNumFmt + 1] = 1u << simd;
  }
  __syncthreads();
  if (t == 0) {
    uint32_t d[kNumFmt + 1] = {}, f = 0, simds = 0;
    for (int w = 0; w < kBlock / 64; ++w) {
      const uint32_t* s = matrix_lds + w * 16;
#pragma unroll
      for (int q = 0; q < kNumFmt; ++q) d[q] += s[q] << w;
      f |= s[kNumFmt];
      simds |= s[kNumFmt + 1];
    }
    u32x4* out = reinterpret_cast<u32x4*>(&records[blockIdx.x]);
    out[0] = u32x4{xcd, cu, simds, f};
    out[1] = u32x4{d[0], d[1], d[2], d[3]};
    out[2] = u32x4{d[4], d[5], d[6], d[7]};
    out[3] = u32x4{d[8], d[9], d[10], 0u};
  }
}

// One wave; out holds tile x tile accumulators (f32, f64 or i32), row-major.
template <int F>
__global__ __launch_bounds__(64) void k_matrix_tile(void* __restrict__ out) {
  const int lane = static_cast<int>(threadIdx.x);
  const auto acc = mfma_tile<F>(lane);
  using T = std::remove_cv_t<std::remove_reference_t<decltype(acc[0])>>;
#pragma unroll
  for (int q = 0; q < Acc<F>::regs; ++q) static_cast<T*>(out)[tile_pos<F>(lane, q)] = acc[q];
}

// --------------------------------------------------------------------- host
template <typename Fn>
bool with_format(int fmt, Fn&& fn) {
  switch (fmt) {
#define XS_CASE(n) \
  case n:          \
    fn(std::integral_constant<int, n>{}); \
    return true;
    XS_CASE(0) XS_CASE(1) XS_CASE(2) XS_CASE(3) XS_CASE(4) XS_CASE(5) XS_CASE(6) XS_CASE(7) XS_CASE(8) XS_CASE(9) XS_CASE(10)
#undef XS_CASE
    default:
      return false;
  }
}
static_assert(kNumFmt == 11, "with_format lists every format");

double decode(uint64_t bits, const Desc& d) {
  if (d.kind == kInt8) return static_cast<int8_t>(bits & 0xff);
  const int bias = (1 << (d.ebits - 1)) - 1;
  const uint64_t man = bits & ((1ull << d.mbits) - 1);
  const int E = static_cast<int>((bits >> d.mbits) & ((1ull << d.ebits) - 1));
  const double v = E ? std::ldexp(static_cast<double>((1ull << d.mbits) + man), E - bias - d.mbits)
                     : std::ldexp(static_cast<double>(man), 1 - bias - d.mbits);
  return (bits >> (d.ebits + d.mbits)) & 1 ? -v : v;
}

template <int F>
void inputs(uint64_t* a, uint64_t* b, uint8_t* sa, uint8_t* sb) {
  constexpr Desc d = kDesc[F];
  constexpr int K = 2 * d.kstep, nb = d.kind == kMx ? K / 32 : 0;
  for (int i = 0; i < d.tile; ++i)
    for (int k = 0; k < K; ++k) {
      if (a) a[i * K + k] = a_code<F>(i, k);
      if (b) b[k * d.tile + i] = b_code<F>(k, i);
    }
  if constexpr (d.kind == kMx)
    for (int i = 0; i < d.tile; ++i)
      for (int kb = 0; kb < nb; ++kb) {
        if (sa) sa[i * nb + kb] = static_cast<uint8_t>(a_scale<F>(i, kb));
        if (sb) sb[kb * d.tile + i] = static_cast<uint8_t>(b_scale<F>(kb, i));
      }
}

// The exact result in units of 2^-frac from the decoded encodings; false when
// a sum leaves the bound the generators state.
template <int F>
bool expected_tile(std::vector<int64_t>& fix) {
  constexpr Desc d = kDesc[F];
  constexpr int K = 2 * d.kstep, T = d.tile;
  const double limit = d.acc == kAccF32 ? 16777216.0 : 2147483648.0;
  fix.assign(T * T, 0);
  for (int i = 0; i < T; ++i)
    for (int j = 0; j < T; ++j) {
      double sum = 0, mag = 0;
      for (int k = 0; k < K; ++k) {
        double p = decode(a_code<F>(i, k), d) * decode(b_code<F>(k, j), d);
        if constexpr (d.kind == kMx)
          p = std::ldexp(p, static_cast<int>(a_scale<F>(i, k / 32)) + static_cast<int>(b_scale<F>(k / 32, j)) - 254);
        p = std::ldexp(p, d.frac);
        if (p != std::nearbyint(p)) return false;
        sum += p;
        mag += std::fabs(p);
      }
      if (mag >= limit) return false;
      fix[i * T + j] = static_cast<int64_t>(sum);
    }
  return true;
}

template <int F>
bool expected_wave_digest(uint32_t* out) {
  std::vector<int64_t> fix;
  if (!expected_tile<F>(fix)) return false;
  uint32_t dsum = 0;
  for (size_t p = 0; p < fix.size(); ++p)
    dsum += static_cast<uint32_t>(static_cast<int32_t>(fix[p])) * (2u * static_cast<uint32_t>(p) + 1u);
  *out = dsum;
  return true;
}

// The inputs are fixed, so the host reference runs once per process (the node
// agent sweeps every GPU again and again).
struct Reference {
  Expect e{};
  uint32_t broken = 0;  // formats whose inputs leave their exactness bound
  Reference() {
    for (int f = 0; f < kNumFmt; ++f) {
      bool ok = false;
      with_format(f, [&](auto F) { ok = expected_wave_digest<decltype(F)::value>(&e.wave[f]); });
      if (!ok) broken |= 1u << f;
    }
  }
};

int expected(uint32_t format_mask, Expect* e) {
  static const Reference ref;
  if (ref.broken & format_mask) {
    std::snprintf(g_matrix_err, sizeof g_matrix_err, "formats %#x: inputs leave their exactness bound",
                  ref.broken & format_mask);
    return kBoundBroken;
  }
  for (int f = 0; f < kNumFmt; ++f) e->wave[f] = (format_mask >> f) & 1u ? ref.e.wave[f] : 0u;
  return 0;
}

}  // namespace

extern "C" {

const char* xs_matrix_sweep_last_error() { return g_matrix_err; }

// Format names, comma-separated, in bit order.
const char* xs_matrix_formats() { return kFmtNames; }

// out5 = {tile, K (both steps), scale blocks along K (0: not block-scaled),
// accumulator (0 f32, 1 f64, 2 i32), frac}.
int xs_matrix_shape(int fmt, int* out5) {
  if (fmt < 0 || fmt >= kNumFmt || !out5) return kBadArgs;
  const Desc& d = kDesc[fmt];
  out5[0] = d.tile;
  out5[1] = 2 * d.kstep;
  out5[2] = d.kind == kMx ? 2 * d.kstep / 32 : 0;
  out5[3] = d.acc;
  out5[4] = d.frac;
  return 0;
}

// Host only. The encodings the generators produce, row-major: a_codes
// [tile][K], b_codes [K][tile] (64-bit slots), and for the block-scaled
// formats a_scales [tile][K/32], b_scales [K/32][tile] (bytes). Null pointers
// are skipped.
int xs_matrix_inputs(int fmt, uint64_t* a_codes, uint64_t* b_codes, uint8_t* a_scales, uint8_t* b_scales) {
  const bool ok = with_format(fmt, [&](auto F) { inputs<decltype(F)::value>(a_codes, b_codes, a_scales, b_scales); });
  return ok ? 0 : kBadArgs;
}

// One wave computes the product of format `fmt`; out receives tile x tile
// doubles (every accumulator type converts exactly), row-major.
int xs_matrix_tile(int dev, int fmt, double* out) {
  if (fmt < 0 || fmt >= kNumFmt || !out) return kBadArgs;
  const Desc& d = kDesc[fmt];
  const size_t n = static_cast<size_t>(d.tile) * d.tile;
  XS_CHECK(hipSetDevice(dev));
  DevMem buf;
  XS_CHECK(hipMalloc(&buf.p, n * 8));
  XS_CHECK(hipMemset(buf.p, 0xff, n * 8));
  with_format(fmt, [&](auto F) { hipLaunchKernelGGL(k_matrix_tile<decltype(F)::value>, dim3(1), dim3(64), 0, 0, buf.p); });
  XS_CHECK(hipGetLastError());
  XS_CHECK(hipDeviceSynchronize());
  std::vector<uint64_t> raw(n);
  XS_CHECK(hipMemcpy(raw.data(), buf.p, n * 8, hipMemcpyDeviceToHost));
  for (size_t p = 0; p < n; ++p) {
    if (d.acc == kAccF64)
      out[p] = reinterpret_cast<const double*>(raw.data())[p];
    else if (d.acc == kAccI32)
      out[p] = reinterpret_cast<const int32_t*>(raw.data())[p];
    else
      out[p] = reinterpret_cast<const float*>(raw.data())[p];
  }
  return 0;
}

// Host only. out[f] = the workgroup digest a healthy CU leaves for format f,
// 0 for a format outside format_mask (out holds one word per format).
int xs_matrix_sweep_expected(uint32_t format_mask, uint32_t* out) {
  if (bad_part_mask(format_mask, kAllFormats) || !out) return kBadArgs;
  Expect e;
  if (int rc = expected(format_mask, &e)) return rc;
  for (int f = 0; f < kNumFmt; ++f) {
    out[f] = 0;
    for (int w = 0; w < kBlock / 64; ++w) out[f] += e.wave[f] << w;
  }
  return 0;
}

// One sweep launch of `blocks` workgroups; 0 is refused, not taken as "4 per
// CU". Writes `blocks` 64-byte records to records_out. Returns 0, -1000 for
// bad arguments (nothing is launched), or a negative HIP error.
int xs_matrix_sweep(int dev, int blocks, uint32_t format_mask, int inject_xcd, int inject_cu, uint32_t inject_formats,
                    void* records_out, int* n_records, double* ms) {
  if (bad_part_mask(format_mask, kAllFormats) || (inject_formats & ~kAllFormats) || blocks == 0) return kBadArgs;
  Expect e;
  if (int rc = expected(format_mask, &e)) return rc;
  return launch_sweep(g_matrix_err, {dev, blocks, inject_xcd, inject_cu, records_out, n_records, ms},
                      reinterpret_cast<const void*>(k_matrix_sweep), kBlock, kLdsUsed, sizeof(MatrixRecord),
                      [&](dim3 grid, dim3 block, size_t smem, void* rec) {
                        hipLaunchKernelGGL(k_matrix_sweep, grid, block, smem, 0, static_cast<MatrixRecord*>(rec),
                                           format_mask, inject_xcd, inject_cu, inject_formats, e);
                      });
}

}  // extern "C"
