// Consensus sweep for gfx950 (MI355X): instructions whose bits no document at
// hand fixes, judged by a vote across CUs.
//
// The other per-CU sweeps compare every result with a value the host computed
// independently, which keeps out whatever has no such value: the raw
// transcendentals off their exact arguments, the division helpers, the
// stochastic roundings, NaN payloads and saturation, the 8-, 6- and 4-bit
// transposed LDS reads, the float LDS atomics, and most MFMA and all SMFMAC
// forms. k_consensus_sweep is the same kind of launch (256-thread workgroups,
// one wave per SIMD, each asking for more than half of a CU's LDS so that no
// two share a CU, 4 x CUs of them, every workgroup self-contained: no wave
// waits on another workgroup) and runs those instructions, each under its own
// mnemonic, on hashed operands that do not depend on where the workgroup
// runs. The device does not judge: a workgroup leaves one digest per part and
// fail = 0. All CUs of a GPU must leave the same digests; the host's vote
// (vote_consensus in ops/hip_probe.py) names the CU that does not.
//
// Parts (bit, name). A part is a list of steps; a step is one instruction (or
// one sequence that is about one: the full division) with 1..16 result words
// per lane. CONSENSUS_STEPS below is the one table: it names each step, gives
// the kind and the word count of its up to four operands and the device code
// that issues it. operand_word() serves the kernel and xs_consensus_operands.
//   0 trans   1 div   2 sr   3 edge   4 ldsx   5 mfma   6 smfmac
//
// Operands. fmix32 is the murmur3 finaliser (part_sweep.h):
//   h(o)    = fmix32(seed ^ (part << 28 | step << 20 | round << 12 | o << 8 | t))
//   h(o, w) = h(o) for w = 0, else fmix32(h(o) + 0x9e3779b9 w)
// step = index within the part, t = thread in the workgroup (64 x wave +
// lane), o = operand 0..3, w = word of the operand (or element, for packed
// 16-bit sources). The key holds neither the workgroup, the CU nor the SIMD.
// x = h(o, w) is shaped by the operand's kind:
//   U32     x                         BIT     x & 1
//   F32N    sign x[31], significand x[22:0], exponent field 1 + x[30:23] % 254 (every finite normal)
//   F32NP   F32N, sign cleared        F32X    F32N on even t, exponent 100 + x[30:23] % 34 on odd t
//   F32REV  exponent 97 + x[30:23] % 38 (|x| < 256 revolutions)
//   F32B    exponent 96 + x[30:23] % 63 (the VALU sweep's band)
//   F64N / F64NP / F64B  high word from h(o, 0): sign, x[19:0], exponent field 1 + x[30:20] % 2046
//           (F64B: 992 + .. % 63); low word h(o, 1)
//   F16N / F16NP  low half: sign x[15], x[9:0], exponent field 1 + x[14:10] % 30; high half 0
//   PKF16   two halves: sign, 10 bits, exponent 8 + e % 15     PKBF16  sign, 7 bits, exponent 120 + e % 15
//   FP8W / BF8W  four bytes, the NaN (and Inf) encodings of OCP e4m3fn / e5m2 taken out
//   SCALE   2^(x % 5 - 2) as f32      SCALE8  four E8M0 bytes 125 + byte % 5
//   EXPI    x % 61 - 30 (an ldexp exponent)
//   E32 / E16PK / EBFPK  class (x >> 24) & 7 (halves: (y >> 10) & 7, (y >> 7) & 7): quiet NaN with payload,
//           signalling NaN, infinity, subnormal, zero, huge, tiny, middle; sign hashed
//   EW32    class (x >> 24) & 7: quiet NaN, infinity, subnormal, zero, else exponent 96 + x[22:0] % 64
//   F32U8   (x % 1216 - 64) / 4 (v_cvt_pk_u8_f32: ties, off-grid values, both saturations)
//   F32NORM exponent 110 + x[30:23] % 19
//   E64     the classes of E32 in double: high word from h(o, 0) (20 hashed bits, middle exponents 1016..1031),
//           low word h(o, 1), 0 for an infinity or a zero
//   SR(target, source, scaled)  an in-range normal of the target times the step's scale (operand 2, SCALE;
//           1 when not scaled): element el of the operand has target exponent e = lo + x[30:23] % n
//           (fp8 -6..7, bf8 -12..12, fp4 0..1, fp6 0..1, bf6 -2..3, f16 -14..14, bf16 -20..20: never the
//           top binade, so rounding up stays finite), the target's mt significand bits x[8 + mt - 1:8] on top
//           and below them L = ms - mt bits that are the fraction of the gap: 0 where (t + round + el) % 8
//           == 0 (representable), else 2^(L-2) + (x >> 3) % (2^(L-1) + 1), which lies in [1/4, 3/4].
//           224 of a round's 256 threads are in that band, so two rounds give every form more than 256.
// `rounds` (1..64) is the number of operand sets per step.
//
// Float mode: the default kernel descriptor (round to nearest even, denormals
// preserved, IEEE mode). The kernel never writes MODE. Every asm statement
// that changes VCC names it as clobbered; none changes EXEC or M0.
//
// ldsx. A wave owns 2 KiB of LDS behind the reduction's words. The transposed
// reads run over 8 hashed words per lane (word j of lane l at 4 (64 j + l)),
// lane l reading at (l & 15) x stride + (l >> 4) x 8 (b96: x 16), strides 64
// and 80 (b96: 96) bytes: every address is aligned to 8 (16) bytes and ends
// below 1,504. The atomics run each lane on the 8 bytes at 8 l: no result
// depends on arrival order. A step returns the value the atomic returned and
// the value then read back.
//
// smfmac. The index operand is hashed per lane. abid is an immediate, so it
// cannot be hashed: every step runs two encodings of its instruction (cbsz:1
// abid:0 and 1 for 8-bit sources, 1 and 3 for 16-bit) on the same operands,
// and its result is the two tiles in turn. On the MI355X the two tiles came
// back equal for all fourteen forms: abid selects nothing at these shapes.
//
// Digest. D_p += got x (2 idx + 1), idx = (round x rows_p + row) x 256 + t
// (part_sweep.h's take_word); the workgroup's digest is the sum over its
// threads, reduced through plain LDS words and a barrier. The sum is
// commutative: it does not depend on which SIMD a wave ran on.
//
// Record (128 bytes per workgroup): {xcd, cu key, simd mask, fail = 0, 7
// digests (0 for a part not selected), 0 x 21}. A digest per wave and part
// would take 28 words more than the 11 used and does not fit, so the host
// names the CU, not the SIMD.
//
// Injection: a workgroup on inject_xcd whose CU key is inject_cu (any with
// -1; -1 for inject_xcd means none; values below -1 are refused) flips bit 0
// of word 0 of each part in the inject mask before the digest. Registers only.
//
// k_consensus_probe is one workgroup of the same device code with a dump
// pointer: it stores every result of one part as [round][row][256].
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <type_traits>

#include "hip/part_sweep.h"

#define XS_ERR_BUF g_consensus_err
#define XS_HD __host__ __device__ __forceinline__
#define XS_D __device__ __forceinline__

namespace {

xsprobe::ErrBuf g_consensus_err;

using namespace xsprobe;

constexpr int kNumParts = 7;
const char kPartNames[] = "trans,div,sr,edge,ldsx,mfma,smfmac";
constexpr uint32_t kAllParts = (1u << kNumParts) - 1;
constexpr int kBlock = kPartBlock;
constexpr int kMaxRounds = 64;
constexpr int kLdsx = 4;

// The reduction's words, then one tile per wave.
constexpr uint32_t kReduceWords = (kNumParts + 1) * kBlock;
constexpr uint32_t kTileOff = kReduceWords * 4, kTileBytes = 2048;
constexpr uint32_t kLdsUsed = kTileOff + 4 * kTileBytes;

// SR kinds carry their parameters: 64 + target x 8 + source x 2 + scaled.
enum SrTarget : int { T_FP8, T_BF8, T_FP4, T_FP6, T_BF6, T_F16, T_BF16 };
enum SrSource : int { S_F32, S_F16, S_BF16 };
constexpr int SR(int target, int source, int scaled) { return 64 + target * 8 + source * 2 + scaled; }

enum Kind : int {
  NONE, U32, BIT, F32N, F32NP, F32X, F32REV, F32B, F64N, F64NP, F64B, F16N, F16NP, PKF16, PKBF16, FP8W, BF8W, SCALE,
  SCALE8, EXPI, E32, E16PK, EBFPK, EW32, F32U8, F32NORM, E64
};

// ------------------------------------------------------------------ operands
XS_HD uint32_t hashv(uint32_t seed, uint32_t p, uint32_t s, uint32_t r, uint32_t o, uint32_t t) {
  return fmix32(seed ^ (p << 28 | s << 20 | r << 12 | o << 8 | t));
}
XS_HD uint32_t hashw(uint32_t h, uint32_t w) { return w ? fmix32(h + 0x9e3779b9u * w) : h; }

XS_HD uint32_t f32_band(uint32_t x, uint32_t lo, uint32_t n, bool sign) {
  return (sign ? x & 0x80000000u : 0u) | (lo + ((x >> 23) & 0xffu) % n) << 23 | (x & 0x7fffffu);
}
XS_HD uint32_t f64_hi(uint32_t x, uint32_t lo, uint32_t n, bool sign) {
  return (sign ? x & 0x80000000u : 0u) | (lo + ((x >> 20) & 0x7ffu) % n) << 20 | (x & 0xfffffu);
}
XS_HD uint32_t f16_band(uint32_t y, uint32_t lo, uint32_t n, bool sign) {
  return (sign ? y & 0x8000u : 0u) | (lo + ((y >> 10) & 31u) % n) << 10 | (y & 0x3ffu);
}
XS_HD uint32_t bf16_band(uint32_t y, uint32_t lo, uint32_t n, bool sign) {
  return (sign ? y & 0x8000u : 0u) | (lo + ((y >> 7) & 0xffu) % n) << 7 | (y & 0x7fu);
}
XS_HD uint32_t fp8_byte(uint32_t b) { return (b & 0x7fu) == 0x7fu ? b & 0xf7u : b; }  // e4m3fn: no NaN
XS_HD uint32_t bf8_byte(uint32_t b) { return (b & 0x7cu) == 0x7cu ? b & 0xbfu : b; }  // e5m2: no Inf / NaN
XS_HD uint32_t bytes4(uint32_t x, bool fp8) {
  uint32_t r = 0;
  for (int i = 0; i < 4; ++i) {
    const uint32_t b = (x >> (8 * i)) & 0xffu;
    r |= (fp8 ? fp8_byte(b) : bf8_byte(b)) << (8 * i);
  }
  return r;
}
// An edge value of a float format with `mbits` significand bits and exponent
// field maximum `emax`, from class c, sign bit s (in place) and hashed bits m.
XS_HD uint32_t edge_float(uint32_t c, uint32_t s, uint32_t m, uint32_t mbits, uint32_t emax, uint32_t mid, uint32_t midn) {
  const uint32_t quiet = 1u << (mbits - 1), inf = emax << mbits;
  switch (c) {
    case 0: return s | inf | quiet | m;
    case 1: return s | inf | (m & (quiet - 1)) | 1u;
    case 2: return s | inf;
    case 3: return s | m | 1u;
    case 4: return s;
    case 5: return s | (emax - 4 + m % 4u) << mbits | m;
    case 6: return s | (1 + m % 4u) << mbits | m;
    default: return s | (mid + m % midn) << mbits | m;
  }
}
XS_HD uint32_t edge_f16(uint32_t y) { return edge_float((y >> 10) & 7u, y & 0x8000u, y & 0x3ffu, 10, 31, 12, 8); }
XS_HD uint32_t edge_bf16(uint32_t y) { return edge_float((y >> 7) & 7u, y & 0x8000u, y & 0x7fu, 7, 255, 120, 16); }
XS_HD uint32_t f32_of_int(int32_t v) {  // |v| < 2^24: exact
  if (v == 0) return 0;
  const uint32_t s = v < 0 ? 0x80000000u : 0u, a = static_cast<uint32_t>(v < 0 ? -v : v);
  const int e = 31 - __builtin_clz(a);
  return s | static_cast<uint32_t>(127 + e) << 23 | ((a << (23 - e)) & 0x7fffffu);
}

struct SrParams {
  int mt, lo, n;  // the target's significand bits, its lowest exponent used and how many
};
XS_HD constexpr SrParams sr_target(int target) {
  switch (target) {
    case T_FP8: return {3, -6, 14};
    case T_BF8: return {2, -12, 25};
    case T_FP4: return {1, 0, 2};
    case T_FP6: return {3, 0, 2};
    case T_BF6: return {2, -2, 6};
    case T_F16: return {10, -14, 29};
    default: return {7, -20, 41};
  }
}
// Element `el` of an SR operand: x its hash, hs the hash of the step's scale.
XS_HD uint32_t sr_element(int kind, uint32_t x, uint32_t hs, uint32_t t, uint32_t r, uint32_t el) {
  const int k = kind - 64, source = (k >> 1) & 3, scaled = k & 1;
  const SrParams p = sr_target(k >> 3);
  const int ms = source == S_F32 ? 23 : source == S_F16 ? 10 : 7, bias = source == S_F16 ? 15 : 127;
  const int L = ms - p.mt;
  const int s = scaled ? static_cast<int>(hs % 5u) - 2 : 0;
  const uint32_t e = static_cast<uint32_t>(p.lo + static_cast<int>(((x >> 23) & 0xffu) % static_cast<uint32_t>(p.n)) + s + bias);
  const uint32_t top = (x >> 8) & ((1u << p.mt) - 1);
  const bool rep = ((t + r + el) & 7u) == 0;
  const uint32_t low = rep ? 0u : (1u << (L - 2)) + (x >> 3) % ((1u << (L - 1)) + 1u);
  const uint32_t mant = top << L | low;
  if (source == S_F32) return (x & 0x80000000u) | e << 23 | mant;
  return ((x >> 16) & 0x8000u) | e << ms | mant;
}

// Word w of operand o of (part p, step s, round r, thread t).
XS_HD uint32_t operand_word(int kind, uint32_t seed, uint32_t p, uint32_t s, uint32_t r, uint32_t o, uint32_t t,
                            uint32_t w) {
  const uint32_t h = hashv(seed, p, s, r, o, t);
  if (kind >= 64) {
    const uint32_t hs = hashv(seed, p, s, r, 2, t);
    if (((kind - 64) >> 1 & 3) == S_F32) return sr_element(kind, hashw(h, w), hs, t, r, w);
    return sr_element(kind, hashw(h, 2 * w), hs, t, r, 2 * w) |
           sr_element(kind, hashw(h, 2 * w + 1), hs, t, r, 2 * w + 1) << 16;
  }
  const uint32_t x = hashw(h, w);
  switch (kind) {
    case U32: return x;
    case BIT: return x & 1u;
    case F32N: return f32_band(x, 1, 254, true);
    case F32NP: return f32_band(x, 1, 254, false);
    case F32X: return (t & 1u) ? f32_band(x, 100, 34, true) : f32_band(x, 1, 254, true);
    case F32REV: return f32_band(x, 97, 38, true);
    case F32B: return f32_band(x, 96, 63, true);
    case F64N: return w ? f64_hi(h, 1, 2046, true) : hashw(h, 1);
    case F64NP: return w ? f64_hi(h, 1, 2046, false) : hashw(h, 1);
    case F64B: return w ? f64_hi(h, 992, 63, true) : hashw(h, 1);
    case F16N: return f16_band(x & 0xffffu, 1, 30, true);
    case F16NP: return f16_band(x & 0xffffu, 1, 30, false);
    case PKF16: return f16_band(x & 0xffffu, 8, 15, true) | f16_band(x >> 16, 8, 15, true) << 16;
    case PKBF16: return bf16_band(x & 0xffffu, 120, 15, true) | bf16_band(x >> 16, 120, 15, true) << 16;
    case FP8W: return bytes4(x, true);
    case BF8W: return bytes4(x, false);
    case SCALE: return (125u + x % 5u) << 23;
    case SCALE8: {
      uint32_t v = 0;
      for (int i = 0; i < 4; ++i) v |= (125u + ((x >> (8 * i)) & 0xffu) % 5u) << (8 * i);
      return v;
    }
    case EXPI: return static_cast<uint32_t>(static_cast<int32_t>(x % 61u) - 30);
    case E32: return edge_float((x >> 24) & 7u, x & 0x80000000u, x & 0x7fffffu, 23, 255, 120, 16);
    case E16PK: return edge_f16(x & 0xffffu) | edge_f16(x >> 16) << 16;
    case EBFPK: return edge_bf16(x & 0xffffu) | edge_bf16(x >> 16) << 16;
    case EW32: {
      const uint32_t sg = x & 0x80000000u, m = x & 0x7fffffu;
      switch ((x >> 24) & 7u) {
        case 0: return sg | 0x7fc00000u | m;
        case 1: return sg | 0x7f800000u;
        case 2: return sg | m | 1u;
        case 3: return sg;
        default: return sg | (96u + m % 64u) << 23 | m;
      }
    }
    case F32U8: {
      const int32_t k = static_cast<int32_t>(x % 1216u) - 64;
      return k ? f32_of_int(k) - (2u << 23) : 0u;
    }
    case F32NORM: return f32_band(x, 110, 19, true);
    case E64: {
      const uint32_t cls = (h >> 24) & 7u;
      if (w) return edge_float(cls, h & 0x80000000u, h & 0xfffffu, 20, 2047, 1016, 16);
      return cls == 2 || cls == 4 ? 0u : hashw(h, 1);
    }
    default: return 0;
  }
}

// ------------------------------------------------------------- device values
template <int N>
struct Words {
  uint32_t w[N ? N : 1];
};
template <int N>
struct Reg {
  typedef uint32_t type __attribute__((ext_vector_type(N)));
};
template <>
struct Reg<0> {
  typedef uint32_t type;
};
template <>
struct Reg<1> {
  typedef uint32_t type;
};
template <int N>
XS_D typename Reg<N>::type reg(const Words<N>& x) {
  if constexpr (N == 0) {
    return 0u;
  } else if constexpr (N == 1) {
    return x.w[0];
  } else {
    typename Reg<N>::type r;
#pragma unroll
    for (int i = 0; i < N; ++i) r[i] = x.w[i];
    return r;
  }
}
template <int N>
XS_D Words<N> words(typename Reg<N>::type r) {
  Words<N> x;
  if constexpr (N == 1) {
    x.w[0] = r;
  } else {
#pragma unroll
    for (int i = 0; i < N; ++i) x.w[i] = r[i];
  }
  return x;
}
XS_D uint64_t u64(const Words<2>& x) { return static_cast<uint64_t>(x.w[1]) << 32 | x.w[0]; }

struct Ctx {
  uint32_t seed, t, rounds, inj;
  uint32_t* dump;  // k_consensus_probe only
  uint32_t tile;   // byte address of the wave's LDS tile
  uint32_t lane;
};

// --------------------------------------------------------------- device code
// The s_nop covers what the assembler does not see inside inline asm (a
// transcendental's result read next). NR is the step's result words.
#define OUT typename Reg<NR>::type o_
#define DONE v = words<NR>(o_)
#define IN4 "v"(reg(a)), "v"(reg(b)), "v"(reg(cc)), "v"(reg(d))
// %0 result, %1..%4 the operands.
#define A(text)                                                  \
  {                                                              \
    OUT;                                                         \
    asm volatile(text "\n\ts_nop 1" : "=&v"(o_) : IN4 : "vcc"); \
    DONE;                                                        \
  }
#define LOW16(text) A(text "\n\ts_nop 1\n\tv_and_b32_e32 %0, 0xffff, %0")
#define LOW8(text) A(text "\n\ts_nop 1\n\tv_and_b32_e32 %0, 0xff, %0")
// A conversion that writes part of its destination: the rest is 0.
#define PART16(text) LOW16("v_mov_b32_e32 %0, 0\n\t" text)
#define PART8(text) LOW8("v_mov_b32_e32 %0, 0\n\t" text)
#define ZEROED(text) A("v_mov_b32_e32 %0, 0\n\t" text)
// v_div_fmas reads VCC, written from operand 3 (BIT) four wait states earlier.
// A compare: the VCC bit it leaves.
#define CMP(text) A(text "\n\tv_cndmask_b32_e64 %0, 0, 1, vcc")
#define FMAS(text) A("v_cmp_ne_u32_e32 vcc, 0, %4\n\ts_nop 3\n\t" text)
// v_div_scale: the scaled value, then the VCC bit it leaves.
#define DIV_SCALE(text, TYPE, NW)                                                                     \
  {                                                                                                   \
    TYPE q_;                                                                                          \
    uint32_t c_;                                                                                      \
    asm volatile(text " %0, vcc, %2, %3, %4\n\tv_cndmask_b32_e64 %1, 0, 1, vcc"                        \
                 : "=&v"(q_), "=&v"(c_)                                                               \
                 : "v"(reg(a)), "v"(reg(b)), "v"(reg(cc))                                             \
                 : "vcc");                                                                            \
    v.w[0] = static_cast<uint32_t>(q_);                                                               \
    if constexpr (NW == 2) v.w[1] = static_cast<uint32_t>(static_cast<uint64_t>(q_) >> 32);           \
    v.w[NW] = c_;                                                                                     \
  }
// a / b: scale both, refine the reciprocal, v_div_fmas, v_div_fixup.
#define DIV_F32                                                                                                  \
  {                                                                                                              \
    uint32_t q_, d_, n_, r_, e_;                                                                                 \
    asm volatile(                                                                                                \
        "v_div_scale_f32 %1, vcc, %6, %6, %5\n\tv_div_scale_f32 %2, vcc, %5, %6, %5\n\tv_rcp_f32_e32 %3, %1\n\t" \
        "s_nop 1\n\tv_fma_f32 %4, -%1, %3, 1.0\n\tv_fma_f32 %3, %4, %3, %3\n\tv_mul_f32_e32 %0, %2, %3\n\t"      \
        "v_fma_f32 %4, -%1, %0, %2\n\tv_fma_f32 %0, %4, %3, %0\n\tv_fma_f32 %4, -%1, %0, %2\n\t"                \
        "v_div_fmas_f32 %0, %4, %3, %0\n\tv_div_fixup_f32 %0, %0, %6, %5\n\ts_nop 1"                            \
        : "=&v"(q_), "=&v"(d_), "=&v"(n_), "=&v"(r_), "=&v"(e_)                                                  \
        : "v"(reg(a)), "v"(reg(b))                                                                               \
        : "vcc");                                                                                                \
    v.w[0] = q_;                                                                                                 \
  }
#define DIV_F64                                                                                                  \
  {                                                                                                              \
    uint64_t q_, d_, n_, r_, e_;                                                                                 \
    asm volatile(                                                                                                \
        "v_div_scale_f64 %1, vcc, %6, %6, %5\n\tv_div_scale_f64 %2, vcc, %5, %6, %5\n\tv_rcp_f64_e32 %3, %1\n\t" \
        "s_nop 1\n\tv_fma_f64 %4, -%1, %3, 1.0\n\tv_fma_f64 %3, %3, %4, %3\n\tv_fma_f64 %4, -%1, %3, 1.0\n\t"    \
        "v_fma_f64 %3, %3, %4, %3\n\tv_mul_f64 %0, %2, %3\n\tv_fma_f64 %4, -%1, %0, %2\n\t"                     \
        "v_div_fmas_f64 %0, %4, %3, %0\n\tv_div_fixup_f64 %0, %0, %6, %5\n\ts_nop 1"                            \
        : "=&v"(q_), "=&v"(d_), "=&v"(n_), "=&v"(r_), "=&v"(e_)                                                  \
        : "v"(u64(a)), "v"(u64(b))                                                                               \
        : "vcc");                                                                                                \
    v.w[0] = static_cast<uint32_t>(q_);                                                                          \
    v.w[1] = static_cast<uint32_t>(q_ >> 32);                                                                    \
  }
// A matrix instruction: its operands were just written by the VALU, and its
// result is read by the VALU next. 24 wait states cover a 16-pass instruction.
#define MFMA_PAD "\n\ts_nop 15\n\ts_nop 7"
#define MFMA(text)                                                                             \
  {                                                                                            \
    OUT;                                                                                       \
    asm volatile("s_nop 4\n\t" text " %0, %1, %2, %3" MFMA_PAD : "=&v"(o_) : IN4);              \
    DONE;                                                                                      \
  }
#define MFMA_MOD(text, mods)                                                                   \
  {                                                                                            \
    OUT;                                                                                       \
    asm volatile("s_nop 4\n\t" text " %0, %1, %2, %3 " mods MFMA_PAD : "=&v"(o_) : IN4);        \
    DONE;                                                                                      \
  }
// The block-scaled form: operand 3 holds the two scale words.
#define MFMA_SCALE(text, mods)                                                                          \
  {                                                                                                     \
    OUT;                                                                                                \
    asm volatile("s_nop 4\n\t" text " %0, %1, %2, %3, %4, %5 op_sel_hi:[0,0,0] " mods MFMA_PAD          \
                 : "=&v"(o_)                                                                            \
                 : "v"(reg(a)), "v"(reg(b)), "v"(reg(cc)), "v"(d.w[0]), "v"(d.w[1]));                   \
    DONE;                                                                                               \
  }
// SMFMAC accumulates in place: operand 3 is C, operand 2 the index. Both abid
// encodings run, each on its own copy of C: the result is the two tiles in turn.
#define SMFMAC(text, lo_abid, hi_abid)                                                                        \
  {                                                                                                           \
    constexpr int NH = NR / 2;                                                                                \
    typename Reg<NH>::type lo_ = reg(d), hi_ = reg(d);                                                        \
    asm volatile("s_nop 4\n\t" text " %0, %1, %2, %3 cbsz:1 abid:" lo_abid MFMA_PAD                           \
                 : "+v"(lo_)                                                                                  \
                 : "v"(reg(a)), "v"(reg(b)), "v"(reg(cc)));                                                   \
    asm volatile("s_nop 4\n\t" text " %0, %1, %2, %3 cbsz:1 abid:" hi_abid MFMA_PAD                           \
                 : "+v"(hi_)                                                                                  \
                 : "v"(reg(a)), "v"(reg(b)), "v"(reg(cc)));                                                   \
    const Words<NH> t0 = words<NH>(lo_), t1 = words<NH>(hi_);                                                 \
    _Pragma("unroll") for (int j = 0; j < NH; ++j) {                                                          \
      v.w[j] = t0.w[j];                                                                                       \
      v.w[NH + j] = t1.w[j];                                                                                  \
    }                                                                                                         \
  }
#define SMFMAC16(text) SMFMAC(text, "1", "3")
#define SMFMAC8(text) SMFMAC(text, "0", "1")

#define XS_LGKM "\n\ts_waitcnt lgkmcnt(0)"
XS_D void ds_w32(uint32_t addr, uint32_t x) { asm volatile("ds_write_b32 %0, %1" XS_LGKM ::"v"(addr), "v"(x) : "memory"); }
XS_D uint32_t ds_r32(uint32_t addr) {
  uint32_t r;
  asm volatile("ds_read_b32 %0, %1" XS_LGKM : "=&v"(r) : "v"(addr) : "memory");
  return r;
}
// A transposed read over the wave's tile: 8 hashed words per lane (operand 0),
// lane l reading at (l & 15) x stride + (l >> 4) x step.
#define LDS_TR(text, stride, step)                                                              \
  {                                                                                             \
    _Pragma("unroll") for (uint32_t j = 0; j < 8; ++j) ds_w32(c.tile + 4 * (64 * j + c.lane), a.w[j]); \
    const uint32_t at = c.tile + (c.lane & 15u) * stride + (c.lane >> 4) * step;                \
    OUT;                                                                                        \
    asm volatile(text " %0, %1" XS_LGKM : "=&v"(o_) : "v"(at) : "memory");                       \
    DONE;                                                                                       \
  }
// A returning LDS atomic of NW words on the lane's own 8 bytes: operand 0 is
// stored, the atomic applies operand 1; the result is {returned, read back}.
#define LDS_ATOMIC(text, NW)                                                                    \
  {                                                                                             \
    const uint32_t at = c.tile + 8 * c.lane;                                                    \
    _Pragma("unroll") for (uint32_t j = 0; j < NW; ++j) ds_w32(at + 4 * j, a.w[j]);              \
    typename Reg<NW>::type o_;                                                                  \
    asm volatile(text " %0, %1, %2" XS_LGKM : "=&v"(o_) : "v"(at), "v"(reg(b)) : "memory");      \
    const Words<NW> got = words<NW>(o_);                                                        \
    _Pragma("unroll") for (uint32_t j = 0; j < NW; ++j) {                                        \
      v.w[j] = got.w[j];                                                                        \
      v.w[NW + j] = ds_r32(at + 4 * j);                                                         \
    }                                                                                           \
  }
// ds_cmpst_rtn_f32: odd lanes compare with what is stored, even lanes with operand 1.
#define LDS_CMPST                                                                               \
  {                                                                                             \
    const uint32_t at = c.tile + 8 * c.lane;                                                    \
    ds_w32(at, a.w[0]);                                                                         \
    const uint32_t cmp = (c.lane & 1u) ? a.w[0] : b.w[0];                                       \
    uint32_t o_;                                                                                \
    asm volatile("ds_cmpst_rtn_f32 %0, %1, %2, %3" XS_LGKM : "=&v"(o_) : "v"(at), "v"(cmp), "v"(cc.w[0]) : "memory"); \
    v.w[0] = o_;                                                                                \
    v.w[1] = ds_r32(at);                                                                        \
  }

// X(part, id, mnemonic, result words, kind a, words a, kind b, words b, kind c, words c, kind d, words d, device code)
// The device code reads a, b, cc, d (Words<n>) and writes v (Words<result words>).
#define CONSENSUS_STEPS(X)                                                                                             \
  /* ---- trans */                                                                                                     \
  X(0, exp_f32, "v_exp_f32", 1, F32X, 1, NONE, 0, NONE, 0, NONE, 0, A("v_exp_f32_e32 %0, %1"))                                  \
  X(0, log_f32, "v_log_f32", 1, F32NP, 1, NONE, 0, NONE, 0, NONE, 0, A("v_log_f32_e32 %0, %1"))                                 \
  X(0, rcp_f32, "v_rcp_f32", 1, F32N, 1, NONE, 0, NONE, 0, NONE, 0, A("v_rcp_f32_e32 %0, %1"))                                  \
  X(0, rsq_f32, "v_rsq_f32", 1, F32NP, 1, NONE, 0, NONE, 0, NONE, 0, A("v_rsq_f32_e32 %0, %1"))                                 \
  X(0, sqrt_f32, "v_sqrt_f32", 1, F32NP, 1, NONE, 0, NONE, 0, NONE, 0, A("v_sqrt_f32_e32 %0, %1"))                              \
  X(0, sin_f32, "v_sin_f32", 1, F32REV, 1, NONE, 0, NONE, 0, NONE, 0, A("v_sin_f32_e32 %0, %1"))                                \
  X(0, cos_f32, "v_cos_f32", 1, F32REV, 1, NONE, 0, NONE, 0, NONE, 0, A("v_cos_f32_e32 %0, %1"))                                \
  X(0, rcp_iflag_f32, "v_rcp_iflag_f32", 1, F32N, 1, NONE, 0, NONE, 0, NONE, 0, A("v_rcp_iflag_f32_e32 %0, %1"))                \
  X(0, exp_legacy_f32, "v_exp_legacy_f32", 1, F32X, 1, NONE, 0, NONE, 0, NONE, 0, A("v_exp_legacy_f32_e32 %0, %1"))             \
  X(0, log_legacy_f32, "v_log_legacy_f32", 1, F32NP, 1, NONE, 0, NONE, 0, NONE, 0, A("v_log_legacy_f32_e32 %0, %1"))            \
  X(0, rcp_f64, "v_rcp_f64", 2, F64N, 2, NONE, 0, NONE, 0, NONE, 0, A("v_rcp_f64_e32 %0, %1"))                                  \
  X(0, rsq_f64, "v_rsq_f64", 2, F64NP, 2, NONE, 0, NONE, 0, NONE, 0, A("v_rsq_f64_e32 %0, %1"))                                 \
  X(0, sqrt_f64, "v_sqrt_f64", 2, F64NP, 2, NONE, 0, NONE, 0, NONE, 0, A("v_sqrt_f64_e32 %0, %1"))                              \
  X(0, rcp_f16, "v_rcp_f16", 1, F16N, 1, NONE, 0, NONE, 0, NONE, 0, LOW16("v_rcp_f16_e32 %0, %1"))                              \
  X(0, rsq_f16, "v_rsq_f16", 1, F16NP, 1, NONE, 0, NONE, 0, NONE, 0, LOW16("v_rsq_f16_e32 %0, %1"))                             \
  X(0, sqrt_f16, "v_sqrt_f16", 1, F16NP, 1, NONE, 0, NONE, 0, NONE, 0, LOW16("v_sqrt_f16_e32 %0, %1"))                          \
  X(0, exp_f16, "v_exp_f16", 1, F16N, 1, NONE, 0, NONE, 0, NONE, 0, LOW16("v_exp_f16_e32 %0, %1"))                              \
  X(0, log_f16, "v_log_f16", 1, F16NP, 1, NONE, 0, NONE, 0, NONE, 0, LOW16("v_log_f16_e32 %0, %1"))                             \
  /* ---- div */                                                                                                       \
  X(1, div_scale_f32, "v_div_scale_f32", 2, F32N, 1, F32N, 1, F32N, 1, NONE, 0, DIV_SCALE("v_div_scale_f32", uint32_t, 1))  \
  X(1, div_fmas_f32, "v_div_fmas_f32", 1, F32B, 1, F32B, 1, F32B, 1, BIT, 1, FMAS("v_div_fmas_f32 %0, %1, %2, %3"))    \
  X(1, div_fixup_f32, "v_div_fixup_f32", 1, F32N, 1, F32N, 1, F32N, 1, NONE, 0, A("v_div_fixup_f32 %0, %1, %2, %3"))        \
  X(1, div_f32, "div_f32", 1, F32N, 1, F32N, 1, NONE, 0, NONE, 0, DIV_F32)                                                       \
  X(1, div_scale_f64, "v_div_scale_f64", 3, F64N, 2, F64N, 2, F64N, 2, NONE, 0, DIV_SCALE("v_div_scale_f64", uint64_t, 2))  \
  X(1, div_fmas_f64, "v_div_fmas_f64", 2, F64B, 2, F64B, 2, F64B, 2, BIT, 1, FMAS("v_div_fmas_f64 %0, %1, %2, %3"))    \
  X(1, div_fixup_f64, "v_div_fixup_f64", 2, F64N, 2, F64N, 2, F64N, 2, NONE, 0, A("v_div_fixup_f64 %0, %1, %2, %3"))        \
  X(1, div_f64, "div_f64", 2, F64N, 2, F64N, 2, NONE, 0, NONE, 0, DIV_F64)                                                       \
  X(1, trig_preop_f64, "v_trig_preop_f64", 2, F64N, 2, U32, 1, NONE, 0, NONE, 0, A("v_trig_preop_f64 %0, %1, %2"))               \
  X(1, mul_legacy_f32, "v_mul_legacy_f32", 1, E32, 1, E32, 1, NONE, 0, NONE, 0, A("v_mul_legacy_f32 %0, %1, %2"))            \
  X(1, fma_legacy_f16, "v_fma_legacy_f16", 1, E16PK, 1, E16PK, 1, E16PK, 1, NONE, 0, LOW16("v_fma_legacy_f16 %0, %1, %2, %3")) \
  X(1, mad_legacy_f16, "v_mad_legacy_f16", 1, E16PK, 1, E16PK, 1, E16PK, 1, NONE, 0, LOW16("v_mad_legacy_f16 %0, %1, %2, %3")) \
  X(1, cubeid_f32, "v_cubeid_f32", 1, F32B, 1, F32B, 1, F32B, 1, NONE, 0, A("v_cubeid_f32 %0, %1, %2, %3"))                 \
  X(1, cubesc_f32, "v_cubesc_f32", 1, F32B, 1, F32B, 1, F32B, 1, NONE, 0, A("v_cubesc_f32 %0, %1, %2, %3"))                 \
  X(1, cubetc_f32, "v_cubetc_f32", 1, F32B, 1, F32B, 1, F32B, 1, NONE, 0, A("v_cubetc_f32 %0, %1, %2, %3"))                 \
  X(1, cubema_f32, "v_cubema_f32", 1, F32B, 1, F32B, 1, F32B, 1, NONE, 0, A("v_cubema_f32 %0, %1, %2, %3"))                 \
  /* ---- sr: value, random word, scale */                                                                             \
  X(2, cvt_sr_fp8_f32, "v_cvt_sr_fp8_f32", 1, SR(T_FP8, S_F32, 0), 1, U32, 1, NONE, 0, NONE, 0,                                  \
    PART8("v_cvt_sr_fp8_f32 %0, %1, %2"))                                                                              \
  X(2, cvt_sr_bf8_f32, "v_cvt_sr_bf8_f32", 1, SR(T_BF8, S_F32, 0), 1, U32, 1, NONE, 0, NONE, 0,                                  \
    PART8("v_cvt_sr_bf8_f32 %0, %1, %2"))                                                                              \
  X(2, cvt_sr_f16_f32, "v_cvt_sr_f16_f32", 1, SR(T_F16, S_F32, 0), 1, U32, 1, NONE, 0, NONE, 0,                                  \
    PART16("v_cvt_sr_f16_f32 %0, %1, %2"))                                                                             \
  X(2, cvt_sr_bf16_f32, "v_cvt_sr_bf16_f32", 1, SR(T_BF16, S_F32, 0), 1, U32, 1, NONE, 0, NONE, 0,                               \
    PART16("v_cvt_sr_bf16_f32 %0, %1, %2"))                                                                            \
  X(2, sr_fp8_f32, "v_cvt_scalef32_sr_fp8_f32", 1, SR(T_FP8, S_F32, 1), 1, U32, 1, SCALE, 1, NONE, 0,                       \
    PART8("v_cvt_scalef32_sr_fp8_f32 %0, %1, %2, %3"))                                                                 \
  X(2, sr_fp8_f16, "v_cvt_scalef32_sr_fp8_f16", 1, SR(T_FP8, S_F16, 1), 1, U32, 1, SCALE, 1, NONE, 0,                       \
    PART8("v_cvt_scalef32_sr_fp8_f16 %0, %1, %2, %3"))                                                                 \
  X(2, sr_fp8_bf16, "v_cvt_scalef32_sr_fp8_bf16", 1, SR(T_FP8, S_BF16, 1), 1, U32, 1, SCALE, 1, NONE, 0,                    \
    PART8("v_cvt_scalef32_sr_fp8_bf16 %0, %1, %2, %3"))                                                                \
  X(2, sr_bf8_f32, "v_cvt_scalef32_sr_bf8_f32", 1, SR(T_BF8, S_F32, 1), 1, U32, 1, SCALE, 1, NONE, 0,                       \
    PART8("v_cvt_scalef32_sr_bf8_f32 %0, %1, %2, %3"))                                                                 \
  X(2, sr_bf8_f16, "v_cvt_scalef32_sr_bf8_f16", 1, SR(T_BF8, S_F16, 1), 1, U32, 1, SCALE, 1, NONE, 0,                       \
    PART8("v_cvt_scalef32_sr_bf8_f16 %0, %1, %2, %3"))                                                                 \
  X(2, sr_bf8_bf16, "v_cvt_scalef32_sr_bf8_bf16", 1, SR(T_BF8, S_BF16, 1), 1, U32, 1, SCALE, 1, NONE, 0,                    \
    PART8("v_cvt_scalef32_sr_bf8_bf16 %0, %1, %2, %3"))                                                                \
  X(2, sr_pk_fp4_f32, "v_cvt_scalef32_sr_pk_fp4_f32", 1, SR(T_FP4, S_F32, 1), 2, U32, 1, SCALE, 1, NONE, 0,                 \
    PART8("v_cvt_scalef32_sr_pk_fp4_f32 %0, %1, %2, %3"))                                                              \
  X(2, sr_pk_fp4_f16, "v_cvt_scalef32_sr_pk_fp4_f16", 1, SR(T_FP4, S_F16, 1), 1, U32, 1, SCALE, 1, NONE, 0,                 \
    PART8("v_cvt_scalef32_sr_pk_fp4_f16 %0, %1, %2, %3"))                                                              \
  X(2, sr_pk_fp4_bf16, "v_cvt_scalef32_sr_pk_fp4_bf16", 1, SR(T_FP4, S_BF16, 1), 1, U32, 1, SCALE, 1, NONE, 0,              \
    PART8("v_cvt_scalef32_sr_pk_fp4_bf16 %0, %1, %2, %3"))                                                             \
  X(2, sr_pk32_fp6_f32, "v_cvt_scalef32_sr_pk32_fp6_f32", 6, SR(T_FP6, S_F32, 1), 32, U32, 1, SCALE, 1, NONE, 0,            \
    A("v_cvt_scalef32_sr_pk32_fp6_f32 %0, %1, %2, %3"))                                                                \
  X(2, sr_pk32_fp6_f16, "v_cvt_scalef32_sr_pk32_fp6_f16", 6, SR(T_FP6, S_F16, 1), 16, U32, 1, SCALE, 1, NONE, 0,            \
    A("v_cvt_scalef32_sr_pk32_fp6_f16 %0, %1, %2, %3"))                                                                \
  X(2, sr_pk32_fp6_bf16, "v_cvt_scalef32_sr_pk32_fp6_bf16", 6, SR(T_FP6, S_BF16, 1), 16, U32, 1, SCALE, 1, NONE, 0,         \
    A("v_cvt_scalef32_sr_pk32_fp6_bf16 %0, %1, %2, %3"))                                                               \
  X(2, sr_pk32_bf6_f32, "v_cvt_scalef32_sr_pk32_bf6_f32", 6, SR(T_BF6, S_F32, 1), 32, U32, 1, SCALE, 1, NONE, 0,            \
    A("v_cvt_scalef32_sr_pk32_bf6_f32 %0, %1, %2, %3"))                                                                \
  X(2, sr_pk32_bf6_f16, "v_cvt_scalef32_sr_pk32_bf6_f16", 6, SR(T_BF6, S_F16, 1), 16, U32, 1, SCALE, 1, NONE, 0,            \
    A("v_cvt_scalef32_sr_pk32_bf6_f16 %0, %1, %2, %3"))                                                                \
  X(2, sr_pk32_bf6_bf16, "v_cvt_scalef32_sr_pk32_bf6_bf16", 6, SR(T_BF6, S_BF16, 1), 16, U32, 1, SCALE, 1, NONE, 0,         \
    A("v_cvt_scalef32_sr_pk32_bf6_bf16 %0, %1, %2, %3"))                                                               \
  X(2, prng_b32, "v_prng_b32", 1, U32, 1, NONE, 0, NONE, 0, NONE, 0, A("v_prng_b32_e32 %0, %1"))                                \
  /* ---- edge: f32 */                                                                                                 \
  X(3, add_f32, "v_add_f32", 1, E32, 1, E32, 1, NONE, 0, NONE, 0, A("v_add_f32_e32 %0, %1, %2"))                                 \
  X(3, mul_f32, "v_mul_f32", 1, E32, 1, E32, 1, NONE, 0, NONE, 0, A("v_mul_f32_e32 %0, %1, %2"))                                 \
  X(3, fma_f32, "v_fma_f32", 1, E32, 1, E32, 1, E32, 1, NONE, 0, A("v_fma_f32 %0, %1, %2, %3"))                             \
  X(3, min_f32, "v_min_f32", 1, E32, 1, E32, 1, NONE, 0, NONE, 0, A("v_min_f32_e32 %0, %1, %2"))                                 \
  X(3, max_f32, "v_max_f32", 1, E32, 1, E32, 1, NONE, 0, NONE, 0, A("v_max_f32_e32 %0, %1, %2"))                                 \
  X(3, med3_f32, "v_med3_f32", 1, E32, 1, E32, 1, E32, 1, NONE, 0, A("v_med3_f32 %0, %1, %2, %3"))                          \
  X(3, minimum3_f32, "v_minimum3_f32", 1, E32, 1, E32, 1, E32, 1, NONE, 0, A("v_minimum3_f32 %0, %1, %2, %3"))              \
  X(3, maximum3_f32, "v_maximum3_f32", 1, E32, 1, E32, 1, E32, 1, NONE, 0, A("v_maximum3_f32 %0, %1, %2, %3"))              \
  X(3, ldexp_f32, "v_ldexp_f32", 1, E32, 1, EXPI, 1, NONE, 0, NONE, 0, A("v_ldexp_f32 %0, %1, %2"))                              \
  X(3, frexp_mant_f32, "v_frexp_mant_f32", 1, E32, 1, NONE, 0, NONE, 0, NONE, 0, A("v_frexp_mant_f32_e32 %0, %1"))              \
  X(3, frexp_exp_i32_f32, "v_frexp_exp_i32_f32", 1, E32, 1, NONE, 0, NONE, 0, NONE, 0, A("v_frexp_exp_i32_f32_e32 %0, %1"))     \
  X(3, fract_f32, "v_fract_f32", 1, E32, 1, NONE, 0, NONE, 0, NONE, 0, A("v_fract_f32_e32 %0, %1"))                             \
  X(3, trunc_f32, "v_trunc_f32", 1, E32, 1, NONE, 0, NONE, 0, NONE, 0, A("v_trunc_f32_e32 %0, %1"))                             \
  X(3, rndne_f32, "v_rndne_f32", 1, E32, 1, NONE, 0, NONE, 0, NONE, 0, A("v_rndne_f32_e32 %0, %1"))                             \
  X(3, floor_f32, "v_floor_f32", 1, E32, 1, NONE, 0, NONE, 0, NONE, 0, A("v_floor_f32_e32 %0, %1"))                             \
  X(3, ceil_f32, "v_ceil_f32", 1, E32, 1, NONE, 0, NONE, 0, NONE, 0, A("v_ceil_f32_e32 %0, %1"))                                \
  X(3, sub_f32, "v_sub_f32", 1, E32, 1, E32, 1, NONE, 0, NONE, 0, A("v_sub_f32_e32 %0, %1, %2"))                                \
  X(3, pk_add_f32, "v_pk_add_f32", 2, E32, 2, E32, 2, NONE, 0, NONE, 0, A("v_pk_add_f32 %0, %1, %2"))                           \
  X(3, pk_mul_f32, "v_pk_mul_f32", 2, E32, 2, E32, 2, NONE, 0, NONE, 0, A("v_pk_mul_f32 %0, %1, %2"))                           \
  X(3, pk_fma_f32, "v_pk_fma_f32", 2, E32, 2, E32, 2, E32, 2, NONE, 0, A("v_pk_fma_f32 %0, %1, %2, %3"))                        \
  X(3, min3_f32, "v_min3_f32", 1, E32, 1, E32, 1, E32, 1, NONE, 0, A("v_min3_f32 %0, %1, %2, %3"))                              \
  X(3, max3_f32, "v_max3_f32", 1, E32, 1, E32, 1, E32, 1, NONE, 0, A("v_max3_f32 %0, %1, %2, %3"))                              \
  X(3, cmp_lt_f32, "v_cmp_lt_f32", 1, E32, 1, E32, 1, NONE, 0, NONE, 0, CMP("v_cmp_lt_f32_e32 vcc, %1, %2"))                    \
  X(3, cmp_eq_f32, "v_cmp_eq_f32", 1, E32, 1, E32, 1, NONE, 0, NONE, 0, CMP("v_cmp_eq_f32_e32 vcc, %1, %2"))                    \
  X(3, cmp_le_f32, "v_cmp_le_f32", 1, E32, 1, E32, 1, NONE, 0, NONE, 0, CMP("v_cmp_le_f32_e32 vcc, %1, %2"))                    \
  X(3, cmp_gt_f32, "v_cmp_gt_f32", 1, E32, 1, E32, 1, NONE, 0, NONE, 0, CMP("v_cmp_gt_f32_e32 vcc, %1, %2"))                    \
  X(3, cmp_lg_f32, "v_cmp_lg_f32", 1, E32, 1, E32, 1, NONE, 0, NONE, 0, CMP("v_cmp_lg_f32_e32 vcc, %1, %2"))                    \
  X(3, cmp_ge_f32, "v_cmp_ge_f32", 1, E32, 1, E32, 1, NONE, 0, NONE, 0, CMP("v_cmp_ge_f32_e32 vcc, %1, %2"))                    \
  X(3, cmp_class_f32, "v_cmp_class_f32", 1, E32, 1, U32, 1, NONE, 0, NONE, 0, CMP("v_cmp_class_f32_e32 vcc, %1, %2"))           \
  /* ---- edge: f16 */                                                                                                 \
  X(3, add_f16, "v_add_f16", 1, E16PK, 1, E16PK, 1, NONE, 0, NONE, 0, LOW16("v_add_f16_e32 %0, %1, %2"))                         \
  X(3, mul_f16, "v_mul_f16", 1, E16PK, 1, E16PK, 1, NONE, 0, NONE, 0, LOW16("v_mul_f16_e32 %0, %1, %2"))                         \
  X(3, fma_f16, "v_fma_f16", 1, E16PK, 1, E16PK, 1, E16PK, 1, NONE, 0, LOW16("v_fma_f16 %0, %1, %2, %3"))                   \
  X(3, pk_add_f16, "v_pk_add_f16", 1, E16PK, 1, E16PK, 1, NONE, 0, NONE, 0, A("v_pk_add_f16 %0, %1, %2"))                        \
  X(3, pk_mul_f16, "v_pk_mul_f16", 1, E16PK, 1, E16PK, 1, NONE, 0, NONE, 0, A("v_pk_mul_f16 %0, %1, %2"))                        \
  X(3, pk_fma_f16, "v_pk_fma_f16", 1, E16PK, 1, E16PK, 1, E16PK, 1, NONE, 0, A("v_pk_fma_f16 %0, %1, %2, %3"))              \
  X(3, pk_min_f16, "v_pk_min_f16", 1, E16PK, 1, E16PK, 1, NONE, 0, NONE, 0, A("v_pk_min_f16 %0, %1, %2"))                        \
  X(3, pk_max_f16, "v_pk_max_f16", 1, E16PK, 1, E16PK, 1, NONE, 0, NONE, 0, A("v_pk_max_f16 %0, %1, %2"))                        \
  X(3, pk_minimum3_f16, "v_pk_minimum3_f16", 1, E16PK, 1, E16PK, 1, E16PK, 1, NONE, 0, A("v_pk_minimum3_f16 %0, %1, %2, %3"))   \
  X(3, pk_maximum3_f16, "v_pk_maximum3_f16", 1, E16PK, 1, E16PK, 1, E16PK, 1, NONE, 0, A("v_pk_maximum3_f16 %0, %1, %2, %3"))   \
  X(3, fma_mix_f32, "v_fma_mix_f32", 1, E16PK, 1, E16PK, 1, E32, 1, NONE, 0,                                                    \
    A("v_fma_mix_f32 %0, %1, %2, %3 op_sel:[0,1,0] op_sel_hi:[1,1,0]"))                                                         \
  X(3, fma_mixlo_f16, "v_fma_mixlo_f16", 1, E16PK, 1, E16PK, 1, E16PK, 1, NONE, 0,                                              \
    ZEROED("v_fma_mixlo_f16 %0, %1, %2, %3 op_sel:[1,0,0] op_sel_hi:[1,1,1]"))                                                  \
  /* ---- edge: cvt */                                                                                                 \
  X(3, cvt_f16_f32, "v_cvt_f16_f32", 1, EW32, 1, NONE, 0, NONE, 0, NONE, 0, LOW16("v_cvt_f16_f32_e32 %0, %1"))                  \
  X(3, cvt_f32_f16, "v_cvt_f32_f16", 1, E16PK, 1, NONE, 0, NONE, 0, NONE, 0, A("v_cvt_f32_f16_e32 %0, %1"))                     \
  X(3, cvt_pk_bf16_f32, "v_cvt_pk_bf16_f32", 1, EW32, 1, EW32, 1, NONE, 0, NONE, 0, A("v_cvt_pk_bf16_f32 %0, %1, %2"))           \
  X(3, cvt_pkrtz_f16_f32, "v_cvt_pkrtz_f16_f32", 1, EW32, 1, EW32, 1, NONE, 0, NONE, 0, A("v_cvt_pkrtz_f16_f32 %0, %1, %2"))     \
  X(3, cvt_pk_fp8_f32, "v_cvt_pk_fp8_f32", 1, EW32, 1, EW32, 1, NONE, 0, NONE, 0, PART16("v_cvt_pk_fp8_f32 %0, %1, %2"))         \
  X(3, cvt_pk_bf8_f32, "v_cvt_pk_bf8_f32", 1, EW32, 1, EW32, 1, NONE, 0, NONE, 0, PART16("v_cvt_pk_bf8_f32 %0, %1, %2"))         \
  X(3, cvt_f32_fp8, "v_cvt_f32_fp8", 1, U32, 1, NONE, 0, NONE, 0, NONE, 0, A("v_cvt_f32_fp8_e32 %0, %1"))                       \
  X(3, cvt_f32_bf8, "v_cvt_f32_bf8", 1, U32, 1, NONE, 0, NONE, 0, NONE, 0, A("v_cvt_f32_bf8_e32 %0, %1"))                       \
  X(3, cvt_i32_f32, "v_cvt_i32_f32", 1, EW32, 1, NONE, 0, NONE, 0, NONE, 0, A("v_cvt_i32_f32_e32 %0, %1"))                      \
  X(3, cvt_u32_f32, "v_cvt_u32_f32", 1, EW32, 1, NONE, 0, NONE, 0, NONE, 0, A("v_cvt_u32_f32_e32 %0, %1"))                      \
  X(3, scalef32_pk_fp8_f32, "v_cvt_scalef32_pk_fp8_f32", 1, EW32, 1, EW32, 1, SCALE, 1, NONE, 0,                            \
    PART16("v_cvt_scalef32_pk_fp8_f32 %0, %1, %2, %3"))                                                                \
  X(3, scalef32_pk_bf8_f32, "v_cvt_scalef32_pk_bf8_f32", 1, EW32, 1, EW32, 1, SCALE, 1, NONE, 0,                            \
    PART16("v_cvt_scalef32_pk_bf8_f32 %0, %1, %2, %3"))                                                                \
  X(3, scalef32_pk_fp4_f32, "v_cvt_scalef32_pk_fp4_f32", 1, EW32, 1, EW32, 1, SCALE, 1, NONE, 0,                            \
    PART8("v_cvt_scalef32_pk_fp4_f32 %0, %1, %2, %3"))                                                                 \
  X(3, pk32_fp6_f16, "v_cvt_scalef32_pk32_fp6_f16", 6, E16PK, 16, SCALE, 1, NONE, 0, NONE, 0,                                    \
    A("v_cvt_scalef32_pk32_fp6_f16 %0, %1, %2"))                                                                       \
  X(3, pk32_bf6_f16, "v_cvt_scalef32_pk32_bf6_f16", 6, E16PK, 16, SCALE, 1, NONE, 0, NONE, 0,                                    \
    A("v_cvt_scalef32_pk32_bf6_f16 %0, %1, %2"))                                                                       \
  X(3, pk32_fp6_bf16, "v_cvt_scalef32_pk32_fp6_bf16", 6, EBFPK, 16, SCALE, 1, NONE, 0, NONE, 0,                                  \
    A("v_cvt_scalef32_pk32_fp6_bf16 %0, %1, %2"))                                                                      \
  X(3, pk32_bf6_bf16, "v_cvt_scalef32_pk32_bf6_bf16", 6, EBFPK, 16, SCALE, 1, NONE, 0, NONE, 0,                                  \
    A("v_cvt_scalef32_pk32_bf6_bf16 %0, %1, %2"))                                                                      \
  X(3, x2pk16_fp6_f32, "v_cvt_scalef32_2xpk16_fp6_f32", 6, EW32, 16, EW32, 16, SCALE, 1, NONE, 0,                           \
    A("v_cvt_scalef32_2xpk16_fp6_f32 %0, %1, %2, %3"))                                                                 \
  X(3, x2pk16_bf6_f32, "v_cvt_scalef32_2xpk16_bf6_f32", 6, EW32, 16, EW32, 16, SCALE, 1, NONE, 0,                           \
    A("v_cvt_scalef32_2xpk16_bf6_f32 %0, %1, %2, %3"))                                                                 \
  X(3, cvt_pk_u8_f32, "v_cvt_pk_u8_f32", 1, F32U8, 1, U32, 1, U32, 1, NONE, 0, A("v_cvt_pk_u8_f32 %0, %1, %2, %3"))         \
  X(3, cvt_pknorm_i16_f32, "v_cvt_pknorm_i16_f32", 1, F32NORM, 1, F32NORM, 1, NONE, 0, NONE, 0,                                  \
    A("v_cvt_pknorm_i16_f32 %0, %1, %2"))                                                                              \
  X(3, cvt_pknorm_u16_f32, "v_cvt_pknorm_u16_f32", 1, F32NORM, 1, F32NORM, 1, NONE, 0, NONE, 0,                                  \
    A("v_cvt_pknorm_u16_f32 %0, %1, %2"))                                                                              \
  X(3, cvt_rpi_i32_f32, "v_cvt_rpi_i32_f32", 1, EW32, 1, NONE, 0, NONE, 0, NONE, 0, A("v_cvt_rpi_i32_f32_e32 %0, %1"))          \
  X(3, cvt_flr_i32_f32, "v_cvt_flr_i32_f32", 1, EW32, 1, NONE, 0, NONE, 0, NONE, 0, A("v_cvt_flr_i32_f32_e32 %0, %1"))          \
  X(3, cvt_f64_f32, "v_cvt_f64_f32", 2, E32, 1, NONE, 0, NONE, 0, NONE, 0, A("v_cvt_f64_f32_e32 %0, %1"))                       \
  X(3, cvt_f32_f64, "v_cvt_f32_f64", 1, E64, 2, NONE, 0, NONE, 0, NONE, 0, A("v_cvt_f32_f64_e32 %0, %1"))                       \
  X(3, cvt_i32_f64, "v_cvt_i32_f64", 1, E64, 2, NONE, 0, NONE, 0, NONE, 0, A("v_cvt_i32_f64_e32 %0, %1"))                       \
  X(3, cvt_pk_f16_f32, "v_cvt_pk_f16_f32", 1, EW32, 1, EW32, 1, NONE, 0, NONE, 0, A("v_cvt_pk_f16_f32 %0, %1, %2"))             \
  X(3, cvt_f32_fp8_b1, "v_cvt_f32_fp8", 1, U32, 1, NONE, 0, NONE, 0, NONE, 0, A("v_cvt_f32_fp8_sdwa %0, %1 src0_sel:BYTE_1"))   \
  X(3, cvt_f32_fp8_b2, "v_cvt_f32_fp8", 1, U32, 1, NONE, 0, NONE, 0, NONE, 0, A("v_cvt_f32_fp8_sdwa %0, %1 src0_sel:BYTE_2"))   \
  X(3, cvt_f32_fp8_b3, "v_cvt_f32_fp8", 1, U32, 1, NONE, 0, NONE, 0, NONE, 0, A("v_cvt_f32_fp8_sdwa %0, %1 src0_sel:BYTE_3"))   \
  X(3, cvt_pk_f32_fp8, "v_cvt_pk_f32_fp8", 2, U32, 1, NONE, 0, NONE, 0, NONE, 0, A("v_cvt_pk_f32_fp8_e32 %0, %1"))              \
  X(3, scalef32_pk_f32_fp8, "v_cvt_scalef32_pk_f32_fp8", 2, U32, 1, SCALE, 1, NONE, 0, NONE, 0,                                 \
    A("v_cvt_scalef32_pk_f32_fp8 %0, %1, %2"))                                                                                  \
  X(3, cvt_f32_bf8_b1, "v_cvt_f32_bf8", 1, U32, 1, NONE, 0, NONE, 0, NONE, 0, A("v_cvt_f32_bf8_sdwa %0, %1 src0_sel:BYTE_1"))   \
  X(3, cvt_f32_bf8_b2, "v_cvt_f32_bf8", 1, U32, 1, NONE, 0, NONE, 0, NONE, 0, A("v_cvt_f32_bf8_sdwa %0, %1 src0_sel:BYTE_2"))   \
  X(3, cvt_f32_bf8_b3, "v_cvt_f32_bf8", 1, U32, 1, NONE, 0, NONE, 0, NONE, 0, A("v_cvt_f32_bf8_sdwa %0, %1 src0_sel:BYTE_3"))   \
  X(3, cvt_pk_f32_bf8, "v_cvt_pk_f32_bf8", 2, U32, 1, NONE, 0, NONE, 0, NONE, 0, A("v_cvt_pk_f32_bf8_e32 %0, %1"))              \
  X(3, scalef32_pk_f32_bf8, "v_cvt_scalef32_pk_f32_bf8", 2, U32, 1, SCALE, 1, NONE, 0, NONE, 0,                                 \
    A("v_cvt_scalef32_pk_f32_bf8 %0, %1, %2"))                                                                                  \
  X(3, scalef32_pk_f32_fp4, "v_cvt_scalef32_pk_f32_fp4", 2, U32, 1, SCALE, 1, NONE, 0, NONE, 0,                                 \
    A("v_cvt_scalef32_pk_f32_fp4 %0, %1, %2"))                                                                                  \
  X(3, pk32_f32_fp6, "v_cvt_scalef32_pk32_f32_fp6", 32, U32, 6, SCALE, 1, NONE, 0, NONE, 0,                                     \
    A("v_cvt_scalef32_pk32_f32_fp6 %0, %1, %2"))                                                                                \
  X(3, pk32_f32_bf6, "v_cvt_scalef32_pk32_f32_bf6", 32, U32, 6, SCALE, 1, NONE, 0, NONE, 0,                                     \
    A("v_cvt_scalef32_pk32_f32_bf6 %0, %1, %2"))                                                                                \
  /* ---- ldsx */                                                                                                      \
  X(4, tr_b8_64, "ds_read_b64_tr_b8", 2, U32, 8, NONE, 0, NONE, 0, NONE, 0, LDS_TR("ds_read_b64_tr_b8", 64u, 8u))               \
  X(4, tr_b8_80, "ds_read_b64_tr_b8", 2, U32, 8, NONE, 0, NONE, 0, NONE, 0, LDS_TR("ds_read_b64_tr_b8", 80u, 8u))               \
  X(4, tr_b4_64, "ds_read_b64_tr_b4", 2, U32, 8, NONE, 0, NONE, 0, NONE, 0, LDS_TR("ds_read_b64_tr_b4", 64u, 8u))               \
  X(4, tr_b4_80, "ds_read_b64_tr_b4", 2, U32, 8, NONE, 0, NONE, 0, NONE, 0, LDS_TR("ds_read_b64_tr_b4", 80u, 8u))               \
  X(4, tr_b6_64, "ds_read_b96_tr_b6", 3, U32, 8, NONE, 0, NONE, 0, NONE, 0, LDS_TR("ds_read_b96_tr_b6", 64u, 16u))              \
  X(4, tr_b6_96, "ds_read_b96_tr_b6", 3, U32, 8, NONE, 0, NONE, 0, NONE, 0, LDS_TR("ds_read_b96_tr_b6", 96u, 16u))              \
  X(4, ds_add_f32, "ds_add_rtn_f32", 2, F32B, 1, F32B, 1, NONE, 0, NONE, 0, LDS_ATOMIC("ds_add_rtn_f32", 1))                     \
  X(4, ds_min_f32, "ds_min_rtn_f32", 2, F32B, 1, F32B, 1, NONE, 0, NONE, 0, LDS_ATOMIC("ds_min_rtn_f32", 1))                     \
  X(4, ds_max_f32, "ds_max_rtn_f32", 2, F32B, 1, F32B, 1, NONE, 0, NONE, 0, LDS_ATOMIC("ds_max_rtn_f32", 1))                     \
  X(4, ds_add_f64, "ds_add_rtn_f64", 4, F64B, 2, F64B, 2, NONE, 0, NONE, 0, LDS_ATOMIC("ds_add_rtn_f64", 2))                     \
  X(4, ds_min_f64, "ds_min_rtn_f64", 4, F64B, 2, F64B, 2, NONE, 0, NONE, 0, LDS_ATOMIC("ds_min_rtn_f64", 2))                     \
  X(4, ds_max_f64, "ds_max_rtn_f64", 4, F64B, 2, F64B, 2, NONE, 0, NONE, 0, LDS_ATOMIC("ds_max_rtn_f64", 2))                     \
  X(4, ds_pk_add_f16, "ds_pk_add_rtn_f16", 2, PKF16, 1, PKF16, 1, NONE, 0, NONE, 0, LDS_ATOMIC("ds_pk_add_rtn_f16", 1))          \
  X(4, ds_pk_add_bf16, "ds_pk_add_rtn_bf16", 2, PKBF16, 1, PKBF16, 1, NONE, 0, NONE, 0, LDS_ATOMIC("ds_pk_add_rtn_bf16", 1))     \
  X(4, ds_cmpst_f32, "ds_cmpst_rtn_f32", 2, F32B, 1, F32B, 1, F32B, 1, NONE, 0, LDS_CMPST)                                  \
  /* ---- mfma: A, B, C, (scales) */                                                                                   \
  X(5, m16x32_f16, "v_mfma_f32_16x16x32_f16", 4, PKF16, 4, PKF16, 4, F32B, 4, NONE, 0, MFMA("v_mfma_f32_16x16x32_f16"))     \
  X(5, m16x32_bf16, "v_mfma_f32_16x16x32_bf16", 4, PKBF16, 4, PKBF16, 4, F32B, 4, NONE, 0, MFMA("v_mfma_f32_16x16x32_bf16")) \
  X(5, m16x16_f16, "v_mfma_f32_16x16x16_f16", 4, PKF16, 2, PKF16, 2, F32B, 4, NONE, 0, MFMA("v_mfma_f32_16x16x16_f16"))     \
  X(5, m16x16_bf16, "v_mfma_f32_16x16x16_bf16", 4, PKBF16, 2, PKBF16, 2, F32B, 4, NONE, 0, MFMA("v_mfma_f32_16x16x16_bf16")) \
  X(5, m16_fp8_fp8, "v_mfma_f32_16x16x32_fp8_fp8", 4, FP8W, 2, FP8W, 2, F32B, 4, NONE, 0, MFMA("v_mfma_f32_16x16x32_fp8_fp8")) \
  X(5, m16_bf8_bf8, "v_mfma_f32_16x16x32_bf8_bf8", 4, BF8W, 2, BF8W, 2, F32B, 4, NONE, 0, MFMA("v_mfma_f32_16x16x32_bf8_bf8")) \
  X(5, m16_fp8_bf8, "v_mfma_f32_16x16x32_fp8_bf8", 4, FP8W, 2, BF8W, 2, F32B, 4, NONE, 0, MFMA("v_mfma_f32_16x16x32_fp8_bf8")) \
  X(5, m16_bf8_fp8, "v_mfma_f32_16x16x32_bf8_fp8", 4, BF8W, 2, FP8W, 2, F32B, 4, NONE, 0, MFMA("v_mfma_f32_16x16x32_bf8_fp8")) \
  X(5, m32_fp8_bf8, "v_mfma_f32_32x32x16_fp8_bf8", 16, FP8W, 2, BF8W, 2, F32B, 16, NONE, 0, MFMA("v_mfma_f32_32x32x16_fp8_bf8")) \
  X(5, m32_bf8_fp8, "v_mfma_f32_32x32x16_bf8_fp8", 16, BF8W, 2, FP8W, 2, F32B, 16, NONE, 0, MFMA("v_mfma_f32_32x32x16_bf8_fp8")) \
  X(5, m16x64_i8, "v_mfma_i32_16x16x64_i8", 4, U32, 4, U32, 4, U32, 4, NONE, 0, MFMA("v_mfma_i32_16x16x64_i8"))             \
  X(5, m16x32_i8, "v_mfma_i32_16x16x32_i8", 4, U32, 2, U32, 2, U32, 4, NONE, 0, MFMA("v_mfma_i32_16x16x32_i8"))             \
  X(5, m16x4_f32, "v_mfma_f32_16x16x4_f32", 4, F32B, 1, F32B, 1, F32B, 4, NONE, 0, MFMA("v_mfma_f32_16x16x4_f32"))          \
  X(5, m4x4_f16, "v_mfma_f32_4x4x4_16b_f16", 4, PKF16, 2, PKF16, 2, F32B, 4, NONE, 0, MFMA("v_mfma_f32_4x4x4_16b_f16"))     \
  X(5, m4x4_bf16, "v_mfma_f32_4x4x4_16b_bf16", 4, PKBF16, 2, PKBF16, 2, F32B, 4, NONE, 0, MFMA("v_mfma_f32_4x4x4_16b_bf16")) \
  X(5, m4x4_f32, "v_mfma_f32_4x4x1_16b_f32", 4, F32B, 1, F32B, 1, F32B, 4, NONE, 0, MFMA("v_mfma_f32_4x4x1_16b_f32"))       \
  X(5, m4x4_i8, "v_mfma_i32_4x4x4_16b_i8", 4, U32, 1, U32, 1, U32, 4, NONE, 0, MFMA("v_mfma_i32_4x4x4_16b_i8"))             \
  X(5, m4x4_f64, "v_mfma_f64_4x4x4_4b_f64", 2, F64B, 2, F64B, 2, F64B, 2, NONE, 0, MFMA("v_mfma_f64_4x4x4_4b_f64"))         \
  X(5, f8f6f4_16, "v_mfma_f32_16x16x128_f8f6f4", 4, FP8W, 8, FP8W, 8, F32B, 4, NONE, 0, MFMA("v_mfma_f32_16x16x128_f8f6f4")) \
  X(5, f8f6f4_16_bf8_fp4, "v_mfma_f32_16x16x128_f8f6f4", 4, BF8W, 8, U32, 4, F32B, 4, NONE, 0,                              \
    MFMA_MOD("v_mfma_f32_16x16x128_f8f6f4", "cbsz:1 blgp:4"))                                                          \
  X(5, f8f6f4_16_fp6_bf6, "v_mfma_f32_16x16x128_f8f6f4", 4, U32, 6, U32, 6, F32B, 4, NONE, 0,                               \
    MFMA_MOD("v_mfma_f32_16x16x128_f8f6f4", "cbsz:2 blgp:3"))                                                          \
  X(5, f8f6f4_32, "v_mfma_f32_32x32x64_f8f6f4", 16, FP8W, 8, FP8W, 8, F32B, 16, NONE, 0, MFMA("v_mfma_f32_32x32x64_f8f6f4")) \
  X(5, f8f6f4_32_bf8_fp6, "v_mfma_f32_32x32x64_f8f6f4", 16, BF8W, 8, U32, 6, F32B, 16, NONE, 0,                             \
    MFMA_MOD("v_mfma_f32_32x32x64_f8f6f4", "cbsz:1 blgp:2"))                                                           \
  X(5, scale_16, "v_mfma_scale_f32_16x16x128_f8f6f4", 4, FP8W, 8, FP8W, 8, F32B, 4, SCALE8, 2,                         \
    MFMA_SCALE("v_mfma_scale_f32_16x16x128_f8f6f4", ""))                                                               \
  X(5, scale_16_bf8_fp4, "v_mfma_scale_f32_16x16x128_f8f6f4", 4, BF8W, 8, U32, 4, F32B, 4, SCALE8, 2,                  \
    MFMA_SCALE("v_mfma_scale_f32_16x16x128_f8f6f4", "cbsz:1 blgp:4"))                                                  \
  X(5, scale_32_fp8_fp6, "v_mfma_scale_f32_32x32x64_f8f6f4", 16, FP8W, 8, U32, 6, F32B, 16, SCALE8, 2,                 \
    MFMA_SCALE("v_mfma_scale_f32_32x32x64_f8f6f4", "cbsz:0 blgp:2"))                                                   \
  /* ---- smfmac: A (sparse), B, index, C */                                                                           \
  X(6, s16_f16, "v_smfmac_f32_16x16x64_f16", 8, PKF16, 4, PKF16, 8, U32, 1, F32B, 4, SMFMAC16("v_smfmac_f32_16x16x64_f16")) \
  X(6, s16_bf16, "v_smfmac_f32_16x16x64_bf16", 8, PKBF16, 4, PKBF16, 8, U32, 1, F32B, 4,                               \
    SMFMAC16("v_smfmac_f32_16x16x64_bf16"))                                                                            \
  X(6, s32_f16, "v_smfmac_f32_32x32x32_f16", 32, PKF16, 4, PKF16, 8, U32, 1, F32B, 16,                                 \
    SMFMAC16("v_smfmac_f32_32x32x32_f16"))                                                                             \
  X(6, s32_bf16, "v_smfmac_f32_32x32x32_bf16", 32, PKBF16, 4, PKBF16, 8, U32, 1, F32B, 16,                             \
    SMFMAC16("v_smfmac_f32_32x32x32_bf16"))                                                                            \
  X(6, s16_i8, "v_smfmac_i32_16x16x128_i8", 8, U32, 4, U32, 8, U32, 1, U32, 4, SMFMAC8("v_smfmac_i32_16x16x128_i8"))   \
  X(6, s32_i8, "v_smfmac_i32_32x32x64_i8", 32, U32, 4, U32, 8, U32, 1, U32, 16, SMFMAC8("v_smfmac_i32_32x32x64_i8"))   \
  X(6, s16_fp8_fp8, "v_smfmac_f32_16x16x128_fp8_fp8", 8, FP8W, 4, FP8W, 8, U32, 1, F32B, 4,                            \
    SMFMAC8("v_smfmac_f32_16x16x128_fp8_fp8"))                                                                         \
  X(6, s16_fp8_bf8, "v_smfmac_f32_16x16x128_fp8_bf8", 8, FP8W, 4, BF8W, 8, U32, 1, F32B, 4,                            \
    SMFMAC8("v_smfmac_f32_16x16x128_fp8_bf8"))                                                                         \
  X(6, s16_bf8_fp8, "v_smfmac_f32_16x16x128_bf8_fp8", 8, BF8W, 4, FP8W, 8, U32, 1, F32B, 4,                            \
    SMFMAC8("v_smfmac_f32_16x16x128_bf8_fp8"))                                                                         \
  X(6, s16_bf8_bf8, "v_smfmac_f32_16x16x128_bf8_bf8", 8, BF8W, 4, BF8W, 8, U32, 1, F32B, 4,                            \
    SMFMAC8("v_smfmac_f32_16x16x128_bf8_bf8"))                                                                         \
  X(6, s32_fp8_fp8, "v_smfmac_f32_32x32x64_fp8_fp8", 32, FP8W, 4, FP8W, 8, U32, 1, F32B, 16,                           \
    SMFMAC8("v_smfmac_f32_32x32x64_fp8_fp8"))                                                                          \
  X(6, s32_fp8_bf8, "v_smfmac_f32_32x32x64_fp8_bf8", 32, FP8W, 4, BF8W, 8, U32, 1, F32B, 16,                           \
    SMFMAC8("v_smfmac_f32_32x32x64_fp8_bf8"))                                                                          \
  X(6, s32_bf8_fp8, "v_smfmac_f32_32x32x64_bf8_fp8", 32, BF8W, 4, FP8W, 8, U32, 1, F32B, 16,                           \
    SMFMAC8("v_smfmac_f32_32x32x64_bf8_fp8"))                                                                          \
  X(6, s32_bf8_bf8, "v_smfmac_f32_32x32x64_bf8_bf8", 32, BF8W, 4, BF8W, 8, U32, 1, F32B, 16,                           \
    SMFMAC8("v_smfmac_f32_32x32x64_bf8_bf8"))

// ------------------------------------------------------------------ the table
#define X(P, ID, NAME, NRES, KA, NA, KB, NB, KC, NC, KD, ND, DEV) G_##ID,
enum StepId : int { CONSENSUS_STEPS(X) kNumSteps };
#undef X

struct StepInfo {
  int part, words;
  int kind[4], n[4];
};
#define X(P, ID, NAME, NRES, KA, NA, KB, NB, KC, NC, KD, ND, DEV) {P, NRES, {KA, KB, KC, KD}, {NA, NB, NC, ND}},
constexpr StepInfo kSteps[kNumSteps] = {CONSENSUS_STEPS(X)};
#undef X

XS_HD constexpr int part_first(int p) {  // global index of the part's first step
  int g = 0;
  while (g < kNumSteps && kSteps[g].part < p) ++g;
  return g;
}
XS_HD constexpr int part_steps(int p) { return part_first(p + 1) - part_first(p); }
XS_HD constexpr int step_row(int g) {  // row of step g's word 0 within its part
  int r = 0;
  for (int i = part_first(kSteps[g].part); i < g; ++i) r += kSteps[i].words;
  return r;
}
XS_HD constexpr int part_rows(int p) {
  int r = 0;
  for (int i = part_first(p); i < part_first(p + 1); ++i) r += kSteps[i].words;
  return r;
}
constexpr int operand_rows_of(const StepInfo& s) { return s.n[0] + s.n[1] + s.n[2] + s.n[3]; }
constexpr int part_operand_rows(int p) {
  int r = 0;
  for (int i = part_first(p); i < part_first(p + 1); ++i) r += operand_rows_of(kSteps[i]);
  return r;
}
constexpr bool parts_in_order() {
  for (int g = 1; g < kNumSteps; ++g)
    if (kSteps[g].part < kSteps[g - 1].part) return false;
  for (int p = 0; p < kNumParts; ++p)
    if (part_steps(p) <= 0 || part_steps(p) > 255) return false;
  return true;
}
static_assert(parts_in_order(), "CONSENSUS_STEPS lists the parts in order, none empty");

struct ConsensusRecord {
  uint32_t xcd, cu, simd_mask, fail;
  uint32_t digest[kNumParts];  // 0 for a part not selected
  uint32_t pad[21];
};
static_assert(sizeof(ConsensusRecord) == 128, "one 128-byte record per workgroup");

// ------------------------------------------------------------------- device
template <int K, int N>
XS_D Words<N> load_operand(const Ctx& c, uint32_t p, uint32_t s, uint32_t r, uint32_t o) {
  Words<N> x;
  x.w[0] = 0;
#pragma unroll
  for (int w = 0; w < N; ++w) x.w[w] = operand_word(K, c.seed, p, s, r, o, c.t, w);
  return x;
}

template <int G, typename Fn>
XS_D void run_step(const Ctx& c, Tally& y, uint32_t r, Fn&& fn) {
  constexpr int p = kSteps[G].part, s = G - part_first(p), row = step_row(G), rows = part_rows(p);
  constexpr int nres = kSteps[G].words;
  const auto a = load_operand<kSteps[G].kind[0], kSteps[G].n[0]>(c, p, s, r, 0);
  const auto b = load_operand<kSteps[G].kind[1], kSteps[G].n[1]>(c, p, s, r, 1);
  const auto cc = load_operand<kSteps[G].kind[2], kSteps[G].n[2]>(c, p, s, r, 2);
  const auto d = load_operand<kSteps[G].kind[3], kSteps[G].n[3]>(c, p, s, r, 3);
  const Words<nres> v = fn(a, b, cc, d);
#pragma unroll
  for (int w = 0; w < nres; ++w) {
    const uint32_t idx = (r * rows + row + w) * kBlock + c.t;
    take_word(y, c.dump, idx, v.w[w], v.w[w], (c.inj >> p) & 1u);
  }
}

template <int PART>
XS_D void run_part(const Ctx& c, Tally& y) {
  for (uint32_t r = 0; r < c.rounds; ++r) {
#define X(P, ID, NAME, NRES, KA, NA, KB, NB, KC, NC, KD, ND, DEV)                                              \
  if constexpr (P == PART)                                                                                     \
    run_step<G_##ID>(c, y, r,                                                                                  \
                     [&](const Words<NA>& a, const Words<NB>& b, const Words<NC>& cc,                          \
                         const Words<ND>& d) -> Words<NRES> {                                                  \
                       constexpr int NR = NRES;                                                                \
                       Words<NRES> v;                                                                          \
                       (void)a, (void)b, (void)cc, (void)d, (void)NR;                                          \
                       DEV;                                                                                    \
                       return v;                                                                               \
                     });
    CONSENSUS_STEPS(X)
#undef X
  }
}

XS_D void run_parts(const Ctx& c, uint32_t mask, Tally (&y)[kNumParts]) {
  if (mask & 1u) run_part<0>(c, y[0]);
  if (mask & 2u) run_part<1>(c, y[1]);
  if (mask & 4u) run_part<2>(c, y[2]);
  if (mask & 8u) run_part<3>(c, y[3]);
  if (mask & 16u) run_part<4>(c, y[4]);
  if (mask & 32u) run_part<5>(c, y[5]);
  if (mask & 64u) run_part<6>(c, y[6]);
}

XS_D Ctx make_ctx(uint32_t seed, uint32_t t, uint32_t rounds, uint32_t inj, uint32_t* dump) {
  return Ctx{seed, t, rounds, inj, dump, kTileOff + (t >> 6) * kTileBytes, t & 63u};
}

__global__ __launch_bounds__(kBlock) void k_consensus_sweep(ConsensusRecord* __restrict__ records, uint32_t part_mask,
                                                           uint32_t seed, uint32_t rounds, int inject_xcd,
                                                           int inject_cu, uint32_t inject_parts) {
  extern __shared__ uint32_t consensus_lds[];
  const uint32_t t = threadIdx.x;
  const uint32_t xcd = xcc_id();
  const uint32_t hw = hw_id();
  const uint32_t cu = cu_key(hw);
  const bool inject = inject_selected(inject_xcd, inject_cu, xcd, cu);
  const Ctx c = make_ctx(seed, t, rounds, inject ? inject_parts : 0u, nullptr);

  Tally y[kNumParts];
  run_parts(c, part_mask, y);

  // Plain LDS words and a barrier: no shuffle, DPP or permute.
  __syncthreads();
#pragma unroll
  for (int p = 0; p < kNumParts; ++p) consensus_lds[p * kBlock + t] = y[p].digest;
  consensus_lds[kNumParts * kBlock + t] = 1u << simd_id(hw);
  __syncthreads();
  if (t == 0) {
    uint32_t sum[kNumParts] = {}, simds = 0;
    for (int u = 0; u < kBlock; ++u) {
#pragma unroll
      for (int p = 0; p < kNumParts; ++p) sum[p] += consensus_lds[p * kBlock + u];
      simds |= consensus_lds[kNumParts * kBlock + u];
    }
    uint32_t w[32] = {xcd, cu, simds, 0u};
#pragma unroll
    for (int p = 0; p < kNumParts; ++p) w[4 + p] = (part_mask >> p) & 1u ? sum[p] : 0u;
    u32x4* out = reinterpret_cast<u32x4*>(&records[blockIdx.x]);
#pragma unroll
    for (uint32_t q = 0; q < 8; ++q) out[q] = u32x4{w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]};
  }
}

// One workgroup; dump holds rounds x rows x 256 words of part `part`.
__global__ __launch_bounds__(kBlock) void k_consensus_probe(uint32_t* __restrict__ dump, int part, uint32_t seed,
                                                           uint32_t rounds) {
  const Ctx c = make_ctx(seed, threadIdx.x, rounds, 0u, dump);
  Tally y[kNumParts];
  run_parts(c, 1u << part, y);
}

// --------------------------------------------------------------------- host
bool bad_rounds(uint32_t r) { return r < 1 || r > kMaxRounds; }

// The rounds a buffer of n_words holds at `per_round` x 256 words a round; 0 when it is no whole number of them.
uint32_t rounds_of(size_t n_words, int per_round) {
  const size_t one = static_cast<size_t>(per_round) * kBlock;
  if (n_words == 0 || n_words % one) return 0;
  const size_t r = n_words / one;
  return r > static_cast<size_t>(kMaxRounds) ? 0 : static_cast<uint32_t>(r);
}

}  // namespace

extern "C" {

const char* xs_consensus_sweep_last_error() { return g_consensus_err; }

// Part names, comma-separated, in bit order.
const char* xs_consensus_parts() { return kPartNames; }

// out3 = {steps, result words of one round (rows), operand words of one round}.
int xs_consensus_shape(int part, int* out3) {
  if (part < 0 || part >= kNumParts || !out3) return kBadArgs;
  out3[0] = part_steps(part);
  out3[1] = part_rows(part);
  out3[2] = part_operand_rows(part);
  return 0;
}

// Host only, no device. out[round][operand row][256]: the operand words of one
// workgroup in the step table's order (per step: the words of operand 0, then
// 1, 2, 3). n_words = rounds x operand rows x 256 says how many rounds.
int xs_consensus_operands(int part, uint32_t seed, uint32_t* out, size_t n_words) {
  if (part < 0 || part >= kNumParts || !out) return kBadArgs;
  const int rows = part_operand_rows(part), first = part_first(part);
  const uint32_t rounds = rounds_of(n_words, rows);
  if (!rounds) return kBadArgs;
  for (uint32_t r = 0; r < rounds; ++r) {
    size_t row = 0;
    for (int g = first; g < first + part_steps(part); ++g)
      for (uint32_t o = 0; o < 4; ++o)
        for (int w = 0; w < kSteps[g].n[o]; ++w, ++row)
          for (uint32_t t = 0; t < kBlock; ++t)
            out[(static_cast<size_t>(r) * rows + row) * kBlock + t] =
                operand_word(kSteps[g].kind[o], seed, part, g - first, r, o, t, w);
  }
  return 0;
}

// One workgroup runs `part` and stores every word it received as
// [round][row][256]; n_words = rounds x rows x 256 says how many rounds.
int xs_consensus_probe(int dev, int part, uint32_t seed, uint32_t* out, size_t n_words) {
  if (part < 0 || part >= kNumParts || !out) return kBadArgs;
  const uint32_t rounds = rounds_of(n_words, part_rows(part));
  if (!rounds) return kBadArgs;
  return launch_probe(g_consensus_err, dev, reinterpret_cast<const void*>(k_consensus_probe), kBlock, kLdsUsed, out,
                      n_words, [&](dim3 grid, dim3 block, size_t smem, void* dump) {
                        hipLaunchKernelGGL(k_consensus_probe, grid, block, smem, 0, static_cast<uint32_t*>(dump), part,
                                           seed, rounds);
                      });
}

// What the runtime reports for k_consensus_sweep on `dev`: out4 = {registers
// per lane, scratch bytes per lane, dynamic LDS bytes per workgroup,
// workgroups that fit on a CU at once}.
int xs_consensus_sweep_info(int dev, int* out4) {
  return sweep_info(g_consensus_err, dev, reinterpret_cast<const void*>(k_consensus_sweep), kBlock, true, out4);
}

// One sweep launch of `blocks` workgroups (0: 4 per CU). Writes `blocks`
// 128-byte records to records_out. inject_xcd / inject_cu: -1 is none / any,
// values below -1 are refused. Returns 0, -1000 for bad arguments (nothing is
// launched), or a negative HIP error.
int xs_consensus_sweep(int dev, int blocks, uint32_t part_mask, uint32_t seed, uint32_t rounds, int inject_xcd,
                       int inject_cu, uint32_t inject_parts, void* records_out, int* n_records, double* ms) {
  if (bad_part_mask(part_mask, kAllParts) || bad_rounds(rounds) || (inject_parts & ~kAllParts)) return kBadArgs;
  return launch_sweep(g_consensus_err, {dev, blocks, inject_xcd, inject_cu, records_out, n_records, ms},
                      reinterpret_cast<const void*>(k_consensus_sweep), kBlock, kLdsUsed, sizeof(ConsensusRecord),
                      [&](dim3 grid, dim3 block, size_t smem, void* rec) {
                        hipLaunchKernelGGL(k_consensus_sweep, grid, block, smem, 0, static_cast<ConsensusRecord*>(rec),
                                           part_mask, seed, rounds, inject_xcd, inject_cu, inject_parts);
                      });
}

}  // extern "C"
