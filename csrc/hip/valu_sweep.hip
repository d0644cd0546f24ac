// VALU sweep for gfx950 (MI355X): the vector ALU of every SIMD, unit by unit.
//
// The VALU engine of k_cu_sweep is an integer multiply-add, a shift-xor and a
// rotate. k_valu_sweep is the same kind of launch as the other per-CU sweeps
// (256-thread workgroups, 4 waves: one per SIMD, each asking for more than
// half of a CU's LDS so that no two share a CU, 4 x CUs of them, every
// workgroup self-contained) and issues, each under its own mnemonic, the
// floating-point, packed, wide-integer, bit-field, dot, conversion and
// transcendental instructions of the VALU on hashed operands. Every result is
// fixed by IEEE-754 or by integer arithmetic: one right answer, no tolerance.
//
// Units (bit, name). A unit is a list of steps; a step is one instruction (or
// one compiler expansion: the correctly rounded a / b and sqrt(a) of C++) with
// one or two result words per lane. VALU_STEPS below is the one table: it
// names each step, gives its operand kinds, the device code that issues it
// and the host expression that says what it must return.
//   0 f32   1 f64   2 f16   3 int   4 bit   5 dot   6 cvt   7 trans
//
// Float mode. The kernel relies on round-to-nearest-even, denormals preserved
// in all three widths and IEEE mode, which is the default kernel descriptor
// (.amdhsa_float_round_mode_32 0, _16_64 0, .amdhsa_float_denorm_mode_32 3,
// _16_64 3, .amdhsa_ieee_mode 1). It never writes the MODE register.
// tests/test_valu_codeobject.py reads all of this back.
//
// Operands. fmix32 is the murmur3 finaliser, as in lane_sweep.hip:
//   h(u, s, r, o, t) = fmix32(seed ^ (u << 28 | s << 20 | r << 12 | o << 8 | t))
// u = unit, s = step within the unit, r = round, t = thread (64 x wave + lane),
// o = operand 0..2, o + 8 for the high word of a 64-bit operand. All keys of a
// launch differ. The hash is shaped by the operand's kind:
//   U32      h                          U64     {h(o), h(o + 8)}
//   F32      sign h[31], significand h[22:0], exponent field 96 + h[30:23] % 63
//   F32P     F32 with the sign cleared  PKF32   two F32 (words o, o + 8)
//   F32GE1   F32, exponent 127 + h[30:23] % 11      (fract: 1 <= |x| < 2^11)
//   F32NEAR  F32, exponent 120 + h[30:23] % 18      (roundings: 2^-7 .. 2^11)
//   F32INT   F32, exponent 120 + h[30:23] % 38      (|x| < 2^31)
//   F32UINT  F32INT with the sign cleared
//   F32H     F32, exponent 114 + h[30:23] % 28      (inside f16's normal range)
//   F32Q     F32, exponent 121 + h[30:23] % 14      (inside fp8 / bf8's range)
//   F32QS    F32, exponent 123 + h[30:23] % 10; SCALE3 2^(h % 5 - 2): the quotient is inside fp8's range
//   F32F4    F32, exponent 126 + h[30:23] % 2; SCALE1 2^(h % 3 - 1): the quotient is below fp4's 6
//   F32B     an integer 0..255 as f32 (v_cvt_pk_u8_f32: its rounding is in no document at hand)
//   F32N8    k / 256, |k| <= 256, k != +-128 (v_cvt_pknorm_i16_f32: k x 32767 / 256 is exact in
//            f32 and never halfway between two integers, so rounding to nearest has one answer
//            whatever the tie rule and the width of the product)
//   F64      sign, 52 hashed significand bits, exponent field 992 + h[30:20] % 63
//   F64P / F64GE1 / F64NEAR / F64INT   as their F32 namesakes (1023 + ...)
//   PKF16    two halves: sign, 10 significand bits, exponent field 13 + e % 9
//   PKF16P   PKF16 with both signs cleared
//   I5       h[4:0] sign-extended (an ldexp exponent)
//   SH4      h % 5 (the shift of v_lshl_add_u64)
//   CLS32 / CLS64   class h % 10 of v_cmp_class: sNaN, qNaN, -Inf, -normal,
//            -subnormal, -0, +0, +subnormal, +normal, +Inf, other bits hashed
//   PERMSEL  four v_perm_b32 selector bytes: h.byte % 10 -> 0..7, 12 (0x00), 13 (0xff)
//   PKSI16 / PKSIBF  two small integers -15..15 as f16 / bf16; SIF32 one
//            integer -1023..1023 as f32 (dot: every partial sum is exact)
//   FP8 / BF8  four bytes, each a finite OCP e4m3fn / e5m2 encoding
//   EXPI     an integer -20..20 as f32      POW2F32 / POW2F64  +-2^n, |n| <= 20
//   POW4F32 / POW4F64  4^n, |n| <= 10       SQINT  k^2, k < 4096, as f32
//   QREV     k / 4, k = 0..7 (v_sin / v_cos take revolutions)
//   POW2F16 +-2^n, |n| <= 7; POW4F16 4^n, |n| <= 3; EXPIF16 an integer -7..7
// In these bands no sum, product, FMA, quotient or root is subnormal, infinite
// or NaN (tests/test_valu_ref.py). `rounds` (1..64) is the number of operand
// sets per step. Rounds 0 and 1 are edge rounds:
//   round 0  the significand (floats) or the whole word (U32, U64) of operand
//            o takes class c = (t >> 3o) & 7 (o = 2: (t >> 6) | (t & 1) << 2):
//            significand 0 all ones, 1 one hashed bit, 2 zero, 3 lowest bit;
//            word 0 0xffffffff, 1 0x80000000, 2 0, 3 1, 4 0x7fffffff; else hashed.
//   round 1  lanes with (lane & 15) < n of a step that has a special take
//            fixed operands (special() below): the subnormal-result sums and
//            FMAs of each width, the f32 FMA triple 24929 x 673 + 2^-40 (the
//            exact sum rounds to 2^24 + 2, through float64 to 2^24), exact
//            ties k + 1/2 for rndne, exact ties for every narrowing cvt but the
//            two fed one exact class (pk_u8, pknorm), equal operands for the
//            compares. A scaled narrowing keeps its hashed power-of-two scale:
//            the quotient of a tie by it is a tie.
// v_cvt_scalef32_pk32_f32_fp6 unpacks the 192 bits of its three U64 operands
// (element i at bits 6i .. 6i + 5, OCP e2m3) into 32 f32, times the scale
// 2^((a >> 32) % 5 - 2); every product is exact. Its two result words are
// folds of the 32: sum of r_i (2i + 1), and the XOR of all r_i. One wrong bit
// in any r_i moves the first word.
// No step produces a NaN.
//
// Comparison. The host computes every expected word from the same table (the
// HOST column: std::fma / fmaf where a fused result is meant, contraction off
// for everything else) and uploads it: [unit][round][row][256], row = the
// words of the unit's steps in order. The device compares by integer equality,
// counts mismatches per unit and accumulates D_u += got * (2 idx + 1), idx =
// (round * rows_u + row) * 256 + t (lane_sweep.hip's rule); part_sweep.h's
// reduce_parts() makes the workgroup's record of them. The comparator leans
// on global loads, v_cmp_eq_u32 and the integer VALU that builds operands: a
// fault there is a mis-compare, not a pass.
//
// Record (128 bytes per workgroup): part_sweep.h's head with a unit per part, a
// reserved word, and six words of bits over the global step index (the order
// of VALU_STEPS) of the steps that mis-compared.
//
// Injection: a workgroup on inject_xcd whose CU key is inject_cu (any with
// -1; -1 for inject_xcd means none; values below -1 are refused) flips bit 0
// of the value thread 0 got at step 0, round 0, word 0 of each unit in the
// inject mask. Registers only. blocks == 0 means 4 per CU.
//
// k_valu_probe is one workgroup of the same device code with a dump pointer:
// it stores every result of one unit as [round][row][256].
//
// What the hardware settled: raw v_sqrt_f64 is not exact on 4^n (every lane of
// every CU returned 2^n with bit 26 of the significand set, the same on both
// seeds), so the step is left out; the correctly rounded sqrt() of the f64
// unit, which refines v_rsq_f64, covers the f64 root. Every other exact class
// above came back exact.
//
// NOT covered: raw v_sqrt_f64, stochastic-rounding conversions and
// v_prng_b32, the transcendentals off their exact arguments, NaN payloads,
// overflow and saturation of the narrow formats, the narrowing fp6 and the bf6
// conversions, v_cvt_pk_u8_f32 and v_cvt_pknorm_i16_f32 off the one class each
// is fed, v_trig_preop_f64, DPP / SDWA modifiers on arithmetic, the scalar ALU
// and the SGPR file, the caches.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

#include "hip/part_sweep.h"

#define XS_ERR_BUF g_valu_err
#define XS_HD __host__ __device__ __forceinline__
#define XS_D __device__ __forceinline__

#pragma clang fp contract(off)

namespace {

xsprobe::ErrBuf g_valu_err;

using namespace xsprobe;

constexpr int kNumUnits = 8;
const char kUnitNames[] = "f32,f64,f16,int,bit,dot,cvt,trans";
constexpr uint32_t kAllUnits = (1u << kNumUnits) - 1;
constexpr int kBlock = kPartBlock;
constexpr int kMaxRounds = 64;

enum Kind : int {
  NONE, U32, U64, F32, F32P, PKF32, F32GE1, F32NEAR, F32INT, F32UINT, F32H, F32Q, F32B, F32N8, F32QS, F32F4, SCALE3, SCALE1,
  F64, F64P, F64NEAR, F64INT, F64GE1, PKF16, PKF16P, I5, SH4, CLS32, CLS64, PERMSEL, PKSI16, PKSIBF, SIF32, FP8, BF8,
  EXPI, POW2F32, POW2F64, POW4F32, POW4F64, SQINT, QREV, POW2F16, POW4F16, EXPIF16
};
enum Special : int {
  SP_NONE, SP_ADD32, SP_FMA32, SP_ADD64, SP_FMA64, SP_ADD16, SP_FMA16, SP_TIE32, SP_TIE64, SP_EQ, SP_CVTH, SP_CVTBF,
  SP_CVTF8, SP_CVTBF8, SP_CVTF4, SP_CVTD, SP_I2F
};

XS_HD constexpr bool is64(int k) {
  return k == U64 || k == PKF32 || k == F64 || k == F64P || k == F64NEAR || k == F64INT || k == F64GE1 || k == CLS64 ||
         k == POW2F64 || k == POW4F64;
}

// ------------------------------------------------------------------ operands
XS_HD uint32_t hashv(uint32_t seed, uint32_t u, uint32_t s, uint32_t r, uint32_t o, uint32_t t) {
  return fmix32(seed ^ (u << 28 | s << 20 | r << 12 | o << 8 | t));
}
XS_HD uint32_t edge_class(uint32_t r, uint32_t o, uint32_t t) {
  if (r != 0) return 7;
  return o == 2 ? ((t >> 6) | (t & 1u) << 2) : (t >> (3 * o)) & 7u;
}
// The significand field (`bits` wide) of a float operand.
XS_HD uint32_t sig(uint32_t h, uint32_t bits, uint32_t cls) {
  const uint32_t m = (1u << bits) - 1;
  switch (cls) {
    case 0: return m;
    case 1: return 1u << ((h & m) % bits);
    case 2: return 0;
    case 3: return 1;
    default: return h & m;
  }
}
XS_HD uint32_t word_class(uint32_t h, uint32_t cls) {
  switch (cls) {
    case 0: return 0xffffffffu;
    case 1: return 0x80000000u;
    case 2: return 0;
    case 3: return 1;
    case 4: return 0x7fffffffu;
    default: return h;
  }
}
XS_HD uint32_t f32_band(uint32_t h, uint32_t cls, uint32_t lo, uint32_t n, bool sign) {
  return (sign ? h & 0x80000000u : 0u) | (lo + ((h >> 23) & 0xffu) % n) << 23 | sig(h, 23, cls);
}
XS_HD uint64_t f64_band(uint32_t h, uint32_t hl, uint32_t cls, uint32_t lo, uint32_t n, bool sign) {
  const uint32_t hi = (sign ? h & 0x80000000u : 0u) | (lo + ((h >> 20) & 0x7ffu) % n) << 20 | (cls == 3 ? 0u : sig(h, 20, cls));
  const uint32_t low = cls == 0 ? 0xffffffffu : cls == 1 || cls == 2 ? 0u : cls == 3 ? 1u : hl;
  return static_cast<uint64_t>(hi) << 32 | low;
}
XS_HD uint32_t f16_half(uint32_t h16, uint32_t cls, bool sign) {
  return (sign ? h16 & 0x8000u : 0u) | (13u + ((h16 >> 10) & 31u) % 9u) << 10 | sig(h16, 10, cls);
}
XS_HD uint32_t f32_of_int(int32_t v) {  // |v| < 2^24: exact
  if (v == 0) return 0;
  const uint32_t s = v < 0 ? 0x80000000u : 0u, a = static_cast<uint32_t>(v < 0 ? -v : v);
  const int e = 31 - __builtin_clz(a);  // a loop here would diverge per lane
  return s | static_cast<uint32_t>(127 + e) << 23 | ((a << (23 - e)) & 0x7fffffu);
}
XS_HD uint32_t f16_of_int(int32_t v) {  // |v| < 2^11
  if (v == 0) return 0;
  const uint32_t s = v < 0 ? 0x8000u : 0u, a = static_cast<uint32_t>(v < 0 ? -v : v);
  const int e = 31 - __builtin_clz(a);
  return s | static_cast<uint32_t>(15 + e) << 10 | ((a << (10 - e)) & 0x3ffu);
}
XS_HD uint32_t class_hi(uint32_t h, uint32_t emax, uint32_t mbits) {  // the high word of a cmp_class operand
  const uint32_t m = (1u << mbits) - 1, frac = (h >> 8) & m, e = 1 + (h >> 4) % (emax - 1);
  switch (h % 10u) {
    case 0: return emax << mbits | (frac & (m >> 1)) | 1u;                    // signalling NaN
    case 1: return (h & 0x80000000u) | emax << mbits | (m >> 1) + 1 | frac;   // quiet NaN
    case 2: return 0x80000000u | emax << mbits;
    case 3: return 0x80000000u | e << mbits | frac;
    case 4: return 0x80000000u | frac | 1u;
    case 5: return 0x80000000u;
    case 6: return 0;
    case 7: return frac | 1u;
    case 8: return e << mbits | frac;
    default: return emax << mbits;
  }
}
XS_HD uint32_t fp8_byte(uint32_t b) { return (b & 0x7fu) == 0x7fu ? b & 0xf7u : b; }           // e4m3fn: no NaN
XS_HD uint32_t fp6_scale(uint64_t a) { return (125u + static_cast<uint32_t>(a >> 32) % 5u) << 23; }
XS_HD uint32_t bf8_byte(uint32_t b) { return (b & 0x7cu) == 0x7cu ? b & 0xbfu : b; }           // e5m2: no Inf / NaN

// Fixed operands of round 1. Returns false when (sp, lane) has none.
XS_HD bool special(int sp, uint32_t o, uint32_t lane, uint64_t* out) {
  const uint32_t k = lane & 15u;
  switch (sp) {
    case SP_ADD32: {
      const uint32_t v[2] = {0x00c00000u, 0x80800000u};
      if (k >= 1 || o > 1) return false;
      *out = v[o];
      return true;
    }
    case SP_FMA32: {
      const uint32_t v[2][3] = {{0x46c2c200u, 0x44284000u, 0x2b800000u}, {0x0d800000u, 0x30c00000u, 0u}};
      if (k >= 2) return false;
      *out = v[k][o];
      return true;
    }
    case SP_ADD64: {
      const uint64_t v[2] = {0x0018000000000000ull, 0x8010000000000000ull};
      if (k >= 1 || o > 1) return false;
      *out = v[o];
      return true;
    }
    case SP_FMA64: {
      const uint64_t v[3] = {0x1a70000000000000ull, 0x2518000000000000ull, 0};
      if (k >= 1) return false;
      *out = v[o];
      return true;
    }
    case SP_ADD16: {
      const uint32_t v[2] = {0x06000600u, 0x84008400u};
      if (k >= 1 || o > 1) return false;
      *out = v[o];
      return true;
    }
    case SP_FMA16: {
      const uint32_t v[3] = {0x1c001c00u, 0x1e001e00u, 0};
      if (k >= 1) return false;
      *out = v[o];
      return true;
    }
    case SP_TIE32:  // (k - 8) + 1/2
      if (k >= 16 || o) return false;
      *out = f32_of_int(2 * (static_cast<int>(k) - 8) + 1) - (1u << 23);  // an odd integer, halved
      return true;
    case SP_TIE64: {
      if (k >= 16 || o) return false;
      const uint32_t f = f32_of_int(2 * (static_cast<int>(k) - 8) + 1) - (1u << 23);  // exact widening by hand
      *out = static_cast<uint64_t>(f & 0x80000000u) << 32 | static_cast<uint64_t>(((f >> 23) & 0xffu) + 896u) << 52 |
             static_cast<uint64_t>(f & 0x7fffffu) << 29;
      return true;
    }
    case SP_EQ:  // operand 1 = operand 0 on odd lanes: the caller copies
      return false;
    case SP_CVTH:  // 1 + (2k + 1) 2^-11: halfway between two f16
      if (k >= 8 || o > 1) return false;
      *out = 0x3f800000u | (2 * k + 1) << 12;
      return true;
    case SP_CVTBF:  // 1 + (2k + 1) 2^-8
      if (k >= 8 || o > 1) return false;
      *out = 0x3f800000u | (2 * k + 1) << 15;
      return true;
    case SP_CVTF8:  // 1 + (2k + 1) 2^-4
      if (k >= 8 || o > 1) return false;
      *out = 0x3f800000u | (2 * k + 1) << 19;
      return true;
    case SP_CVTBF8:  // 1 + (2k + 1) 2^-3
      if (k >= 4 || o > 1) return false;
      *out = 0x3f800000u | (2 * k + 1) << 20;
      return true;
    case SP_CVTF4:  // 1 + (2k + 1) 2^-2
      if (k >= 2 || o > 1) return false;
      *out = 0x3f800000u | (2 * k + 1) << 21;
      return true;
    case SP_CVTD:  // 1 + (2k + 1) 2^-24: halfway between two f32
      if (k >= 8 || o) return false;
      *out = 0x3ff0000000000000ull | static_cast<uint64_t>(2 * k + 1) << 28;
      return true;
    case SP_I2F:  // 2^24 + 2k + 1: halfway between two f32
      if (k >= 8 || o) return false;
      *out = 0x01000001u + 2 * k;
      return true;
    default: return false;
  }
}

XS_HD uint64_t shaped(int kind, uint32_t seed, uint32_t u, uint32_t s, uint32_t r, uint32_t o, uint32_t t) {
  if (kind == NONE) return 0;
  const uint32_t h = hashv(seed, u, s, r, o, t), cls = edge_class(r, o, t);
  const uint32_t h2 = is64(kind) ? hashv(seed, u, s, r, o + 8, t) : 0u;
  const uint32_t n20 = h % 41u, n10 = h % 21u;
  switch (kind) {
    case U32: return word_class(h, cls);
    case U64: return static_cast<uint64_t>(word_class(h2, cls)) << 32 | word_class(h, cls);
    case F32: return f32_band(h, cls, 96, 63, true);
    case F32P: return f32_band(h, cls, 96, 63, false);
    case PKF32: return static_cast<uint64_t>(f32_band(h2, cls, 96, 63, true)) << 32 | f32_band(h, cls, 96, 63, true);
    case F32GE1: return f32_band(h, cls, 127, 11, true);
    case F32NEAR: return f32_band(h, cls, 120, 18, true);
    case F32INT: return f32_band(h, cls, 120, 38, true);
    case F32UINT: return f32_band(h, cls, 120, 38, false);
    case F32H: return f32_band(h, cls, 114, 28, true);
    case F32Q: return f32_band(h, cls, 121, 14, true);
    case F32QS: return f32_band(h, cls, 123, 10, true);
    case F32F4: return f32_band(h, cls, 126, 2, true);
    case SCALE3: return (125u + h % 5u) << 23;
    case SCALE1: return (126u + h % 3u) << 23;
    case F32B: return f32_of_int(static_cast<int32_t>(h & 0xffu));
    case F32N8: {
      const int32_t k = static_cast<int32_t>(h % 513u) - 256, n = k == 128 || k == -128 ? k + 1 : k;
      return n ? f32_of_int(n) - (8u << 23) : 0u;
    }
    case F64: return f64_band(h, h2, cls, 992, 63, true);
    case F64P: return f64_band(h, h2, cls, 992, 63, false);
    case F64NEAR: return f64_band(h, h2, cls, 1016, 18, true);
    case F64INT: return f64_band(h, h2, cls, 1016, 38, true);
    case F64GE1: return f64_band(h, h2, cls, 1023, 11, true);
    case PKF16: return f16_half(h >> 16, cls, true) << 16 | f16_half(h & 0xffffu, cls, true);
    case PKF16P: return f16_half(h >> 16, cls, false) << 16 | f16_half(h & 0xffffu, cls, false);
    case I5: return static_cast<uint32_t>(static_cast<int32_t>(h << 27) >> 27);
    case SH4: return h % 5u;
    case CLS32: return class_hi(h, 0xff, 23);
    case CLS64: return static_cast<uint64_t>(class_hi(h, 0x7ff, 20)) << 32;
    case PERMSEL: {
      uint32_t v = 0;
      for (int i = 0; i < 4; ++i) {
        const uint32_t b = ((h >> (8 * i)) & 0xffu) % 10u;
        v |= (b < 8 ? b : b + 4) << (8 * i);
      }
      return v;
    }
    case PKSI16:
      return f16_of_int(static_cast<int32_t>((h >> 16) % 31u) - 15) << 16 | f16_of_int(static_cast<int32_t>(h % 31u) - 15);
    case PKSIBF:
      return (f32_of_int(static_cast<int32_t>((h >> 16) % 31u) - 15) & 0xffff0000u) |
             f32_of_int(static_cast<int32_t>(h % 31u) - 15) >> 16;
    case SIF32: return f32_of_int(static_cast<int32_t>(h % 2047u) - 1023);
    case FP8:
      return fp8_byte(h >> 24) << 24 | fp8_byte((h >> 16) & 0xffu) << 16 | fp8_byte((h >> 8) & 0xffu) << 8 | fp8_byte(h & 0xffu);
    case BF8:
      return bf8_byte(h >> 24) << 24 | bf8_byte((h >> 16) & 0xffu) << 16 | bf8_byte((h >> 8) & 0xffu) << 8 | bf8_byte(h & 0xffu);
    case EXPI: return f32_of_int(static_cast<int32_t>(n20) - 20);
    case POW2F32: return (h & 0x80000000u) | (107u + n20) << 23;
    case POW2F64: return static_cast<uint64_t>((h & 0x80000000u) | (1003u + n20) << 20) << 32;
    case POW4F32: return (107u + 2 * n10) << 23;
    case POW4F64: return static_cast<uint64_t>((1003u + 2 * n10) << 20) << 32;
    case SQINT: return f32_of_int(static_cast<int32_t>((h & 4095u) * (h & 4095u)));
    case QREV: return (h & 7u) ? f32_of_int(static_cast<int32_t>(h & 7u)) - (2u << 23) : 0u;
    case POW2F16: return (h & 0x8000u) | (8u + (h >> 16) % 15u) << 10;
    case POW4F16: return (9u + 2 * ((h >> 16) % 7u)) << 10;
    default: return f16_of_int(static_cast<int32_t>((h >> 16) % 15u) - 7);  // EXPIF16
  }
}

XS_HD uint64_t operand(int kind, int sp, uint32_t seed, uint32_t u, uint32_t s, uint32_t r, uint32_t o, uint32_t t) {
  if (kind == NONE) return 0;
  if (r == 1 && sp != SP_NONE) {
    uint64_t v;
    if (special(sp, o, t & 63u, &v)) return v;
  }
  return shaped(kind, seed, u, s, r, o, t);
}

// ---------------------------------------------------------------- host maths
template <typename To, typename From>
To bits_as(From v) {
  static_assert(sizeof(To) == sizeof(From), "same size");
  To r;
  std::memcpy(&r, &v, sizeof r);
  return r;
}
float F(uint64_t v) { return bits_as<float>(static_cast<uint32_t>(v)); }
uint64_t FB(float v) { return bits_as<uint32_t>(v); }
double D(uint64_t v) { return bits_as<double>(v); }
uint64_t DB(double v) { return bits_as<uint64_t>(v); }
uint64_t LO(uint64_t v) { return v & 0xffffffffu; }
uint64_t HI(uint64_t v) { return v >> 32; }
uint64_t PK(uint64_t lo, uint64_t hi) { return LO(lo) | hi << 32; }
int32_t I(uint64_t v) { return static_cast<int32_t>(static_cast<uint32_t>(v)); }
int32_t SX(uint64_t v, int bits) { return static_cast<int32_t>(static_cast<uint32_t>(v) << (32 - bits)) >> (32 - bits); }

// A narrow float (`eb` exponent bits, `mb` significand bits) from a double
// that holds the exact value: round to nearest even, subnormals kept. The
// scaling is exact and nearbyint rounds once, in the default rounding mode.
uint64_t enc(double v, int eb, int mb) {
  const int bias = (1 << (eb - 1)) - 1, emin = 1 - bias;
  const uint64_t s = std::signbit(v) ? 1u : 0u;
  v = std::fabs(v);
  if (v == 0) return s << (eb + mb);
  int e;
  std::frexp(v, &e);
  e = std::max(e - 1, emin);
  const double q = std::nearbyint(std::ldexp(v, mb - e));
  return s << (eb + mb) | ((static_cast<uint64_t>(e - emin) << mb) + static_cast<uint64_t>(q));
}
double dec(uint64_t b, int eb, int mb) {
  const int bias = (1 << (eb - 1)) - 1;
  const uint64_t m = b & ((1u << mb) - 1), f = (b >> mb) & ((1u << eb) - 1);
  const double v = f ? std::ldexp(static_cast<double>(m + (1u << mb)), static_cast<int>(f) - bias - mb)
                     : std::ldexp(static_cast<double>(m), 1 - bias - mb);
  return (b >> (eb + mb)) & 1 ? -v : v;
}
double H(uint64_t v) { return dec(v & 0xffffu, 5, 10); }
double HH(uint64_t v) { return dec((v >> 16) & 0xffffu, 5, 10); }
uint64_t HB(double v) { return enc(v, 5, 10); }
double BF(uint64_t v) { return F((v & 0xffffu) << 16); }
uint64_t BFB(double v) { return enc(v, 8, 7); }
uint64_t PKH(double lo, double hi) { return HB(lo) | HB(hi) << 16; }
double Q8(uint64_t v, int byte) { return dec((v >> (8 * byte)) & 0xffu, 4, 3); }
double B8(uint64_t v, int byte) { return dec((v >> (8 * byte)) & 0xffu, 5, 2); }
float med3(float a, float b, float c) { return std::fmax(std::fmin(a, b), std::fmin(std::fmax(a, b), c)); }
uint64_t fclass(uint64_t hi, uint32_t emax, int mbits, bool low_nonzero) {
  const uint32_t h = static_cast<uint32_t>(hi), e = (h >> mbits) & emax, m = h & ((1u << mbits) - 1);
  const bool neg = h >> 31, frac = m || low_nonzero;
  if (e == emax && frac) return (m >> (mbits - 1)) & 1 ? 1 : 0;
  if (e == emax) return neg ? 2 : 9;
  if (e) return neg ? 3 : 8;
  if (frac) return neg ? 4 : 7;
  return neg ? 5 : 6;
}
uint64_t perm(uint64_t s0, uint64_t s1, uint64_t sel) {
  const uint64_t both = LO(s1) | LO(s0) << 32;
  uint64_t r = 0;
  for (int i = 0; i < 4; ++i) {
    const uint32_t c = (sel >> (8 * i)) & 0xffu;
    r |= (c < 8 ? (both >> (8 * c)) & 0xffu : c == 12 ? 0u : 0xffu) << (8 * i);
  }
  return r;
}
uint64_t bitop3(uint64_t a, uint64_t b, uint64_t c, uint32_t tt) {
  uint64_t r = 0;
  for (int i = 0; i < 32; ++i) {
    const uint64_t idx = ((a >> i) & 1) << 2 | ((b >> i) & 1) << 1 | ((c >> i) & 1);
    r |= static_cast<uint64_t>((tt >> idx) & 1u) << i;
  }
  return r;
}
uint64_t bfe_i(uint64_t a, uint32_t off, uint32_t w) {
  if (!w) return 0;
  if (off + w >= 32) return LO(static_cast<uint32_t>(I(a) >> off));
  return LO(static_cast<uint32_t>(static_cast<int32_t>(static_cast<uint32_t>(a) << (32 - off - w)) >> (32 - w)));
}
uint64_t bfe_u(uint64_t a, uint32_t off, uint32_t w) { return w ? (LO(a) >> off) & ((1ull << w) - 1) : 0; }
uint64_t ffbh_i(uint64_t a) {
  const uint32_t v = static_cast<uint32_t>(a), x = v ^ static_cast<uint32_t>(I(a) >> 31);
  return x ? static_cast<uint32_t>(__builtin_clz(x)) : 0xffffffffu;
}
int64_t dot4(uint64_t a, uint64_t b, bool sgn) {
  int64_t r = 0;
  for (int i = 0; i < 4; ++i)
    r += sgn ? static_cast<int64_t>(SX(a >> (8 * i), 8)) * SX(b >> (8 * i), 8)
             : static_cast<int64_t>((a >> (8 * i)) & 0xff) * ((b >> (8 * i)) & 0xff);
  return r;
}
int64_t dot8(uint64_t a, uint64_t b, bool sgn) {
  int64_t r = 0;
  for (int i = 0; i < 8; ++i)
    r += sgn ? static_cast<int64_t>(SX(a >> (4 * i), 4)) * SX(b >> (4 * i), 4)
             : static_cast<int64_t>((a >> (4 * i)) & 0xf) * ((b >> (4 * i)) & 0xf);
  return r;
}
uint64_t sad(uint64_t a, uint64_t b, uint64_t c) {
  uint64_t r = c;
  for (int i = 0; i < 4; ++i) {
    const int x = static_cast<int>((a >> (8 * i)) & 0xff), y = static_cast<int>((b >> (8 * i)) & 0xff);
    r += static_cast<uint64_t>(std::abs(x - y));
  }
  return LO(r);
}
uint64_t msad(uint64_t a, uint64_t b, uint64_t c) {  // a byte of the reference b that is 0 masks its difference
  uint64_t r = c;
  for (int i = 0; i < 4; ++i) {
    const int x = static_cast<int>((a >> (8 * i)) & 0xff), y = static_cast<int>((b >> (8 * i)) & 0xff);
    if (y) r += static_cast<uint64_t>(std::abs(x - y));
  }
  return LO(r);
}
uint64_t pk16(uint64_t a, uint64_t b, uint64_t c, int op) {
  uint64_t r = 0;
  for (int i = 0; i < 2; ++i) {
    const uint32_t x = (a >> (16 * i)) & 0xffffu, y = (b >> (16 * i)) & 0xffffu, z = (c >> (16 * i)) & 0xffffu;
    uint32_t v = 0;
    switch (op) {
      case 0: v = x + y; break;
      case 1: v = x * y + z; break;  // low 16 bits: signedness does not matter
      case 2: v = x * y; break;
      case 3: v = static_cast<uint32_t>(std::min(SX(x, 16), SX(y, 16))); break;
      case 4: v = std::max(x, y); break;
      case 5: v = y << (x & 15u); break;
      default: v = static_cast<uint32_t>(SX(y, 16) >> (x & 15u)); break;
    }
    r |= static_cast<uint64_t>(v & 0xffffu) << (16 * i);
  }
  return r;
}
uint64_t sat_i(int64_t v, int64_t lo, int64_t hi) { return static_cast<uint64_t>(std::min(std::max(v, lo), hi)); }
unsigned __int128 wide(uint64_t lo, uint64_t hi) { return static_cast<unsigned __int128>(hi) << 64 | lo; }
uint64_t snorm16(float v) { return static_cast<uint64_t>(static_cast<int64_t>(std::nearbyint(v * 32767.0))) & 0xffffu; }
uint64_t fp6_fold(uint64_t a, uint64_t b, uint64_t c) {
  const uint64_t w[3] = {a, b, c};
  const double scale = F(fp6_scale(a));
  uint32_t sum = 0, x = 0;
  for (uint32_t i = 0; i < 32; ++i) {
    const uint32_t at = 6 * i, off = at % 64;
    uint64_t e = w[at / 64] >> off;
    if (off > 58) e |= w[at / 64 + 1] << (64 - off);
    const uint32_t r = static_cast<uint32_t>(FB(static_cast<float>(dec(e & 63u, 2, 3) * scale)));
    sum += r * (2 * i + 1);
    x ^= r;
  }
  return static_cast<uint64_t>(x) << 32 | sum;
}
uint64_t cvt_u8(double v) { return static_cast<uint64_t>(std::nearbyint(v)) & 0xffu; }

// --------------------------------------------------------------- device code
// One instruction on VGPR operands; the s_nop covers what the assembler does
// not see inside inline asm (a transcendental's or an SDWA result read next).
#define A(text) asm volatile(text "\n\ts_nop 1" : "=&v"(v) : "v"(a), "v"(b), "v"(cc) : "vcc")
#define CMP(text) A(text "\n\tv_cndmask_b32_e64 %0, 0, 1, vcc")
// A transcendental's result needs a wait state before a plain VALU reads it.
#define LOW16(text) A(text "\n\ts_nop 1\n\tv_and_b32_e32 %0, 0xffff, %0")
#define LOW8(text) A(text "\n\ts_nop 1\n\tv_and_b32_e32 %0, 0xff, %0")
#define FBITS(x) __builtin_bit_cast(uint32_t, static_cast<float>(x))
#define FVAL(x) __builtin_bit_cast(float, static_cast<uint32_t>(x))
#define DBITS(x) __builtin_bit_cast(uint64_t, static_cast<double>(x))
#define DVAL(x) __builtin_bit_cast(double, static_cast<uint64_t>(x))
#define WIDE_ADD(op0, opc)                                                                                            \
  {                                                                                                                   \
    uint32_t w0, w1, w2, w3;                                                                                          \
    asm volatile(op0 " %0, vcc, %4, %6\n\t" opc " %1, vcc, %5, %7, vcc\n\t" opc " %2, vcc, %8, %6, vcc\n\t" opc        \
                     " %3, vcc, %9, %7, vcc"                                                                          \
                 : "=&v"(w0), "=&v"(w1), "=&v"(w2), "=&v"(w3)                                                          \
                 : "v"(static_cast<uint32_t>(a)), "v"(static_cast<uint32_t>(a >> 32)), "v"(static_cast<uint32_t>(b)),  \
                   "v"(static_cast<uint32_t>(b >> 32)), "v"(static_cast<uint32_t>(cc)),                                \
                   "v"(static_cast<uint32_t>(cc >> 32))                                                                \
                 : "vcc");                                                                                            \
    v = static_cast<uint64_t>(w3) << 32 | w2;                                                                         \
  }

// The 32 results of v_cvt_scalef32_pk32_f32_fp6, folded to two words (the header's rule).
XS_D uint64_t fp6_unpack_fold(uint64_t a, uint64_t b, uint64_t c) {
  typedef uint32_t u32x6 __attribute__((ext_vector_type(6)));
  typedef float f32x32 __attribute__((ext_vector_type(32)));
  const u32x6 src = {static_cast<uint32_t>(a), static_cast<uint32_t>(a >> 32), static_cast<uint32_t>(b),
                     static_cast<uint32_t>(b >> 32), static_cast<uint32_t>(c), static_cast<uint32_t>(c >> 32)};
  const f32x32 r = __builtin_amdgcn_cvt_scalef32_pk32_f32_fp6(src, FVAL(fp6_scale(a)));
  uint32_t sum = 0, x = 0;
#pragma unroll
  for (uint32_t i = 0; i < 32; ++i) {
    sum += FBITS(r[i]) * (2 * i + 1);
    x ^= FBITS(r[i]);
  }
  return static_cast<uint64_t>(x) << 32 | sum;
}

// X(unit, id, name, result words, kind a, kind b, kind c, special, device code, host value)
// The device code reads a, b, cc and writes v; the host value is an
// expression in a, b, c (uint64_t), word 0 in its low half.
#define VALU_STEPS(X)                                                                                                  \
  /* ---- f32 */                                                                                                       \
  X(0, add_f32, "v_add_f32", 1, F32, F32, NONE, SP_ADD32, A("v_add_f32_e32 %0, %1, %2"), FB(F(a) + F(b)))              \
  X(0, sub_f32, "v_sub_f32", 1, F32, F32, NONE, SP_NONE, A("v_sub_f32_e32 %0, %1, %2"), FB(F(a) - F(b)))               \
  X(0, mul_f32, "v_mul_f32", 1, F32, F32, NONE, SP_NONE, A("v_mul_f32_e32 %0, %1, %2"), FB(F(a) * F(b)))               \
  X(0, fma_f32, "v_fma_f32", 1, F32, F32, F32, SP_FMA32, A("v_fma_f32 %0, %1, %2, %3"), FB(std::fmaf(F(a), F(b), F(c)))) \
  X(0, pk_add_f32, "v_pk_add_f32", 2, PKF32, PKF32, NONE, SP_NONE, A("v_pk_add_f32 %0, %1, %2"),                       \
    PK(FB(F(LO(a)) + F(LO(b))), FB(F(HI(a)) + F(HI(b)))))                                                              \
  X(0, pk_mul_f32, "v_pk_mul_f32", 2, PKF32, PKF32, NONE, SP_NONE, A("v_pk_mul_f32 %0, %1, %2"),                       \
    PK(FB(F(LO(a)) * F(LO(b))), FB(F(HI(a)) * F(HI(b)))))                                                              \
  X(0, pk_fma_f32, "v_pk_fma_f32", 2, PKF32, PKF32, PKF32, SP_NONE, A("v_pk_fma_f32 %0, %1, %2, %3"),                  \
    PK(FB(std::fmaf(F(LO(a)), F(LO(b)), F(LO(c)))), FB(std::fmaf(F(HI(a)), F(HI(b)), F(HI(c))))))                      \
  X(0, min_f32, "v_min_f32", 1, F32, F32, NONE, SP_NONE, A("v_min_f32_e32 %0, %1, %2"), FB(std::fmin(F(a), F(b))))     \
  X(0, max_f32, "v_max_f32", 1, F32, F32, NONE, SP_NONE, A("v_max_f32_e32 %0, %1, %2"), FB(std::fmax(F(a), F(b))))     \
  X(0, med3_f32, "v_med3_f32", 1, F32, F32, F32, SP_NONE, A("v_med3_f32 %0, %1, %2, %3"), FB(med3(F(a), F(b), F(c))))  \
  X(0, min3_f32, "v_min3_f32", 1, F32, F32, F32, SP_NONE, A("v_min3_f32 %0, %1, %2, %3"),                              \
    FB(std::fmin(std::fmin(F(a), F(b)), F(c))))                                                                        \
  X(0, max3_f32, "v_max3_f32", 1, F32, F32, F32, SP_NONE, A("v_max3_f32 %0, %1, %2, %3"),                              \
    FB(std::fmax(std::fmax(F(a), F(b)), F(c))))                                                                        \
  X(0, minimum3_f32, "v_minimum3_f32", 1, F32, F32, F32, SP_NONE, A("v_minimum3_f32 %0, %1, %2, %3"),                  \
    FB(std::fmin(std::fmin(F(a), F(b)), F(c))))                                                                        \
  X(0, maximum3_f32, "v_maximum3_f32", 1, F32, F32, F32, SP_NONE, A("v_maximum3_f32 %0, %1, %2, %3"),                  \
    FB(std::fmax(std::fmax(F(a), F(b)), F(c))))                                                                        \
  X(0, ldexp_f32, "v_ldexp_f32", 1, F32, I5, NONE, SP_NONE, A("v_ldexp_f32 %0, %1, %2"), FB(std::ldexp(F(a), I(b))))   \
  X(0, frexp_mant_f32, "v_frexp_mant_f32", 1, F32, NONE, NONE, SP_NONE, A("v_frexp_mant_f32_e32 %0, %1"),              \
    FB(std::frexp(F(a), &tmp)))                                                                                        \
  X(0, frexp_exp_i32_f32, "v_frexp_exp_i32_f32", 1, F32, NONE, NONE, SP_NONE, A("v_frexp_exp_i32_f32_e32 %0, %1"),     \
    (std::frexp(F(a), &tmp), LO(static_cast<uint32_t>(tmp))))                                                          \
  X(0, fract_f32, "v_fract_f32", 1, F32GE1, NONE, NONE, SP_NONE, A("v_fract_f32_e32 %0, %1"),                          \
    FB(F(a) - std::floor(F(a))))                                                                                       \
  X(0, trunc_f32, "v_trunc_f32", 1, F32NEAR, NONE, NONE, SP_TIE32, A("v_trunc_f32_e32 %0, %1"), FB(std::trunc(F(a))))  \
  X(0, rndne_f32, "v_rndne_f32", 1, F32NEAR, NONE, NONE, SP_TIE32, A("v_rndne_f32_e32 %0, %1"),                        \
    FB(std::nearbyint(F(a))))                                                                                          \
  X(0, floor_f32, "v_floor_f32", 1, F32NEAR, NONE, NONE, SP_TIE32, A("v_floor_f32_e32 %0, %1"), FB(std::floor(F(a))))  \
  X(0, ceil_f32, "v_ceil_f32", 1, F32NEAR, NONE, NONE, SP_TIE32, A("v_ceil_f32_e32 %0, %1"), FB(std::ceil(F(a))))      \
  X(0, cmp_lt_f32, "v_cmp_lt_f32", 1, F32, F32, NONE, SP_EQ, CMP("v_cmp_lt_f32_e32 vcc, %1, %2"), F(a) < F(b))         \
  X(0, cmp_eq_f32, "v_cmp_eq_f32", 1, F32, F32, NONE, SP_EQ, CMP("v_cmp_eq_f32_e32 vcc, %1, %2"), F(a) == F(b))        \
  X(0, cmp_le_f32, "v_cmp_le_f32", 1, F32, F32, NONE, SP_EQ, CMP("v_cmp_le_f32_e32 vcc, %1, %2"), F(a) <= F(b))        \
  X(0, cmp_gt_f32, "v_cmp_gt_f32", 1, F32, F32, NONE, SP_EQ, CMP("v_cmp_gt_f32_e32 vcc, %1, %2"), F(a) > F(b))         \
  X(0, cmp_lg_f32, "v_cmp_lg_f32", 1, F32, F32, NONE, SP_EQ, CMP("v_cmp_lg_f32_e32 vcc, %1, %2"), F(a) != F(b))        \
  X(0, cmp_ge_f32, "v_cmp_ge_f32", 1, F32, F32, NONE, SP_EQ, CMP("v_cmp_ge_f32_e32 vcc, %1, %2"), F(a) >= F(b))        \
  X(0, cmp_class_f32, "v_cmp_class_f32", 1, CLS32, U32, NONE, SP_NONE, CMP("v_cmp_class_f32_e32 vcc, %1, %2"),         \
    (b >> fclass(a, 0xff, 23, false)) & 1)                                                                             \
  X(0, div_f32, "div_f32", 1, F32, F32, NONE, SP_NONE, v = FBITS(FVAL(a) / FVAL(b)), FB(F(a) / F(b)))                  \
  X(0, sqrt_f32, "sqrt_f32", 1, F32P, NONE, NONE, SP_NONE, v = FBITS(__builtin_sqrtf(FVAL(a))), FB(std::sqrt(F(a))))   \
  /* ---- f64 */                                                                                                       \
  X(1, add_f64, "v_add_f64", 2, F64, F64, NONE, SP_ADD64, A("v_add_f64 %0, %1, %2"), DB(D(a) + D(b)))                  \
  X(1, mul_f64, "v_mul_f64", 2, F64, F64, NONE, SP_NONE, A("v_mul_f64 %0, %1, %2"), DB(D(a) * D(b)))                   \
  X(1, fma_f64, "v_fma_f64", 2, F64, F64, F64, SP_FMA64, A("v_fma_f64 %0, %1, %2, %3"), DB(std::fma(D(a), D(b), D(c)))) \
  X(1, min_f64, "v_min_f64", 2, F64, F64, NONE, SP_NONE, A("v_min_f64 %0, %1, %2"), DB(std::fmin(D(a), D(b))))         \
  X(1, max_f64, "v_max_f64", 2, F64, F64, NONE, SP_NONE, A("v_max_f64 %0, %1, %2"), DB(std::fmax(D(a), D(b))))         \
  X(1, ldexp_f64, "v_ldexp_f64", 2, F64, I5, NONE, SP_NONE, A("v_ldexp_f64 %0, %1, %2"), DB(std::ldexp(D(a), I(b))))   \
  X(1, frexp_mant_f64, "v_frexp_mant_f64", 2, F64, NONE, NONE, SP_NONE, A("v_frexp_mant_f64_e32 %0, %1"),              \
    DB(std::frexp(D(a), &tmp)))                                                                                        \
  X(1, frexp_exp_i32_f64, "v_frexp_exp_i32_f64", 1, F64, NONE, NONE, SP_NONE, A("v_frexp_exp_i32_f64_e32 %0, %1"),     \
    (std::frexp(D(a), &tmp), LO(static_cast<uint32_t>(tmp))))                                                          \
  X(1, fract_f64, "v_fract_f64", 2, F64GE1,  NONE, NONE, SP_NONE, A("v_fract_f64_e32 %0, %1"),                         \
    DB(D(a) - std::floor(D(a))))                                                                                       \
  X(1, trunc_f64, "v_trunc_f64", 2, F64NEAR, NONE, NONE, SP_TIE64, A("v_trunc_f64_e32 %0, %1"), DB(std::trunc(D(a))))  \
  X(1, rndne_f64, "v_rndne_f64", 2, F64NEAR, NONE, NONE, SP_TIE64, A("v_rndne_f64_e32 %0, %1"),                        \
    DB(std::nearbyint(D(a))))                                                                                          \
  X(1, floor_f64, "v_floor_f64", 2, F64NEAR, NONE, NONE, SP_TIE64, A("v_floor_f64_e32 %0, %1"), DB(std::floor(D(a))))  \
  X(1, ceil_f64, "v_ceil_f64", 2, F64NEAR, NONE, NONE, SP_TIE64, A("v_ceil_f64_e32 %0, %1"), DB(std::ceil(D(a))))      \
  X(1, cmp_lt_f64, "v_cmp_lt_f64", 1, F64, F64, NONE, SP_EQ, CMP("v_cmp_lt_f64_e32 vcc, %1, %2"), D(a) < D(b))         \
  X(1, cmp_eq_f64, "v_cmp_eq_f64", 1, F64, F64, NONE, SP_EQ, CMP("v_cmp_eq_f64_e32 vcc, %1, %2"), D(a) == D(b))        \
  X(1, cmp_class_f64, "v_cmp_class_f64", 1, CLS64, U32, NONE, SP_NONE, CMP("v_cmp_class_f64_e32 vcc, %1, %2"),         \
    (b >> fclass(HI(a), 0x7ff, 20, LO(a) != 0)) & 1)                                                                   \
  X(1, div_f64, "div_f64", 2, F64, F64, NONE, SP_NONE, v = DBITS(DVAL(a) / DVAL(b)), DB(D(a) / D(b)))                  \
  X(1, sqrt_f64, "sqrt_f64", 2, F64P, NONE, NONE, SP_NONE, v = DBITS(__builtin_sqrt(DVAL(a))), DB(std::sqrt(D(a))))    \
  /* ---- f16 */                                                                                                       \
  X(2, add_f16, "v_add_f16", 1, PKF16, PKF16, NONE, SP_ADD16, LOW16("v_add_f16_e32 %0, %1, %2"), HB(H(a) + H(b)))      \
  X(2, mul_f16, "v_mul_f16", 1, PKF16, PKF16, NONE, SP_NONE, LOW16("v_mul_f16_e32 %0, %1, %2"), HB(H(a) * H(b)))       \
  X(2, fma_f16, "v_fma_f16", 1, PKF16, PKF16, PKF16, SP_FMA16, LOW16("v_fma_f16 %0, %1, %2, %3"),                      \
    HB(std::fma(H(a), H(b), H(c))))                                                                                    \
  X(2, pk_add_f16, "v_pk_add_f16", 1, PKF16, PKF16, NONE, SP_ADD16, A("v_pk_add_f16 %0, %1, %2"),                      \
    PKH(H(a) + H(b), HH(a) + HH(b)))                                                                                   \
  X(2, pk_mul_f16, "v_pk_mul_f16", 1, PKF16, PKF16, NONE, SP_NONE, A("v_pk_mul_f16 %0, %1, %2"),                       \
    PKH(H(a) * H(b), HH(a) * HH(b)))                                                                                   \
  X(2, pk_fma_f16, "v_pk_fma_f16", 1, PKF16, PKF16, PKF16, SP_FMA16, A("v_pk_fma_f16 %0, %1, %2, %3"),                 \
    PKH(std::fma(H(a), H(b), H(c)), std::fma(HH(a), HH(b), HH(c))))                                                    \
  X(2, pk_min_f16, "v_pk_min_f16", 1, PKF16, PKF16, NONE, SP_NONE, A("v_pk_min_f16 %0, %1, %2"),                       \
    PKH(std::fmin(H(a), H(b)), std::fmin(HH(a), HH(b))))                                                               \
  X(2, pk_max_f16, "v_pk_max_f16", 1, PKF16, PKF16, NONE, SP_NONE, A("v_pk_max_f16 %0, %1, %2"),                       \
    PKH(std::fmax(H(a), H(b)), std::fmax(HH(a), HH(b))))                                                               \
  X(2, pk_minimum3_f16, "v_pk_minimum3_f16", 1, PKF16, PKF16, PKF16, SP_NONE, A("v_pk_minimum3_f16 %0, %1, %2, %3"),   \
    PKH(std::fmin(std::fmin(H(a), H(b)), H(c)), std::fmin(std::fmin(HH(a), HH(b)), HH(c))))                            \
  X(2, pk_maximum3_f16, "v_pk_maximum3_f16", 1, PKF16, PKF16, PKF16, SP_NONE, A("v_pk_maximum3_f16 %0, %1, %2, %3"),   \
    PKH(std::fmax(std::fmax(H(a), H(b)), H(c)), std::fmax(std::fmax(HH(a), HH(b)), HH(c))))                            \
  X(2, fma_mix_f32, "v_fma_mix_f32", 1, PKF16, PKF16, F32, SP_NONE,                                                    \
    A("v_fma_mix_f32 %0, %1, %2, %3 op_sel:[0,1,0] op_sel_hi:[1,1,0]"),                                                \
    FB(std::fmaf(static_cast<float>(H(a)), static_cast<float>(HH(b)), F(c))))                                          \
  X(2, fma_mixlo_f16, "v_fma_mixlo_f16", 1, PKF16, PKF16, PKF16, SP_NONE,                                              \
    A("v_mov_b32_e32 %0, 0\n\tv_fma_mixlo_f16 %0, %1, %2, %3 op_sel:[1,0,0] op_sel_hi:[1,1,1]"),                        \
    HB(std::fmaf(static_cast<float>(HH(a)), static_cast<float>(H(b)), static_cast<float>(H(c)))))                      \
  /* ---- int */                                                                                                       \
  X(3, mul_lo_u32, "v_mul_lo_u32", 1, U32, U32, NONE, SP_NONE, A("v_mul_lo_u32 %0, %1, %2"), LO(a * b))                \
  X(3, mul_hi_u32, "v_mul_hi_u32", 1, U32, U32, NONE, SP_NONE, A("v_mul_hi_u32 %0, %1, %2"), HI(a * b))                \
  X(3, mul_hi_i32, "v_mul_hi_i32", 1, U32, U32, NONE, SP_NONE, A("v_mul_hi_i32 %0, %1, %2"),                           \
    HI(static_cast<uint64_t>(static_cast<int64_t>(I(a)) * I(b))))                                                      \
  X(3, mad_u64_u32, "v_mad_u64_u32", 2, U32, U32, U64, SP_NONE, A("v_mad_u64_u32 %0, vcc, %1, %2, %3"), a * b + c)     \
  X(3, mad_i64_i32, "v_mad_i64_i32", 2, U32, U32, U64, SP_NONE, A("v_mad_i64_i32 %0, vcc, %1, %2, %3"),                \
    static_cast<uint64_t>(static_cast<int64_t>(I(a)) * I(b)) + c)                                                      \
  X(3, mul_u32_u24, "v_mul_u32_u24", 1, U32, U32, NONE, SP_NONE, A("v_mul_u32_u24_e32 %0, %1, %2"),                    \
    LO((a & 0xffffff) * (b & 0xffffff)))                                                                               \
  X(3, mul_hi_u32_u24, "v_mul_hi_u32_u24", 1, U32, U32, NONE, SP_NONE, A("v_mul_hi_u32_u24_e32 %0, %1, %2"),           \
    HI((a & 0xffffff) * (b & 0xffffff)))                                                                               \
  X(3, mad_u32_u24, "v_mad_u32_u24", 1, U32, U32, U32, SP_NONE, A("v_mad_u32_u24 %0, %1, %2, %3"),                     \
    LO((a & 0xffffff) * (b & 0xffffff) + c))                                                                           \
  X(3, mad_i32_i24, "v_mad_i32_i24", 1, U32, U32, U32, SP_NONE, A("v_mad_i32_i24 %0, %1, %2, %3"),                     \
    LO(static_cast<uint64_t>(static_cast<int64_t>(SX(a, 24)) * SX(b, 24)) + c))                                        \
  X(3, mad_u32_u16, "v_mad_u32_u16", 1, U32, U32, U32, SP_NONE, A("v_mad_u32_u16 %0, %1, %2, %3"),                     \
    LO((a & 0xffff) * (b & 0xffff) + c))                                                                               \
  X(3, pk_add_u16, "v_pk_add_u16", 1, U32, U32, NONE, SP_NONE, A("v_pk_add_u16 %0, %1, %2"), pk16(a, b, c, 0))         \
  X(3, pk_mad_i16, "v_pk_mad_i16", 1, U32, U32, U32, SP_NONE, A("v_pk_mad_i16 %0, %1, %2, %3"), pk16(a, b, c, 1))      \
  X(3, pk_mul_lo_u16, "v_pk_mul_lo_u16", 1, U32, U32, NONE, SP_NONE, A("v_pk_mul_lo_u16 %0, %1, %2"), pk16(a, b, c, 2)) \
  X(3, pk_min_i16, "v_pk_min_i16", 1, U32, U32, NONE, SP_NONE, A("v_pk_min_i16 %0, %1, %2"), pk16(a, b, c, 3))         \
  X(3, pk_max_u16, "v_pk_max_u16", 1, U32, U32, NONE, SP_NONE, A("v_pk_max_u16 %0, %1, %2"), pk16(a, b, c, 4))         \
  X(3, pk_lshlrev_b16, "v_pk_lshlrev_b16", 1, U32, U32, NONE, SP_NONE, A("v_pk_lshlrev_b16 %0, %1, %2"),               \
    pk16(a, b, c, 5))                                                                                                  \
  X(3, pk_ashrrev_i16, "v_pk_ashrrev_i16", 1, U32, U32, NONE, SP_NONE, A("v_pk_ashrrev_i16 %0, %1, %2"),               \
    pk16(a, b, c, 6))                                                                                                  \
  X(3, add128, "add128", 2, U64, U64, U64, SP_NONE, WIDE_ADD("v_add_co_u32_e32", "v_addc_co_u32_e32"),                 \
    static_cast<uint64_t>((wide(a, c) + wide(b, b)) >> 64))                                                            \
  X(3, sub128, "sub128", 2, U64, U64, U64, SP_NONE, WIDE_ADD("v_sub_co_u32_e32", "v_subb_co_u32_e32"),                 \
    static_cast<uint64_t>((wide(a, c) - wide(b, b)) >> 64))                                                            \
  X(3, add3_u32, "v_add3_u32", 1, U32, U32, U32, SP_NONE, A("v_add3_u32 %0, %1, %2, %3"), LO(a + b + c))               \
  X(3, lshl_add_u32, "v_lshl_add_u32", 1, U32, U32, U32, SP_NONE, A("v_lshl_add_u32 %0, %1, %2, %3"),                  \
    LO((a << (b & 31)) + c))                                                                                           \
  X(3, xad_u32, "v_xad_u32", 1, U32, U32, U32, SP_NONE, A("v_xad_u32 %0, %1, %2, %3"), LO((a ^ b) + c))                \
  X(3, lshl_add_u64, "v_lshl_add_u64", 2, U64, SH4, U64, SP_NONE, A("v_lshl_add_u64 %0, %1, %2, %3"), (a << b) + c)    \
  X(3, lshlrev_b64, "v_lshlrev_b64", 2, U32, U64, NONE, SP_NONE, A("v_lshlrev_b64 %0, %1, %2"), b << (a & 63))         \
  X(3, lshrrev_b64, "v_lshrrev_b64", 2, U32, U64, NONE, SP_NONE, A("v_lshrrev_b64 %0, %1, %2"), b >> (a & 63))         \
  X(3, ashrrev_i64, "v_ashrrev_i64", 2, U32, U64, NONE, SP_NONE, A("v_ashrrev_i64 %0, %1, %2"),                        \
    static_cast<uint64_t>(static_cast<int64_t>(b) >> (a & 63)))                                                        \
  X(3, sad_u8, "v_sad_u8", 1, U32, U32, U32, SP_NONE, A("v_sad_u8 %0, %1, %2, %3"), sad(a, b, c))                      \
  X(3, msad_u8, "v_msad_u8", 1, U32, U32, U32, SP_NONE, A("v_msad_u8 %0, %1, %2, %3"), msad(a, b, c))                 \
  X(3, cmp_lt_u64, "v_cmp_lt_u64", 1, U64, U64, NONE, SP_EQ, CMP("v_cmp_lt_u64_e32 vcc, %1, %2"), a < b)               \
  X(3, cmp_ge_i32, "v_cmp_ge_i32", 1, U32, U32, NONE, SP_EQ, CMP("v_cmp_ge_i32_e32 vcc, %1, %2"), I(a) >= I(b))        \
  /* ---- bit */                                                                                                       \
  X(4, perm_b32, "v_perm_b32", 1, U32, U32, PERMSEL, SP_NONE, A("v_perm_b32 %0, %1, %2, %3"), perm(a, b, c))           \
  X(4, alignbit_b32, "v_alignbit_b32", 1, U32, U32, U32, SP_NONE, A("v_alignbit_b32 %0, %1, %2, %3"),                  \
    LO((a << 32 | b) >> (c & 31)))                                                                                     \
  X(4, alignbyte_b32, "v_alignbyte_b32", 1, U32, U32, U32, SP_NONE, A("v_alignbyte_b32 %0, %1, %2, %3"),               \
    LO((a << 32 | b) >> (8 * (c & 3))))                                                                                \
  X(4, bfe_u32, "v_bfe_u32", 1, U32, U32, U32, SP_NONE, A("v_bfe_u32 %0, %1, %2, %3"), bfe_u(a, b & 31, c & 31))       \
  X(4, bfe_i32, "v_bfe_i32", 1, U32, U32, U32, SP_NONE, A("v_bfe_i32 %0, %1, %2, %3"), bfe_i(a, b & 31, c & 31))       \
  X(4, bfi_b32, "v_bfi_b32", 1, U32, U32, U32, SP_NONE, A("v_bfi_b32 %0, %1, %2, %3"), (a & b) | (~a & c & 0xffffffffu)) \
  X(4, bitop3_b32_96, "v_bitop3_b32:0x96", 1, U32, U32, U32, SP_NONE, A("v_bitop3_b32 %0, %1, %2, %3 bitop3:0x96"),    \
    bitop3(a, b, c, 0x96))                                                                                             \
  X(4, bitop3_b32_e8, "v_bitop3_b32:0xe8", 1, U32, U32, U32, SP_NONE, A("v_bitop3_b32 %0, %1, %2, %3 bitop3:0xe8"),    \
    bitop3(a, b, c, 0xe8))                                                                                             \
  X(4, bitop3_b32_f0, "v_bitop3_b32:0xf0", 1, U32, U32, U32, SP_NONE, A("v_bitop3_b32 %0, %1, %2, %3 bitop3:0xf0"),    \
    bitop3(a, b, c, 0xf0))                                                                                             \
  X(4, bitop3_b32_cc, "v_bitop3_b32:0xcc", 1, U32, U32, U32, SP_NONE, A("v_bitop3_b32 %0, %1, %2, %3 bitop3:0xcc"),    \
    bitop3(a, b, c, 0xcc))                                                                                             \
  X(4, bitop3_b32_aa, "v_bitop3_b32:0xaa", 1, U32, U32, U32, SP_NONE, A("v_bitop3_b32 %0, %1, %2, %3 bitop3:0xaa"),    \
    bitop3(a, b, c, 0xaa))                                                                                             \
  X(4, bitop3_b32_1b, "v_bitop3_b32:0x1b", 1, U32, U32, U32, SP_NONE, A("v_bitop3_b32 %0, %1, %2, %3 bitop3:0x1b"),    \
    bitop3(a, b, c, 0x1b))                                                                                             \
  X(4, bitop3_b32_2d, "v_bitop3_b32:0x2d", 1, U32, U32, U32, SP_NONE, A("v_bitop3_b32 %0, %1, %2, %3 bitop3:0x2d"),    \
    bitop3(a, b, c, 0x2d))                                                                                             \
  X(4, bitop3_b32_ca, "v_bitop3_b32:0xca", 1, U32, U32, U32, SP_NONE, A("v_bitop3_b32 %0, %1, %2, %3 bitop3:0xca"),    \
    bitop3(a, b, c, 0xca))                                                                                             \
  X(4, bitop3_b16_96, "v_bitop3_b16:0x96", 1, U32, U32, U32, SP_NONE, LOW16("v_bitop3_b16 %0, %1, %2, %3 bitop3:0x96"), \
    bitop3(a, b, c, 0x96) & 0xffff)                                                                                    \
  X(4, bitop3_b16_e8, "v_bitop3_b16:0xe8", 1, U32, U32, U32, SP_NONE, LOW16("v_bitop3_b16 %0, %1, %2, %3 bitop3:0xe8"), \
    bitop3(a, b, c, 0xe8) & 0xffff)                                                                                    \
  X(4, bitop3_b16_f0, "v_bitop3_b16:0xf0", 1, U32, U32, U32, SP_NONE, LOW16("v_bitop3_b16 %0, %1, %2, %3 bitop3:0xf0"), \
    bitop3(a, b, c, 0xf0) & 0xffff)                                                                                    \
  X(4, bitop3_b16_cc, "v_bitop3_b16:0xcc", 1, U32, U32, U32, SP_NONE, LOW16("v_bitop3_b16 %0, %1, %2, %3 bitop3:0xcc"), \
    bitop3(a, b, c, 0xcc) & 0xffff)                                                                                    \
  X(4, bitop3_b16_aa, "v_bitop3_b16:0xaa", 1, U32, U32, U32, SP_NONE, LOW16("v_bitop3_b16 %0, %1, %2, %3 bitop3:0xaa"), \
    bitop3(a, b, c, 0xaa) & 0xffff)                                                                                    \
  X(4, bitop3_b16_1b, "v_bitop3_b16:0x1b", 1, U32, U32, U32, SP_NONE, LOW16("v_bitop3_b16 %0, %1, %2, %3 bitop3:0x1b"), \
    bitop3(a, b, c, 0x1b) & 0xffff)                                                                                    \
  X(4, bitop3_b16_2d, "v_bitop3_b16:0x2d", 1, U32, U32, U32, SP_NONE, LOW16("v_bitop3_b16 %0, %1, %2, %3 bitop3:0x2d"), \
    bitop3(a, b, c, 0x2d) & 0xffff)                                                                                    \
  X(4, bitop3_b16_ca, "v_bitop3_b16:0xca", 1, U32, U32, U32, SP_NONE, LOW16("v_bitop3_b16 %0, %1, %2, %3 bitop3:0xca"), \
    bitop3(a, b, c, 0xca) & 0xffff)                                                                                    \
  X(4, and_or_b32, "v_and_or_b32", 1, U32, U32, U32, SP_NONE, A("v_and_or_b32 %0, %1, %2, %3"), (a & b) | c)           \
  X(4, lshl_or_b32, "v_lshl_or_b32", 1, U32, U32, U32, SP_NONE, A("v_lshl_or_b32 %0, %1, %2, %3"),                     \
    LO(a << (b & 31)) | c)                                                                                             \
  X(4, bfrev_b32, "v_bfrev_b32", 1, U32, NONE, NONE, SP_NONE, A("v_bfrev_b32_e32 %0, %1"), bitrev(a))                  \
  X(4, ffbh_u32, "v_ffbh_u32", 1, U32, NONE, NONE, SP_NONE, A("v_ffbh_u32_e32 %0, %1"),                                \
    a ? static_cast<uint32_t>(__builtin_clz(static_cast<uint32_t>(a))) : 0xffffffffu)                                  \
  X(4, ffbl_b32, "v_ffbl_b32", 1, U32, NONE, NONE, SP_NONE, A("v_ffbl_b32_e32 %0, %1"),                                \
    a ? static_cast<uint32_t>(__builtin_ctz(static_cast<uint32_t>(a))) : 0xffffffffu)                                  \
  X(4, ffbh_i32, "v_ffbh_i32", 1, U32, NONE, NONE, SP_NONE, A("v_ffbh_i32_e32 %0, %1"), ffbh_i(a))                     \
  X(4, bcnt_u32_b32, "v_bcnt_u32_b32", 1, U32, U32, NONE, SP_NONE, A("v_bcnt_u32_b32 %0, %1, %2"),                     \
    LO(static_cast<uint64_t>(__builtin_popcountll(a)) + b))                                                            \
  X(4, mbcnt_lo_u32_b32, "v_mbcnt_lo_u32_b32", 1, U32, U32, NONE, SP_NONE, A("v_mbcnt_lo_u32_b32 %0, %1, %2"),         \
    LO(static_cast<uint64_t>(__builtin_popcountll(a & LO((1ull << (t & 63)) - 1))) + b))                               \
  X(4, mbcnt_hi_u32_b32, "v_mbcnt_hi_u32_b32", 1, U32, U32, NONE, SP_NONE, A("v_mbcnt_hi_u32_b32 %0, %1, %2"),         \
    LO(static_cast<uint64_t>(__builtin_popcountll(a & HI((1ull << (t & 63)) - 1))) + b))                               \
  /* ---- dot */                                                                                                       \
  X(5, dot2_f32_f16, "v_dot2_f32_f16", 1, PKSI16, PKSI16, SIF32, SP_NONE, A("v_dot2_f32_f16 %0, %1, %2, %3"),          \
    FB(static_cast<float>(H(a) * H(b) + HH(a) * HH(b) + F(c))))                                                        \
  X(5, dot2_f32_bf16, "v_dot2_f32_bf16", 1, PKSIBF, PKSIBF, SIF32, SP_NONE, A("v_dot2_f32_bf16 %0, %1, %2, %3"),       \
    FB(static_cast<float>(BF(a) * BF(b) + BF(a >> 16) * BF(b >> 16) + F(c))))                                          \
  X(5, dot2c_f32_bf16, "v_dot2c_f32_bf16", 1, PKSIBF, PKSIBF, SIF32, SP_NONE,                                          \
    A("v_mov_b32_e32 %0, %3\n\ts_nop 0\n\tv_dot2c_f32_bf16_e32 %0, %1, %2"),                                           \
    FB(static_cast<float>(BF(a) * BF(b) + BF(a >> 16) * BF(b >> 16) + F(c))))                                          \
  X(5, dot4_i32_i8, "v_dot4_i32_i8", 1, U32, U32, U32, SP_NONE, A("v_dot4_i32_i8 %0, %1, %2, %3"),                     \
    LO(static_cast<uint64_t>(dot4(a, b, true)) + c))                                                                   \
  X(5, dot4_u32_u8, "v_dot4_u32_u8", 1, U32, U32, U32, SP_NONE, A("v_dot4_u32_u8 %0, %1, %2, %3"),                     \
    LO(static_cast<uint64_t>(dot4(a, b, false)) + c))                                                                  \
  X(5, dot8_i32_i4, "v_dot8_i32_i4", 1, U32, U32, U32, SP_NONE, A("v_dot8_i32_i4 %0, %1, %2, %3"),                     \
    LO(static_cast<uint64_t>(dot8(a, b, true)) + c))                                                                   \
  X(5, dot8_u32_u4, "v_dot8_u32_u4", 1, U32, U32, U32, SP_NONE, A("v_dot8_u32_u4 %0, %1, %2, %3"),                     \
    LO(static_cast<uint64_t>(dot8(a, b, false)) + c))                                                                  \
  /* ---- cvt */                                                                                                       \
  X(6, cvt_f32_i32, "v_cvt_f32_i32", 1, U32, NONE, NONE, SP_I2F, A("v_cvt_f32_i32_e32 %0, %1"),                        \
    FB(static_cast<float>(I(a))))                                                                                      \
  X(6, cvt_f32_u32, "v_cvt_f32_u32", 1, U32, NONE, NONE, SP_I2F, A("v_cvt_f32_u32_e32 %0, %1"),                        \
    FB(static_cast<float>(static_cast<uint32_t>(a))))                                                                  \
  X(6, cvt_i32_f32, "v_cvt_i32_f32", 1, F32INT, NONE, NONE, SP_TIE32, A("v_cvt_i32_f32_e32 %0, %1"),                   \
    LO(static_cast<uint32_t>(static_cast<int32_t>(F(a)))))                                                             \
  X(6, cvt_u32_f32, "v_cvt_u32_f32", 1, F32UINT, NONE, NONE, SP_NONE, A("v_cvt_u32_f32_e32 %0, %1"),                   \
    LO(static_cast<uint32_t>(F(a))))                                                                                   \
  X(6, cvt_rpi_i32_f32, "v_cvt_rpi_i32_f32", 1, F32INT, NONE, NONE, SP_TIE32, A("v_cvt_rpi_i32_f32_e32 %0, %1"),       \
    LO(static_cast<uint32_t>(static_cast<int32_t>(std::floor(static_cast<double>(F(a)) + 0.5)))))                      \
  X(6, cvt_flr_i32_f32, "v_cvt_flr_i32_f32", 1, F32INT, NONE, NONE, SP_TIE32, A("v_cvt_flr_i32_f32_e32 %0, %1"),       \
    LO(static_cast<uint32_t>(static_cast<int32_t>(std::floor(F(a))))))                                                 \
  X(6, cvt_f64_f32, "v_cvt_f64_f32", 2, F32, NONE, NONE, SP_NONE, A("v_cvt_f64_f32_e32 %0, %1"),                       \
    DB(static_cast<double>(F(a))))                                                                                     \
  X(6, cvt_f32_f64, "v_cvt_f32_f64", 1, F64, NONE, NONE, SP_CVTD, A("v_cvt_f32_f64_e32 %0, %1"),                       \
    FB(static_cast<float>(D(a))))                                                                                      \
  X(6, cvt_f64_i32, "v_cvt_f64_i32", 2, U32, NONE, NONE, SP_NONE, A("v_cvt_f64_i32_e32 %0, %1"),                       \
    DB(static_cast<double>(I(a))))                                                                                     \
  X(6, cvt_i32_f64, "v_cvt_i32_f64", 1, F64INT, NONE, NONE, SP_TIE64, A("v_cvt_i32_f64_e32 %0, %1"),                   \
    LO(static_cast<uint32_t>(static_cast<int32_t>(D(a)))))                                                             \
  X(6, cvt_f32_ubyte0, "v_cvt_f32_ubyte0", 1, U32, NONE, NONE, SP_NONE, A("v_cvt_f32_ubyte0_e32 %0, %1"),              \
    FB(static_cast<float>(a & 0xff)))                                                                                  \
  X(6, cvt_f32_ubyte1, "v_cvt_f32_ubyte1", 1, U32, NONE, NONE, SP_NONE, A("v_cvt_f32_ubyte1_e32 %0, %1"),              \
    FB(static_cast<float>((a >> 8) & 0xff)))                                                                           \
  X(6, cvt_f32_ubyte2, "v_cvt_f32_ubyte2", 1, U32, NONE, NONE, SP_NONE, A("v_cvt_f32_ubyte2_e32 %0, %1"),              \
    FB(static_cast<float>((a >> 16) & 0xff)))                                                                          \
  X(6, cvt_f32_ubyte3, "v_cvt_f32_ubyte3", 1, U32, NONE, NONE, SP_NONE, A("v_cvt_f32_ubyte3_e32 %0, %1"),              \
    FB(static_cast<float>((a >> 24) & 0xff)))                                                                          \
  X(6, cvt_pk_u8_f32, "v_cvt_pk_u8_f32", 1, F32B, U32, U32, SP_NONE, A("v_cvt_pk_u8_f32 %0, %1, %2, %3"),              \
    (c & ~(0xffull << (8 * (b & 3)))) | cvt_u8(F(a)) << (8 * (b & 3)))                                                 \
  X(6, cvt_f16_f32, "v_cvt_f16_f32", 1, F32H, NONE, NONE, SP_CVTH, LOW16("v_cvt_f16_f32_e32 %0, %1"), HB(F(a)))        \
  X(6, cvt_f32_f16, "v_cvt_f32_f16", 1, PKF16, NONE, NONE, SP_NONE, A("v_cvt_f32_f16_e32 %0, %1"),                     \
    FB(static_cast<float>(H(a))))                                                                                      \
  X(6, cvt_pk_f16_f32, "v_cvt_pk_f16_f32", 1, F32H, F32H, NONE, SP_CVTH, A("v_cvt_pk_f16_f32 %0, %1, %2"),             \
    PKH(F(a), F(b)))                                                                                                   \
  X(6, cvt_pkrtz_f16_f32, "v_cvt_pkrtz_f16_f32", 1, F32H, F32H, NONE, SP_CVTH, A("v_cvt_pkrtz_f16_f32 %0, %1, %2"),    \
    HB(F(a & 0xffffe000u)) | HB(F(b & 0xffffe000u)) << 16)                                                             \
  X(6, cvt_pk_bf16_f32, "v_cvt_pk_bf16_f32", 1, F32, F32, NONE, SP_CVTBF, A("v_cvt_pk_bf16_f32 %0, %1, %2"),           \
    BFB(F(a)) | BFB(F(b)) << 16)                                                                                       \
  X(6, cvt_pk_i16_i32, "v_cvt_pk_i16_i32", 1, U32, U32, NONE, SP_NONE, A("v_cvt_pk_i16_i32 %0, %1, %2"),               \
    (sat_i(I(a), -32768, 32767) & 0xffff) | (sat_i(I(b), -32768, 32767) & 0xffff) << 16)                               \
  X(6, cvt_pk_u16_u32, "v_cvt_pk_u16_u32", 1, U32, U32, NONE, SP_NONE, A("v_cvt_pk_u16_u32 %0, %1, %2"),               \
    std::min<uint64_t>(a, 0xffff) | std::min<uint64_t>(b, 0xffff) << 16)                                               \
  X(6, cvt_pknorm_i16_f32, "v_cvt_pknorm_i16_f32", 1, F32N8, F32N8, NONE, SP_NONE,                                     \
    A("v_cvt_pknorm_i16_f32 %0, %1, %2"), snorm16(F(a)) | snorm16(F(b)) << 16)                                         \
  X(6, ashr_pk_i8_i32, "v_ashr_pk_i8_i32", 1, U32, U32, U32, SP_NONE, LOW16("v_ashr_pk_i8_i32 %0, %1, %2, %3"),        \
    (sat_i(I(a) >> (c & 31), -128, 127) & 0xff) | (sat_i(I(b) >> (c & 31), -128, 127) & 0xff) << 8)                    \
  X(6, ashr_pk_u8_i32, "v_ashr_pk_u8_i32", 1, U32, U32, U32, SP_NONE, LOW16("v_ashr_pk_u8_i32 %0, %1, %2, %3"),        \
    (sat_i(I(a) >> (c & 31), 0, 255) & 0xff) | (sat_i(I(b) >> (c & 31), 0, 255) & 0xff) << 8)                          \
  X(6, cvt_pk_fp8_f32, "v_cvt_pk_fp8_f32", 1, F32Q, F32Q, NONE, SP_CVTF8,                                              \
    LOW16("v_mov_b32_e32 %0, 0\n\tv_cvt_pk_fp8_f32 %0, %1, %2"), enc(F(a), 4, 3) | enc(F(b), 4, 3) << 8)               \
  X(6, cvt_pk_bf8_f32, "v_cvt_pk_bf8_f32", 1, F32Q, F32Q, NONE, SP_CVTBF8,                                             \
    LOW16("v_mov_b32_e32 %0, 0\n\tv_cvt_pk_bf8_f32 %0, %1, %2"), enc(F(a), 5, 2) | enc(F(b), 5, 2) << 8)               \
  X(6, cvt_f32_fp8_0, "v_cvt_f32_fp8:0", 1, FP8, NONE, NONE, SP_NONE, A("v_cvt_f32_fp8_sdwa %0, %1 src0_sel:BYTE_0"),  \
    FB(static_cast<float>(Q8(a, 0))))                                                                                  \
  X(6, cvt_f32_fp8_1, "v_cvt_f32_fp8:1", 1, FP8, NONE, NONE, SP_NONE, A("v_cvt_f32_fp8_sdwa %0, %1 src0_sel:BYTE_1"),  \
    FB(static_cast<float>(Q8(a, 1))))                                                                                  \
  X(6, cvt_f32_fp8_2, "v_cvt_f32_fp8:2", 1, FP8, NONE, NONE, SP_NONE, A("v_cvt_f32_fp8_sdwa %0, %1 src0_sel:BYTE_2"),  \
    FB(static_cast<float>(Q8(a, 2))))                                                                                  \
  X(6, cvt_f32_fp8_3, "v_cvt_f32_fp8:3", 1, FP8, NONE, NONE, SP_NONE, A("v_cvt_f32_fp8_sdwa %0, %1 src0_sel:BYTE_3"),  \
    FB(static_cast<float>(Q8(a, 3))))                                                                                  \
  X(6, cvt_f32_bf8_0, "v_cvt_f32_bf8:0", 1, BF8, NONE, NONE, SP_NONE, A("v_cvt_f32_bf8_sdwa %0, %1 src0_sel:BYTE_0"),  \
    FB(static_cast<float>(B8(a, 0))))                                                                                  \
  X(6, cvt_f32_bf8_1, "v_cvt_f32_bf8:1", 1, BF8, NONE, NONE, SP_NONE, A("v_cvt_f32_bf8_sdwa %0, %1 src0_sel:BYTE_1"),  \
    FB(static_cast<float>(B8(a, 1))))                                                                                  \
  X(6, cvt_f32_bf8_2, "v_cvt_f32_bf8:2", 1, BF8, NONE, NONE, SP_NONE, A("v_cvt_f32_bf8_sdwa %0, %1 src0_sel:BYTE_2"),  \
    FB(static_cast<float>(B8(a, 2))))                                                                                  \
  X(6, cvt_f32_bf8_3, "v_cvt_f32_bf8:3", 1, BF8, NONE, NONE, SP_NONE, A("v_cvt_f32_bf8_sdwa %0, %1 src0_sel:BYTE_3"),  \
    FB(static_cast<float>(B8(a, 3))))                                                                                  \
  X(6, cvt_pk_f32_fp8, "v_cvt_pk_f32_fp8", 2, FP8, NONE, NONE, SP_NONE, A("v_cvt_pk_f32_fp8_e32 %0, %1"),              \
    PK(FB(static_cast<float>(Q8(a, 0))), FB(static_cast<float>(Q8(a, 1)))))                                            \
  X(6, cvt_scalef32_pk_fp8_f32, "v_cvt_scalef32_pk_fp8_f32", 1, F32QS, F32QS, SCALE3, SP_CVTF8,                        \
    LOW16("v_mov_b32_e32 %0, 0\n\tv_cvt_scalef32_pk_fp8_f32 %0, %1, %2, %3"),                                           \
    enc(F(a) / F(c), 4, 3) | enc(F(b) / F(c), 4, 3) << 8)                                                              \
  X(6, cvt_scalef32_pk_f32_fp8, "v_cvt_scalef32_pk_f32_fp8", 2, FP8, SCALE3, NONE, SP_NONE,                            \
    A("v_cvt_scalef32_pk_f32_fp8 %0, %1, %2"),                                                                         \
    PK(FB(static_cast<float>(Q8(a, 0) * F(b))), FB(static_cast<float>(Q8(a, 1) * F(b)))))                              \
  X(6, cvt_scalef32_pk_fp4_f32, "v_cvt_scalef32_pk_fp4_f32", 1, F32F4, F32F4, SCALE1, SP_CVTF4,                        \
    LOW8("v_mov_b32_e32 %0, 0\n\tv_cvt_scalef32_pk_fp4_f32 %0, %1, %2, %3"),                                            \
    enc(F(a) / F(c), 2, 1) | enc(F(b) / F(c), 2, 1) << 4)                                                              \
  X(6, cvt_scalef32_pk_f32_fp4, "v_cvt_scalef32_pk_f32_fp4", 2, U32, SCALE1, NONE, SP_NONE,                            \
    A("v_cvt_scalef32_pk_f32_fp4 %0, %1, %2"),                                                                         \
    PK(FB(static_cast<float>(dec(a & 15, 2, 1) * F(b))), FB(static_cast<float>(dec((a >> 4) & 15, 2, 1) * F(b)))))     \
  X(6, cvt_scalef32_pk32_f32_fp6, "v_cvt_scalef32_pk32_f32_fp6", 2, U64, U64, U64, SP_NONE,                            \
    v = fp6_unpack_fold(a, b, cc), fp6_fold(a, b, c))                                                                  \
  /* ---- trans */                                                                                                     \
  X(7, exp_f32, "v_exp_f32", 1, EXPI, NONE, NONE, SP_NONE, A("v_exp_f32_e32 %0, %1"), FB(std::exp2(F(a))))             \
  X(7, log_f32, "v_log_f32", 1, POW4F32, NONE, NONE, SP_NONE, A("v_log_f32_e32 %0, %1"), FB(std::log2(F(a))))          \
  X(7, rcp_f32, "v_rcp_f32", 1, POW2F32, NONE, NONE, SP_NONE, A("v_rcp_f32_e32 %0, %1"), FB(1.0f / F(a)))              \
  X(7, rsq_f32, "v_rsq_f32", 1, POW4F32, NONE, NONE, SP_NONE, A("v_rsq_f32_e32 %0, %1"), FB(1.0f / std::sqrt(F(a))))   \
  X(7, sqrt_f32_pow4, "v_sqrt_f32:4^n", 1, POW4F32, NONE, NONE, SP_NONE, A("v_sqrt_f32_e32 %0, %1"),                   \
    FB(std::sqrt(F(a))))                                                                                               \
  X(7, sqrt_f32_sq, "v_sqrt_f32:k^2", 1, SQINT, NONE, NONE, SP_NONE, A("v_sqrt_f32_e32 %0, %1"), FB(std::sqrt(F(a))))  \
  X(7, sin_f32, "v_sin_f32", 1, QREV, NONE, NONE, SP_NONE, A("v_sin_f32_e32 %0, %1"), FB(quarter_sin(F(a) * 4.0f)))    \
  X(7, cos_f32, "v_cos_f32", 1, QREV, NONE, NONE, SP_NONE, A("v_cos_f32_e32 %0, %1"),                                  \
    FB(quarter_sin(F(a) * 4.0f + 1.0f)))                                                                               \
  X(7, rcp_f64, "v_rcp_f64", 2, POW2F64, NONE, NONE, SP_NONE, A("v_rcp_f64_e32 %0, %1"), DB(1.0 / D(a)))               \
  X(7, rsq_f64, "v_rsq_f64", 2, POW4F64, NONE, NONE, SP_NONE, A("v_rsq_f64_e32 %0, %1"), DB(1.0 / std::sqrt(D(a))))    \
  X(7, rcp_f16, "v_rcp_f16", 1, POW2F16, NONE, NONE, SP_NONE, LOW16("v_rcp_f16_e32 %0, %1"), HB(1.0 / H(a)))           \
  X(7, rsq_f16, "v_rsq_f16", 1, POW4F16, NONE, NONE, SP_NONE, LOW16("v_rsq_f16_e32 %0, %1"), HB(1.0 / std::sqrt(H(a)))) \
  X(7, sqrt_f16, "v_sqrt_f16", 1, POW4F16, NONE, NONE, SP_NONE, LOW16("v_sqrt_f16_e32 %0, %1"), HB(std::sqrt(H(a))))   \
  X(7, exp_f16, "v_exp_f16", 1, EXPIF16, NONE, NONE, SP_NONE, LOW16("v_exp_f16_e32 %0, %1"), HB(std::exp2(H(a))))      \
  X(7, log_f16, "v_log_f16", 1, POW4F16, NONE, NONE, SP_NONE, LOW16("v_log_f16_e32 %0, %1"), HB(std::log2(H(a))))

// ------------------------------------------------------------------ the table
#define X(U, ID, NAME, NRES, KA, KB, KC, SP, DEV, HOST) G_##ID,
enum StepId : int { VALU_STEPS(X) kNumSteps };
#undef X
static_assert(kNumSteps <= 192, "the record's step mask has 192 bits");

struct StepInfo {
  int unit, words, ka, kb, kc, sp;
};
#define X(U, ID, NAME, NRES, KA, KB, KC, SP, DEV, HOST) {U, NRES, KA, KB, KC, SP},
constexpr StepInfo kSteps[kNumSteps] = {VALU_STEPS(X)};
#undef X
#define X(U, ID, NAME, NRES, KA, KB, KC, SP, DEV, HOST) NAME,
const char* const kStepNames[kNumSteps] = {VALU_STEPS(X)};
#undef X

XS_HD constexpr int unit_first(int u) {  // global index of the unit's first step
  int g = 0;
  while (g < kNumSteps && kSteps[g].unit < u) ++g;
  return g;
}
XS_HD constexpr int unit_steps(int u) { return unit_first(u + 1) - unit_first(u); }
XS_HD constexpr int step_row(int g) {  // row of step g's word 0 within its unit
  int r = 0;
  for (int i = unit_first(kSteps[g].unit); i < g; ++i) r += kSteps[i].words;
  return r;
}
XS_HD constexpr int unit_rows(int u) {
  int r = 0;
  for (int i = unit_first(u); i < unit_first(u + 1); ++i) r += kSteps[i].words;
  return r;
}
XS_HD constexpr int rows_before(int u) {
  int r = 0;
  for (int i = 0; i < unit_first(u); ++i) r += kSteps[i].words;
  return r;
}
constexpr int kTotalRows = rows_before(kNumUnits);
constexpr bool units_in_order() {
  for (int g = 1; g < kNumSteps; ++g)
    if (kSteps[g].unit < kSteps[g - 1].unit) return false;
  for (int u = 0; u < kNumUnits; ++u)
    if (unit_steps(u) <= 0 || unit_steps(u) > 255) return false;
  return true;
}
static_assert(units_in_order(), "VALU_STEPS lists the units in order, none empty");

// Words of the expected table before unit u's: [unit][round][row][256].
XS_HD size_t table_offset(int u, uint32_t rounds) { return static_cast<size_t>(rows_before(u)) * rounds * kBlock; }

constexpr uint32_t kLdsUsed = part_reduction_words(kNumUnits, 6) * 4;  // the step mask is reduced too

struct ValuRecord {
  PartRecordHead<kNumUnits> head;
  uint32_t reserved;
  uint32_t bad_steps[6];
  uint32_t pad[4];
};
static_assert(sizeof(ValuRecord) == 128, "one 128-byte record per workgroup");

using Expect = PartExpect<kNumUnits>;

// ------------------------------------------------------------------- device
struct Ctx {
  uint32_t seed, t, rounds, inj;
  const uint32_t* want;  // the whole expected table
  uint32_t* dump;        // k_valu_probe only
};

template <int K>
struct OpT {
  using type = std::conditional_t<is64(K), uint64_t, uint32_t>;
};
template <int N>
struct ResT {
  using type = std::conditional_t<N == 2, uint64_t, uint32_t>;
};

template <int G, typename Fn>
XS_D void run_step(const Ctx& c, Tally& y, uint32_t (&stepbad)[6], uint32_t r, Fn&& fn) {
  constexpr StepInfo si{kSteps[G].unit, kSteps[G].words, kSteps[G].ka, kSteps[G].kb, kSteps[G].kc, kSteps[G].sp};
  constexpr int u = si.unit, s = G - unit_first(u), row = step_row(G), rows = unit_rows(u);
  using TA = typename OpT<si.ka>::type;
  using TB = typename OpT<si.kb>::type;
  using TC = typename OpT<si.kc>::type;
  const TA a = static_cast<TA>(operand(si.ka, si.sp, c.seed, u, s, r, 0, c.t));
  TB b = static_cast<TB>(operand(si.kb, si.sp, c.seed, u, s, r, 1, c.t));
  const TC cc = static_cast<TC>(operand(si.kc, si.sp, c.seed, u, s, r, 2, c.t));
  if constexpr (si.sp == SP_EQ)
    if (r == 1 && (c.t & 1u)) b = static_cast<TB>(a);
  const uint64_t v = fn(a, b, cc);
  const uint32_t* want = c.want + table_offset(u, c.rounds);
  uint32_t miss = 0;
#pragma unroll
  for (int w = 0; w < si.words; ++w) {
    const uint32_t idx = (r * rows + row + w) * kBlock + c.t;
    miss |= take_word(y, c.dump, idx, static_cast<uint32_t>(v >> (32 * w)), want[idx], (c.inj >> u) & 1u);
  }
  if (miss) stepbad[G / 32] |= 1u << (G % 32);
}

template <int UNIT>
XS_D void run_unit(const Ctx& c, Tally& y, uint32_t (&stepbad)[6]) {
  for (uint32_t r = 0; r < c.rounds; ++r) {
#define X(U, ID, NAME, NRES, KA, KB, KC, SP, DEV, HOST)                                                         \
  if constexpr (U == UNIT)                                                                                      \
    run_step<G_##ID>(c, y, stepbad, r,                                                                          \
                     [&](typename OpT<KA>::type a, typename OpT<KB>::type b, typename OpT<KC>::type cc) -> uint64_t { \
                       typename ResT<NRES>::type v;                                                             \
                       (void)a, (void)b, (void)cc;                                                              \
                       DEV;                                                                                     \
                       return v;                                                                                \
                     });
    VALU_STEPS(X)
#undef X
  }
}

XS_D void run_units(const Ctx& c, uint32_t mask, Tally (&y)[kNumUnits], uint32_t (&stepbad)[6]) {
  if (mask & 1u) run_unit<0>(c, y[0], stepbad);
  if (mask & 2u) run_unit<1>(c, y[1], stepbad);
  if (mask & 4u) run_unit<2>(c, y[2], stepbad);
  if (mask & 8u) run_unit<3>(c, y[3], stepbad);
  if (mask & 16u) run_unit<4>(c, y[4], stepbad);
  if (mask & 32u) run_unit<5>(c, y[5], stepbad);
  if (mask & 64u) run_unit<6>(c, y[6], stepbad);
  if (mask & 128u) run_unit<7>(c, y[7], stepbad);
}

// Two waves per SIMD is the register budget, not the occupancy (the LDS keeps
// a CU to one workgroup): it holds the kernel to 256 registers a lane.
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(2))) void k_valu_sweep(
    ValuRecord* __restrict__ records, const uint32_t* __restrict__ want, uint32_t unit_mask, uint32_t seed,
    uint32_t rounds, int inject_xcd, int inject_cu, uint32_t inject_units, Expect expect) {
  extern __shared__ uint32_t valu_lds[];
  const uint32_t t = threadIdx.x;
  const uint32_t xcd = xcc_id();
  const uint32_t hw = hw_id();
  const uint32_t cu = cu_key(hw);
  const uint32_t simd = simd_id(hw);
  const bool inject = inject_selected(inject_xcd, inject_cu, xcd, cu);
  const Ctx c{seed, t, rounds, inject ? inject_units : 0u, want, nullptr};

  Tally y[kNumUnits];
  uint32_t stepbad[6] = {};
  run_units(c, unit_mask, y, stepbad);

  reduce_parts<kNumUnits, 6>(valu_lds, t, simd, y, stepbad, unit_mask, expect, xcd, cu, &records[blockIdx.x]);
}

// One workgroup; dump holds rounds x rows x 256 words of unit `unit`.
__global__ __launch_bounds__(kBlock) void k_valu_probe(uint32_t* __restrict__ dump, const uint32_t* __restrict__ want,
                                                      int unit, uint32_t seed, uint32_t rounds) {
  const uint32_t t = threadIdx.x;
  const Ctx c{seed, t, rounds, 0u, want, dump};
  Tally y[kNumUnits];
  uint32_t stepbad[6] = {};
  run_units(c, 1u << unit, y, stepbad);
}

// --------------------------------------------------------------------- host
uint64_t bitrev(uint64_t a) {
  uint64_t r = 0;
  for (int i = 0; i < 32; ++i) r |= ((a >> i) & 1) << (31 - i);
  return r;
}
// sin of q quarter revolutions, q a small integer: exactly 0, 1, 0, -1.
float quarter_sin(float q) {
  const int k = static_cast<int>(q) & 3;
  return k == 1 ? 1.0f : k == 3 ? -1.0f : 0.0f;
}

using HostFn = uint64_t (*)(uint64_t, uint64_t, uint64_t, uint32_t);
#define X(U, ID, NAME, NRES, KA, KB, KC, SP, DEV, HOST)                                 \
  [](uint64_t a, uint64_t b, uint64_t c, uint32_t t) -> uint64_t {                      \
    int tmp = 0;                                                                        \
    (void)a, (void)b, (void)c, (void)t, (void)tmp;                                      \
    return static_cast<uint64_t>(HOST);                                                 \
  },
const HostFn kHostFns[kNumSteps] = {VALU_STEPS(X)};
#undef X

// out[round][row][256] of unit u.
void expected_unit(int u, uint32_t seed, uint32_t rounds, uint32_t* out) {
  const int first = unit_first(u), rows = unit_rows(u);
  for (uint32_t r = 0; r < rounds; ++r) {
    int row = 0;
    for (int g = first; g < first + unit_steps(u); ++g) {
      const StepInfo si = kSteps[g];
      const uint32_t s = static_cast<uint32_t>(g - first);
      for (uint32_t t = 0; t < kBlock; ++t) {
        const uint64_t a = operand(si.ka, si.sp, seed, u, s, r, 0, t);
        uint64_t b = operand(si.kb, si.sp, seed, u, s, r, 1, t);
        const uint64_t c = operand(si.kc, si.sp, seed, u, s, r, 2, t);
        if (si.sp == SP_EQ && r == 1 && (t & 1u)) b = a;
        const uint64_t v = kHostFns[g](a, b, c, t);
        for (int w = 0; w < si.words; ++w)
          out[(static_cast<size_t>(r) * rows + row + w) * kBlock + t] = static_cast<uint32_t>(v >> (32 * w));
      }
      row += si.words;
    }
  }
}

uint32_t digest_of(const uint32_t* v, size_t n) {
  uint32_t d = 0;
  for (size_t i = 0; i < n; ++i) d += v[i] * (2u * static_cast<uint32_t>(i) + 1u);
  return d;
}

// The node agent sweeps with one seed and round count again and again: keep the last.
struct Table {
  std::vector<uint32_t> words;  // [unit][round][row][256]
  uint32_t digest[kNumUnits];
};
std::mutex g_table_mu;
Table g_table;
bool g_have = false;
uint32_t g_seed = 0, g_rounds = 0;

// Call with g_table_mu held.
const Table& table(uint32_t seed, uint32_t rounds) {
  if (!g_have || g_seed != seed || g_rounds != rounds) {
    g_table.words.assign(static_cast<size_t>(kTotalRows) * rounds * kBlock, 0u);
    for (int u = 0; u < kNumUnits; ++u) {
      uint32_t* at = g_table.words.data() + table_offset(u, rounds);
      expected_unit(u, seed, rounds, at);
      g_table.digest[u] = digest_of(at, static_cast<size_t>(unit_rows(u)) * rounds * kBlock);
    }
    g_have = true, g_seed = seed, g_rounds = rounds;
  }
  return g_table;
}

bool bad_rounds(uint32_t r) { return r < 1 || r > kMaxRounds; }

int upload_table(uint32_t seed, uint32_t rounds, DevMem& buf, Expect* e, uint32_t mask) {
  std::lock_guard<std::mutex> g(g_table_mu);
  const Table& tb = table(seed, rounds);
  if (e)
    for (int u = 0; u < kNumUnits; ++u) e->digest[u] = (mask >> u) & 1u ? tb.digest[u] : 0u;
  XS_CHECK(hipMalloc(&buf.p, tb.words.size() * 4));
  XS_CHECK(hipMemcpy(buf.p, tb.words.data(), tb.words.size() * 4, hipMemcpyHostToDevice));
  return 0;
}

}  // namespace

extern "C" {

const char* xs_valu_sweep_last_error() { return g_valu_err; }

// Unit names, comma-separated, in bit order.
const char* xs_valu_units() { return kUnitNames; }

// Step names of one unit, comma-separated, in order; nullptr for a bad unit.
const char* xs_valu_steps(int unit) {
  static std::string names[kNumUnits];
  static std::once_flag once;
  std::call_once(once, [] {
    for (int g = 0; g < kNumSteps; ++g) {
      std::string& s = names[kSteps[g].unit];
      if (!s.empty()) s += ',';
      s += kStepNames[g];
    }
  });
  return unit < 0 || unit >= kNumUnits ? nullptr : names[unit].c_str();
}

// out2 = {steps, result words of one round (rows)}.
int xs_valu_shape(int unit, int* out2) {
  if (unit < 0 || unit >= kNumUnits || !out2) return kBadArgs;
  out2[0] = unit_steps(unit);
  out2[1] = unit_rows(unit);
  return 0;
}

// Host only. out[round][row][256], n_words = rounds x rows x 256: what every
// thread of a healthy SIMD gets.
int xs_valu_expected(int unit, uint32_t seed, uint32_t rounds, uint32_t* out, size_t n_words) {
  if (unit < 0 || unit >= kNumUnits || !out || bad_rounds(rounds)) return kBadArgs;
  if (n_words != static_cast<size_t>(unit_rows(unit)) * rounds * kBlock) return kBadArgs;
  expected_unit(unit, seed, rounds, out);
  return 0;
}

// One workgroup runs `unit` and stores every result, laid out as xs_valu_expected's.
int xs_valu_probe(int dev, int unit, uint32_t seed, uint32_t rounds, uint32_t* out, size_t n_words) {
  if (unit < 0 || unit >= kNumUnits || !out || bad_rounds(rounds)) return kBadArgs;
  const size_t n = static_cast<size_t>(unit_rows(unit)) * rounds * kBlock;
  if (n_words != n) return kBadArgs;
  DevMem want;
  return launch_probe(
      g_valu_err, dev, reinterpret_cast<const void*>(k_valu_probe), kBlock, 0, out, n,
      [&](dim3 grid, dim3 block, size_t smem, void* dump) {
        hipLaunchKernelGGL(k_valu_probe, grid, block, smem, 0, static_cast<uint32_t*>(dump), want.as<const uint32_t>(),
                           unit, seed, rounds);
      },
      [&] { return upload_table(seed, rounds, want, nullptr, 0); });
}

// Host only. out8[u] = the workgroup digest a healthy CU leaves for unit u, 0
// for a unit outside unit_mask.
int xs_valu_sweep_expected(uint32_t unit_mask, uint32_t seed, uint32_t rounds, uint32_t* out8) {
  if (bad_part_mask(unit_mask, kAllUnits) || bad_rounds(rounds) || !out8) return kBadArgs;
  std::lock_guard<std::mutex> g(g_table_mu);
  const Table& tb = table(seed, rounds);
  for (int u = 0; u < kNumUnits; ++u) out8[u] = (unit_mask >> u) & 1u ? tb.digest[u] : 0u;
  return 0;
}

// What the runtime reports for k_valu_sweep on `dev`: out4 = {registers per
// lane, scratch bytes per lane, dynamic LDS bytes per workgroup, workgroups
// that fit on a CU at once}.
int xs_valu_sweep_info(int dev, int* out4) {
  return sweep_info(g_valu_err, dev, reinterpret_cast<const void*>(k_valu_sweep), kBlock, true, out4);
}

// One sweep launch of `blocks` workgroups (0: 4 per CU). Writes `blocks`
// 128-byte records to records_out. inject_xcd / inject_cu: -1 is none / any,
// values below -1 are refused. Returns 0, -1000 for bad arguments (nothing is
// launched), or a negative HIP error.
int xs_valu_sweep(int dev, int blocks, uint32_t unit_mask, uint32_t seed, uint32_t rounds, int inject_xcd,
                  int inject_cu, uint32_t inject_units, void* records_out, int* n_records, double* ms) {
  if (bad_part_mask(unit_mask, kAllUnits) || bad_rounds(rounds) || (inject_units & ~kAllUnits)) return kBadArgs;
  Expect e;
  DevMem want;
  return launch_sweep(
      g_valu_err, {dev, blocks, inject_xcd, inject_cu, records_out, n_records, ms},
      reinterpret_cast<const void*>(k_valu_sweep), kBlock, kLdsUsed, sizeof(ValuRecord),
      [&](dim3 grid, dim3 block, size_t smem, void* rec) {
        hipLaunchKernelGGL(k_valu_sweep, grid, block, smem, 0, static_cast<ValuRecord*>(rec),
                           want.as<const uint32_t>(), unit_mask, seed, rounds, inject_xcd, inject_cu, inject_units, e);
      },
      [&] { return upload_table(seed, rounds, want, &e, unit_mask); });
}

}  // extern "C"
