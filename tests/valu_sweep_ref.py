"""Reference of the VALU sweep (csrc/hip/valu_sweep.hip), written from IEEE-754,
the ISA's integer definitions and the operand rules in that file's header. It
shares no code with the C++: add, mul, div, sqrt go through numpy, every
fused step and every narrowing conversion through exact rationals rounded
once, the integer and bit steps through Python integers.

A launch's thread is t = 64 * wave + lane; arrays are [round][row][256], row
running over the result words of the unit's steps in order."""
from fractions import Fraction
from functools import lru_cache
from math import floor, ceil, isqrt

import numpy as np

SEEDS = (0x1B873593, 0xC0FFEE11)
UNITS = ["f32", "f64", "f16", "int", "bit", "dot", "cvt", "trans"]
M32 = 0xFFFFFFFF
M64 = (1 << 64) - 1
T = np.arange(256, dtype=np.int64)
HALF = Fraction(1, 2)


def fmix32(h):
    """murmur3's 32-bit finaliser on an int64 array of 32-bit values."""
    h = np.asarray(h, np.int64) & M32
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & M32
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & M32
    h ^= h >> 16
    return h


def key(unit, step, rnd_, operand, t=T):
    return (unit << 28) | (step << 20) | (rnd_ << 12) | (operand << 8) | t


def hashes(seed, unit, step, rnd_, operand):
    return [int(v) for v in fmix32(seed ^ key(unit, step, rnd_, operand))]


# ------------------------------------------------------------ number formats
F16, BF16, F32, F64, E4M3, E5M2, E2M1, E2M3 = (5, 10), (8, 7), (8, 23), (11, 52), (4, 3), (5, 2), (2, 1), (2, 3)


def dec(bits, fmt):
    """The finite value of an encoding, exactly."""
    eb, mb = fmt
    bias = (1 << (eb - 1)) - 1
    m, f = bits & ((1 << mb) - 1), (bits >> mb) & ((1 << eb) - 1)
    v = Fraction(m + (1 << mb)) * Fraction(2) ** (f - bias - mb) if f else Fraction(m) * Fraction(2) ** (1 - bias - mb)
    return -v if bits >> (eb + mb) & 1 else v


def ilog2(x):
    """floor(log2(x)) of a positive rational."""
    e = x.numerator.bit_length() - x.denominator.bit_length()
    while Fraction(2) ** e > x:
        e -= 1
    while Fraction(2) ** (e + 1) <= x:
        e += 1
    return e


def enc(x, fmt, toward_zero=False):
    """x rounded once to the format: nearest even (or toward zero), subnormals kept."""
    eb, mb = fmt
    if x == 0:
        return 0
    bias = (1 << (eb - 1)) - 1
    emin = 1 - bias
    s, x = x < 0, abs(x)
    e = max(ilog2(x), emin)
    q = x / Fraction(2) ** (e - mb)
    n = floor(q)
    rem = q - n
    if not toward_zero and (rem > HALF or (rem == HALF and n & 1)):
        n += 1
    return (int(s) << (eb + mb)) | (((e - emin) << mb) + n)


def is_normal_finite(bits, fmt):
    eb, mb = fmt
    f = (bits >> mb) & ((1 << eb) - 1)
    return 0 < f < (1 << eb) - 1


def sx(v, bits):
    v &= (1 << bits) - 1
    return v - (1 << bits) if v >> (bits - 1) else v


def widen(bits, fmt, to):
    """An exact widening conversion; a zero keeps its sign."""
    return enc(dec(bits, fmt), to) | (bits >> sum(fmt) & 1) << sum(to)


def scaled(bits, fmt, scale):
    """A narrow float times a power-of-two scale, as f32; a zero keeps its sign."""
    return enc(dec(bits, fmt) * fr(scale), F32) | (bits >> sum(fmt) & 1) << 31


def f32_of_int(v):
    return enc(Fraction(v), F32)


# ------------------------------------------------------------------ operands
def edge_class(r, o, t):
    if r != 0:
        return 7
    return ((t >> 6) | (t & 1) << 2) if o == 2 else (t >> (3 * o)) & 7


def sig(h, bits, cls):
    m = (1 << bits) - 1
    return [m, 1 << ((h & m) % bits), 0, 1][cls] if cls < 4 else h & m


def word_class(h, cls):
    return [M32, 0x80000000, 0, 1, 0x7FFFFFFF][cls] if cls < 5 else h


def f32_band(h, cls, lo, n, sign=True):
    return (h & 0x80000000 if sign else 0) | (lo + ((h >> 23) & 0xFF) % n) << 23 | sig(h, 23, cls)


def f64_band(h, hl, cls, lo, n, sign=True):
    hi = (h & 0x80000000 if sign else 0) | (lo + ((h >> 20) & 0x7FF) % n) << 20 | (0 if cls == 3 else sig(h, 20, cls))
    low = {0: M32, 1: 0, 2: 0, 3: 1}.get(cls, hl)
    return hi << 32 | low


def f16_half(h16, cls, sign=True):
    return (h16 & 0x8000 if sign else 0) | (13 + ((h16 >> 10) & 31) % 9) << 10 | sig(h16, 10, cls)


def class_hi(h, emax, mbits):
    m = (1 << mbits) - 1
    frac, e = (h >> 8) & m, 1 + (h >> 4) % (emax - 1)
    return [emax << mbits | (frac & (m >> 1)) | 1, (h & 0x80000000) | emax << mbits | ((m >> 1) + 1) | frac,
            0x80000000 | emax << mbits, 0x80000000 | e << mbits | frac, 0x80000000 | frac | 1, 0x80000000, 0,
            frac | 1, e << mbits | frac, emax << mbits][h % 10]


def fp8_byte(b):
    return b & 0xF7 if b & 0x7F == 0x7F else b


def bf8_byte(b):
    return b & 0xBF if b & 0x7C == 0x7C else b


WIDE = {"U64", "PKF32", "F64", "F64P", "F64NEAR", "F64INT", "F64GE1", "CLS64", "POW2F64", "POW4F64"}
FLOAT_KINDS = {"F32": F32, "F32P": F32, "F64": F64, "F64P": F64, "PKF16": F16, "PKF32": F32}


def shaped(kind, h, h2, cls):
    n20, n10 = h % 41, h % 21
    by = [(h >> (8 * i)) & 0xFF for i in range(4)]
    if kind == "U32":
        return word_class(h, cls)
    if kind == "U64":
        return word_class(h2, cls) << 32 | word_class(h, cls)
    if kind in ("F32", "F32P"):
        return f32_band(h, cls, 96, 63, kind == "F32")
    if kind == "PKF32":
        return f32_band(h2, cls, 96, 63) << 32 | f32_band(h, cls, 96, 63)
    bands = {"F32GE1": (127, 11, True), "F32NEAR": (120, 18, True), "F32INT": (120, 38, True),
             "F32UINT": (120, 38, False), "F32H": (114, 28, True), "F32Q": (121, 14, True),
             "F32QS": (123, 10, True), "F32F4": (126, 2, True)}
    if kind in bands:
        lo, n, sign = bands[kind]
        return f32_band(h, cls, lo, n, sign)
    if kind == "SCALE3":
        return enc(Fraction(2) ** (h % 5 - 2), F32)
    if kind == "SCALE1":
        return enc(Fraction(2) ** (h % 3 - 1), F32)
    if kind == "F32B":
        return f32_of_int(h & 0xFF)
    if kind == "F32N8":
        k = h % 513 - 256
        return enc(Fraction(k + 1 if abs(k) == 128 else k, 256), F32)
    bands64 = {"F64": (992, 63, True), "F64P": (992, 63, False), "F64NEAR": (1016, 18, True),
               "F64INT": (1016, 38, True), "F64GE1": (1023, 11, True)}
    if kind in bands64:
        lo, n, sign = bands64[kind]
        return f64_band(h, h2, cls, lo, n, sign)
    if kind in ("PKF16", "PKF16P"):
        return f16_half(h >> 16, cls, kind == "PKF16") << 16 | f16_half(h & 0xFFFF, cls, kind == "PKF16")
    if kind == "I5":
        return sx(h, 5) & M32
    if kind == "SH4":
        return h % 5
    if kind == "CLS32":
        return class_hi(h, 0xFF, 23)
    if kind == "CLS64":
        return class_hi(h, 0x7FF, 20) << 32
    if kind == "PERMSEL":
        return sum((b % 10 if b % 10 < 8 else b % 10 + 4) << (8 * i) for i, b in enumerate(by))
    if kind == "PKSI16":
        return enc(Fraction((h >> 16) % 31 - 15), F16) << 16 | enc(Fraction(h % 31 - 15), F16)
    if kind == "PKSIBF":
        return enc(Fraction((h >> 16) % 31 - 15), BF16) << 16 | enc(Fraction(h % 31 - 15), BF16)
    if kind == "SIF32":
        return f32_of_int(h % 2047 - 1023)
    if kind == "FP8":
        return sum(fp8_byte(b) << (8 * i) for i, b in enumerate(by))
    if kind == "BF8":
        return sum(bf8_byte(b) << (8 * i) for i, b in enumerate(by))
    if kind == "EXPI":
        return f32_of_int(n20 - 20)
    if kind == "POW2F32":
        return (h & 0x80000000) | enc(Fraction(2) ** (n20 - 20), F32)
    if kind == "POW2F64":
        return ((h & 0x80000000) << 32) | enc(Fraction(2) ** (n20 - 20), F64)
    if kind == "POW4F32":
        return enc(Fraction(4) ** (n10 - 10), F32)
    if kind == "POW4F64":
        return enc(Fraction(4) ** (n10 - 10), F64)
    if kind == "SQINT":
        return f32_of_int((h & 4095) ** 2)
    if kind == "QREV":
        return enc(Fraction(h & 7, 4), F32)
    if kind == "POW2F16":
        return (h & 0x8000) | enc(Fraction(2) ** ((h >> 16) % 15 - 7), F16)
    if kind == "POW4F16":
        return enc(Fraction(4) ** ((h >> 16) % 7 - 3), F16)
    if kind == "EXPIF16":
        return enc(Fraction((h >> 16) % 15 - 7), F16)
    raise KeyError(kind)


# The FMA triple whose exact sum rounds differently through float64.
FMA32_TRIPLE = (f32_of_int(24929), f32_of_int(673), enc(Fraction(1, 1 << 40), F32))


def special(sp, o, lane):
    """The fixed operand of round 1, or None."""
    k = lane & 15
    tie = Fraction(2 * (k - 8) + 1, 2)
    table = {
        "ADD32": (1, 2, lambda: [enc(Fraction(3, 2) * Fraction(2) ** -126, F32), enc(-Fraction(2) ** -126, F32)][o]),
        "FMA32": (2, 3, lambda: [FMA32_TRIPLE,
                                 (enc(Fraction(2) ** -100, F32), enc(Fraction(3, 2) * Fraction(2) ** -30, F32), 0)][k][o]),
        "ADD64": (1, 2, lambda: [enc(Fraction(3, 2) * Fraction(2) ** -1022, F64), enc(-Fraction(2) ** -1022, F64)][o]),
        "FMA64": (1, 3, lambda: [enc(Fraction(2) ** -600, F64), enc(Fraction(3, 2) * Fraction(2) ** -430, F64), 0][o]),
        "ADD16": (1, 2, lambda: [enc(Fraction(3, 2) * Fraction(2) ** -14, F16), enc(-Fraction(2) ** -14, F16)][o] * 0x10001),
        "FMA16": (1, 3, lambda: [enc(Fraction(2) ** -8, F16), enc(Fraction(3, 2) * Fraction(2) ** -8, F16), 0][o] * 0x10001),
        "TIE32": (16, 1, lambda: enc(tie, F32)),
        "TIE64": (16, 1, lambda: enc(tie, F64)),
        "CVTH": (8, 2, lambda: enc(1 + Fraction(2 * k + 1, 1 << 11), F32)),
        "CVTBF": (8, 2, lambda: enc(1 + Fraction(2 * k + 1, 1 << 8), F32)),
        "CVTF8": (8, 2, lambda: enc(1 + Fraction(2 * k + 1, 1 << 4), F32)),
        "CVTBF8": (4, 2, lambda: enc(1 + Fraction(2 * k + 1, 1 << 3), F32)),
        "CVTF4": (2, 2, lambda: enc(1 + Fraction(2 * k + 1, 1 << 2), F32)),
        "CVTD": (8, 1, lambda: enc(1 + Fraction(2 * k + 1, 1 << 24), F64)),
        "I2F": (8, 1, lambda: (1 << 24) + 2 * k + 1),
    }
    if sp not in table:
        return None
    lanes, ops, value = table[sp]
    return value() if k < lanes and o < ops else None


def operands(unit, sidx, seed, r):
    """(a, b, c) of one step and round: three lists of 256 integers (0 for an operand the step has not)."""
    u = UNITS.index(unit)
    _, _, kinds, sp, _ = STEPS_FULL[unit][sidx]
    out = []
    for o, kind in enumerate(kinds):
        if kind is None:
            out.append([0] * 256)
            continue
        h = hashes(seed, u, sidx, r, o)
        h2 = hashes(seed, u, sidx, r, o + 8) if kind in WIDE else [0] * 256
        vals = []
        for t in range(256):
            v = special(sp, o, t & 63) if r == 1 and sp else None
            vals.append(shaped(kind, h[t], h2[t], edge_class(r, o, t)) if v is None else v)
        out.append(vals)
    if sp == "EQ" and r == 1:
        out[1] = [a if t & 1 else b for t, (a, b) in enumerate(zip(out[0], out[1]))]
    return out


def all_keys(rounds=8):
    """Every key a launch hashes (operands 0..2 and their high words 8..10)."""
    out = []
    for u, unit in enumerate(UNITS):
        for s in range(len(STEPS_FULL[unit])):
            for r in range(rounds):
                for o in (0, 1, 2, 8, 9, 10):
                    out.append(key(u, s, r, o))
    return np.concatenate(out)


# --------------------------------------------------------------------- steps
def lo(v):
    return v & M32


def hi(v):
    return (v >> 32) & M32


def h0(v):
    return dec(v & 0xFFFF, F16)


def h1(v):
    return dec((v >> 16) & 0xFFFF, F16)


def fr(v):
    return dec(v & M32, F32)


def fd(v):
    return dec(v & M64, F64)


def np32(fn):
    """A whole-array step on float32 views."""
    def run(a, b, c):
        x, y = (np.array(v, np.uint64).astype(np.uint32).view(np.float32) for v in (a, b))
        with np.errstate(all="ignore"):
            return [int(w) for w in np.asarray(fn(x, y), np.float32).view(np.uint32)]
    run.whole = True
    return run


def np64(fn):
    def run(a, b, c):
        x, y = (np.array(v, np.uint64).view(np.float64) for v in (a, b))
        with np.errstate(all="ignore"):
            return [int(w) for w in np.asarray(fn(x, y), np.float64).view(np.uint64)]
    run.whole = True
    return run


def pk32(fn):
    """A packed-f32 step from the rational function of one element."""
    return lambda a, b, c, t: enc(fn(fr(lo(a)), fr(lo(b)), fr(lo(c))), F32) | enc(fn(fr(hi(a)), fr(hi(b)), fr(hi(c))), F32) << 32


def pk16(fn):
    return lambda a, b, c, t: enc(fn(h0(a), h0(b), h0(c)), F16) | enc(fn(h1(a), h1(b), h1(c)), F16) << 16


def pick(fmt, chooser, n):
    """min / max / median over the first n operands, decoded in `fmt`; the result is the chosen encoding."""
    mask = (1 << (sum(fmt) + 1)) - 1
    return lambda a, b, c, t: chooser(sorted([a & mask, b & mask, c & mask][:n], key=lambda v: dec(v, fmt)))


def frexp_parts(x):
    e = ilog2(abs(x)) + 1
    return x / Fraction(2) ** e, e


def rne(x):
    n = floor(x)
    rem = x - n
    return n + 1 if rem > HALF or (rem == HALF and n & 1) else n


def trunc(x):
    return floor(x) if x >= 0 else ceil(x)


CLASS_ORDER = ["snan", "qnan", "-inf", "-normal", "-subnormal", "-0", "+0", "+subnormal", "+normal", "+inf"]


def fclass(bits, fmt):
    eb, mb = fmt
    s, f, m = bits >> (eb + mb) & 1, (bits >> mb) & ((1 << eb) - 1), bits & ((1 << mb) - 1)
    if f == (1 << eb) - 1:
        name = ("qnan" if m >> (mb - 1) else "snan") if m else "-inf" if s else "+inf"
    else:
        name = ("-" if s else "+") + ("normal" if f else "subnormal" if m else "0")
    return CLASS_ORDER.index(name)


def perm(a, b, sel):
    src = (lo(a) << 32 | lo(b)).to_bytes(8, "little")
    out = 0
    for i in range(4):
        code = (sel >> (8 * i)) & 0xFF
        out |= (src[code] if code < 8 else 0 if code == 12 else 0xFF) << (8 * i)
    return out


def bitop3(tt, bits=32):
    def run(a, b, c, t):
        out = 0
        for i in range(bits):
            out |= (tt >> ((a >> i & 1) << 2 | (b >> i & 1) << 1 | (c >> i & 1)) & 1) << i
        return out
    return run


def bfe_i(a, off, w):
    if w == 0:
        return 0
    return (sx(a, 32) >> off) & M32 if off + w >= 32 else sx(a >> off, w) & M32


def lead(a):
    return 32 - a.bit_length() if a else M32


def halves(a, b, c, fn):
    out = 0
    for i in range(2):
        x, y, z = ((v >> (16 * i)) & 0xFFFF for v in (a, b, c))
        out |= (fn(x, y, z) & 0xFFFF) << (16 * i)
    return out


def dot(a, b, width, signed):
    n = 32 // width
    part = (lambda v, i: sx(v >> (width * i), width)) if signed else (lambda v, i: (v >> (width * i)) & ((1 << width) - 1))
    return sum(part(a, i) * part(b, i) for i in range(n))


def msad(a, b, c):
    """Sum of absolute byte differences on top of c; a zero byte of the reference b masks its term."""
    terms = [((a >> s) & 0xFF, (b >> s) & 0xFF) for s in (0, 8, 16, 24)]
    return (c + sum(abs(x - y) for x, y in terms if y)) & M32


def snorm16(bits):
    """f32 in [-1, 1] to a signed normalised 16-bit integer: x * 32767, to the nearest integer."""
    return rne(fr(bits) * 32767) & 0xFFFF


def fp6_scale(a):
    return enc(Fraction(2) ** ((a >> 32) % 5 - 2), F32)


def fp6_unpack(a, b, c):
    """The 32 f32 encodings of the e2m3 elements packed in c:b:a (element i at bit 6i), times the scale."""
    packed = c << 128 | b << 64 | a
    return [scaled(packed >> (6 * i) & 63, E2M3, fp6_scale(a)) for i in range(32)]


def fp6_fold(a, b, c, t=0):
    r = fp6_unpack(a, b, c)
    x = 0
    for v in r:
        x ^= v
    return x << 32 | sum(v * (2 * i + 1) for i, v in enumerate(r)) & M32


def sat(v, lo_, hi_):
    return max(lo_, min(hi_, v))


def exact_sqrt(x):
    n, d = isqrt(x.numerator), isqrt(x.denominator)
    assert n * n == x.numerator and d * d == x.denominator, x
    return Fraction(n, d)


def exact_log2(x):
    e = ilog2(x)
    assert Fraction(2) ** e == x, x
    return Fraction(e)


QUARTER_SIN = [0, 1, 0, -1]


def cmp_(fmt, op):
    dec_ = (lambda v: v) if fmt is None else (lambda v: dec(v, fmt))
    return lambda a, b, c, t: int(op(dec_(a), dec_(b)))


def bitop_steps(width):
    return [(f"v_bitop3_b{width}:0x{tt:02x}", 1, ("U32", "U32", "U32"), None, bitop3(tt, width))
            for tt in (0x96, 0xE8, 0xF0, 0xCC, 0xAA, 0x1B, 0x2D, 0xCA)]


def fp8_sel(name, kind, fmt):
    return [(f"{name}:{i}", 1, (kind, None, None), None,
             (lambda i: lambda a, b, c, t: widen((a >> (8 * i)) & 0xFF, fmt, F32))(i)) for i in range(4)]


U3 = ("U32", "U32", "U32")
U2 = ("U32", "U32", None)
U1 = ("U32", None, None)
FF = ("F32", "F32", None)
FFF = ("F32", "F32", "F32")
DD = ("F64", "F64", None)
HH2 = ("PKF16", "PKF16", None)
HH3 = ("PKF16", "PKF16", "PKF16")

# (name, result words, operand kinds, special, function). A function takes one
# thread's (a, b, c, t) and returns the result (word 0 in the low half); one
# marked `whole` takes the three lists of 256 and returns the list.
STEPS_FULL = {
    "f32": [
        ("v_add_f32", 1, FF, "ADD32", np32(lambda x, y: x + y)),
        ("v_sub_f32", 1, FF, None, np32(lambda x, y: x - y)),
        ("v_mul_f32", 1, FF, None, np32(lambda x, y: x * y)),
        ("v_fma_f32", 1, FFF, "FMA32", lambda a, b, c, t: enc(fr(a) * fr(b) + fr(c), F32)),
        ("v_pk_add_f32", 2, ("PKF32", "PKF32", None), None, pk32(lambda x, y, z: x + y)),
        ("v_pk_mul_f32", 2, ("PKF32", "PKF32", None), None, pk32(lambda x, y, z: x * y)),
        ("v_pk_fma_f32", 2, ("PKF32", "PKF32", "PKF32"), None, pk32(lambda x, y, z: x * y + z)),
        ("v_min_f32", 1, FF, None, pick(F32, lambda s: s[0], 2)),
        ("v_max_f32", 1, FF, None, pick(F32, lambda s: s[-1], 2)),
        ("v_med3_f32", 1, FFF, None, pick(F32, lambda s: s[1], 3)),
        ("v_min3_f32", 1, FFF, None, pick(F32, lambda s: s[0], 3)),
        ("v_max3_f32", 1, FFF, None, pick(F32, lambda s: s[-1], 3)),
        ("v_minimum3_f32", 1, FFF, None, pick(F32, lambda s: s[0], 3)),
        ("v_maximum3_f32", 1, FFF, None, pick(F32, lambda s: s[-1], 3)),
        ("v_ldexp_f32", 1, ("F32", "I5", None), None, lambda a, b, c, t: enc(fr(a) * Fraction(2) ** sx(b, 32), F32)),
        ("v_frexp_mant_f32", 1, ("F32", None, None), None, lambda a, b, c, t: enc(frexp_parts(fr(a))[0], F32)),
        ("v_frexp_exp_i32_f32", 1, ("F32", None, None), None, lambda a, b, c, t: frexp_parts(fr(a))[1] & M32),
        ("v_fract_f32", 1, ("F32GE1", None, None), None, lambda a, b, c, t: enc(fr(a) - floor(fr(a)), F32)),
        ("v_trunc_f32", 1, ("F32NEAR", None, None), "TIE32",
         lambda a, b, c, t: enc(Fraction(trunc(fr(a))), F32) | (a & 0x80000000)),
        ("v_rndne_f32", 1, ("F32NEAR", None, None), "TIE32",
         lambda a, b, c, t: enc(Fraction(rne(fr(a))), F32) | (a & 0x80000000)),
        ("v_floor_f32", 1, ("F32NEAR", None, None), "TIE32",
         lambda a, b, c, t: enc(Fraction(floor(fr(a))), F32) | (a & 0x80000000)),
        ("v_ceil_f32", 1, ("F32NEAR", None, None), "TIE32",
         lambda a, b, c, t: enc(Fraction(ceil(fr(a))), F32) | (a & 0x80000000)),
        ("v_cmp_lt_f32", 1, FF, "EQ", cmp_(F32, lambda x, y: x < y)),
        ("v_cmp_eq_f32", 1, FF, "EQ", cmp_(F32, lambda x, y: x == y)),
        ("v_cmp_le_f32", 1, FF, "EQ", cmp_(F32, lambda x, y: x <= y)),
        ("v_cmp_gt_f32", 1, FF, "EQ", cmp_(F32, lambda x, y: x > y)),
        ("v_cmp_lg_f32", 1, FF, "EQ", cmp_(F32, lambda x, y: x != y)),
        ("v_cmp_ge_f32", 1, FF, "EQ", cmp_(F32, lambda x, y: x >= y)),
        ("v_cmp_class_f32", 1, ("CLS32", "U32", None), None, lambda a, b, c, t: b >> fclass(a, F32) & 1),
        ("div_f32", 1, FF, None, np32(lambda x, y: x / y)),
        ("sqrt_f32", 1, ("F32P", None, None), None, np32(lambda x, y: np.sqrt(x))),
    ],
    "f64": [
        ("v_add_f64", 2, DD, "ADD64", np64(lambda x, y: x + y)),
        ("v_mul_f64", 2, DD, None, np64(lambda x, y: x * y)),
        ("v_fma_f64", 2, ("F64", "F64", "F64"), "FMA64", lambda a, b, c, t: enc(fd(a) * fd(b) + fd(c), F64)),
        ("v_min_f64", 2, DD, None, pick(F64, lambda s: s[0], 2)),
        ("v_max_f64", 2, DD, None, pick(F64, lambda s: s[-1], 2)),
        ("v_ldexp_f64", 2, ("F64", "I5", None), None, lambda a, b, c, t: enc(fd(a) * Fraction(2) ** sx(b, 32), F64)),
        ("v_frexp_mant_f64", 2, ("F64", None, None), None, lambda a, b, c, t: enc(frexp_parts(fd(a))[0], F64)),
        ("v_frexp_exp_i32_f64", 1, ("F64", None, None), None, lambda a, b, c, t: frexp_parts(fd(a))[1] & M32),
        ("v_fract_f64", 2, ("F64GE1", None, None), None, lambda a, b, c, t: enc(fd(a) - floor(fd(a)), F64)),
        ("v_trunc_f64", 2, ("F64NEAR", None, None), "TIE64", lambda a, b, c, t: enc(Fraction(trunc(fd(a))), F64) | (a & 1 << 63)),
        ("v_rndne_f64", 2, ("F64NEAR", None, None), "TIE64", lambda a, b, c, t: enc(Fraction(rne(fd(a))), F64) | (a & 1 << 63)),
        ("v_floor_f64", 2, ("F64NEAR", None, None), "TIE64", lambda a, b, c, t: enc(Fraction(floor(fd(a))), F64) | (a & 1 << 63)),
        ("v_ceil_f64", 2, ("F64NEAR", None, None), "TIE64", lambda a, b, c, t: enc(Fraction(ceil(fd(a))), F64) | (a & 1 << 63)),
        ("v_cmp_lt_f64", 1, DD, "EQ", cmp_(F64, lambda x, y: x < y)),
        ("v_cmp_eq_f64", 1, DD, "EQ", cmp_(F64, lambda x, y: x == y)),
        ("v_cmp_class_f64", 1, ("CLS64", "U32", None), None, lambda a, b, c, t: b >> fclass(a, F64) & 1),
        ("div_f64", 2, DD, None, np64(lambda x, y: x / y)),
        ("sqrt_f64", 2, ("F64P", None, None), None, np64(lambda x, y: np.sqrt(x))),
    ],
    "f16": [
        ("v_add_f16", 1, HH2, "ADD16", lambda a, b, c, t: enc(h0(a) + h0(b), F16)),
        ("v_mul_f16", 1, HH2, None, lambda a, b, c, t: enc(h0(a) * h0(b), F16)),
        ("v_fma_f16", 1, HH3, "FMA16", lambda a, b, c, t: enc(h0(a) * h0(b) + h0(c), F16)),
        ("v_pk_add_f16", 1, HH2, "ADD16", pk16(lambda x, y, z: x + y)),
        ("v_pk_mul_f16", 1, HH2, None, pk16(lambda x, y, z: x * y)),
        ("v_pk_fma_f16", 1, HH3, "FMA16", pk16(lambda x, y, z: x * y + z)),
        ("v_pk_min_f16", 1, HH2, None, pk16(lambda x, y, z: min(x, y))),
        ("v_pk_max_f16", 1, HH2, None, pk16(lambda x, y, z: max(x, y))),
        ("v_pk_minimum3_f16", 1, HH3, None, pk16(min)),
        ("v_pk_maximum3_f16", 1, HH3, None, pk16(max)),
        # a, b are f16 (the low half of a, the high half of b), c is f32; one rounding, to f32.
        ("v_fma_mix_f32", 1, ("PKF16", "PKF16", "F32"), None, lambda a, b, c, t: enc(h0(a) * h1(b) + fr(c), F32)),
        # all three f16 (the high half of a); the FMA rounds to f32, the result to f16.
        ("v_fma_mixlo_f16", 1, HH3, None, lambda a, b, c, t: enc(dec(enc(h1(a) * h0(b) + h0(c), F32), F32), F16)),
    ],
    "int": [
        ("v_mul_lo_u32", 1, U2, None, lambda a, b, c, t: a * b & M32),
        ("v_mul_hi_u32", 1, U2, None, lambda a, b, c, t: a * b >> 32),
        ("v_mul_hi_i32", 1, U2, None, lambda a, b, c, t: (sx(a, 32) * sx(b, 32) >> 32) & M32),
        ("v_mad_u64_u32", 2, ("U32", "U32", "U64"), None, lambda a, b, c, t: (a * b + c) & M64),
        ("v_mad_i64_i32", 2, ("U32", "U32", "U64"), None, lambda a, b, c, t: (sx(a, 32) * sx(b, 32) + c) & M64),
        ("v_mul_u32_u24", 1, U2, None, lambda a, b, c, t: (a & 0xFFFFFF) * (b & 0xFFFFFF) & M32),
        ("v_mul_hi_u32_u24", 1, U2, None, lambda a, b, c, t: (a & 0xFFFFFF) * (b & 0xFFFFFF) >> 32),
        ("v_mad_u32_u24", 1, U3, None, lambda a, b, c, t: ((a & 0xFFFFFF) * (b & 0xFFFFFF) + c) & M32),
        ("v_mad_i32_i24", 1, U3, None, lambda a, b, c, t: (sx(a, 24) * sx(b, 24) + c) & M32),
        ("v_mad_u32_u16", 1, U3, None, lambda a, b, c, t: ((a & 0xFFFF) * (b & 0xFFFF) + c) & M32),
        ("v_pk_add_u16", 1, U2, None, lambda a, b, c, t: halves(a, b, c, lambda x, y, z: x + y)),
        ("v_pk_mad_i16", 1, U3, None, lambda a, b, c, t: halves(a, b, c, lambda x, y, z: sx(x, 16) * sx(y, 16) + sx(z, 16))),
        ("v_pk_mul_lo_u16", 1, U2, None, lambda a, b, c, t: halves(a, b, c, lambda x, y, z: x * y)),
        ("v_pk_min_i16", 1, U2, None, lambda a, b, c, t: halves(a, b, c, lambda x, y, z: min(sx(x, 16), sx(y, 16)))),
        ("v_pk_max_u16", 1, U2, None, lambda a, b, c, t: halves(a, b, c, lambda x, y, z: max(x, y))),
        ("v_pk_lshlrev_b16", 1, U2, None, lambda a, b, c, t: halves(a, b, c, lambda x, y, z: y << (x & 15))),
        ("v_pk_ashrrev_i16", 1, U2, None, lambda a, b, c, t: halves(a, b, c, lambda x, y, z: sx(y, 16) >> (x & 15))),
        # x = c:a, y = b:b as 128-bit numbers; the result is the high 64 bits.
        ("add128", 2, ("U64", "U64", "U64"), None, lambda a, b, c, t: ((c << 64 | a) + (b << 64 | b)) >> 64 & M64),
        ("sub128", 2, ("U64", "U64", "U64"), None, lambda a, b, c, t: ((c << 64 | a) - (b << 64 | b)) >> 64 & M64),
        ("v_add3_u32", 1, U3, None, lambda a, b, c, t: (a + b + c) & M32),
        ("v_lshl_add_u32", 1, U3, None, lambda a, b, c, t: ((a << (b & 31)) + c) & M32),
        ("v_xad_u32", 1, U3, None, lambda a, b, c, t: ((a ^ b) + c) & M32),
        ("v_lshl_add_u64", 2, ("U64", "SH4", "U64"), None, lambda a, b, c, t: ((a << b) + c) & M64),
        ("v_lshlrev_b64", 2, ("U32", "U64", None), None, lambda a, b, c, t: (b << (a & 63)) & M64),
        ("v_lshrrev_b64", 2, ("U32", "U64", None), None, lambda a, b, c, t: b >> (a & 63)),
        ("v_ashrrev_i64", 2, ("U32", "U64", None), None, lambda a, b, c, t: (sx(b, 64) >> (a & 63)) & M64),
        ("v_sad_u8", 1, U3, None,
         lambda a, b, c, t: (c + sum(abs((a >> s & 0xFF) - (b >> s & 0xFF)) for s in (0, 8, 16, 24))) & M32),
        ("v_msad_u8", 1, U3, None, lambda a, b, c, t: msad(a, b, c)),
        ("v_cmp_lt_u64", 1, ("U64", "U64", None), "EQ", cmp_(None, lambda x, y: x < y)),
        ("v_cmp_ge_i32", 1, U2, "EQ", lambda a, b, c, t: int(sx(a, 32) >= sx(b, 32))),
    ],
    "bit": [
        ("v_perm_b32", 1, ("U32", "U32", "PERMSEL"), None, lambda a, b, c, t: perm(a, b, c)),
        ("v_alignbit_b32", 1, U3, None, lambda a, b, c, t: ((a << 32 | b) >> (c & 31)) & M32),
        ("v_alignbyte_b32", 1, U3, None, lambda a, b, c, t: ((a << 32 | b) >> (8 * (c & 3))) & M32),
        ("v_bfe_u32", 1, U3, None, lambda a, b, c, t: (a >> (b & 31)) & ((1 << (c & 31)) - 1)),
        ("v_bfe_i32", 1, U3, None, lambda a, b, c, t: bfe_i(a, b & 31, c & 31)),
        ("v_bfi_b32", 1, U3, None, lambda a, b, c, t: (a & b) | (~a & c & M32)),
        *bitop_steps(32),
        *bitop_steps(16),
        ("v_and_or_b32", 1, U3, None, lambda a, b, c, t: (a & b) | c),
        ("v_lshl_or_b32", 1, U3, None, lambda a, b, c, t: ((a << (b & 31)) & M32) | c),
        ("v_bfrev_b32", 1, U1, None, lambda a, b, c, t: int(f"{a:032b}"[::-1], 2)),
        ("v_ffbh_u32", 1, U1, None, lambda a, b, c, t: lead(a)),
        ("v_ffbl_b32", 1, U1, None, lambda a, b, c, t: (a & -a).bit_length() - 1 if a else M32),
        ("v_ffbh_i32", 1, U1, None, lambda a, b, c, t: lead(a ^ (M32 if a >> 31 else 0))),
        ("v_bcnt_u32_b32", 1, U2, None, lambda a, b, c, t: (bin(a).count("1") + b) & M32),
        ("v_mbcnt_lo_u32_b32", 1, U2, None, lambda a, b, c, t: (bin(a & ((1 << (t & 63)) - 1) & M32).count("1") + b) & M32),
        ("v_mbcnt_hi_u32_b32", 1, U2, None, lambda a, b, c, t: (bin(a & ((1 << (t & 63)) - 1) >> 32).count("1") + b) & M32),
    ],
    "dot": [
        ("v_dot2_f32_f16", 1, ("PKSI16", "PKSI16", "SIF32"), None,
         lambda a, b, c, t: enc(h0(a) * h0(b) + h1(a) * h1(b) + fr(c), F32)),
        ("v_dot2_f32_bf16", 1, ("PKSIBF", "PKSIBF", "SIF32"), None,
         lambda a, b, c, t: enc(dec(a & 0xFFFF, BF16) * dec(b & 0xFFFF, BF16)
                                + dec(a >> 16, BF16) * dec(b >> 16, BF16) + fr(c), F32)),
        ("v_dot2c_f32_bf16", 1, ("PKSIBF", "PKSIBF", "SIF32"), None,
         lambda a, b, c, t: enc(dec(a & 0xFFFF, BF16) * dec(b & 0xFFFF, BF16)
                                + dec(a >> 16, BF16) * dec(b >> 16, BF16) + fr(c), F32)),
        ("v_dot4_i32_i8", 1, U3, None, lambda a, b, c, t: (dot(a, b, 8, True) + c) & M32),
        ("v_dot4_u32_u8", 1, U3, None, lambda a, b, c, t: (dot(a, b, 8, False) + c) & M32),
        ("v_dot8_i32_i4", 1, U3, None, lambda a, b, c, t: (dot(a, b, 4, True) + c) & M32),
        ("v_dot8_u32_u4", 1, U3, None, lambda a, b, c, t: (dot(a, b, 4, False) + c) & M32),
    ],
    "cvt": [
        ("v_cvt_f32_i32", 1, U1, "I2F", lambda a, b, c, t: enc(Fraction(sx(a, 32)), F32)),
        ("v_cvt_f32_u32", 1, U1, "I2F", lambda a, b, c, t: enc(Fraction(a), F32)),
        ("v_cvt_i32_f32", 1, ("F32INT", None, None), "TIE32", lambda a, b, c, t: trunc(fr(a)) & M32),
        ("v_cvt_u32_f32", 1, ("F32UINT", None, None), None, lambda a, b, c, t: trunc(fr(a)) & M32),
        ("v_cvt_rpi_i32_f32", 1, ("F32INT", None, None), "TIE32", lambda a, b, c, t: floor(fr(a) + HALF) & M32),
        ("v_cvt_flr_i32_f32", 1, ("F32INT", None, None), "TIE32", lambda a, b, c, t: floor(fr(a)) & M32),
        ("v_cvt_f64_f32", 2, ("F32", None, None), None, lambda a, b, c, t: enc(fr(a), F64)),
        ("v_cvt_f32_f64", 1, ("F64", None, None), "CVTD", lambda a, b, c, t: enc(fd(a), F32)),
        ("v_cvt_f64_i32", 2, U1, None, lambda a, b, c, t: enc(Fraction(sx(a, 32)), F64)),
        ("v_cvt_i32_f64", 1, ("F64INT", None, None), "TIE64", lambda a, b, c, t: trunc(fd(a)) & M32),
        *[(f"v_cvt_f32_ubyte{i}", 1, U1, None, (lambda i: lambda a, b, c, t: f32_of_int(a >> (8 * i) & 0xFF))(i))
          for i in range(4)],
        ("v_cvt_pk_u8_f32", 1, ("F32B", "U32", "U32"), None,
         lambda a, b, c, t: (c & ~(0xFF << (8 * (b & 3))) & M32) | int(fr(a)) << (8 * (b & 3))),
        ("v_cvt_f16_f32", 1, ("F32H", None, None), "CVTH", lambda a, b, c, t: enc(fr(a), F16)),
        ("v_cvt_f32_f16", 1, ("PKF16", None, None), None, lambda a, b, c, t: enc(h0(a), F32)),
        ("v_cvt_pk_f16_f32", 1, ("F32H", "F32H", None), "CVTH", lambda a, b, c, t: enc(fr(a), F16) | enc(fr(b), F16) << 16),
        ("v_cvt_pkrtz_f16_f32", 1, ("F32H", "F32H", None), "CVTH",
         lambda a, b, c, t: enc(fr(a), F16, True) | enc(fr(b), F16, True) << 16),
        ("v_cvt_pk_bf16_f32", 1, FF, "CVTBF", lambda a, b, c, t: enc(fr(a), BF16) | enc(fr(b), BF16) << 16),
        ("v_cvt_pk_i16_i32", 1, U2, None,
         lambda a, b, c, t: (sat(sx(a, 32), -32768, 32767) & 0xFFFF) | (sat(sx(b, 32), -32768, 32767) & 0xFFFF) << 16),
        ("v_cvt_pk_u16_u32", 1, U2, None, lambda a, b, c, t: min(a, 0xFFFF) | min(b, 0xFFFF) << 16),
        ("v_cvt_pknorm_i16_f32", 1, ("F32N8", "F32N8", None), None, lambda a, b, c, t: snorm16(a) | snorm16(b) << 16),
        ("v_ashr_pk_i8_i32", 1, U3, None,
         lambda a, b, c, t: (sat(sx(a, 32) >> (c & 31), -128, 127) & 0xFF) | (sat(sx(b, 32) >> (c & 31), -128, 127) & 0xFF) << 8),
        ("v_ashr_pk_u8_i32", 1, U3, None,
         lambda a, b, c, t: sat(sx(a, 32) >> (c & 31), 0, 255) | sat(sx(b, 32) >> (c & 31), 0, 255) << 8),
        ("v_cvt_pk_fp8_f32", 1, ("F32Q", "F32Q", None), "CVTF8", lambda a, b, c, t: enc(fr(a), E4M3) | enc(fr(b), E4M3) << 8),
        ("v_cvt_pk_bf8_f32", 1, ("F32Q", "F32Q", None), "CVTBF8", lambda a, b, c, t: enc(fr(a), E5M2) | enc(fr(b), E5M2) << 8),
        *fp8_sel("v_cvt_f32_fp8", "FP8", E4M3),
        *fp8_sel("v_cvt_f32_bf8", "BF8", E5M2),
        ("v_cvt_pk_f32_fp8", 2, ("FP8", None, None), None,
         lambda a, b, c, t: widen(a & 0xFF, E4M3, F32) | widen(a >> 8 & 0xFF, E4M3, F32) << 32),
        ("v_cvt_scalef32_pk_fp8_f32", 1, ("F32QS", "F32QS", "SCALE3"), "CVTF8",
         lambda a, b, c, t: enc(fr(a) / fr(c), E4M3) | enc(fr(b) / fr(c), E4M3) << 8),
        ("v_cvt_scalef32_pk_f32_fp8", 2, ("FP8", "SCALE3", None), None,
         lambda a, b, c, t: scaled(a & 0xFF, E4M3, b) | scaled(a >> 8 & 0xFF, E4M3, b) << 32),
        ("v_cvt_scalef32_pk_fp4_f32", 1, ("F32F4", "F32F4", "SCALE1"), "CVTF4",
         lambda a, b, c, t: enc(fr(a) / fr(c), E2M1) | enc(fr(b) / fr(c), E2M1) << 4),
        ("v_cvt_scalef32_pk_f32_fp4", 2, ("U32", "SCALE1", None), None,
         lambda a, b, c, t: scaled(a & 15, E2M1, b) | scaled(a >> 4 & 15, E2M1, b) << 32),
        # 32 results a lane, folded to two words: sum r_i (2i + 1), and the XOR of all r_i.
        ("v_cvt_scalef32_pk32_f32_fp6", 2, ("U64", "U64", "U64"), None, fp6_fold),
    ],
    "trans": [
        ("v_exp_f32", 1, ("EXPI", None, None), None, lambda a, b, c, t: enc(Fraction(2) ** int(fr(a)), F32)),
        ("v_log_f32", 1, ("POW4F32", None, None), None, lambda a, b, c, t: enc(exact_log2(fr(a)), F32)),
        ("v_rcp_f32", 1, ("POW2F32", None, None), None, lambda a, b, c, t: enc(1 / fr(a), F32)),
        ("v_rsq_f32", 1, ("POW4F32", None, None), None, lambda a, b, c, t: enc(1 / exact_sqrt(fr(a)), F32)),
        ("v_sqrt_f32:4^n", 1, ("POW4F32", None, None), None, lambda a, b, c, t: enc(exact_sqrt(fr(a)), F32)),
        ("v_sqrt_f32:k^2", 1, ("SQINT", None, None), None, lambda a, b, c, t: enc(exact_sqrt(fr(a)), F32)),
        ("v_sin_f32", 1, ("QREV", None, None), None, lambda a, b, c, t: enc(Fraction(QUARTER_SIN[int(fr(a) * 4) & 3]), F32)),
        ("v_cos_f32", 1, ("QREV", None, None), None,
         lambda a, b, c, t: enc(Fraction(QUARTER_SIN[(int(fr(a) * 4) + 1) & 3]), F32)),
        ("v_rcp_f64", 2, ("POW2F64", None, None), None, lambda a, b, c, t: enc(1 / fd(a), F64)),
        ("v_rsq_f64", 2, ("POW4F64", None, None), None, lambda a, b, c, t: enc(1 / exact_sqrt(fd(a)), F64)),
        ("v_rcp_f16", 1, ("POW2F16", None, None), None, lambda a, b, c, t: enc(1 / h0(a), F16)),
        ("v_rsq_f16", 1, ("POW4F16", None, None), None, lambda a, b, c, t: enc(1 / exact_sqrt(h0(a)), F16)),
        ("v_sqrt_f16", 1, ("POW4F16", None, None), None, lambda a, b, c, t: enc(exact_sqrt(h0(a)), F16)),
        ("v_exp_f16", 1, ("EXPIF16", None, None), None, lambda a, b, c, t: enc(Fraction(2) ** int(h0(a)), F16)),
        ("v_log_f16", 1, ("POW4F16", None, None), None, lambda a, b, c, t: enc(exact_log2(h0(a)), F16)),
    ],
}

STEPS = {u: [s[0] for s in v] for u, v in STEPS_FULL.items()}
SHAPES = {u: (len(v), sum(s[1] for s in v)) for u, v in STEPS_FULL.items()}  # (steps, result words per round)


def step_values(unit, sidx, seed, r):
    """The results of one step and round: 256 integers (word 0 in the low half)."""
    _, _, _, _, fn = STEPS_FULL[unit][sidx]
    a, b, c = operands(unit, sidx, seed, r)
    if getattr(fn, "whole", False):
        return fn(a, b, c)
    return [fn(a[t], b[t], c[t], t) for t in range(256)]


@lru_cache(maxsize=None)
def _round(unit, seed, r):
    rows = []
    for sidx, (_, words, _, _, _) in enumerate(STEPS_FULL[unit]):
        v = step_values(unit, sidx, seed, r)
        for w in range(words):
            rows.append([x >> (32 * w) & M32 for x in v])
    out = np.array(rows, np.uint32)
    out.setflags(write=False)
    return out


def expected(unit, seed, rounds):
    """uint32 [rounds, words, 256]: what a healthy SIMD returns."""
    return np.stack([_round(unit, seed, r) for r in range(rounds)])


def digest_of(values):
    """D = sum got * (2 idx + 1) mod 2^32 over the flattened [round][row][256]."""
    v = np.asarray(values, np.uint64).reshape(-1)
    idx = np.arange(v.size, dtype=np.uint64)
    return int(((v * (2 * idx + 1)) & M32).sum() & M32)


def digest(unit, seed, rounds):
    return digest_of(expected(unit, seed, rounds))


def row_names(unit):
    """(step name, word) of every row of the unit."""
    return [(name, w) for name, words, _, _, _ in STEPS_FULL[unit] for w in range(words)]
