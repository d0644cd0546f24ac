"""Reference for the scalar sweep (csrc/hip/scalar_sweep.hip): what every thread
of a healthy CU must hold after every step, from the ISA's definition of each
instruction. Python integers and numpy only; nothing here comes from the C++.

Layout. A workgroup is 1,024 threads, thread t = 64 x wave + lane. A part's
words are [word][1024]; a looped step contributes its result words (low word
first) and then the SCC it left, a mask step D, the active lanes, SCC and the
first active lane, a lane step its result words alone.

Operands. h(p, s, w, o, l) = fmix32(seed ^ (p << 28 | s << 20 | w << 14 |
o << 8 | l)); o: 0 a0, 1 a1, 2 b0, 3 b1, 4 c (bit 0). Lanes 0..15 are edge
lanes: k = 16 w + l crosses EDGE over a0 (k % 5), b0 (k // 5 % 5, from the
table of the step's kind), a1 (k // 25 % 5) and b1 (k // 125).

Rules (GFX9 / CDNA ISA), as implemented below:
  * shift counts and bit numbers take 5 bits in the 32-bit forms, 6 in the 64-bit forms;
  * s_bfe: offset = S1[4:0] (S1[5:0] for 64 bits), width = S1[22:16]; a width
    of 0 gives 0; a field that runs past the top ends at the top; the signed
    forms extend the field's last bit;
  * s_ff1 / s_ff0 / s_flbit of a value without such a bit give -1, and so does
    the signed s_flbit_i32 of 0 and of -1;
  * s_abs_i32 of 0x80000000 is 0x80000000;
  * SCC: carry (add_u32, addc), borrow (sub_u32, subb), signed overflow
    (add_i32, sub_i32, addk_i32), "the first operand was chosen" (min, max;
    strict), result non-zero (logic, shifts, bfe, wqm, quadmask, bcnt, not,
    abs, absdiff), unchanged otherwise;
  * s_wqm: a quad with any bit set becomes 1111; s_quadmask: bit q of the
    result is the OR of quad q.
"""
import numpy as np

PARTS = ["arith", "logic", "bits", "cmp", "branch", "mask", "movrel", "sgpr"]
SEEDS = (0x1B873593, 0x5EED1E55)
BLOCK = 1024
M32 = 0xFFFFFFFF
M64 = 0xFFFFFFFFFFFFFFFF
EDGE = (0, 1, 0xFFFFFFFF, 0x80000000, 0x7FFFFFFF)
EDGE_SHIFT = (0, 31, 32, 63, 1)
EDGE_FIELD = (0x00000000, 0x0020001F, 0x00400000, 0x007F0020, 0x0001001F)
KIND = {"val": EDGE, "sh": EDGE_SHIFT, "bfe": EDGE_FIELD}
IMMS = (0x7FFF, 0x8000, 1, 0xFFFF)


# ------------------------------------------------------------------ operands
def fmix32(h):
    """murmur3's finaliser over an array of uint64 holding 32-bit values."""
    h = h & M32
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & M32
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & M32
    h ^= h >> 16
    return h


_T = np.arange(BLOCK, dtype=np.uint64)


def hashv(seed, p, s, o):
    """h(p, s, wave, o, lane) of all 1,024 threads, as Python ints."""
    key = (p << 28) | (s << 20) | (o << 8)
    return [int(v) for v in fmix32(np.uint64(seed) ^ (np.uint64(key) | ((_T >> 6) << 14) | (_T & 63)))]


def operands(seed, p, s, kind):
    """Per thread (a0, a1, b0, b1, c)."""
    a0, a1, b0, b1 = (hashv(seed, p, s, o) for o in range(4))
    c = [v & 1 for v in hashv(seed, p, s, 4)]
    for t in range(BLOCK):
        w, l = divmod(t, 64)
        if l < 16:
            k = 16 * w + l
            a0[t] = EDGE[k % 5]
            b0[t] = KIND[kind][k // 5 % 5]
            a1[t] = EDGE[k // 25 % 5]
            b1[t] = EDGE[k // 125]
    return list(zip(a0, a1, b0, b1, c))


# ------------------------------------------------------------- ISA, by hand
def s32(v):
    v &= M32
    return v - (1 << 32) if v >> 31 else v


def s64(v):
    v &= M64
    return v - (1 << 64) if v >> 63 else v


def sext(v, bits):
    v &= (1 << bits) - 1
    return v - (1 << bits) if v >> (bits - 1) else v


def nz(d):
    return 1 if d else 0


def add_carry(a, b, cin=0):
    r = a + b + cin
    return r & M32, r >> 32


def sub_borrow(a, b, cin=0):
    r = a - b - cin
    return r & M32, 1 if r < 0 else 0


def add_signed(a, b):
    r = s32(a) + s32(b)
    return r & M32, 0 if -(1 << 31) <= r < (1 << 31) else 1


def sub_signed(a, b):
    r = s32(a) - s32(b)
    return r & M32, 0 if -(1 << 31) <= r < (1 << 31) else 1


def absdiff(a, b):
    d = (a - b) & M32  # D.i = S0.i - S1.i in 32 bits
    if d >> 31:
        d = (-d) & M32
    return d


def abs32(a):
    return (-s32(a)) & M32 if a >> 31 else a


def bfe(src, ctl, bits, signed):
    off = ctl & (bits - 1)
    width = (ctl >> 16) & 0x7F
    width = min(width, bits - off)
    if width == 0:
        return 0
    field = (src >> off) & ((1 << width) - 1)
    if signed:
        field = sext(field, width)
    return field & ((1 << bits) - 1)


def brev(a, bits):
    return int(format(a, "0%db" % bits)[::-1], 2)


def wqm(a, bits):
    r = 0
    for q in range(bits // 4):
        if (a >> (4 * q)) & 0xF:
            r |= 0xF << (4 * q)
    return r


def quadmask(a, bits):
    r = 0
    for q in range(bits // 4):
        if (a >> (4 * q)) & 0xF:
            r |= 1 << q
    return r


def ones(a):
    return bin(a).count("1")


def ff1(a, bits):
    for i in range(bits):
        if (a >> i) & 1:
            return i
    return M32


def ff0(a, bits):
    return ff1(~a & ((1 << bits) - 1), bits)


def flbit(a, bits):
    for i in range(bits):
        if (a >> (bits - 1 - i)) & 1:
            return i
    return M32


def flbit_signed(a, bits):
    sign = (a >> (bits - 1)) & 1
    for i in range(1, bits):
        if ((a >> (bits - 1 - i)) & 1) != sign:
            return i
    return M32


def bitreplicate(a):
    r = 0
    for i in range(32):
        if (a >> i) & 1:
            r |= 3 << (2 * i)
    return r


def u64(lo, hi):
    return lo | hi << 32


def words(v, n=2):
    return tuple((v >> (32 * i)) & M32 for i in range(n))


# ------------------------------------------------------------------ the steps
# A looped step: fn(a0, a1, b0, b1, c) -> (result words..., SCC). `scc_in` is c.
STEPS = []  # (part, name, class, kind, fn)


def step(part, name, kind="val", cls="loop"):
    def deco(fn):
        STEPS.append((part, name, cls, kind, fn))
        return fn
    return deco


def loop1(part, name, fn, kind="val"):
    """A 32-bit step: fn(a0, b0, c) -> (d, scc or None: unchanged)."""
    def run(a0, a1, b0, b1, c):
        d, scc = fn(a0, b0, c)
        return d & M32, c if scc is None else scc
    STEPS.append((part, name, "loop", kind, run))


def loop2(part, name, fn, kind="val"):
    """A step on 64-bit operands: fn(a, b, b0, c) -> (d64, scc or None)."""
    def run(a0, a1, b0, b1, c):
        d, scc = fn(u64(a0, a1), u64(b0, b1), b0, c)
        return (d & M32, (d >> 32) & M32, c if scc is None else scc)
    STEPS.append((part, name, "loop", kind, run))


def scc_only(part, name, fn, kind="val"):
    """fn(a0, a1, b0, b1) -> SCC."""
    STEPS.append((part, name, "loop", kind, lambda a0, a1, b0, b1, c: (1 if fn(a0, a1, b0, b1) else 0,)))


# arith
loop1(0, "s_add_u32", lambda a, b, c: add_carry(a, b))
loop1(0, "s_sub_u32", lambda a, b, c: sub_borrow(a, b))
loop1(0, "s_add_i32", lambda a, b, c: add_signed(a, b))
loop1(0, "s_sub_i32", lambda a, b, c: sub_signed(a, b))
loop1(0, "s_addc_u32", lambda a, b, c: add_carry(a, b, c))
loop1(0, "s_subb_u32", lambda a, b, c: sub_borrow(a, b, c))


def chain_operands(a0, a1, b0, b1):
    """The 128-bit operands of the carry chain: X = b1:b0:a1:a0, Y = a1:a0:b1:b0."""
    return a0 | a1 << 32 | b0 << 64 | b1 << 96, b0 | b1 << 32 | a0 << 64 | a1 << 96


@step(0, "add128")
def _add128(a0, a1, b0, b1, c):
    x, y = chain_operands(a0, a1, b0, b1)
    r = x + y
    return words(r, 4) + (r >> 128,)


@step(0, "sub128")
def _sub128(a0, a1, b0, b1, c):
    x, y = chain_operands(a0, a1, b0, b1)
    r = x - y
    return words(r & ((1 << 128) - 1), 4) + (1 if r < 0 else 0,)


loop1(0, "s_min_i32", lambda a, b, c: (a, 1) if s32(a) < s32(b) else (b, 0))
loop1(0, "s_min_u32", lambda a, b, c: (a, 1) if a < b else (b, 0))
loop1(0, "s_max_i32", lambda a, b, c: (a, 1) if s32(a) > s32(b) else (b, 0))
loop1(0, "s_max_u32", lambda a, b, c: (a, 1) if a > b else (b, 0))
loop1(0, "s_absdiff_i32", lambda a, b, c: (absdiff(a, b), nz(absdiff(a, b))))
loop1(0, "s_abs_i32", lambda a, b, c: (abs32(a), nz(abs32(a))))
loop1(0, "s_mul_i32", lambda a, b, c: (a * b, None))
loop1(0, "s_mul_hi_u32", lambda a, b, c: ((a * b) >> 32, None))
loop1(0, "s_mul_hi_i32", lambda a, b, c: ((s32(a) * s32(b)) >> 32, None))
for _n in (1, 2, 3, 4):
    loop1(0, "s_lshl%d_add_u32" % _n, lambda a, b, c, n=_n: (((a << n) + b) & M32, ((a << n) + b) >> 32 != 0))
for _imm in IMMS:
    loop1(0, "s_addk_i32", lambda a, b, c, k=_imm: add_signed(a, sext(k, 16) & M32))
    loop1(0, "s_mulk_i32", lambda a, b, c, k=_imm: (s32(a) * sext(k, 16), None))

# logic
for _name, _fn in (("and", lambda a, b: a & b), ("or", lambda a, b: a | b), ("xor", lambda a, b: a ^ b),
                   ("andn2", lambda a, b: a & ~b), ("orn2", lambda a, b: a | ~b), ("nand", lambda a, b: ~(a & b)),
                   ("nor", lambda a, b: ~(a | b)), ("xnor", lambda a, b: ~(a ^ b))):
    loop1(1, "s_%s_b32" % _name, lambda a, b, c, f=_fn: (f(a, b) & M32, nz(f(a, b) & M32)))
    loop2(1, "s_%s_b64" % _name, lambda a, b, b0, c, f=_fn: (f(a, b) & M64, nz(f(a, b) & M64)))
loop1(1, "s_not_b32", lambda a, b, c: (~a & M32, nz(~a & M32)))
loop2(1, "s_not_b64", lambda a, b, b0, c: (~a & M64, nz(~a & M64)))
loop1(1, "s_lshl_b32", lambda a, b, c: ((a << (b & 31)) & M32, nz((a << (b & 31)) & M32)), "sh")
loop1(1, "s_lshr_b32", lambda a, b, c: (a >> (b & 31), nz(a >> (b & 31))), "sh")
loop1(1, "s_ashr_i32", lambda a, b, c: ((s32(a) >> (b & 31)) & M32, nz((s32(a) >> (b & 31)) & M32)), "sh")
loop2(1, "s_lshl_b64", lambda a, b, b0, c: ((a << (b0 & 63)) & M64, nz((a << (b0 & 63)) & M64)), "sh")
loop2(1, "s_lshr_b64", lambda a, b, b0, c: (a >> (b0 & 63), nz(a >> (b0 & 63))), "sh")
loop2(1, "s_ashr_i64", lambda a, b, b0, c: ((s64(a) >> (b0 & 63)) & M64, nz((s64(a) >> (b0 & 63)) & M64)), "sh")
loop1(1, "s_bfm_b32", lambda a, b, c: ((((1 << (a & 31)) - 1) << (b & 31)) & M32, None), "sh")
STEPS.append((1, "s_bfm_b64", "loop", "sh",
              lambda a0, a1, b0, b1, c: words((((1 << (a0 & 63)) - 1) << (b0 & 63)) & M64) + (c,)))
loop1(1, "s_bfe_u32", lambda a, b, c: (bfe(a, b, 32, False), nz(bfe(a, b, 32, False))), "bfe")
loop1(1, "s_bfe_i32", lambda a, b, c: (bfe(a, b, 32, True), nz(bfe(a, b, 32, True))), "bfe")
loop2(1, "s_bfe_u64", lambda a, b, b0, c: (bfe(a, b0, 64, False), nz(bfe(a, b0, 64, False))), "bfe")
loop2(1, "s_bfe_i64", lambda a, b, b0, c: (bfe(a, b0, 64, True), nz(bfe(a, b0, 64, True))), "bfe")
loop1(1, "s_pack_ll_b32_b16", lambda a, b, c: ((a & 0xFFFF) | (b & 0xFFFF) << 16, None))
loop1(1, "s_pack_lh_b32_b16", lambda a, b, c: ((a & 0xFFFF) | (b >> 16) << 16, None))
loop1(1, "s_pack_hh_b32_b16", lambda a, b, c: ((a >> 16) | (b >> 16) << 16, None))

# bits
loop1(2, "s_brev_b32", lambda a, b, c: (brev(a, 32), None))
loop2(2, "s_brev_b64", lambda a, b, b0, c: (brev(a, 64), None))
loop1(2, "s_wqm_b32", lambda a, b, c: (wqm(a, 32), nz(wqm(a, 32))))
loop2(2, "s_wqm_b64", lambda a, b, b0, c: (wqm(a, 64), nz(wqm(a, 64))))
loop1(2, "s_quadmask_b32", lambda a, b, c: (quadmask(a, 32), nz(quadmask(a, 32))))
loop2(2, "s_quadmask_b64", lambda a, b, b0, c: (quadmask(a, 64), nz(quadmask(a, 64))))


def from64(part, name, fn):
    """A 32-bit result of a 64-bit source: fn(a) -> (d, scc or None)."""
    def run(a0, a1, b0, b1, c):
        d, scc = fn(u64(a0, a1))
        return d & M32, c if scc is None else scc
    STEPS.append((part, name, "loop", "val", run))


loop1(2, "s_bcnt0_i32_b32", lambda a, b, c: (32 - ones(a), nz(32 - ones(a))))
from64(2, "s_bcnt0_i32_b64", lambda a: (64 - ones(a), nz(64 - ones(a))))
loop1(2, "s_bcnt1_i32_b32", lambda a, b, c: (ones(a), nz(ones(a))))
from64(2, "s_bcnt1_i32_b64", lambda a: (ones(a), nz(ones(a))))
loop1(2, "s_ff0_i32_b32", lambda a, b, c: (ff0(a, 32), None))
from64(2, "s_ff0_i32_b64", lambda a: (ff0(a, 64), None))
loop1(2, "s_ff1_i32_b32", lambda a, b, c: (ff1(a, 32), None))
from64(2, "s_ff1_i32_b64", lambda a: (ff1(a, 64), None))
loop1(2, "s_flbit_i32_b32", lambda a, b, c: (flbit(a, 32), None))
from64(2, "s_flbit_i32_b64", lambda a: (flbit(a, 64), None))
loop1(2, "s_flbit_i32", lambda a, b, c: (flbit_signed(a, 32), None))
from64(2, "s_flbit_i32_i64", lambda a: (flbit_signed(a, 64), None))
loop1(2, "s_sext_i32_i8", lambda a, b, c: (sext(a, 8), None))
loop1(2, "s_sext_i32_i16", lambda a, b, c: (sext(a, 16), None))
# the destination starts as b; the bit number is a0
loop1(2, "s_bitset0_b32", lambda a, b, c: (b & ~(1 << (a & 31)), None))
STEPS.append((2, "s_bitset0_b64", "loop", "val",
              lambda a0, a1, b0, b1, c: words(u64(b0, b1) & ~(1 << (a0 & 63))) + (c,)))
loop1(2, "s_bitset1_b32", lambda a, b, c: (b | 1 << (a & 31), None))
STEPS.append((2, "s_bitset1_b64", "loop", "val",
              lambda a0, a1, b0, b1, c: words(u64(b0, b1) | 1 << (a0 & 63)) + (c,)))
STEPS.append((2, "s_bitreplicate_b64_b32", "loop", "val", lambda a0, a1, b0, b1, c: words(bitreplicate(a0)) + (c,)))

# cmp
_CMP = (("eq", lambda x, y: x == y), ("lg", lambda x, y: x != y), ("gt", lambda x, y: x > y),
        ("ge", lambda x, y: x >= y), ("lt", lambda x, y: x < y), ("le", lambda x, y: x <= y))
for _name, _fn in _CMP:
    scc_only(3, "s_cmp_%s_i32" % _name, lambda a0, a1, b0, b1, f=_fn: f(s32(a0), s32(b0)))
    scc_only(3, "s_cmp_%s_u32" % _name, lambda a0, a1, b0, b1, f=_fn: f(a0, b0))
scc_only(3, "s_cmp_eq_u64", lambda a0, a1, b0, b1: u64(a0, a1) == u64(b0, b1))
scc_only(3, "s_cmp_lg_u64", lambda a0, a1, b0, b1: u64(a0, a1) != u64(b0, b1))
for _name, _fn in _CMP:
    for _imm in IMMS:
        scc_only(3, "s_cmpk_%s_i32" % _name, lambda a0, a1, b0, b1, f=_fn, k=_imm: f(s32(a0), sext(k, 16)))
        scc_only(3, "s_cmpk_%s_u32" % _name, lambda a0, a1, b0, b1, f=_fn, k=_imm: f(a0, k))
scc_only(3, "s_bitcmp0_b32", lambda a0, a1, b0, b1: not (a0 >> (b0 & 31)) & 1, "sh")
scc_only(3, "s_bitcmp0_b64", lambda a0, a1, b0, b1: not (u64(a0, a1) >> (b0 & 63)) & 1, "sh")
scc_only(3, "s_bitcmp1_b32", lambda a0, a1, b0, b1: (a0 >> (b0 & 31)) & 1, "sh")
scc_only(3, "s_bitcmp1_b64", lambda a0, a1, b0, b1: (u64(a0, a1) >> (b0 & 63)) & 1, "sh")
loop1(3, "s_cselect_b32", lambda a, b, c: (a if c else b, None))
loop2(3, "s_cselect_b64", lambda a, b, b0, c: (a if c else b, None))
loop1(3, "s_cmov_b32", lambda a, b, c: (a if c else b, None))  # the destination starts as b
loop2(3, "s_cmov_b64", lambda a, b, b0, c: (a if c else b, None))
for _imm in IMMS:
    loop1(3, "s_movk_i32", lambda a, b, c, k=_imm: (sext(k, 16), None))
    loop1(3, "s_cmovk_i32", lambda a, b, c, k=_imm: (sext(k, 16) if c else b, None))
for _const in (-16, 64, 0x3F800000, 0x3F000000, 0x12345678):  # -16, 64, 1.0, 0.5, a literal
    loop1(3, "s_mov_b32", lambda a, b, c, k=_const: (k, None))

# branch: 1 when taken, 2 when not; VCC / EXEC is a when c, else 0
TAKEN, FELL = 1, 2
loop1(4, "s_cbranch_scc0", lambda a, b, c: (FELL if c else TAKEN, None))
loop1(4, "s_cbranch_scc1", lambda a, b, c: (TAKEN if c else FELL, None))
for _name, _when_zero in (("s_cbranch_vccz", True), ("s_cbranch_vccnz", False),
                          ("s_cbranch_execz", True), ("s_cbranch_execnz", False)):
    STEPS.append((4, _name, "loop", "val",
                  lambda a0, a1, b0, b1, c, z=_when_zero:
                  (TAKEN if ((u64(a0, a1) if c else 0) == 0) == z else FELL, c)))


# mask: EXEC = b; D, new EXEC of `insn D, a`
def mask_step(name, new_exec, returns_new=False):
    def run(a0, a1, b0, b1, c):
        a, old = u64(a0, a1), u64(b0, b1)
        new = new_exec(a, old) & M64
        d = new if returns_new else old
        first = ff1(new, 64) if new else 0  # v_readfirstlane_b32 reads lane 0 under an empty EXEC
        return words(d) + words(new) + (nz(new), first)
    STEPS.append((5, name, "mask", "val", run))


mask_step("s_and_saveexec_b64", lambda s, e: s & e)
mask_step("s_or_saveexec_b64", lambda s, e: s | e)
mask_step("s_xor_saveexec_b64", lambda s, e: s ^ e)
mask_step("s_andn2_saveexec_b64", lambda s, e: s & ~e)
mask_step("s_orn2_saveexec_b64", lambda s, e: s | ~e)
mask_step("s_nand_saveexec_b64", lambda s, e: ~(s & e))
mask_step("s_nor_saveexec_b64", lambda s, e: ~(s | e))
mask_step("s_xnor_saveexec_b64", lambda s, e: ~(s ^ e))
mask_step("s_andn1_saveexec_b64", lambda s, e: ~s & e)
mask_step("s_orn1_saveexec_b64", lambda s, e: ~s | e)
mask_step("s_andn1_wrexec_b64", lambda s, e: ~s & e, True)
mask_step("s_andn2_wrexec_b64", lambda s, e: s & ~e, True)
for _name, _fn in (("lt", lambda x, y: x < y), ("eq", lambda x, y: x == y), ("le", lambda x, y: x <= y),
                   ("gt", lambda x, y: x > y), ("ne", lambda x, y: x != y), ("ge", lambda x, y: x >= y)):
    for _to in ("e64", "e32"):  # into an SGPR pair, into VCC
        STEPS.append((5, "v_cmp_%s_u32_%s" % (_name, _to), "lane", "val",
                      lambda a0, a1, b0, b1, c, f=_fn: (1 if f(a0, b0) else 0,)))
STEPS.append((5, "v_addc_co_u32", "lane", "val",
              lambda a0, a1, b0, b1, c: words((u64(a0, a1) + u64(b0, b1)) & M64) + ((u64(a0, a1) + u64(b0, b1)) >> 64,)))

# movrel: forms 0 movrels_b32, 1 movrels_b64, 2 movreld_b32, 3 movreld_b64 over a
# block of 16 registers; M0 = 0..15, for the _b64 forms (M0 must be even) 0, 2, .. 14.
MOVREL_FORMS = ("s_movrels_b32", "s_movrels_b64", "s_movreld_b32", "s_movreld_b64")


def movrel_indexes(form):
    return range(0, 16, 2) if form & 1 else range(16)


def movrel_words(seed, form):
    """[word][1024] of one form: the block is h(6, form, w, 0..15, l), the source of movreld o = 16, 17."""
    block = [hashv(seed, 6, form, j) for j in range(16)]
    src = [hashv(seed, 6, form, 16 + j) for j in range(2)]
    rows = []
    for k in movrel_indexes(form):
        if form == 0:
            rows.append(block[k])
        elif form == 1:
            rows += [block[k], block[k + 1]]
        else:
            regs = list(block)  # SGPR[D + M0] = S, nothing else moves
            regs[k] = src[0]
            if form == 3:
                regs[k + 1] = src[1]
                rows += [regs[k], regs[k + 1], regs[(k + 2) % 16]]
            else:
                rows += [regs[k], regs[(k + 1) % 16], regs[(k + 15) % 16]]
    return rows


# sgpr: phase 0 holds s52..s99 and VCC (registers 106, 107), phase 1 s0..s51.
SGPR_PHASES = (tuple(range(52, 100)) + (106, 107), tuple(range(52)))


def sgpr_words(seed):
    """Register N of a phase is lane N % 64 of word N // 64; a lane with no register keeps 0.
    Words: phase 0 p low, p high, ~p low, ~p high; phase 1 p, ~p."""
    rows = []
    for phase, regs in enumerate(SGPR_PHASES):
        n_words = 1 + max(regs) // 64
        pattern = [hashv(seed, 7, phase, hi) for hi in range(n_words)]
        for flip in (0, M32):
            for hi in range(n_words):
                lanes = {n % 64 for n in regs if n // 64 == hi}
                rows.append([(pattern[hi][t] ^ flip) if t % 64 in lanes else 0 for t in range(BLOCK)])
    return rows


# ------------------------------------------------------------------ the parts
def _table_part(part, seed):
    rows = []
    mine = [s for s in STEPS if s[0] == part]
    for index, (_, _name, _cls, kind, fn) in enumerate(mine):
        cols = [fn(*ops) for ops in operands(seed, part, index, kind)]
        rows += [[int(c[w]) & M32 for c in cols] for w in range(len(cols[0]))]
    return rows


_CACHE = {}


def expected(part, seed):
    """uint32 [words, 1024]: what every thread holds after `part`."""
    key = (part, seed)
    if key not in _CACHE:
        p = PARTS.index(part)
        if part == "movrel":
            rows = [r for f in range(4) for r in movrel_words(seed, f)]
        elif part == "sgpr":
            rows = sgpr_words(seed)
        else:
            rows = _table_part(p, seed)
        out = np.array(rows, dtype=np.uint64).astype(np.uint32)
        out.setflags(write=False)
        _CACHE[key] = out
    return _CACHE[key]


def digest(part, seed):
    """The workgroup digest: sum of word x (2 idx + 1) mod 2^32, idx = word row x 1024 + thread."""
    v = expected(part, seed).astype(np.uint64).reshape(-1)
    idx = np.arange(v.size, dtype=np.uint64)
    return int(((v * ((2 * idx + 1) & M32)) & M32).sum() & M32)


def _steps_of(part):
    if part == "movrel":
        return sum(len(movrel_indexes(f)) for f in range(4))
    if part == "sgpr":
        return len(SGPR_PHASES)
    return sum(1 for s in STEPS if s[0] == PARTS.index(part))


# part -> (steps, words per thread)
SHAPES = {part: (_steps_of(part), expected(part, SEEDS[0]).shape[0]) for part in PARTS}
