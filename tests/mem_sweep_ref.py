"""numpy reference of the memory-path sweep (csrc/hip/mem_sweep.hip), written
from the ISA's rules and the maps in that file's header. It shares no code
with the C++ and does not use the kernel's closed forms: it keeps a byte array
for a workgroup's slab (and its LDS tile), executes every store and load of a
step on it the way the instruction is documented to move bytes, and records
what each load returns. Integer atomics are integer arithmetic; the float
ones use numpy's own IEEE types (bf16, which numpy lacks, as the upper half of
a float32 whose value fits eight significand bits).

A launch's thread is t = 64 * wave + lane; arrays are [step][word][256]."""
import numpy as np

SEEDS = (0x1B873593, 0xC0FFEE11)
ROUTES = ["gwidth", "buffer", "flat", "atomic", "l1", "l2", "scalar"]
SHAPES = {"gwidth": (18, 4), "buffer": (12, 4), "flat": (8, 4), "atomic": (25, 4), "l1": (64, 4), "l2": (512, 4),
          "scalar": (8, 36)}
M32 = 0xFFFFFFFF
T = np.arange(256, dtype=np.int64)
LANE, WAVE = T & 63, T >> 6

# A workgroup's 144 KiB of the arena; addresses below count from the slab's
# first byte, behind the front guard band.
GUARD = 4096
TILE = 128 << 10
L1_TILE = 16 << 10
WORK = TILE
BUF = WORK + 4096
SLAB = BUF + 4096
STRIDE = GUARD + SLAB + GUARD
LDS = SLAB + GUARD  # the simulator keeps the wave's LDS tiles behind the back guard band
WAVE_BYTES, SLOT = 1024, 16
RANGE_SLOTS = 48  # where both buffer descriptors end
TABLE_WORDS = 1024

ATOMIC_OPS = ["add", "sub", "smin", "smax", "umin", "umax", "and", "or", "xor", "swap", "cmpswap", "inc", "dec",
              "add_x2", "smin_x2", "umax_x2", "swap_x2", "cmpswap_x2", "add_f32", "pk_add_f16", "pk_add_bf16",
              "add_f64", "min_f64", "max_f64", "contended"]
SCALAR_SIZES = (1, 2, 4, 8, 16, 1, 4)
L1_MUL, L2_MUL = (5, 13, 27, 45), (5, 29, 67, 111)


def fmix32(h):
    """murmur3's 32-bit finaliser on an int64 array of 32-bit values."""
    h = np.asarray(h, np.int64) & M32
    h = h ^ (h >> 16)
    h = (h * 0x85EBCA6B) & M32
    h = h ^ (h >> 13)
    h = (h * 0xC2B2AE35) & M32
    h = h ^ (h >> 16)
    return h


def key(route, step, word, wave, lane, kind=0):
    return (kind << 28) | (ROUTES.index(route) << 24) | (step << 12) | ((4 * wave + word) << 6) | lane


def src(seed, route, step, word, kind=0):
    """src (kind 1: aux) values of one (step, word): [256] by thread."""
    return fmix32(seed ^ key(route, step, word, WAVE, LANE, kind))


def aux(seed, route, step, word):
    return src(seed, route, step, word, 1)


def til(seed, route, d, kind=2):
    """Tile dword d (kind 3: the rewritten value)."""
    return fmix32(seed ^ ((kind << 28) | (ROUTES.index(route) << 24) | np.asarray(d, np.int64)))


def sentinel(i):
    return ((np.asarray(i, np.int64) * 0x9E3779B1) & M32) ^ 0xA5A5A5A5


def slot(k, lane=LANE):
    return ((2 * k + 3) * lane + k) & 63


def all_keys():
    """Every key a launch hashes, as one array: src and aux of every (route,
    step, word, thread), the tile and rewrite keys of l1, l2 and the table."""
    out = []
    for r in ROUTES:
        steps = SHAPES[r][0] if r != "scalar" else 8 * SHAPES[r][0]
        for kind in (0, 1):
            for s in range(steps):
                for w in range(4):
                    out.append(key(r, s, w, WAVE, LANE, kind))
    for r, n in (("l1", L1_TILE // 4), ("l2", TILE // 4), ("scalar", TABLE_WORDS)):
        for kind in (2, 3):
            out.append((kind << 28) | (ROUTES.index(r) << 24) | np.arange(n, dtype=np.int64))
    return np.concatenate(out)


def sext(v, bits):
    v = np.asarray(v, np.int64) & ((1 << bits) - 1)
    return np.where(v >> (bits - 1), v | (M32 ^ ((1 << bits) - 1)), v)


# ------------------------------------------------------------------- memory
class Memory:
    """The bytes of one workgroup's 144 KiB as the host fills them, and behind
    them 4 KiB of LDS (zero). Thread-vector stores and loads, little-endian."""

    def __init__(self):
        words = sentinel(np.arange(STRIDE // 4)).astype("<u4")
        self.b = np.concatenate([words.view(np.uint8), np.zeros(4096, np.uint8)])

    def store(self, addr, value, nbytes, mask=None):
        """The low `nbytes` (at most 4) of value[t] to addr[t], where mask[t]."""
        addr, value = np.broadcast_to(np.asarray(addr, np.int64), (256,)), np.asarray(value, np.int64)
        sel = np.ones(256, bool) if mask is None else np.asarray(mask, bool)
        assert (addr[sel] >= -GUARD).all() and (addr[sel] + nbytes <= LDS + 4096).all()  # guards_intact() tells
        for k in range(nbytes):
            self.b[GUARD + addr[sel] + k] = (value[sel] >> (8 * k)) & 0xFF

    def store_dwords(self, addr, values, mask=None):
        for j, v in enumerate(values):
            self.store(np.asarray(addr) + 4 * j, v, 4, mask)

    def load(self, addr, nbytes, signed=False):
        """nbytes (at most 4) from addr[t], zero- or sign-extended to 32 bits."""
        addr = np.broadcast_to(np.asarray(addr, np.int64), (256,))
        assert (addr >= 0).all()
        v = np.zeros(256, np.int64)
        for k in range(nbytes):
            v |= self.b[GUARD + addr + k].astype(np.int64) << (8 * k)
        return sext(v, 8 * nbytes) if signed and nbytes < 4 else v

    def load_dwords(self, addr, n):
        return [self.load(np.asarray(addr) + 4 * j, 4) for j in range(n)]

    def guards_intact(self):
        words = self.b[:STRIDE].view("<u4").astype(np.int64)
        want = sentinel(np.arange(STRIDE // 4))
        g = GUARD // 4
        return (words[:g] == want[:g]).all() and (words[-g:] == want[-g:]).all()


def d16(dst, value):
    """A *_d16 load: bits [15:0] of the destination <- the value. The ISA text
    keeps [31:16] of `dst`; the MI355X writes zero there (settled on the
    hardware, see the kernel's header)."""
    return value & 0xFFFF


def d16_hi(dst, value):
    return (value & 0xFFFF) << 16


# ------------------------------------------------------------------- gwidth
def gwidth(seed):
    m = Memory()
    out = np.zeros((18, 4, 256), np.int64)
    for s in range(18):
        combo = s % 9
        A = WORK + WAVE * WAVE_BYTES + SLOT * slot(s)
        x = [src(seed, "gwidth", s, j) for j in range(4)]
        a = [aux(seed, "gwidth", s, j) for j in range(4)]
        if combo == 0:
            m.store_dwords(A, x)
            g = [m.load(A + 4 * j, 4) for j in range(4)]
        elif combo == 1:
            m.store_dwords(A, x[:3])
            m.store(A + 12, x[3], 4)
            g = m.load_dwords(A, 4)
        elif combo == 2:
            m.store_dwords(A, x[:2])
            m.store_dwords(A + 8, x[2:])
            g = m.load_dwords(A, 3) + [m.load(A + 12, 4)]
        elif combo == 3:
            for j in range(4):
                m.store(A + 4 * j, x[j], 4)
            g = m.load_dwords(A, 2) + m.load_dwords(A + 8, 2)
        elif combo == 4:
            for b in range(4):
                m.store(A + b, x[0] >> (8 * b), 1)
                m.store(A + 4 + b, x[1] >> (8 * b), 1)
            g = [m.load(A, 2), m.load(A + 2, 2, True), m.load(A + 4, 2, True), m.load(A + 6, 2)]
        elif combo == 5:
            m.store(A, x[0], 2)
            m.store(A + 2, x[0] >> 16, 2)
            m.store(A + 4, x[1], 2)
            m.store(A + 6, x[1] >> 16, 2)
            g = [m.load(A, 1), m.load(A + 1, 1, True), m.load(A + 6, 1, True), m.load(A + 7, 1)]
        elif combo == 6:
            m.store_dwords(A, x[:2])
            g = [d16(a[0], m.load(A, 2)), d16_hi(a[1], m.load((A + 18) - 16, 2)), d16(a[2], m.load(A + 5, 1)),
                 d16_hi(a[3], m.load(A + 7, 1, True))]
        elif combo == 7:
            m.store_dwords(A, a[:2])
            m.store(A, x[0] >> 16, 2)  # short_d16_hi: bits [31:16] of the data register
            m.store(A + 5, x[1] >> 16, 1)  # byte_d16_hi: bits [23:16]
            g = m.load_dwords(A, 2) + [d16_hi(a[2], m.load(A + 1, 1)), d16(a[3], m.load(A + 5, 1, True))]
        else:
            m.store((A - 4095) + 4095, x[0], 4)
            g0 = m.load((A + 4096) - 4096, 4)
            m.store((A + 4 + 4096) - 4096, x[1], 4)
            g1 = m.load((A + 4 - 4095) + 4095, 4)
            m.store_dwords((A + 8 + 4096) - 4096, x[2:])
            g = [g0, g1] + m.load_dwords((A + 8 - 4095) + 4095, 2)
        out[s] = g
    assert m.guards_intact()
    return out


# ------------------------------------------------------------------- buffer
class Descriptor:
    """base, stride and num_records of a buffer resource; the range check of
    the header: stride 0 checks offset + size against num_records bytes, idxen
    checks the index against num_records. soffset is outside the check."""

    def __init__(self, base, stride, num_records):
        self.base, self.stride, self.num_records = base, stride, num_records

    def resolve(self, size, index=0, offset=0, soffset=0):
        index, offset = np.asarray(index, np.int64), np.asarray(offset, np.int64)
        if self.stride == 0:
            ok = offset + size <= self.num_records
        else:
            ok = (index < self.num_records) & (offset + size <= self.stride)
        return self.base + soffset + index * self.stride + offset, np.broadcast_to(ok, (256,))

    def store(self, m, values, nbytes=4, **where):
        addr, ok = self.resolve(nbytes * len(values), **where)
        for j, v in enumerate(values):
            m.store(np.where(ok, addr, 0) + nbytes * j, v, nbytes, ok)

    def load(self, m, n=1, nbytes=4, signed=False, **where):
        addr, ok = self.resolve(nbytes * n, **where)
        return [np.where(ok, m.load(np.where(ok, addr, 0) + nbytes * j, nbytes, signed), 0) for j in range(n)]


def buffer_out_of_range(step):
    """Which threads' slot lies beyond the descriptors' end in `step`."""
    return slot(step) >= RANGE_SLOTS


def buffer(seed):
    m = Memory()
    out = np.zeros((12, 4, 256), np.int64)
    base = BUF + WAVE * WAVE_BYTES
    R, S = Descriptor(base, 0, RANGE_SLOTS * SLOT), Descriptor(base, SLOT, RANGE_SLOTS)
    for s in range(12):
        combo = s % 6
        sl = slot(s)
        off = SLOT * sl
        x = [src(seed, "buffer", s, j) for j in range(4)]
        if combo == 0:
            R.store(m, x, offset=off)
            g = [R.load(m, offset=off + 4 * j)[0] for j in range(4)]
        elif combo == 1:
            for j in range(4):
                S.store(m, [x[j]], index=sl, offset=4 * j)
            g = S.load(m, 4, index=sl)
        elif combo == 2:
            S.store(m, x[:2], index=sl, offset=0)
            S.store(m, x[2:], index=sl, offset=8)
            g = R.load(m, 3, offset=off) + R.load(m, offset=off, soffset=12)
        elif combo == 3:
            R.store(m, x[:3], offset=off)
            R.store(m, [x[3]], offset=off, soffset=12)
            g = S.load(m, 2, index=sl, offset=0) + S.load(m, 2, index=sl, offset=8)
        elif combo == 4:
            for b in range(4):
                R.store(m, [x[0] >> (8 * b)], 1, offset=off + b)
            R.store(m, [x[1]], 2, offset=off + 4)
            R.store(m, [x[1] >> 16], 2, offset=off + 6)
            g = (R.load(m, 1, 1, offset=off) + R.load(m, 1, 1, True, offset=off + 3) + R.load(m, 1, 2, offset=off + 4)
                 + R.load(m, 1, 2, True, offset=off + 6))
        else:
            R.store(m, x, offset=off)
            g = m.load_dwords(base + off, 4)
        out[s] = g
    assert m.guards_intact()
    return out


# --------------------------------------------------------------------- flat
def flat(seed):
    m = Memory()
    out = np.zeros((8, 4, 256), np.int64)
    for s in range(8):
        combo = s % 4
        off = SLOT * slot(s)
        in_lds = ((LANE + s) & 1) == 1
        A = np.where(in_lds, LDS, WORK) + WAVE * WAVE_BYTES + off
        x = [src(seed, "flat", s, j) for j in range(4)]
        if combo == 0:
            m.store_dwords(A, x)
            g = [m.load(A + 4 * j, 4) for j in range(4)]
        elif combo == 1:
            for j in range(4):
                m.store(A + 4 * j, x[j], 4)
            g = m.load_dwords(A, 4)
        elif combo == 2:
            m.store_dwords(A, x[:2])
            m.store_dwords(A + 8, x[2:])
            g = m.load_dwords(A, 3) + [m.load(A + 12, 4)]
        else:
            m.store(A, x[0], 2)
            m.store(A + 2, x[0] >> 16, 2)
            for b in range(4):
                m.store(A + 4 + b, x[1] >> (8 * b), 1)
            g = [m.load(A, 2), m.load(A + 2, 2, True), m.load(A + 4, 1), m.load(A + 7, 1, True)]
        out[s] = g
    assert m.guards_intact()
    return out


# ------------------------------------------------------------------- atomic
def _signed(v, bits):
    v = int(v) & ((1 << bits) - 1)
    return v - (1 << bits) if v >> (bits - 1) else v


def integer_atomic(op, old, b, cmp, bits):
    """The value an integer atomic leaves in memory (it returns `old`)."""
    mask = (1 << bits) - 1
    if op == "add":
        return (old + b) & mask
    if op == "sub":
        return (old - b) & mask
    if op == "smin":
        return old if _signed(old, bits) <= _signed(b, bits) else b
    if op == "smax":
        return old if _signed(old, bits) >= _signed(b, bits) else b
    if op == "umin":
        return min(old, b)
    if op == "umax":
        return max(old, b)
    if op == "and":
        return old & b
    if op == "or":
        return old | b
    if op == "xor":
        return old ^ b
    if op == "swap":
        return b
    if op == "cmpswap":
        return b if old == cmp else old
    if op == "inc":
        return 0 if old >= b else old + 1
    if op == "dec":
        return b if old == 0 or old > b else old - 1
    raise ValueError(op)


def _f32_bits(v):
    return np.asarray(v, np.float32).view(np.uint32).astype(np.int64)


def _f16_bits(v):
    return np.asarray(v, np.float16).view(np.uint16).astype(np.int64)


def _bf16_bits(v):
    bits = _f32_bits(v)
    assert not (bits & 0xFFFF).any()  # the value fits bf16's eight significand bits
    return bits >> 16


def _f64_bits(v):
    return np.asarray(v, np.float64).view(np.uint64)


def _sign(h):
    return np.where(h >> 31, -1, 1)


def atomic_operands(seed, op, j=0):
    """What the word holds before the atomic, its operand and cmpswap's compare
    value, by thread, as Python ints (32-bit ops: data set j; 64-bit: j unused).
    The float ones as (word bits, operand bits, result bits)."""
    s = ATOMIC_OPS.index(op)
    odd = (T & 1) == 1
    if s <= 12:
        a, b = src(seed, "atomic", s, 2 * j), aux(seed, "atomic", s, 2 * j)
        cmp = a ^ j
        if op == "inc" and j == 1:
            b = np.where(odd, M32, a)
        if op == "dec" and j == 1:
            a, b = np.where(odd, a, 0), np.where(odd, M32, b)
        return [int(v) for v in a], [int(v) for v in b], [int(v) for v in cmp]
    if s <= 17:
        a = src(seed, "atomic", s, 0) | (src(seed, "atomic", s, 1) << 32)
        b = aux(seed, "atomic", s, 0) | (aux(seed, "atomic", s, 1) << 32)
        a, b = [int(v) for v in a.astype(np.uint64)], [int(v) for v in b.astype(np.uint64)]
        return a, b, [v ^ int(o) for v, o in zip(a, odd)]
    if s <= 20:
        ha, hb = src(seed, "atomic", s, 2 * j), aux(seed, "atomic", s, 2 * j)
        if op == "add_f32":
            fa = (4096 + (ha & 0xFFF)).astype(np.float32)
            fb = (_sign(hb) * (1024 + (hb & 0x3FF))).astype(np.float32)
            return _f32_bits(fa), _f32_bits(fb), _f32_bits(fa + fb)
        if op == "pk_add_f16":
            def pack(h):
                return (256 + (h & 0xFF)).astype(np.float16), (256 + ((h >> 8) & 0xFF)).astype(np.float16)
            bits = _f16_bits
        else:
            def pack(h):
                return (64 + (h & 31)).astype(np.float32), (64 + ((h >> 8) & 31)).astype(np.float32)
            bits = _bf16_bits
        (alo, ahi), (blo, bhi) = pack(ha), pack(hb)
        return (bits(alo) | bits(ahi) << 16, bits(blo) | bits(bhi) << 16, bits(alo + blo) | bits(ahi + bhi) << 16)
    ha, hb = src(seed, "atomic", s, 0), aux(seed, "atomic", s, 0)
    if op == "add_f64":
        fa = ((1 << 30) + (ha & 0x3FFFFFFF)).astype(np.float64)
        fb = (_sign(hb) * ((1 << 29) + (hb & 0x1FFFFFFF))).astype(np.float64)
        r = fa + fb
    else:
        fa = (_sign(ha) * ((1 << 30) + (ha & 0x3FFFFFFF))).astype(np.float64)
        fb = (_sign(hb) * ((1 << 30) + (hb & 0x3FFFFFFF))).astype(np.float64)
        r = np.minimum(fa, fb) if op == "min_f64" else np.maximum(fa, fb)
    assert np.isfinite(r).all() and (r != 0).all()
    return _f64_bits(fa), _f64_bits(fb), _f64_bits(r)


def contended_operands(seed):
    s = ATOMIC_OPS.index("contended")
    return [np.ones(256, np.int64), 1 << (T & 31), src(seed, "atomic", s, 2), src(seed, "atomic", s, 3)]


def atomic(seed):
    out = np.zeros((25, 4, 256), np.int64)
    for s, op in enumerate(ATOMIC_OPS):
        if s <= 12:
            for j in range(2):
                a, b, cmp = atomic_operands(seed, op, j)
                out[s, 2 * j] = a
                out[s, 2 * j + 1] = [integer_atomic(op, a[t], b[t], cmp[t], 32) for t in range(256)]
        elif s <= 17:
            a, b, cmp = atomic_operands(seed, op)
            left = [integer_atomic(op[:-3], a[t], b[t], cmp[t], 64) for t in range(256)]
            out[s] = [[v & M32 for v in a], [v >> 32 for v in a], [v & M32 for v in left], [v >> 32 for v in left]]
        elif s <= 20:
            for j in range(2):
                a, _, r = atomic_operands(seed, op, j)
                out[s, 2 * j], out[s, 2 * j + 1] = a, r
        elif s <= 23:
            a, _, r = atomic_operands(seed, op)
            out[s] = [(a & M32).astype(np.int64), (a >> 32).astype(np.int64), (r & M32).astype(np.int64),
                      (r >> 32).astype(np.int64)]
        else:
            ops = contended_operands(seed)
            v = [int(aux(seed, "atomic", s, j)[0]) for j in range(4)]
            for t in range(256):  # any arrival order leaves the same words
                v[0] = (v[0] + int(ops[0][t])) & M32
                v[1] |= int(ops[1][t])
                v[2] = max(v[2], int(ops[2][t]))
                v[3] ^= int(ops[3][t])
            out[s] = np.repeat(np.array(v, np.int64)[:, None], 256, 1)
    return out


# ------------------------------------------------------------------ l1, l2
def l1_dword(p, i):
    """The dword of the 16 KiB tile that load i (0..63) of pass p reads, by thread."""
    q = (L1_MUL[p] * i + 17 * WAVE + p) & 63
    line = 2 * q + ((LANE >> 5) ^ (i & 1))
    return line * 32 + ((5 * (LANE & 31) + i) & 31)


def l1_rewrites():
    """The dwords wave 0 rewrites before pass 2: two per lane."""
    l = np.arange(64)
    return np.concatenate([(l + 64 * h) * 32 + ((5 * l + 3) & 31) for h in range(2)])


def l1(seed):
    tile = til(seed, "l1", np.arange(L1_TILE // 4))
    out = np.zeros((64, 4, 256), np.int64)
    for p in range(4):
        if p == 2:
            d = l1_rewrites()
            tile[d] = til(seed, "l1", d, 3)
        for i in range(64):
            out[16 * p + i // 4, i % 4] = tile[l1_dword(p, i)]
    return out


def l2_chunk(p, i):
    """The 16-byte chunk of the 128 KiB tile that load i (0..127) of pass p reads, by thread."""
    g = (L2_MUL[p] * i + 37 * WAVE + p) & 127
    return 64 * g + ((9 * LANE + 5 * p) & 63)


def l2(seed):
    tile = til(seed, "l2", np.arange(TILE // 4))
    out = np.zeros((512, 4, 256), np.int64)
    for p in range(4):
        if p == 3:
            tile = tile ^ M32
        for i in range(128):
            c = l2_chunk(p, i)
            for j in range(4):
                out[128 * p + i, j] = tile[4 * c + j]
    return out


# ------------------------------------------------------------------- scalar
def scalar_offsets(seed, step):
    """[7][256]: the dword offset each of the seven instructions reads at, uniform per wave."""
    out = []
    for n, size in enumerate(SCALAR_SIZES):
        h = fmix32(seed ^ key("scalar", 8 * step + n, 0, WAVE, 0, 1))
        out.append(h % (TABLE_WORDS // size) * size)
    return out


def scalar(seed):
    table = til(seed, "scalar", np.arange(TABLE_WORDS))
    out = np.zeros((8, 36, 256), np.int64)
    for s in range(8):
        w = 0
        for off, size in zip(scalar_offsets(seed, s), SCALAR_SIZES):
            for j in range(size):
                out[s, w] = table[off + j]
                w += 1
        assert w == 36
    return out


_BUILD = {"gwidth": gwidth, "buffer": buffer, "flat": flat, "atomic": atomic, "l1": l1, "l2": l2, "scalar": scalar}
_cache: dict = {}


def expected(route, seed):
    """What every thread receives: uint32 [steps, words, 256]. Computed once; do not write to it."""
    if (route, seed) not in _cache:
        a = (_BUILD[route](seed) & M32).astype(np.uint32)
        assert a.shape == (*SHAPES[route], 256)
        a.setflags(write=False)
        _cache[route, seed] = a
    return _cache[route, seed]


def digest(route, seed, flip_first=False):
    """The workgroup digest: sum of got * (2 idx + 1) mod 2^32 over idx =
    (step * words + word) * 256 + t. `flip_first`: with bit 0 of value 0 flipped."""
    v = expected(route, seed).astype(np.int64).ravel().copy()
    if flip_first:
        v[0] ^= 1
    idx = np.arange(v.size, dtype=np.int64)
    return int(((v * ((2 * idx + 1) & M32)) & M32).sum() & M32)
