"""Independent reference of the FP8 load sweep (csrc/hip/f8load_sweep.hip): numpy
only, nothing shared with the C++. The hash, the byte mask, an e4m3 decode and
A Bt^T in float64, the scales, bf16 round-to-nearest-even on the float32 bits,
set_of, the order the ring is read back in and the four digests mod 2^32."""
import functools

import numpy as np

PARTS = ["operand", "gemm", "round", "store"]
ROWS = (128, 256)  # of A and of Bt
SETS = 16
M32 = 0xFFFFFFFF


def fmix32(h):
    h = np.asarray(h, np.uint64) & M32
    h ^= h >> 16
    h = h * 0x85EBCA6B & M32
    h ^= h >> 13
    h = h * 0xC2B2AE35 & M32
    return h ^ h >> 16


@functools.lru_cache(maxsize=200)
def operands(seed, s, ksteps):
    """(A uint8 [128, K], Bt uint8 [256, K], sa float32 [128], sb float32 [256]) of set s, K = 64 ksteps."""
    panels, scales = [], []
    for p, rows in enumerate(ROWS):
        h = fmix32(seed ^ (s << 23 | p << 22) ^ np.arange(rows * 16 * ksteps, dtype=np.uint64))
        b = h.astype("<u4").view(np.uint8).astype(np.uint32)
        panels.append(((b & 0x87) | ((6 + ((b >> 3) & 3)) << 3)).astype(np.uint8).reshape(rows, 64 * ksteps))
        g = fmix32(seed ^ (1 << 30 | s << 23 | p << 22) ^ np.arange(rows, dtype=np.uint64)).astype(np.int64)
        scales.append(np.exp2((g & 1) if p else (g & 3) - 2).astype(np.float32))
    return (*panels, *scales)


def e4m3(b):
    """OCP e4m3 bytes as float64: bias 7, subnormals, no infinity, S.1111.111 is NaN."""
    b = b.astype(np.int64)
    e, m = b >> 3 & 15, b & 7
    v = np.where(e == 0, m / 8 * 2.0 ** -6, (1 + m / 8) * np.exp2(e - 7.0))
    v = np.where((e == 15) & (m == 7), np.nan, v)
    return np.where(b & 0x80, -v, v)


@functools.lru_cache(maxsize=200)
def product(seed, s, ksteps):
    """C = A Bt^T of set s as float64 [128, 256]: every sum is exact."""
    a, bt, _, _ = operands(seed, s, ksteps)
    return e4m3(a) @ e4m3(bt).T


@functools.lru_cache(maxsize=200)
def tile(seed, s, ksteps):
    """Y = bf16(C sa sb) of set s as dwords [128, 128]: column 2n in the low half."""
    _, _, sa, sb = operands(seed, s, ksteps)
    y = (product(seed, s, ksteps) * sa[:, None] * sb[None, :]).astype(np.float32)
    assert (y.astype(np.float64) == product(seed, s, ksteps) * sa[:, None] * sb[None, :]).all()
    bits = (y + np.float32(0)).view(np.uint32).astype(np.uint64)  # an exact zero sum is +0
    half = (bits + 0x7FFF + (bits >> 16 & 1)) >> 16
    return (half[:, 0::2] | half[:, 1::2] << 16).astype(np.uint32)


def set_of(g, lap, laps, sets=SETS):
    """The set workgroup g reads in `lap`: rotated by g below the last whole round of the sets."""
    return ((g if lap < laps - laps % sets else 0) + lap) % sets


def read_back_order(laps, slots):
    """The laps whose tile is read back, in order: lap l - slots at the start of lap l, the rest behind the last."""
    return [lap - slots for lap in range(slots, laps)] + list(range(max(laps - slots, 0), laps))


def fold(w, first=0):
    """sum of rotl32(word, index & 31) mod 2^32, the index counted from `first`."""
    w = np.asarray(w, np.uint64).ravel()
    s = (np.arange(w.size, dtype=np.uint64) + first) & 31
    return int(((w << s | w >> (32 - s)) & M32).sum() & M32)


def digests(seed, laps, ksteps, slots, g=0):
    """The four workgroup digests of a healthy CU."""
    d = dict.fromkeys(PARTS, 0)
    weight = 2 * np.arange(ROWS[0] * ROWS[1], dtype=np.uint64) + 1
    for lap in range(laps):
        s = set_of(g, lap, laps)
        a, bt = (m.view("<u4") for m in operands(seed, s, ksteps)[:2])
        d["operand"] += 4 * fold(a) + 2 * fold(bt, a.size)  # an A dword is read by four waves, a Bt dword by two
        fix = (product(seed, s, ksteps) * 256).astype(np.int64).ravel().astype(np.uint64) & M32
        d["gemm"] += int((fix * weight & M32).sum())
        d["round"] += fold(tile(seed, s, ksteps))
    d["store"] = sum(fold(tile(seed, set_of(g, lap, laps), ksteps)) for lap in read_back_order(laps, slots))
    return {part: v & M32 for part, v in d.items()}
