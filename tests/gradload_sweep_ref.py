"""Independent reference of the gradient load sweep (csrc/hip/gradload_sweep.hip):
numpy only, nothing shared with the C++. The hash, X and dY as bf16 bits and as
integers, X^T dY per k-half in int64 (units of 2^-7), the epoch sums, set_of and
the four digests mod 2^32."""
import functools

import numpy as np

PARTS = ["stage", "transpose", "gemm", "accum"]
TILE = 128
M32 = 0xFFFFFFFF
WEIGHT = 2 * np.arange(TILE * TILE, dtype=np.int64) + 1  # 2 (128 row + col) + 1; int64 wraps mod 2^64


def fmix32(h):
    h = np.asarray(h, np.uint64) & M32
    h ^= h >> 16
    h = h * 0x85EBCA6B & M32
    h ^= h >> 13
    h = h * 0xC2B2AE35 & M32
    return h ^ h >> 16


def groups_of(epoch):
    return max(1, 32 // epoch)


@functools.lru_cache(maxsize=600)
def words(seed, s, ksteps):
    """The 4,096 ksteps dwords of set s as the arena holds them: X[K][128], then dY[K][128], two bf16 a dword."""
    w = np.arange(2048 * ksteps, dtype=np.uint64)
    x = fmix32(seed ^ (s << 22) ^ w) & 0x807F807F | 0x3F803F80
    h = fmix32(seed ^ (s << 22 | 1 << 21) ^ w)
    lo, hi = h & 0xFFFF, h >> 16
    ints = np.array([0x3F80, 0x4000, 0x4040, 0x4080, 0x40A0, 0x40C0, 0x40E0, 0x4100], np.uint64)  # 1.0 .. 8.0
    dy = (lo & 0x8000 | ints[lo & 7]) | (hi & 0x8000 | ints[hi & 7]) << 16
    return np.concatenate([x, dy])


def operands(seed, s, ksteps):
    """(X uint16 [K, 128], dY uint16 [K, 128]) of set s."""
    halves = words(seed, s, ksteps).astype("<u4").view("<u2").reshape(2, 32 * ksteps, TILE)
    return halves[0], halves[1]


def values(seed, s, ksteps):
    """(X in units of 2^-7, +-(128..255); dY, +-(1..8)) as int64, decoded from the bf16 bits."""
    x, dy = (np.left_shift(b.astype(np.uint32), 16).view(np.float32).astype(np.float64) for b in operands(seed, s, ksteps))
    assert (np.abs(x * 128) >= 128).all() and (np.abs(x * 128) <= 255).all() and (np.abs(dy) >= 1).all()
    assert (x * 128 == np.rint(x * 128)).all() and (dy == np.rint(dy)).all() and (np.abs(dy) <= 8).all()
    return (x * 128).astype(np.int64), dy.astype(np.int64)


@functools.lru_cache(maxsize=600)
def partials(seed, s, ksteps):
    """[2, 128, 128] int64: X^T dY over either k-half (tokens 16 half ..+15 of every 32), in units of 2^-7."""
    x, dy = values(seed, s, ksteps)
    half = (np.arange(32 * ksteps) >> 4 & 1).astype(bool)
    return np.stack([x[~half].T @ dy[~half], x[half].T @ dy[half]])


def set_of(g, lap, laps, epoch):
    """The set workgroup g reads in `lap`: its epoch's group, rotated by g below the last whole round."""
    groups, e = groups_of(epoch), lap // epoch
    full = laps - laps % (epoch * groups)
    group = (e + g * 40503 % groups) % groups if lap < full else e % groups
    return group * epoch + lap % epoch


def epoch_sums(seed, laps, ksteps, epoch, g=0):
    """[ceil(laps / epoch), 128, 128] int64: what a slab holds when it is read back; the last may be partial."""
    out = np.zeros((-(-laps // epoch), TILE, TILE), np.int64)
    for lap in range(laps):
        out[lap // epoch] += partials(seed, set_of(g, lap, laps, epoch), ksteps).sum(0)
    return out


def fold(w, index):
    """sum of rotl32(word, index & 31) mod 2^32."""
    s = np.asarray(index, np.uint64) & 31
    return int(((w << s | w >> (32 - s)) & M32).sum() & M32)


def digest(fix):
    return int(((fix.ravel() & M32) * WEIGHT).sum() & M32)


def digests(seed, laps, ksteps, epoch, g=0):
    """The four workgroup digests of a healthy CU."""
    d = dict.fromkeys(PARTS, 0)
    n = np.arange(TILE, dtype=np.uint64)
    for lap in range(laps):
        s = set_of(g, lap, laps, epoch)
        w = words(seed, s, ksteps)
        d["stage"] += fold(w, np.arange(w.size))
        for m in operands(seed, s, ksteps):  # word (j, n) = M[2j][n] | M[2j+1][n] << 16; each read by two waves
            m = m.astype(np.uint64)
            d["transpose"] += 2 * fold(m[0::2] | m[1::2] << 16, np.broadcast_to(n, m[0::2].shape))
        d["gemm"] += sum(digest(half) for half in partials(seed, s, ksteps))
    d["accum"] = sum(digest(e) for e in epoch_sums(seed, laps, ksteps, epoch, g))
    return {part: v & M32 for part, v in d.items()}
