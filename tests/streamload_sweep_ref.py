"""Independent reference of the stream load sweep (csrc/hip/streamload_sweep.hip):
numpy only, nothing shared with the C++. The two hashes, the untiling maps to
the logical Wt and X, Ct as an int64 product, panel_of and the three digests
mod 2^32."""
import numpy as np

PARTS = ["stage", "act", "gemm"]
ROWS = TOKENS = 16
WAVES = 8
M32 = 0xFFFFFFFF


def fmix32(h):
    h = np.asarray(h, np.uint64) & M32
    h ^= h >> 16
    h = h * 0x85EBCA6B & M32
    h ^= h >> 13
    h = h * 0xC2B2AE35 & M32
    return h ^ h >> 16


def panel_words(seed, panel, ksteps):
    """The 256 ksteps dwords of one panel as the arena holds them, and their indices in the arena."""
    i = np.arange(256 * ksteps, dtype=np.uint64) + 256 * ksteps * panel
    return fmix32(seed ^ i), i


def x_words(seed, ksteps):
    i = np.arange(256 * ksteps, dtype=np.uint64)
    return fmix32(seed ^ 0x40000000 ^ i), i


def untile(words, ksteps):
    """int8 [16, 64 ksteps] from tiled dwords: byte (k >> 6) 1024 + ((k >> 4) & 3) 256 + 16 row + (k & 15)."""
    b = words.astype("<u4").view(np.int8)
    k = np.arange(64 * ksteps)
    at = (k >> 6) * 1024 + ((k >> 4) & 3) * 256 + (k & 15)
    return b[at[None, :] + 16 * np.arange(16)[:, None]]


def operands(seed, panel, ksteps):
    """(Wt int8 [16, K] of one panel, X int8 [16, K])."""
    return untile(panel_words(seed, panel, ksteps)[0], ksteps), untile(x_words(seed, ksteps)[0], ksteps)


def product(seed, panel, ksteps):
    """Ct [16 weight rows, 16 tokens] of one panel, int64."""
    wt, x = operands(seed, panel, ksteps)
    return wt.astype(np.int64) @ x.astype(np.int64).T


def panel_of(g, lap, wave, laps, panels):
    r = panels // WAVES
    group = (lap + g * 40503 % r) % r if lap < laps - laps % r else lap % r
    return WAVES * group + wave


def fold(words, index):
    """sum of rotl32(word, index & 31) mod 2^32."""
    s = np.asarray(index, np.uint64) & 31
    return int(((words << s | words >> (32 - s)) & M32).sum() & M32)


def digests(seed, laps, ksteps, panels, g=0):
    """The three workgroup digests of a healthy CU."""
    d = dict.fromkeys(PARTS, 0)
    act = fold(*x_words(seed, ksteps))
    weight = 2 * np.arange(ROWS * TOKENS, dtype=np.int64) + 1  # 2 (16 n + m) + 1; int64 wraps mod 2^64
    for lap in range(laps):
        for wave in range(WAVES):
            p = panel_of(g, lap, wave, laps, panels)
            d["stage"] += fold(*panel_words(seed, p, ksteps))
            d["act"] += act
            d["gemm"] += int(((product(seed, p, ksteps).ravel() & M32) * (weight + 512 * p)).sum() & M32)
    return {part: v & M32 for part, v in d.items()}
