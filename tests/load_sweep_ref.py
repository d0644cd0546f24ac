"""Independent reference of the load sweep (csrc/hip/load_sweep.hip): numpy
only, nothing shared with the C++. The operand bytes from the key, the product
in int64, the three folds and the gemm digest mod 2^32."""
import numpy as np

PARTS = ["stage", "lds", "gemm", "valu"]
BLOCK = 512
ROWS_A, ROWS_B = 128, 256
VALU_ROUNDS = 2
M32 = 0xFFFFFFFF


def fmix32(h):
    h = np.asarray(h, np.uint64) & M32
    h ^= h >> 16
    h = h * 0x85EBCA6B & M32
    h ^= h >> 13
    h = h * 0xC2B2AE35 & M32
    return h ^ h >> 16


def panel_words(seed, set_, panel, ksteps):
    """The dwords of one panel (0: A, 1: Bt), uint64 holding 32 bits."""
    n = (ROWS_B if panel else ROWS_A) * 16 * ksteps
    return fmix32(seed ^ (set_ << 23 | panel << 22 | np.arange(n, dtype=np.uint64)))


def operands(seed, set_, ksteps):
    """(A int8 [128, K], Bt int8 [256, K]), K = 64 ksteps: the words, little-endian."""
    a, bt = (panel_words(seed, set_, p, ksteps).astype("<u4").view(np.int8) for p in (0, 1))
    return a.reshape(ROWS_A, -1), bt.reshape(ROWS_B, -1)


def product(seed, set_, ksteps):
    a, bt = operands(seed, set_, ksteps)
    return a.astype(np.int64) @ bt.astype(np.int64).T


def fold(words, first=0):
    """sum of rotl32(word, i & 31) mod 2^32, i counted from `first`."""
    s = (first + np.arange(len(words), dtype=np.uint64)) & 31
    return int(((words << s | words >> (32 - s)) & M32).sum() & M32)


def set_of(lap, laps, sets, g=0):
    return ((g if lap < laps - laps % sets else 0) + lap) % sets


def valu_final(seed, laps, ksteps):
    """Every thread's chain value after the launch, uint64 [512]."""
    s = fmix32(seed ^ 0x80000000 ^ np.arange(BLOCK, dtype=np.uint64))
    for gi in range(laps * ksteps):
        for _ in range(VALU_ROUNDS):
            s = fmix32(s ^ gi)
    return s


def digests(seed, laps, ksteps, sets):
    """The four workgroup digests of a healthy CU."""
    d = dict.fromkeys(PARTS, 0)
    weight = 2 * np.arange(ROWS_A * ROWS_B, dtype=np.int64) + 1
    per_set = {}
    for lap in range(laps):
        s = set_of(lap, laps, sets)
        if s not in per_set:
            fa = fold(panel_words(seed, s, 0, ksteps))
            fb = fold(panel_words(seed, s, 1, ksteps), ROWS_A * 16 * ksteps)
            # int64 wraps mod 2^64, of which 2^32 is a divisor
            per_set[s] = (fa + fb, 4 * fa + 2 * fb, int((product(seed, s, ksteps).ravel() * weight).sum()))
        for part, v in zip(PARTS, per_set[s]):
            d[part] = (d[part] + v) & M32
    t = np.arange(BLOCK, dtype=np.uint64)
    d["valu"] = int((valu_final(seed, laps, ksteps) * (2 * t + 1) & M32).sum() & M32)
    return d
