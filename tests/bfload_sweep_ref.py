"""Independent reference of the bf16 load sweep (csrc/hip/bfload_sweep.hip):
numpy only, nothing shared with the C++. The masked bf16 elements from the
keys, their decode to float64, the product in int64 units of 2^-14, set_of, the
three folds and the gemm digest mod 2^32, in the logical order of the operands."""
import numpy as np

PARTS = ["stage", "operand", "transpose", "gemm"]
BLOCK = 512
ROWS_A, COLS_B = 128, 256
M32 = 0xFFFFFFFF


def fmix32(h):
    h = np.asarray(h, np.uint64) & M32
    h ^= h >> 16
    h = h * 0x85EBCA6B & M32
    h ^= h >> 13
    h = h * 0xC2B2AE35 & M32
    return h ^ h >> 16


def panel_words(seed, set_, panel, ksteps):
    """The dwords of one panel (0: A, 1: B), uint64 holding 32 bits: two bf16
    with sign and mantissa from the hash and the biased exponent 127."""
    n = (4096 if panel else 2048) * ksteps
    return fmix32(seed ^ (set_ << 23 | panel << 22 | np.arange(n, dtype=np.uint64))) & 0x807F807F | 0x3F803F80


def operands(seed, set_, ksteps):
    """(A bits uint16 [128, 32 ksteps], B bits uint16 [32 ksteps, 256]), low half first."""
    a, b = (panel_words(seed, set_, p, ksteps).astype("<u4").view("<u2") for p in (0, 1))
    return a.reshape(ROWS_A, -1), b.reshape(-1, COLS_B)


def values(bits):
    """bf16 bits as float64: the float32 whose upper half they are."""
    return (bits.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def product_units(seed, set_, ksteps):
    """C 2^14 as int64 [128, 256]; the bound that keeps every float32 partial sum exact is asserted."""
    va, vb = (values(x) for x in operands(seed, set_, ksteps))
    assert (np.abs(va) @ np.abs(vb) * 2 ** 14).max() < 1 << 24  # any partial sum in any order
    c = va @ vb * 2 ** 14  # float64 holds these sums exactly: they are below 2^24 units
    assert (c == np.rint(c)).all()
    return c.astype(np.int64)


def product(seed, set_, ksteps):
    """C as float32 [128, 256]: exact."""
    return (product_units(seed, set_, ksteps) / 2 ** 14).astype(np.float32)


def fold(words, index):
    """sum of rotl32(word, index & 31) mod 2^32."""
    s = np.asarray(index, np.uint64) & 31
    return int(((words << s | words >> (32 - s)) & M32).sum() & M32)


def transposed_words(b):
    """B as the transposed reads deliver it: word (j, n) = B[2j][n] | B[2j+1][n] << 16, index 256 j + n."""
    return (b[0::2].astype(np.uint64) | b[1::2].astype(np.uint64) << 16).ravel()


def set_of(lap, laps, sets, g=0):
    return ((g if lap < laps - laps % sets else 0) + lap) % sets


def digests(seed, laps, ksteps, sets):
    """The four workgroup digests of a healthy CU. Every dword is staged once; an
    A dword is read back by four waves, a transposed B word by two."""
    d = dict.fromkeys(PARTS, 0)
    weight = 2 * np.arange(ROWS_A * COLS_B, dtype=np.int64) + 1
    per_set = {}
    for lap in range(laps):
        s = set_of(lap, laps, sets)
        if s not in per_set:
            a, b = panel_words(seed, s, 0, ksteps), panel_words(seed, s, 1, ksteps)
            fa = fold(a, np.arange(len(a)))
            tr = transposed_words(operands(seed, s, ksteps)[1])
            # int64 wraps mod 2^64, of which 2^32 is a divisor
            per_set[s] = (fa + fold(b, len(a) + np.arange(len(b))), 4 * fa, 2 * fold(tr, np.arange(len(tr))),
                          int((product_units(seed, s, ksteps).ravel() * weight).sum()))
        for part, v in zip(PARTS, per_set[s]):
            d[part] = (d[part] + v) & M32
    return d
