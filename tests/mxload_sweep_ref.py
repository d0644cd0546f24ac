"""Independent reference of the MX load sweep (csrc/hip/mxload_sweep.hip):
numpy only, nothing shared with the C++. The element and scale bytes from the
keys, the e2m1 decode, the product in int64 units of 2^-3, the two folds and
the gemm digest mod 2^32, in the logical order of the operands."""
import numpy as np

PARTS = ["operand", "scale", "gemm"]
BLOCK = 512
ROWS_A, ROWS_B = 128, 256
M32 = 0xFFFFFFFF
E2M1 = np.array([0, 0.5, 1, 1.5, 2, 3, 4, 6, -0.0, -0.5, -1, -1.5, -2, -3, -4, -6])


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


def scale_bytes(seed, set_, panel, ksteps):
    """E8M0 codes uint8 [rows, 4 ksteps]: block g of (row, step) from bits 8g.. of the hash."""
    rows = ROWS_B if panel else ROWS_A
    h = fmix32(seed ^ (1 << 30 | set_ << 23 | panel << 22 | np.arange(rows * ksteps, dtype=np.uint64)))
    bits = h[:, None] >> (8 * np.arange(4, dtype=np.uint64))
    code = 127 + (bits & 1) if panel else 126 + (bits & 3)
    return code.astype(np.uint8).reshape(rows, 4 * ksteps)


def operands(seed, set_, ksteps):
    """(A bytes [128, 64 ksteps], Bt bytes [256, 64 ksteps], A scales, Bt scales)."""
    a, bt = (panel_words(seed, set_, p, ksteps).astype("<u4").view(np.uint8) for p in (0, 1))
    return (a.reshape(ROWS_A, -1), bt.reshape(ROWS_B, -1), scale_bytes(seed, set_, 0, ksteps),
            scale_bytes(seed, set_, 1, ksteps))


def values(packed, scales):
    """The scaled elements as float64 [rows, K]: low nibble first, one scale per 32 of k."""
    codes = np.stack([packed & 15, packed >> 4], axis=-1).reshape(packed.shape[0], -1)
    return E2M1[codes] * np.repeat(np.exp2(scales.astype(np.int64) - 127), 32, axis=1)


def product_units(seed, set_, ksteps):
    """8 C as int64 [128, 256]; the bound that keeps every float32 partial sum exact is asserted."""
    a, bt, sa, sbt = operands(seed, set_, ksteps)
    va, vb = values(a, sa), values(bt, sbt)
    assert np.abs(va).max() <= 24 and np.abs(vb).max() <= 12 and 255 not in sa and 255 not in sbt
    assert (np.abs(va) @ np.abs(vb).T * 8).max() < 1 << 24  # any partial sum in any order
    c8 = va @ vb.T * 8  # float64 holds these sums exactly: they are below 2^24 units
    assert (c8 == np.rint(c8)).all()
    return c8.astype(np.int64)


def product(seed, set_, ksteps):
    """C as float32 [128, 256]: exact."""
    return (product_units(seed, set_, ksteps) / 8).astype(np.float32)


def fold(words, first=0):
    """sum of rotl32(word, i & 31) mod 2^32, i counted from `first`."""
    s = (first + np.arange(len(words), dtype=np.uint64)) & 31
    return int(((words << s | words >> (32 - s)) & M32).sum() & M32)


def set_of(lap, laps, sets, g=0):
    return ((g if lap < laps - laps % sets else 0) + lap) % sets


def digests(seed, laps, ksteps, sets):
    """The three workgroup digests of a healthy CU. An A operand dword is read
    by four waves and a Bt dword by two; a scale word by both lane halves of each."""
    d = dict.fromkeys(PARTS, 0)
    weight = 2 * np.arange(ROWS_A * ROWS_B, dtype=np.int64) + 1
    per_set = {}
    for lap in range(laps):
        s = set_of(lap, laps, sets)
        if s not in per_set:
            fa = fold(panel_words(seed, s, 0, ksteps))
            fb = fold(panel_words(seed, s, 1, ksteps), ROWS_A * 16 * ksteps)
            sa, sb = (scale_bytes(seed, s, p, ksteps).view("<u4").ravel().astype(np.uint64) for p in (0, 1))
            # int64 wraps mod 2^64, of which 2^32 is a divisor
            per_set[s] = (4 * fa + 2 * fb, 8 * fold(sa) + 4 * fold(sb, ROWS_A * ksteps),
                          int((product_units(seed, s, ksteps).ravel() * weight).sum()))
        for part, v in zip(PARTS, per_set[s]):
            d[part] = (d[part] + v) & M32
    return d
