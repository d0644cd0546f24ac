"""Independent reference of the attention load sweep (csrc/hip/attnload_sweep.hip):
numpy only, nothing shared with the C++. The operands from the hash, S, e, m, l
and O in float64 (exact there), set_of and the five digests mod 2^32."""
import numpy as np

PARTS = ["stage", "score", "stat", "transpose", "out"]
ROWS, DIM, BLOCK_KEYS = 256, 64, 64
M32 = 0xFFFFFFFF


def fmix32(h):
    h = np.asarray(h, np.uint64) & M32
    h ^= h >> 16
    h = h * 0x85EBCA6B & M32
    h ^= h >> 13
    h = h * 0xC2B2AE35 & M32
    return h ^ h >> 16


def panel_words(seed, set_, panel, kvsteps):
    """The dwords of one panel (0: Q, 1: K, 2: V) in its logical order, uint64 holding 32 bits."""
    h = fmix32(seed ^ (set_ << 23 | panel << 21 | np.arange(2048 * kvsteps if panel else 8192, dtype=np.uint64)))
    if panel < 2:  # two bf16 of one binade: sign and mantissa from the hash
        return h & 0x807F807F | (0x3F803F80 if panel else 0x3D803D80)
    b = np.stack([h & 0xFF, h >> 16 & 0xFF])  # a byte per half: the integer +-(b & 127) as bf16
    half = (b & 127).astype(np.float32).view(np.uint32).astype(np.uint64) >> 16 | (b & 128) << 8
    return half[0] | half[1] << 16


def operands(seed, set_, kvsteps):
    """(Q bits uint16 [256, 64], K bits [64 kvsteps, 64], V bits [64 kvsteps, 64]), low half first."""
    return tuple(panel_words(seed, set_, p, kvsteps).astype("<u4").view("<u2").reshape(-1, DIM) for p in range(3))


def values(bits):
    """bf16 bits as float64: the float32 whose upper half they are."""
    return (bits.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def attention(seed, set_, kvsteps):
    """{"e": clamped exponents [256, N], "m" [256], "l" [256], "out" [256, 64] unnormalised, "first_m": the
    running maximum after the first key block}, all float64 and exact; the bounds of the header are asserted."""
    q, k, v = (values(x) for x in operands(seed, set_, kvsteps))
    assert (np.abs(q) @ np.abs(k).T).max() < 16  # any partial sum of S in any order: 22 bits
    assert np.abs(v).sum(0).max() * 128 < 1 << 24  # any partial sum of O at any running maximum
    e = np.clip(np.floor(q @ k.T), -4, 3)
    m = e.max(1)
    p = 2.0 ** (e - m[:, None])
    return {"e": e, "m": m, "l": p.sum(1), "out": p @ v, "first_m": e[:, :BLOCK_KEYS].max(1)}


def fold(words, index):
    """sum of rotl32(word, index & 31) mod 2^32."""
    s = np.asarray(index, np.uint64) & 31
    return int(((words << s | words >> (32 - s)) & M32).sum() & M32)


def set_of(lap, laps, sets, g=0):
    return ((g if lap < laps - laps % sets else 0) + lap) % sets


def set_digests(seed, set_, kvsteps):
    """The five digests of one lap on one set, mod 2^32."""
    n = BLOCK_KEYS * kvsteps
    q, k, v = (panel_words(seed, set_, p, kvsteps) for p in range(3))
    # The arena's order: Q, then per key block its 2,048 dwords of K and its 2,048 of V.
    arena = np.concatenate([q] + [x[2048 * t:2048 * (t + 1)] for t in range(kvsteps) for x in (k, v)])
    vb = operands(seed, set_, kvsteps)[2].astype(np.uint64)
    tr = (vb[0::2] | vb[1::2] << 16).ravel()  # word (j, n) = V[2j][n] | V[2j+1][n] << 16, index 64 j + n
    a = attention(seed, set_, kvsteps)
    rows = np.arange(ROWS, dtype=np.int64)
    # int64 wraps mod 2^64, of which 2^32 is a divisor
    score = ((a["e"] + 4).astype(np.int64) * (2 * (n * rows[:, None] + np.arange(n)) + 1)).sum()
    stat = ((a["l"] * 128).astype(np.int64) * (2 * rows + 1) + (a["m"] + 4).astype(np.int64) * (2 * (ROWS + rows) + 1)).sum()
    out = ((a["out"] * 128).astype(np.int64).ravel() * (2 * np.arange(ROWS * DIM, dtype=np.int64) + 1)).sum()
    return [fold(arena, np.arange(len(arena))), int(score) & M32, 2 * int(stat) & M32,  # a row is held by two lanes
            8 * fold(tr, np.arange(len(tr))) & M32, int(out) & M32]  # every wave reads all of V


def digests(seed, laps, kvsteps, sets):
    """The five workgroup digests of a healthy CU."""
    per_set = {s: set_digests(seed, s, kvsteps) for s in {set_of(lap, laps, sets) for lap in range(laps)}}
    return {part: sum(per_set[set_of(lap, laps, sets)][i] for lap in range(laps)) & M32 for i, part in enumerate(PARTS)}
