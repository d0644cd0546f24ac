"""numpy reference of the HBM sweep's pattern (csrc/hip/hbm_sweep.hip), written
from the formula, not from the C++:

    mix32(x): x ^= x>>16; x *= 0x7feb352d; x ^= x>>15; x *= 0x846ca68b; x ^= x>>16
    word_j(v) = mix32(lo + 0x9E3779B9*(j+1)) ^ mix32(hi ^ seed)     j = 0..3, mod 2^32

with lo / hi the halves of the 64-bit vector index v; the inverted pattern is
the complement."""
from functools import lru_cache

import numpy as np

M = np.uint64(0xFFFFFFFF)
SEED = 0x5EED1E55


def mix32(x: np.ndarray) -> np.ndarray:
    x = x.astype(np.uint64) & M
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & M
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846CA68B)) & M
    x ^= x >> np.uint64(16)
    return x


def pattern_of(v: np.ndarray, seed: int = SEED, inverted: bool = False) -> np.ndarray:
    """uint32 [len(v), 4] for the vector indices `v` (uint64)."""
    v = np.asarray(v, dtype=np.uint64)
    lo, hi = v & M, v >> np.uint64(32)
    hterm = mix32(hi ^ np.uint64(seed))
    out = np.empty((len(v), 4), np.uint32)
    for j in range(4):
        w = mix32((lo + np.uint64(0x9E3779B9 * (j + 1) & 0xFFFFFFFF)) & M) ^ hterm
        out[:, j] = (~w & M if inverted else w).astype(np.uint32)
    return out


@lru_cache(maxsize=8)
def _pattern(first_vec: int, n: int, seed: int, inverted: bool) -> np.ndarray:
    out = pattern_of(np.uint64(first_vec) + np.arange(n, dtype=np.uint64), seed, inverted)
    out.setflags(write=False)  # shared among tests
    return out


def pattern(first_vec: int, n: int, seed: int = SEED, inverted: bool = False) -> np.ndarray:
    return _pattern(int(first_vec), int(n), int(seed), bool(inverted))


def fold(words: np.ndarray) -> int:
    """XOR of the two little-endian 64-bit halves of every vector."""
    return int(np.bitwise_xor.reduce(np.ascontiguousarray(words).view(np.uint64).ravel()))
