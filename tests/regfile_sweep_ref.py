"""numpy reference of the register-file sweep's pattern and digest, written
from the formulas and not from the C:

    c(r)     = (((r + 1) * 0x9E3779B1) mod 2^32) ^ seed          r = 0..511
    p0(r, l) = c(r) * (2l + 1) mod 2^32                          l = 0..63
    p1       = ~p0
    D_s      = sum_{r,l} p_s(r, l) * (2(64r + l) + 1) mod 2^32
    wave     = D_0 ^ rotl(D_1, 16)
    group    = sum_{w<4} wave << w  mod 2^32   (= 15 * wave)
"""
import numpy as np

CELLS, LANES = 512, 64
M = 0xFFFFFFFF
SEEDS = (0x5BD1E995, 0xA5A5A5A5)


def pattern(seed: int, inverted: bool = False) -> np.ndarray:
    """uint64 [512, 64] holding the 32-bit value of every cell of a wave."""
    r = np.arange(CELLS, dtype=np.uint64)[:, None]
    lane = np.arange(LANES, dtype=np.uint64)[None, :]
    c = (((r + 1) * 0x9E3779B1) & M) ^ np.uint64(seed)
    p = (c * (2 * lane + 1)) & M
    return (p ^ np.uint64(M)) if inverted else p


def pass_digest(values: np.ndarray) -> int:
    r = np.arange(CELLS, dtype=np.uint64)[:, None]
    lane = np.arange(LANES, dtype=np.uint64)[None, :]
    w = 2 * (64 * r + lane) + 1
    return int(((values * w) & M).sum() & M)  # 32768 terms below 2^32: no uint64 overflow


def rotl(x: int, s: int) -> int:
    return ((x << s) | (x >> (32 - s))) & M


def wave_digest(seed: int) -> int:
    return pass_digest(pattern(seed)) ^ rotl(pass_digest(pattern(seed, True)), 16)


def group_digest(seed: int) -> int:
    d = wave_digest(seed)
    return sum(d << w for w in range(4)) & M
