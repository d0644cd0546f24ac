"""Independent reference of the fetch sweep (csrc/hip/fetch_sweep.hip) in
Python integers: the hash, the key, the literal and the encoding kind of every
step of every region, the segment order per wave, the `call` permutation, the
`align` targets, the flat index of every word, the words of every thread and
the digest of every part. It shares nothing with the C++; numpy only carries
256 lanes at a time.

A step first rotates the accumulator left by 5 (v_alignbit_b32 acc, acc, acc,
27), then, by the kind j & 3 of its place j in the run of steps it stands in:
  0 V  acc ^= L                       (VOP2 with a literal)
  1 S  s = C ^ L; acc ^= s            (SOP2 with a literal)
  2 K  s += sext16(L); acc ^= s       (SOPK, on the s that kind 1 left)
  3 X  acc = (acc ^ C) + thread       (VOP3 without a literal)
s is an SGPR of the wave, C = 0x5bd1e995.
"""
from __future__ import annotations

from functools import lru_cache

import numpy as np

M32 = 0xFFFFFFFF
PARTS = ["stream", "loop", "call", "align", "refill"]
BLOCK = 256
KINDS = "VSKX"
KIND_BYTES = {"V": 16, "S": 20, "K": 16, "X": 16}  # the 8-byte rotate and what follows it

# Regions.
STREAM, LOOP0, CALL, ALIGN = 0, 1, 5, 6
SEGMENTS, SEGMENT_BYTES, SEGMENT_STRIDE = 32, 8192, 512
LOOP_BYTES = [16, 64, 1024, 16384]
LOOP_TRIPS = [2048, 512, 64, 16]
CALL_BLOCKS, BLOCK_BYTES, BLOCK_STRIDE = 256, 64, 4
TRAMPOLINES, TARGETS = 32, 17
RETURN_BYTES = 4  # s_setpc_b64


def fmix32(h: int) -> int:
    h &= M32
    h ^= h >> 16
    h = h * 0x85EBCA6B & M32
    h ^= h >> 13
    h = h * 0xC2B2AE35 & M32
    h ^= h >> 16
    return h


def key(region: int, i: int) -> int:
    """A bijection of (region < 4096, step < 2^20)."""
    assert 0 <= region < 1 << 12 and 0 <= i < 1 << 20
    return region << 20 | i


@lru_cache(maxsize=None)
def literal(region: int, i: int) -> int:
    return fmix32(key(region, i)) | 0x01000100


def kind(i: int) -> str:
    return KINDS[i & 3]


def steps_that_fit(nbytes: int) -> tuple[int, int]:
    """(steps, s_nop 0 behind them) of a run that fills `nbytes`: steps in kind
    order from kind 0 while the next one fits, then padding."""
    n = used = 0
    while used + KIND_BYTES[kind(n)] <= nbytes:
        used += KIND_BYTES[kind(n)]
        n += 1
    assert (nbytes - used) % 4 == 0
    return n, (nbytes - used) // 4


SEGMENT_STEPS, SEGMENT_NOPS = steps_that_fit(SEGMENT_BYTES - RETURN_BYTES)
LOOP_STEPS = [steps_that_fit(b)[0] for b in LOOP_BYTES]
LOOP_NOPS = [steps_that_fit(b)[1] for b in LOOP_BYTES]
BLOCK_STEPS, BLOCK_NOPS = steps_that_fit(BLOCK_BYTES - RETURN_BYTES)


def run_steps(region: int) -> list[list[int]]:
    """The step indexes of every run of a region, runs in address order."""
    if region == STREAM:
        return [[s * SEGMENT_STRIDE + j for j in range(SEGMENT_STEPS)] for s in range(SEGMENTS)]
    if LOOP0 <= region < LOOP0 + 4:
        return [list(range(LOOP_STEPS[region - LOOP0]))]
    if region == CALL:  # the extra block (b = 256) lies in front of block 0
        return [[b * BLOCK_STRIDE + j for j in range(BLOCK_STEPS)] for b in [CALL_BLOCKS, *range(CALL_BLOCKS)]]
    assert region == ALIGN
    return [[k] for k in range(TARGETS)]


def region_literals(region: int) -> list[int]:
    """The literals of a region that stand in its code, in address order: a step of kind X has none, a step of
    kind K holds the low 16 bits."""
    out = []
    for run in run_steps(region):
        for j, i in enumerate(run):
            k = "V" if region == ALIGN else kind(j)
            if k == "K":
                out.append(literal(region, i) & 0xFFFF)
            elif k != "X":
                out.append(literal(region, i))
    return out


def distinct_literals(region: int) -> tuple[int, int]:
    """(32-bit literals in the code of a region, how many of them are distinct)."""
    lits = []
    for run in run_steps(region):
        lits += [literal(region, i) for j, i in enumerate(run) if region == ALIGN or kind(j) in "VS"]
    return len(lits), len(set(lits))


def start_values(seed: int, part: int, sub: int) -> np.ndarray:
    return np.array([fmix32(seed ^ (part << 28 | sub << 16 | t)) for t in range(BLOCK)], np.uint32)


def segment_order(wave: int) -> list[int]:
    return [(8 * wave + k) % SEGMENTS for k in range(SEGMENTS)]


def call_order(seed: int, r: int) -> list[int]:
    h = fmix32(seed + 0x9E3779B9 * (r + 1))
    a, b = (h & 0xFF) | 1, (h >> 8) & 0xFF
    return [(a * i + b) % CALL_BLOCKS for i in range(CALL_BLOCKS)]


def target_of(j: int) -> int:
    return j if j < TARGETS else j - TARGETS


def rotl5(v: np.ndarray) -> np.ndarray:
    return (v << np.uint32(5)) | (v >> np.uint32(27))


C = 0x5BD1E995


class Lanes:
    """Lanes `threads` of one wave order: `acc` per lane, one `s`."""

    def __init__(self, acc: np.ndarray, threads: np.ndarray | None = None):
        self.acc = acc.astype(np.uint32).copy()
        self.t = (np.arange(BLOCK) if threads is None else threads).astype(np.uint32)
        self.s = 0

    def run(self, region: int, steps: list[int]) -> None:
        for j, i in enumerate(steps):
            lit = literal(region, i)
            acc = rotl5(self.acc)
            k = kind(j)
            if k == "V":
                acc ^= np.uint32(lit)
            elif k == "S":
                self.s = C ^ lit
                acc ^= np.uint32(self.s)
            elif k == "K":
                low = lit & 0xFFFF
                self.s = (self.s + (low - 0x10000 if low & 0x8000 else low)) & M32
                acc ^= np.uint32(self.s)
            else:
                acc = (acc ^ np.uint32(C)) + self.t  # uint32 arithmetic wraps
            self.acc = acc


def rows_of(part: str, rounds: int) -> int:
    return {"stream": SEGMENTS, "loop": 4 * rounds, "call": rounds, "align": TRAMPOLINES, "refill": 2}[part]


def flat_index(row: int, thread: int) -> int:
    return row * BLOCK + thread


@lru_cache(maxsize=None)
def _words(part: str, seed: int, rounds: int) -> np.ndarray:
    p = PARTS.index(part)
    out = np.zeros((rows_of(part, rounds), BLOCK), np.uint32)
    if part == "stream":
        segs = run_steps(STREAM)
        start = start_values(seed, p, 0)
        for w in range(4):
            lanes = Lanes(start[64 * w:64 * w + 64], np.arange(64 * w, 64 * w + 64))
            for k, s in enumerate(segment_order(w)):
                lanes.run(STREAM, segs[s])
                out[k, 64 * w:64 * w + 64] = lanes.acc
    elif part == "loop":
        for b in range(4):
            lanes = Lanes(start_values(seed, p, b))
            body = run_steps(LOOP0 + b)[0]
            for r in range(rounds):
                for _ in range(LOOP_TRIPS[b]):
                    lanes.run(LOOP0 + b, body)
                out[b * rounds + r] = lanes.acc
    elif part == "call":
        lanes = Lanes(start_values(seed, p, 0))
        extra = [CALL_BLOCKS * BLOCK_STRIDE + j for j in range(BLOCK_STEPS)]
        for r in range(rounds):
            for b in call_order(seed, r):
                lanes.run(CALL, [b * BLOCK_STRIDE + j for j in range(BLOCK_STEPS)])
                lanes.run(CALL, extra)
            out[r] = lanes.acc
    elif part == "align":
        acc = start_values(seed, p, 0)
        for j in range(TRAMPOLINES):
            acc = rotl5(acc ^ np.uint32(literal(ALIGN, target_of(j))))
            out[j] = acc
    else:
        lanes = Lanes(start_values(seed, p, 0))
        lanes.run(LOOP0 + 3, run_steps(LOOP0 + 3)[0])
        out[0] = out[1] = lanes.acc
    out.setflags(write=False)
    return out


def words(part: str, seed: int, rounds: int = 1) -> np.ndarray:
    """uint32 [rows, 256]: what every thread of a healthy CU hands over. Read-only, computed once."""
    return _words(part, seed & M32, rounds)


def digest(w: np.ndarray) -> int:
    flat = w.reshape(-1).astype(np.uint64)
    idx = np.arange(flat.size, dtype=np.uint64)
    return int((flat * (2 * idx + 1) & np.uint64(M32)).sum() & np.uint64(M32))


def digests(parts, seed: int, rounds: int = 1) -> dict:
    return {p: digest(words(p, seed, rounds)) for p in parts}
