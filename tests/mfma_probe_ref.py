"""Plain numpy reference (float64 / int64) for csrc/hip/mfma_probe.hip and the
health pattern of csrc/hip/hbm_probe.hip. Nothing here comes from the C side:
the maps are the ones the header of mfma_probe.hip documents.

v_mfma_f32_32x32x16_bf16, lane l, r = l & 31, h = l >> 5:
  * operand element j (0..7) of the lane is A[r][8h + j] and B[8h + j][r];
  * accumulator register q (0..15) is C[(q & 3) + 8 (q >> 2) + 4h][r]."""
import numpy as np

LANES, FRAG, REGS, TILE, STEP = 64, 8, 16, 32, 16
PEAK_THREADS, PEAK_ACC = 256, 4  # k_mfma_peak: 4 waves, 4 accumulators per wave
FLOP_PER_MFMA = 2 * 32 * 32 * 16  # 32,768


# --------------------------------------------------------------------- bf16
def bf16_decode(bits) -> np.ndarray:
    """bf16 bit patterns (uint16) -> float64, exactly."""
    b = np.asarray(bits, np.uint16)
    with np.errstate(invalid="ignore"):  # a signalling NaN pattern widens to a quiet one
        return (b.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def bf16_encode(x) -> np.ndarray:
    """float -> bf16 bit patterns, round to nearest even; NaN -> quiet NaN."""
    f = np.asarray(x, np.float64).astype(np.float32)
    u = np.ascontiguousarray(f).view(np.uint32).astype(np.uint64)
    rounded = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    nan = np.isnan(f)
    return np.where(nan, ((u >> 16) & 0x8000 | 0x7FC0).astype(np.uint16), rounded).astype(np.uint16)


def bf16_exact(x) -> np.ndarray:
    """Bit patterns of values that must be representable in bf16 as they are."""
    x = np.asarray(x, np.float64)
    bits = bf16_encode(x)
    back = bf16_decode(bits)
    assert np.array_equal(back, x, equal_nan=True), "not exact in bf16"
    return bits


# ------------------------------------------------------------ the product
def tile_float64(a_bits, b_bits) -> np.ndarray:
    """C[32, 32] = A·B in float64 from bf16 bit patterns, one rank-1 update
    per k (Inf and NaN propagate as IEEE arithmetic has them)."""
    a, b = bf16_decode(a_bits), bf16_decode(b_bits)
    assert a.shape[0] == TILE and b.shape == (a.shape[1], TILE)
    c = np.zeros((TILE, TILE), np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(a.shape[1]):
            c += a[:, k:k + 1] * b[k:k + 1, :]
    return c


def tile_int64(a_int, b_int) -> np.ndarray:
    return np.asarray(a_int, np.int64) @ np.asarray(b_int, np.int64)


def abs_product_sum(a_bits, b_bits) -> np.ndarray:
    """sum_k |a_ik| |b_kj| in float64."""
    return np.abs(bf16_decode(a_bits)) @ np.abs(bf16_decode(b_bits))


# ------------------------------------------------------------------- maps
def operand_index(lane: int, j: int) -> tuple[int, int]:
    """(r, k): element j of lane's fragment is A[r][k] and B[k][r]."""
    return lane & 31, 8 * (lane >> 5) + j


def c_index(lane: int, q: int) -> tuple[int, int]:
    """(row, col) of accumulator register q of a lane."""
    return (q & 3) + 8 * (q >> 2) + 4 * (lane >> 5), lane & 31


def tiles_from_fragments(a_frag, b_frag) -> tuple[np.ndarray, np.ndarray]:
    """One wave's fragments [64, 8] through the operand map: A[32, 16], B[16, 32]."""
    a, b = np.zeros((TILE, STEP), np.float64), np.zeros((STEP, TILE), np.float64)
    for lane in range(LANES):
        for j in range(FRAG):
            r, k = operand_index(lane, j)
            a[r, k] = a_frag[lane][j]
            b[k, r] = b_frag[lane][j]
    return a, b


def lanes_from_tile(c) -> np.ndarray:
    """A C[32, 32] as the accumulators hold it: [64 lanes, 16 registers]."""
    out = np.zeros((LANES, REGS), np.float64)
    for lane in range(LANES):
        for q in range(REGS):
            out[lane, q] = c[c_index(lane, q)]
    return out


# -------------------------------------------------------------- k_mfma_peak
def peak_fragments() -> tuple[np.ndarray, np.ndarray]:
    """Every thread's operands from the kernel's formula: [256, 8] each."""
    tid = np.arange(PEAK_THREADS)[:, None]
    j = np.arange(FRAG)[None, :]
    return 0.125 * ((tid + j) & 7), 0.0625 * ((3 * tid + j) & 15)


def peak_tiles() -> np.ndarray:
    """T[4 waves, 32, 32]: the float64 product of each wave's operands."""
    fa, fb = peak_fragments()
    bf16_exact(fa), bf16_exact(fb)
    out = np.zeros((PEAK_THREADS // LANES, TILE, TILE), np.float64)
    for w in range(PEAK_THREADS // LANES):
        a, b = tiles_from_fragments(fa[LANES * w:LANES * (w + 1)], fb[LANES * w:LANES * (w + 1)])
        out[w] = a @ b
    return out


def peak_accumulators(iters: int) -> np.ndarray:
    """What every accumulator of a workgroup holds after `iters` steps:
    [256 threads, 16 registers], float64 (the same for each of the kAcc)."""
    t = peak_tiles()
    return iters * np.concatenate([lanes_from_tile(t[w]) for w in range(t.shape[0])])


def peak_exact_iters_limit() -> float:
    """Every T is a multiple of 2^-7, so iters x T is exact in fp32, whatever
    the order of the additions, while iters x max T < 2^24 x 2^-7."""
    t = peak_tiles()
    assert np.array_equal(t * 128, np.round(t * 128))
    return (1 << 17) / float(t.max())


def peak_flops(active_blocks: int, iters: int) -> int:
    return active_blocks * (PEAK_THREADS // LANES) * PEAK_ACC * iters * FLOP_PER_MFMA


# --------------------------------------------------------- xs_mfma_check
def check_inputs(k: int) -> tuple[np.ndarray, np.ndarray]:
    """The production check's integers: A[32, k] in [-8, 8], B[k, 32] in [-6, 6]."""
    i = np.arange(TILE)[:, None]
    kk = np.arange(k)[None, :]
    a = (3 * i + 7 * kk) % 17 - 8
    kr = np.arange(k)[:, None]
    j = np.arange(TILE)[None, :]
    b = (5 * kr + 11 * j + np.where(j > kr, 3, 0)) % 13 - 6
    return a.astype(np.int64), b.astype(np.int64)


# ------------------------------------------------------------ health pattern
def health_pattern(n: int) -> np.ndarray:
    """k_pattern: word i = uint32(i * 2654435761) ^ 0xa5a5a5a5."""
    i = np.arange(n, dtype=np.uint64)
    return (((i * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)) ^ np.uint64(0xA5A5A5A5)).astype(np.uint32)
