"""numpy reference of the lane sweep (csrc/hip/lane_sweep.hip), written from
the lane maps and the hash definition in that file's header. It shares no
code with the C++: every expected array is built by moving source values with
index arithmetic, the way the instruction is documented to move them.

A launch's thread is t = 64 * wave + lane; arrays are [step][word][256]."""
import numpy as np

SEEDS = (0x1B873593, 0xC0FFEE11)
PATHS = ["dpp", "permlane", "readlane", "bpermute", "ldswide", "ldstr", "ldsatomic", "ldsdma"]
SHAPES = {"dpp": (75, 1), "permlane": (4, 2), "readlane": (133, 1), "bpermute": (137, 1), "ldswide": (112, 4),
          "ldstr": (32, 2), "ldsatomic": (13, 4), "ldsdma": (6, 4)}
M32 = 0xFFFFFFFF
T = np.arange(256, dtype=np.int64)
LANE, WAVE = T & 63, T >> 6


def fmix32(h):
    """murmur3's 32-bit finaliser on an int64 array of 32-bit values."""
    h = np.asarray(h, np.int64) & M32
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & M32
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & M32
    h ^= h >> 16
    return h


def key(path, step, word, wave, lane, aux=0):
    return (aux << 28) | (PATHS.index(path) << 24) | (step << 12) | ((4 * wave + word) << 6) | lane


def src(seed, path, step, word, aux=0):
    """Source (aux=1: unmoved operand) values of one (step, word): [256] by thread."""
    return fmix32(seed ^ key(path, step, word, WAVE, LANE, aux))


def all_keys():
    """Every key a launch hashes, src and aux, as one array (with repeats removed by construction)."""
    out = []
    for p in PATHS:
        steps, words = SHAPES[p]
        for aux in (0, 1):
            for s in range(steps):
                for w in range(4):  # a path may use fewer; the key space is what must not collide
                    out.append(key(p, s, w, WAVE, LANE, aux))
    return np.concatenate(out)


def from_lane(values, lanes):
    """values[256] gathered so that thread t receives the value of lane lanes[t] of its own wave."""
    return values[(T & ~63) | (np.asarray(lanes) & 63)]


# ----------------------------------------------------------------------- dpp
def dpp_steps():
    """(name, source lane per lane or -1, row_mask, bank_mask, bound_ctrl) per step."""
    l = np.arange(64)
    row = l & 15
    out = []
    for sel in ([0, 1, 2, 3], [1, 2, 3, 0], [2, 3, 0, 1], [3, 0, 1, 2]):
        out.append((f"quad_perm:{sel}", (l & ~3) + np.array(sel)[l & 3], 0xF, 0xF, 0))
    for n in range(1, 16):
        out.append((f"row_shl:{n}", np.where(row + n <= 15, l + n, -1), 0xF, 0xF, 0))
    for n in range(1, 16):
        out.append((f"row_shr:{n}", np.where(row - n >= 0, l - n, -1), 0xF, 0xF, 0))
    for n in range(1, 16):
        out.append((f"row_ror:{n}", (l & ~15) | ((l - n) & 15), 0xF, 0xF, 0))
    out.append(("row_mirror", (l & ~15) | (15 - row), 0xF, 0xF, 0))
    out.append(("row_half_mirror", (l & ~7) | (7 - (l & 7)), 0xF, 0xF, 0))
    # A row the broadcast gives no source reads its own lane (settled on the hardware).
    out.append(("row_bcast15", np.where(l >= 16, (l & ~15) - 1, l), 0xF, 0xF, 0))
    out.append(("row_bcast31", np.where(l >= 32, 31, l), 0xF, 0xF, 0))
    out.append(("wave_shl:1", np.where(l < 63, l + 1, -1), 0xF, 0xF, 0))
    out.append(("wave_rol:1", (l + 1) & 63, 0xF, 0xF, 0))
    out.append(("wave_shr:1", np.where(l > 0, l - 1, -1), 0xF, 0xF, 0))
    out.append(("wave_ror:1", (l - 1) & 63, 0xF, 0xF, 0))
    for n in range(16):
        out.append((f"row_newbcast:{n}", (l & ~15) | n, 0xF, 0xF, 0))
    out.append(("row_shr:3 bound_ctrl", np.where(row - 3 >= 0, l - 3, -1), 0xF, 0xF, 1))
    out.append(("row_ror:5 row_mask:0xa bank_mask:0x5", (l & ~15) | ((l - 5) & 15), 0xA, 0x5, 0))
    return out


def dpp_enabled(row_mask, bank_mask):
    l = np.arange(64)
    return (((row_mask >> (l >> 4)) & 1) & ((bank_mask >> ((l & 15) >> 2)) & 1)).astype(bool)


def expected_dpp(seed):
    out = np.zeros((75, 1, 256), np.int64)
    for s, (_, lanes, rm, bm, bc) in enumerate(dpp_steps()):
        x, old = src(seed, "dpp", s, 0), src(seed, "dpp", s, 0, aux=1)
        lanes = np.tile(lanes, 4)
        moved = from_lane(x, np.maximum(lanes, 0))
        got = np.where(lanes >= 0, moved, 0 if bc else old)
        out[s, 0] = np.where(np.tile(dpp_enabled(rm, bm), 4), got, old)
    return out


# ------------------------------------------------------------------ permlane
def expected_permlane(seed):
    out = np.zeros((4, 2, 256), np.int64)
    for s in range(4):
        span = 32 if s < 2 else 16
        vdst, vsrc = src(seed, "permlane", s, 0).copy(), src(seed, "permlane", s, 1).copy()
        for w in range(4):
            for lo in range(0, 64, 2 * span):  # vdst lanes lo+span.. <-> src lanes lo..
                a = slice(64 * w + lo + span, 64 * w + lo + 2 * span)
                b = slice(64 * w + lo, 64 * w + lo + span)
                vdst[a], vsrc[b] = vsrc[b].copy(), vdst[a].copy()
        out[s, 0], out[s, 1] = vdst, vsrc
    return out


# ------------------------------------------------------------------ readlane
FIRST_LANES = (0, 1, 31, 32, 63)


def expected_readlane(seed):
    out = np.zeros((133, 1, 256), np.int64)
    for s in range(64):
        out[s, 0] = from_lane(src(seed, "readlane", s, 0), np.full(256, s))
    for s in range(64, 128):
        x = src(seed, "readlane", s, 0).copy()
        v = from_lane(src(seed, "readlane", s, 0, aux=1), np.zeros(256, np.int64))
        hit = LANE == s - 64
        x[hit] = v[hit]
        out[s, 0] = x
    for k, f in enumerate(FIRST_LANES):
        s = 128 + k
        x, keep = src(seed, "readlane", s, 0), src(seed, "readlane", s, 0, aux=1)
        out[s, 0] = np.where(LANE >= f, from_lane(x, np.full(256, f)), keep)
    return out


# ------------------------------------------------------------------ bpermute
def swizzle_steps():
    """(name, source lane per lane) of ds_swizzle steps 128..136."""
    l = np.arange(64)

    def bits(a, o, x):
        return (l & 32) | ((((l & 31) & a) | o) ^ x)

    out = [(f"xor:{x}", bits(0x1F, 0, x)) for x in (1, 2, 4, 8, 16)]
    out.append(("and:0x10", bits(0x10, 0, 0)))
    out.append(("or:3", bits(0x1F, 3, 0)))
    for sel in ([3, 2, 1, 0], [1, 2, 3, 0]):
        out.append((f"quad:{sel}", (l & ~3) + np.array(sel)[l & 3]))
    return out


def expected_bpermute(seed):
    out = np.zeros((137, 1, 256), np.int64)
    for s in range(64):  # dst[l] = src[(addr[l] >> 2) & 63], addr = 4 ((l + s) % 64)
        out[s, 0] = from_lane(src(seed, "bpermute", s, 0), (LANE + s) % 64)
    for s in range(64, 128):  # dst[(addr[l] >> 2) & 63] = src[l]
        x = src(seed, "bpermute", s, 0)
        dst = np.zeros(256, np.int64)
        dst[(T & ~63) | ((LANE + s - 64) % 64)] = x
        out[s, 0] = dst
    for k, (_, lanes) in enumerate(swizzle_steps()):
        out[128 + k, 0] = from_lane(src(seed, "bpermute", 128 + k, 0), np.tile(lanes, 4))
    return out


# ------------------------------------------------------------------- ldswide
def ldswide_dwords(rot):
    """The four dwords of its wave's tile that each lane's 16-byte slot holds: [64, 4]."""
    return 4 * ((np.arange(64)[:, None] + rot) % 64) + np.arange(4)[None, :]


def sext(v, bits):
    v = np.asarray(v, np.int64) & ((1 << bits) - 1)
    return np.where(v >> (bits - 1), v | (M32 ^ ((1 << bits) - 1)), v)


def expected_ldswide(seed):
    out = np.zeros((112, 4, 256), np.int64)
    for s in range(112):
        rot, combo = divmod(s, 7)
        x = np.stack([src(seed, "ldswide", s, j) for j in range(4)])  # [word][thread]
        if combo < 4:
            out[s] = x  # written with one width, read back whole with another
        elif combo == 4:  # bytes written, halves read: u16, i16, i16, u16
            out[s] = np.stack([x[0] & 0xFFFF, sext(x[0] >> 16, 16), sext(x[1], 16), x[1] >> 16])
        elif combo == 5:  # halves written, bytes read: u8, i8, i8, u8
            out[s] = np.stack([x[0] & 0xFF, sext(x[0] >> 8, 8), sext(x[1] >> 16, 8), x[1] >> 24])
        else:  # build each wave's 256-dword tile, read dwords D, D+64, D+128, D+192
            for w in range(4):
                tile = np.zeros(256, np.int64)
                tile[ldswide_dwords(rot)] = x[:, 64 * w:64 * w + 64].T
                d = (np.arange(64) + rot) % 64
                for j in range(4):
                    out[s, j, 64 * w:64 * w + 64] = tile[d + 64 * j]
    return out


# --------------------------------------------------------------------- ldstr
TR_ROWS, TR_COLS, TR_STRIDES = 16, 64, (128, 136)


def tr_tile(seed, stride_idx, wave):
    """The [16][64] tile of 16-bit elements of one wave."""
    i = ((stride_idx * 4 + wave) * TR_ROWS + np.arange(TR_ROWS)[:, None]) * TR_COLS + np.arange(TR_COLS)[None, :]
    return (i * 0x9E37 + seed) & 0xFFFF


def tr_block(step, group):
    """(block row, block column) that lane group `group` reads in `step`."""
    b = (step % 16 + 5 * group) % 16
    return b >> 2, b & 3


def tr_read(image, addr):
    """ds_read_b64_tr_b16 over a byte image of LDS: addr[64] per lane -> [64, 4] elements."""
    out = np.zeros((64, 4), np.int64)
    for g in range(4):
        for i in range(16):  # lane i of the group receives column i of the four rows
            for q in range(4):  # row q comes from the address lane 4q + p supplies, p = i // 4
                a = addr[16 * g + 4 * q + i // 4] + 2 * (i % 4)
                out[16 * g + i, q] = image[a] | image[a + 1] << 8
    return out


def expected_ldstr(seed):
    out = np.zeros((32, 2, 256), np.int64)
    l = np.arange(64)
    for s in range(32):
        h, stride = s // 16, TR_STRIDES[s // 16]
        for w in range(4):
            tile = tr_tile(seed, h, w)
            image = np.zeros(TR_ROWS * stride, np.int64)
            for r in range(TR_ROWS):  # little-endian elements, rows `stride` bytes apart
                image[r * stride:r * stride + 2 * TR_COLS:2] = tile[r] & 0xFF
                image[r * stride + 1:r * stride + 2 * TR_COLS:2] = tile[r] >> 8
            br = np.array([tr_block(s, g)[0] for g in l >> 4])
            bc = np.array([tr_block(s, g)[1] for g in l >> 4])
            i = l & 15
            addr = (4 * br + (i >> 2)) * stride + 2 * (16 * bc + 4 * (i & 3))
            assert (addr % 8 == 0).all() and (addr + 8 <= image.size).all()
            e = tr_read(image, addr)
            out[s, 0, 64 * w:64 * w + 64] = e[:, 0] | e[:, 1] << 16
            out[s, 1, 64 * w:64 * w + 64] = e[:, 2] | e[:, 3] << 16
    return out


# ----------------------------------------------------------------- ldsatomic
def s32(v):
    v = np.asarray(v, np.int64) & M32
    return np.where(v >> 31, v - (1 << 32), v)


ATOMIC_OPS = [
    ("add", lambda a, b: (a + b) & M32), ("sub", lambda a, b: (a - b) & M32), ("and", lambda a, b: a & b),
    ("or", lambda a, b: a | b), ("xor", lambda a, b: a ^ b),
    ("min_i32", lambda a, b: np.minimum(s32(a), s32(b)) & M32), ("max_i32", lambda a, b: np.maximum(s32(a), s32(b)) & M32),
    ("min_u32", np.minimum), ("max_u32", np.maximum), ("exchange", lambda a, b: b)]


def expected_ldsatomic(seed):
    out = np.zeros((13, 4, 256), np.int64)
    for s, (_, op) in enumerate(ATOMIC_OPS):
        for j in range(2):
            a, b = src(seed, "ldsatomic", s, 2 * j), src(seed, "ldsatomic", s, 2 * j, aux=1)
            out[s, 2 * j], out[s, 2 * j + 1] = a, op(a, b)
    for j in range(2):  # compare-swap: j = 0 compares with the word (swaps), j = 1 with word ^ 1 (does not)
        a, b = src(seed, "ldsatomic", 10, 2 * j), src(seed, "ldsatomic", 10, 2 * j, aux=1)
        out[10, 2 * j], out[10, 2 * j + 1] = a, (b if j == 0 else a)
    lo = [int(v) for v in src(seed, "ldsatomic", 11, 0)]
    hi = [int(v) for v in src(seed, "ldsatomic", 11, 1)]
    blo = [int(v) for v in src(seed, "ldsatomic", 11, 0, aux=1)]
    bhi = [int(v) for v in src(seed, "ldsatomic", 11, 1, aux=1)]
    for t in range(256):
        a, b = lo[t] | hi[t] << 32, blo[t] | bhi[t] << 32
        f = (a + b) & ((1 << 64) - 1)
        out[11, :, t] = [a & M32, a >> 32, f & M32, f >> 32]
    for j, name in enumerate(("add", "xor", "max_u32", "min_u32")):
        op = dict(ATOMIC_OPS)[name]
        v = src(seed, "ldsatomic", 12, j, aux=1)[0]  # thread 0 initialises the word
        for x in src(seed, "ldsatomic", 12, j):
            v = op(v, x)
        out[12, j] = v
    return out


# -------------------------------------------------------------------- ldsdma
def dma_source(seed):
    """The device buffer: [step][wave][64][4] of src(step, word j, lane q)."""
    g = np.zeros((6, 4, 64, 4), np.int64)
    for s in range(6):
        for j in range(4):
            g[s, :, :, j] = src(seed, "ldsdma", s, j).reshape(4, 64)
    return g


def dma_perm(step):
    return ((2 * step + 3) * np.arange(64) + step) % 64


def expected_ldsdma(seed):
    g = dma_source(seed)
    out = np.zeros((6, 4, 256), np.int64)
    for s in range(6):
        q = dma_perm(s)
        for w in range(4):
            lds = np.zeros(512, np.int64)  # the wave's tile in dwords; destination = base + lane * size
            if s < 2:  # four _dword, word j into plane j
                for j in range(4):
                    lds[64 * j + np.arange(64)] = g[s, w, q, j]
                got = [lds[64 * j + np.arange(64)] for j in range(4)]
            elif s < 4:  # _dwordx3 steps 16 B per lane (settled on the hardware); word 3 by _dword at 1024 + 4 l
                for j in range(3):
                    lds[4 * np.arange(64) + j] = g[s, w, q, j]
                lds[256 + np.arange(64)] = g[s, w, q, 3]
                got = [lds[4 * np.arange(64) + j] for j in range(3)] + [lds[256 + np.arange(64)]]
            else:  # _dwordx4 at 16 l
                for j in range(4):
                    lds[4 * np.arange(64) + j] = g[s, w, q, j]
                got = [lds[4 * np.arange(64) + j] for j in range(4)]
            for j in range(4):
                out[s, j, 64 * w:64 * w + 64] = got[j]
    return out


EXPECTED = {"dpp": expected_dpp, "permlane": expected_permlane, "readlane": expected_readlane,
            "bpermute": expected_bpermute, "ldswide": expected_ldswide, "ldstr": expected_ldstr,
            "ldsatomic": expected_ldsatomic, "ldsdma": expected_ldsdma}
_cache: dict = {}


def expected(path, seed):
    """uint32 [steps, words, 256]: what every thread must receive. Computed
    once per (path, seed); callers must not modify it."""
    if (path, seed) not in _cache:
        a = (EXPECTED[path](seed) & M32).astype(np.uint32)
        assert a.shape == (*SHAPES[path], 256)
        a.setflags(write=False)
        _cache[path, seed] = a
    return _cache[path, seed]


def digest(path, seed):
    """Workgroup digest: sum of got * (2 idx + 1) mod 2^32, idx the flat [step][word][thread] index."""
    a = expected(path, seed).astype(np.uint64).ravel()
    idx = np.arange(a.size, dtype=np.uint64)
    m = np.uint64(M32)
    return int(((a * ((idx * np.uint64(2) + np.uint64(1)) & m)) & m).sum() & m)
