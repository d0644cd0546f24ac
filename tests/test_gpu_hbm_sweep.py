"""k_hbm_fill / k_hbm_verify and the whole HBM sweep on the GPU
(csrc/hip/hbm_sweep.hip).

The reference is tests/hbm_sweep_ref.py: numpy, written from the pattern's
formula, never from xs_hbm_sweep_pattern. Every comparison is equality: the
pattern is integer arithmetic. Buffers sit between 4 KiB sentinels, so a store
outside the buffer fails the test that made it. Corruption is done with torch
(or by the sweep's own host-side injection) in buffers the test owns."""
import numpy as np
import pytest
import torch

from flex_gpu_scheduler_amd.control.node_agent import GpuHealth, hip_health_fn
from flex_gpu_scheduler_amd.ops.hip_probe import ProbeError, probe
from hbm_sweep_ref import fold, pattern

pytestmark = pytest.mark.gpu

MIB = 1 << 20
GUARD = 4096
SENTINEL = 0xA5
# (vectors, grid). grid 2: a row is 512 vectors and the unrolled body takes 4
# rows, so 2047 / 2048 / 2049 / 2048+512+1 put the end of the buffer in the
# body, on the body/tail hand-over and in the tail. 0: the production grid.
SIZES = [(1, 0), (1, 2), (2047, 2), (2048, 2), (2049, 2), (2048 + 512 + 1, 2), (64 * MIB // 16, 0)]
IDS = [f"{n}v-grid{g}" for n, g in SIZES]


@pytest.fixture(scope="module")
def p():
    return probe()


@pytest.fixture(scope="module")
def xcds(p):
    return max(1, int(p.props(0)["computeUnits"]) // 32)


def guarded(n: int):
    """(whole allocation, the n-vector buffer inside it)."""
    whole = torch.full((2 * GUARD + 16 * n,), SENTINEL, dtype=torch.uint8, device="cuda:0")
    return whole, whole[GUARD:GUARD + 16 * n]


def words_of(buf) -> np.ndarray:
    return buf.cpu().numpy().view(np.uint32).reshape(-1, 4)


def put(buf, words: np.ndarray) -> None:
    buf.copy_(torch.from_numpy(np.ascontiguousarray(words).view(np.uint8).reshape(-1).copy()))


def sentinels_intact(whole) -> bool:
    return bool((whole[:GUARD] == SENTINEL).all()) and bool((whole[-GUARD:] == SENTINEL).all())


def flip(buf, vec: int, word: int, mask: int) -> None:
    w = buf.view(torch.int32)
    m = mask - (1 << 32) if mask >> 31 else mask
    w[4 * vec + word] ^= m
    torch.cuda.synchronize()


def popcount(x: int) -> int:
    return bin(x).count("1")


# --------------------------------------------------------------------- fill
@pytest.mark.parametrize("n,grid", SIZES, ids=IDS)
def test_fill_is_exact(p, n, grid):
    whole, buf = guarded(n)
    assert p.hbm_sweep_op(buf, 0, grid=grid) is None
    got = words_of(buf)
    want = pattern(0, n)
    bad = np.argwhere(got != want)
    print("mismatching words:", len(bad), "first:", bad[:4].tolist())
    assert np.array_equal(got, want)
    assert sentinels_intact(whole)


def test_fill_across_the_high_index_word(p):
    first, n = 2 ** 32 - 3, 8
    whole, buf = guarded(n)
    p.hbm_sweep_op(buf, 0, first_vec=first, grid=2)
    want = pattern(first, n)
    assert np.array_equal(words_of(buf), want)
    assert sentinels_intact(whole)
    # the high term matters: the same low indices below the carry differ in every word
    low = pattern(0, 5)
    assert (want[3:] != low).all()
    # and verifying with the same indices reads the carry the same way
    r = p.hbm_sweep_op(buf, 1, first_vec=first, grid=2)
    assert r["bad_vectors"] == 0 and r["vectors_read"] == n
    assert np.array_equal(words_of(buf), pattern(first, n, inverted=True))
    r = p.hbm_sweep_op(buf, 2, first_vec=first + 1, grid=2)  # shifted by one: every vector is another's
    assert r["bad_vectors"] == n


def test_fill_depends_on_the_seed(p):
    whole, buf = guarded(64)
    p.hbm_sweep_op(buf, 0, seed=12345)
    assert np.array_equal(words_of(buf), pattern(0, 64, seed=12345))
    assert (words_of(buf) != pattern(0, 64)).all()


# ------------------------------------------------------------------- verify
@pytest.mark.parametrize("n,grid", SIZES, ids=IDS)
def test_verify_sees_every_vector_once(p, n, grid):
    whole, buf = guarded(n)
    comp = pattern(0, n, inverted=True)
    put(buf, comp)
    r = p.hbm_sweep_op(buf, 2, grid=grid)
    print({k: r[k] for k in ("vectors_read", "fold", "bad_vectors")}, "want fold", fold(comp))
    assert r["vectors_read"] == n
    assert r["fold"] == fold(comp)
    assert r["bad_vectors"] == 0 and r["bad_bits"] == 0 and r["log"] == [] and r["log_claims"] == 0
    assert r["flip_or"] == [0, 0, 0, 0] and r["reader_xcd_mask"] == 0
    assert np.array_equal(words_of(buf), comp)  # pass 2 writes nothing
    assert sentinels_intact(whole)


@pytest.mark.parametrize("n,grid", SIZES[:-1], ids=IDS[:-1])
def test_invert_visits_and_rewrites_every_vector(p, n, grid):
    whole, buf = guarded(n)
    put(buf, pattern(0, n))
    r = p.hbm_sweep_op(buf, 1, grid=grid)
    assert r["vectors_read"] == n and r["fold"] == fold(pattern(0, n)) and r["bad_vectors"] == 0
    assert np.array_equal(words_of(buf), pattern(0, n, inverted=True))
    assert sentinels_intact(whole)


def test_invert_writes_the_expected_value_not_what_it_read(p):
    n, grid, vec = 2048 + 512 + 1, 2, 1234
    whole, buf = guarded(n)
    p.hbm_sweep_op(buf, 0, grid=grid)
    flip(buf, vec, 3, 1 << 9)
    r = p.hbm_sweep_op(buf, 1, grid=grid)
    assert r["bad_vectors"] == 1 and r["bad_bits"] == 1 and r["vectors_read"] == n
    assert [e["v"] for e in r["log"]] == [vec] and r["log"][0]["pass"] == 1
    assert r["flip_or"] == [0, 0, 0, 1 << 9]
    # everywhere, the corrupted vector included: the error does not propagate
    assert np.array_equal(words_of(buf), pattern(0, n, inverted=True))
    r2 = p.hbm_sweep_op(buf, 2, grid=grid)
    assert r2["bad_vectors"] == 0 and r2["vectors_read"] == n
    assert sentinels_intact(whole)


def test_faults_are_located_exactly(p, xcds):
    n, grid, first = 2048 + 512 + 1, 2, 1000
    want = pattern(first, n)
    whole, buf = guarded(n)
    put(buf, want)
    # the first vector (unrolled body), one in the remainder loop, the last (remainder loop too)
    vecs = [0, 2050, n - 1]
    e0 = int(want[0, 1])
    low_set, low_clear = e0 & -e0, ~e0 & (e0 + 1)
    assert low_set and low_clear
    masks = {0: (1, low_set | low_clear),            # two bits of one word, one in each direction
             2050: (0, 1 << 31),
             n - 1: (2, 0x00010000)}
    for v, (word, mask) in masks.items():
        flip(buf, v, word, mask)
    r = p.hbm_sweep_op(buf, 1, first_vec=first, grid=grid)
    log = sorted(r["log"], key=lambda e: e["v"])
    assert [e["v"] for e in log] == [first + v for v in vecs]
    down = up = 0
    flip_or = [0, 0, 0, 0]
    for e, v in zip(log, vecs):
        word, mask = masks[v]
        exp = [int(w) for w in want[v]]
        act = list(exp)
        act[word] ^= mask
        assert e["expected"] == exp and e["actual"] == act and e["pass"] == 1
        assert 0 <= e["xcd"] < xcds
        down += popcount(mask & exp[word])
        up += popcount(mask & ~exp[word])
        flip_or[word] |= mask
    assert down >= 1 and up >= 1  # both directions are in the test
    assert r["bad_vectors"] == 3 and r["bad_bits"] == 4 == down + up
    assert r["one_to_zero"] == down and r["zero_to_one"] == up
    assert r["flip_or"] == flip_or
    mask = r["reader_xcd_mask"]
    assert 1 <= popcount(mask) <= 3 and mask < 1 << xcds
    assert mask == sum({1 << e["xcd"] for e in log})
    assert r["vectors_read"] == n and r["log_claims"] == 3
    corrupted = want.copy()
    for v, (word, m) in masks.items():
        corrupted[v, word] ^= m
    assert r["fold"] == fold(corrupted)
    assert sentinels_intact(whole)


def test_log_is_capped_and_the_count_is_not(p):
    n, grid = 2048 + 512 + 1, 2
    whole, buf = guarded(n)
    comp = pattern(0, n, inverted=True)
    put(buf, comp)
    vecs = sorted(np.random.default_rng(7).choice(n, size=40, replace=False).tolist())
    for v in vecs:
        flip(buf, v, v % 4, 1 << (v % 32))
    r = p.hbm_sweep_op(buf, 2, grid=grid)
    assert r["bad_vectors"] == 40 and r["bad_bits"] == 40 and r["log_claims"] == 40
    logged = [e["v"] for e in r["log"]]
    assert len(logged) == 32 and len(set(logged)) == 32 and set(logged) <= set(vecs)
    for e in r["log"]:
        v = e["v"]
        assert e["pass"] == 2 and e["expected"] == [int(w) for w in comp[v]]
        assert e["actual"][v % 4] == e["expected"][v % 4] ^ (1 << (v % 32))


# -------------------------------------------------------------- whole sweep
SWEEP_BYTES, SWEEP_CHUNK = 48 * MIB + 16, 16 * MIB
SWEEP_VECS = SWEEP_BYTES // 16


def test_whole_sweep_is_clean_and_counts_both_verify_passes(p):
    out = p.hbm_sweep(0, nbytes=SWEEP_BYTES, chunk_bytes=SWEEP_CHUNK)
    raw, s = out["raw"], out["summary"]
    print("hbm_sweep 48 MiB:", {k: s[k] for k in ("bytes_tested", "ms", "GBps", "vectors_read")})
    assert s["healthy"] and s["bad_vectors"] == 0 and s["bad_bits"] == 0 and s["faults"] == []
    assert s["bytes_tested"] == SWEEP_BYTES and not s["short"] and raw["chunks"] == 4  # a 16-byte last chunk
    assert s["vectors_read"] == 2 * SWEEP_VECS
    assert s["from_dram"] is False
    assert s["bad_chunks"] == {} and s["flip_mask"] == "0" * 32 and s["reader_xcds"] == []
    f = fold(pattern(0, SWEEP_VECS))
    assert raw["fold"] == [f, f]  # one global index across the chunks, in both passes
    assert len(s["ms"]) == 3 and all(t > 0 for t in s["ms"]) and all(g > 0 for g in s["GBps"])


@pytest.mark.parametrize("after", [0, 1])
def test_whole_sweep_reports_an_injected_flip(p, xcds, after):
    vec, word, bit = SWEEP_CHUNK // 16 + 12345, 2, 7  # in the second chunk
    out = p.hbm_sweep(0, nbytes=SWEEP_BYTES, chunk_bytes=SWEEP_CHUNK, inject=(vec, word, 1 << bit, after))
    s = out["summary"]
    assert not s["healthy"] and s["bad_vectors"] == 1 and s["bad_bits"] == 1
    assert s["vectors_read"] == 2 * SWEEP_VECS
    assert s["bad_chunks"] == {1: 1}
    assert len(s["faults"]) == 1
    f = s["faults"][0]
    # after pass 0 the flip sits in the pattern and pass 1 reads it (and repairs it);
    # after pass 1 it sits in the complement and pass 2 reads it
    exp = [int(w) for w in pattern(vec, 1, inverted=bool(after))[0]]
    assert f["v"] == vec and f["offset"] == 16 * vec and f["pass"] == after + 1
    assert f["expected"] == exp and f["bits"] == [32 * word + bit]
    was_one = bool(exp[word] >> bit & 1)
    assert f["one_to_zero"] == ([32 * word + bit] if was_one else [])
    assert f["zero_to_one"] == ([] if was_one else [32 * word + bit])
    assert (s["one_to_zero"], s["zero_to_one"]) == ((1, 0) if was_one else (0, 1))
    assert int(s["flip_mask"], 16) == 1 << (32 * word + bit)
    assert s["reader_xcds"] == [f["xcd"]] and f["xcd"] < xcds


# ---------------------------------------------------------------- refusals
def test_refusals(p):
    whole, buf = guarded(4)
    with pytest.raises(ProbeError) as e:
        p.hbm_sweep_op(buf[:24], 0)  # bytes % 16
    assert e.value.rc == -1000
    with pytest.raises(ProbeError) as e:
        p.hbm_sweep_op(buf, 7)
    assert e.value.rc == -1000
    with pytest.raises(ProbeError) as e:
        p.hbm_sweep_op(buf[8:40], 0)  # 32 bytes, 8 off a 16-byte boundary
    assert e.value.rc == -1001
    with pytest.raises(ProbeError) as e:
        p.hbm_sweep_op(buf[:0], 0)
    assert e.value.rc == -1000
    with pytest.raises(ProbeError) as e:
        p.hbm_sweep(0, nbytes=MIB, chunk_bytes=MIB, inject=(MIB // 16, 0, 1, 0))  # one past the end
    assert e.value.rc == -1000
    assert bool((whole == SENTINEL).all())  # nothing ran


# ---------------------------------------------------------- health callback
def test_health_fn_with_the_hbm_sweep(p):
    assert hip_health_fn(hbm=True, hbm_gib=1 / 16, hbm_args={"chunk_bytes": 16 * MIB})(0)
    v = hip_health_fn(hbm=True, hbm_gib=1 / 16,
                      hbm_args={"chunk_bytes": 16 * MIB, "inject": (MIB + 5, 1, 0x10, 0)})(0)
    assert isinstance(v, GpuHealth) and not v.ok and not v
    hf = v.detail["hbmFaults"]
    assert hf["badVectors"] == 1 and hf["badBits"] == 1 and int(hf["flipMask"], 16) == 0x10 << 32
    assert hf["fromDram"] is False and hf["testedGiB"] == round(1 / 16, 3)
    assert v.detail["hbmSweep"]["bad_chunks"] == {1: 1}
