"""The fetch sweep's reference (tests/fetch_sweep_ref.py) against answers
worked by hand: the hash, the first literals of every region written out, the
sizes of the runs, the orders, the distinct-literal counts and a few words
folded step by step in plain integers."""
import numpy as np
import pytest

import fetch_sweep_ref as ref

SEED = 0x1B873593
M32 = 0xFFFFFFFF


def rotl(v, s):
    return (v << s | v >> (32 - s)) & M32


def test_fmix32_is_murmur3s_finaliser():
    assert ref.fmix32(0) == 0 and ref.fmix32(1) == 0x514E28B7 and ref.fmix32(M32) == 0x81F16F39
    # The values the issue worked for the scratch key i + 0x1000.
    assert [ref.fmix32(0x1000 + i) | 0x01000100 for i in range(4)] == [0x7B94D36D, 0x0BC3839B, 0x55BBA7CF, 0x65C75942]
    assert len({ref.fmix32(i) for i in range(4096)}) == 4096


def test_the_key_is_a_bijection_of_region_and_step():
    keys = {ref.key(r, i) for r in range(7) for i in (0, 1, 511, 512, 16383, (1 << 20) - 1)}
    assert len(keys) == 7 * 6
    assert ref.key(0, 513) == 513 and ref.key(5, 1024) == 0x500400 and ref.key(6, 16) == 0x600010
    with pytest.raises(AssertionError):
        ref.key(0, 1 << 20)


def test_the_first_literals_of_every_region():
    first = {r: [ref.literal(r, i) for i in ref.run_steps(r)[0][:4]] for r in range(7)}
    assert first[ref.STREAM] == [0x01000100, 0x514E29B7, 0x31F4C306, 0x85F0B527]  # fmix32(0) = 0: the OR alone
    assert first[ref.LOOP0] == [0xEFFACDE3]
    assert first[ref.LOOP0 + 1] == [0xDFF499C6, 0xFF1183EE, 0xA92EDD8B]
    assert first[ref.LOOP0 + 2] == [0x8B8EC785, 0xAFE12F0F, 0xB9C1EFD3, 0x01EC3F7B]
    assert first[ref.LOOP0 + 3] == [0xBFE8338C, 0x49890131, 0x337D994E, 0xD5F889FE]
    assert first[ref.CALL] == [0x0B82F3E1, 0xD3DE3FC8, 0xF5A38D09]  # the extra block, b = 256 (i from 1024), lies first
    assert [ref.literal(ref.CALL, 4 * 255 + j) for j in range(3)] == [0xE7969B40, 0x977193D2, 0x6763457F]  # block 255
    assert ref.run_steps(ref.CALL)[0] == [1024, 1025, 1026] and ref.run_steps(ref.CALL)[1] == [0, 1, 2]
    assert first[ref.ALIGN] == [0xD7CF9F84] and ref.literal(ref.ALIGN, 16) == 0xDBC36167
    # The last segment of `stream` starts at step 31 x 512.
    assert [ref.literal(0, 31 * 512 + j) for j in range(3)] == [0xA3DDF766, 0x07DB9545, 0x391E53BF]
    for r in range(7):
        for run in ref.run_steps(r):
            assert all(ref.literal(r, i) & 0x01000100 == 0x01000100 for i in run)


def test_no_literal_is_an_inline_constant():
    # 0..64 and the float constants lack one of the two bits the OR sets; -16..-1 have both, so the OR alone does
    # not exclude them: no step's literal is one (and tests/test_fetch_codeobject.py holds every step to its size).
    small = set(range(0, 65)) | {0x3F000000, 0xBF000000, 0x3F800000, 0xBF800000, 0x40000000, 0xC0000000, 0x40800000,
                                 0xC0800000, 0x3E22F983}
    assert not any(v & 0x01000100 == 0x01000100 for v in small)
    negative = {(-n) & M32 for n in range(1, 17)}
    for r in range(7):
        assert not negative & {ref.literal(r, i) for run in ref.run_steps(r) for i in run}, r


def test_the_runs_fill_their_bytes():
    assert ref.KIND_BYTES == {"V": 16, "S": 20, "K": 16, "X": 16}
    assert [ref.kind(j) for j in range(6)] == ["V", "S", "K", "X", "V", "S"]
    assert ref.steps_that_fit(16) == (1, 0) and ref.steps_that_fit(64) == (3, 3)
    assert ref.steps_that_fit(1024) == (60, 1) and ref.steps_that_fit(16384) == (963, 3)
    assert (ref.SEGMENT_STEPS, ref.SEGMENT_NOPS) == (481, 3) and (ref.BLOCK_STEPS, ref.BLOCK_NOPS) == (3, 2)
    assert ref.LOOP_STEPS == [1, 3, 60, 963] and ref.LOOP_NOPS == [0, 3, 1, 3]
    assert ref.SEGMENTS * ref.SEGMENT_BYTES == 256 << 10 and ref.CALL_BLOCKS * ref.BLOCK_BYTES == 16 << 10
    assert ref.SEGMENT_STEPS <= ref.SEGMENT_STRIDE and ref.BLOCK_STEPS <= ref.BLOCK_STRIDE


def test_distinct_literals_per_region():
    # (32-bit literals in the code, distinct among them): the OR made no two equal.
    assert [ref.distinct_literals(r) for r in range(7)] == [(7712, 7712), (1, 1), (2, 2), (30, 30), (482, 482),
                                                            (514, 514), (17, 17)]
    assert 7712 == 32 * 241  # a segment's 481 steps: 121 of kind V, 120 each of S, K and X
    assert [len(ref.region_literals(r)) for r in range(7)] == [32 * 361, 1, 3, 45, 723, 257 * 3, 17]


def test_every_wave_calls_every_segment_from_its_own_start():
    for w in range(4):
        order = ref.segment_order(w)
        assert sorted(order) == list(range(32)) and order[0] == 8 * w and order[-1] == (8 * w - 1) % 32
    assert ref.segment_order(3)[:10] == [24, 25, 26, 27, 28, 29, 30, 31, 0, 1]


@pytest.mark.parametrize("seed", [SEED, 0x9E3779B9, 0, 1, M32])
def test_the_call_order_is_a_permutation(seed):
    for r in range(4):
        assert sorted(ref.call_order(seed, r)) == list(range(256))
    assert ref.call_order(seed, 0) != ref.call_order(seed, 1)


def test_the_call_order_written_out():
    assert ref.call_order(SEED, 0)[:6] == [39, 130, 221, 56, 147, 238]  # a = 91, b = 39
    assert ref.call_order(0x9E3779B9, 0)[:6] == [227, 214, 201, 188, 175, 162]  # a = 243, b = 227
    assert ref.call_order(SEED, 0) != ref.call_order(0x9E3779B9, 0)


def test_the_align_targets():
    assert [ref.target_of(j) for j in range(32)] == [*range(17), *range(15)]


def test_rows_and_flat_index():
    assert {p: ref.rows_of(p, 1) for p in ref.PARTS} == {"stream": 32, "loop": 4, "call": 1, "align": 32, "refill": 2}
    assert {p: ref.rows_of(p, 3) for p in ref.PARTS} == {"stream": 32, "loop": 12, "call": 3, "align": 32, "refill": 2}
    assert ref.flat_index(0, 0) == 0 and ref.flat_index(2, 5) == 517


def test_words_folded_by_hand():
    start = ref.start_values(SEED, 0, 0)
    assert [int(v) for v in start[:2]] == [0x67A2A8EE, 0x9A24E9C9] and int(start[1]) == ref.fmix32(SEED ^ 1)
    assert int(ref.start_values(SEED, 1, 2)[0]) == 0xCF0FD6FF == ref.fmix32(SEED ^ 0x10020000)
    # `align`, thread 0: xor the target's literal, then rotate.
    acc = ref.fmix32(SEED ^ 0x30000000)
    w = ref.words("align", SEED)
    for j in range(32):
        acc = rotl(acc ^ ref.literal(6, j if j < 17 else j - 17), 5)
        assert int(w[j, 0]) == acc
    assert int(w[0, 0]) == 0x966056C6
    # `loop`, the 64-byte body (V, S, K), thread 5, the first of its 512 trips and then all of them.
    c, t = 0x5BD1E995, 5
    lits = [0xDFF499C6, 0xFF1183EE, 0xA92EDD8B]
    acc = ref.fmix32(SEED ^ (1 << 28 | 1 << 16 | t))
    for trip in range(512):
        acc = rotl(acc, 5) ^ lits[0]
        s = c ^ lits[1]
        acc = rotl(acc, 5) ^ s
        s = (s + (lits[2] & 0xFFFF) - 0x10000) & M32  # 0xdd8b is negative as a simm16
        acc = rotl(acc, 5) ^ s
    assert int(ref.words("loop", SEED)[1, t]) == acc == 0x0AD71E73
    # Kind X on the 1 KiB body: its fourth step adds the thread number.
    lanes = ref.Lanes(np.array([7, 7], np.uint32), np.array([0, 200]))
    lanes.run(ref.LOOP0 + 2, [0, 1, 2, 3])
    a, b = (int(v) for v in lanes.acc)
    assert (b - a) & M32 == 200


def test_refill_rows_are_equal_and_words_are_cached_read_only():
    w = ref.words("refill", SEED)
    assert (w[0] == w[1]).all() and w.shape == (2, 256)
    assert ref.words("refill", SEED) is w and not w.flags.writeable
    assert ref.digest(np.array([[1, 2], [3, 4]], np.uint32)) == 1 * 1 + 2 * 3 + 3 * 5 + 4 * 7
    assert ref.digest(np.array([M32, M32], np.uint32)) == (M32 + 3 * M32) & M32
