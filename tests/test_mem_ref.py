"""The numpy reference of the memory-path sweep on its own: that its values are
distinct, its maps bijections, its tile passes complete, and that the operand
rounds hold the cases the sweep is there for. What it says a thread receives
is held against the GPU in tests/test_gpu_mem_sweep.py and against the host
library's digests in tests/test_mem_health.py."""
import numpy as np
import pytest

import mem_sweep_ref as ref

SEED = ref.SEEDS[0]


def test_shapes_and_dtypes():
    for r in ref.ROUTES:
        e = ref.expected(r, SEED)
        assert e.shape == (*ref.SHAPES[r], 256) and e.dtype == np.uint32 and not e.flags.writeable
        assert ref.expected(r, SEED) is e  # computed once
        assert 0 <= ref.digest(r, SEED) <= ref.M32
    assert ref.STRIDE == 144 << 10 and ref.TILE == 128 << 10 and ref.GUARD == 4096


def test_every_key_of_a_launch_is_distinct():
    keys = ref.all_keys()
    assert len(np.unique(keys)) == len(keys)
    for seed in ref.SEEDS:  # fmix32 is a bijection, so the values are as distinct as the keys
        sample = keys[:: max(1, len(keys) // 200000)]
        assert len(np.unique(ref.fmix32(seed ^ sample))) == len(sample)


@pytest.mark.parametrize("route", ["gwidth", "buffer", "flat", "atomic"])
def test_source_values_of_a_route_are_distinct(route):
    v = np.concatenate([ref.src(SEED, route, s, w, kind) for s in range(ref.SHAPES[route][0]) for w in range(4)
                        for kind in (0, 1)])
    assert len(np.unique(v)) == len(v)


def test_tile_and_table_values_are_distinct():
    for route, n in (("l1", ref.L1_TILE // 4), ("l2", ref.TILE // 4), ("scalar", ref.TABLE_WORDS)):
        v = np.concatenate([ref.til(SEED, route, np.arange(n)), ref.til(SEED, route, np.arange(n), 3)])
        assert len(np.unique(v)) == len(v)
    s = ref.sentinel(np.arange(ref.STRIDE // 4))
    assert len(np.unique(s)) == len(s)  # an odd multiplier


def test_slot_maps_are_bijections_with_a_stride_that_is_not_the_width():
    for k in range(max(ref.SHAPES[r][0] for r in ("gwidth", "buffer", "flat", "atomic"))):  # the steps that use it
        sl = ref.slot(k, np.arange(64))
        assert sorted(sl) == list(range(64))
        step = (sl[1] - sl[0]) & 63
        assert step % 2 == 1 and step != 1  # neighbours are never adjacent slots


def test_l1_passes_touch_every_line_once_per_wave_and_every_dword_position():
    lines = ref.L1_TILE // 128
    seen_pos = np.zeros((256, 32), bool)
    for p in range(4):
        q = np.array([(ref.L1_MUL[p] * i + p) & 63 for i in range(64)])
        assert sorted(q) == list(range(64))  # the line-pair order is a permutation of the loads
        touched = np.zeros((4, lines), int)
        for i in range(64):
            d = ref.l1_dword(p, i)
            assert d.min() >= 0 and d.max() < ref.L1_TILE // 4
            for w in range(4):
                here = np.unique(d[ref.WAVE == w] >> 5)
                assert len(here) == 2  # one wave-instruction reads one line pair
                touched[w, here] += 1
            seen_pos[ref.T, d & 31] = True
        assert (touched == 1).all()
    assert seen_pos.all()  # every lane position receives from every dword of a line
    # Within one load the 64 lanes read 64 different dwords.
    assert all(len(np.unique(ref.l1_dword(p, i)[:64])) == 64 for p in range(4) for i in range(64))


def test_l1_rewrites_one_dword_of_every_line():
    d = ref.l1_rewrites()
    assert sorted(d >> 5) == list(range(ref.L1_TILE // 128))
    e = ref.expected("l1", SEED).astype(np.int64)
    before, after = e[:32], e[32:]
    new = set(ref.til(SEED, "l1", d, 3).tolist())
    assert not new & set(before.ravel().tolist())
    hit = np.isin(after, list(new))
    assert hit.any() and hit[:, :, ref.WAVE != 0].any()  # the other three waves read the rewritten words


def test_l2_passes_touch_every_line_once_per_wave():
    chunks = ref.TILE // 16
    for p in range(4):
        touched = np.zeros((4, chunks), int)
        for i in range(128):
            c = ref.l2_chunk(p, i)
            assert c.min() >= 0 and c.max() < chunks
            for w in range(4):
                touched[w, c[ref.WAVE == w]] += 1
        assert (touched == 1).all()  # every 16-byte chunk, so every 128-byte line, once per wave
        first = np.array([ref.l2_chunk(p, i)[0] >> 6 for i in range(128)])
        assert sorted(first) == list(range(128)) and (np.diff(first) != 1).all()  # no linear walk
    lane_step = (ref.l2_chunk(0, 0)[1] - ref.l2_chunk(0, 0)[0]) & 63
    assert lane_step not in (0, 1)
    e = ref.expected("l2", SEED)
    assert set((e[:384] ^ 0xFFFFFFFF).ravel().tolist()) == set(e[384:].ravel().tolist())  # the complement pass


def test_buffer_has_lanes_in_and_out_of_range_in_every_step_and_wave():
    e = ref.expected("buffer", SEED)
    for s in range(12):
        out = ref.buffer_out_of_range(s)
        for w in range(4):
            n = int(out[ref.WAVE == w].sum())
            assert n == 64 - ref.RANGE_SLOTS  # neither none nor all
        if s % 6 == 5:  # the store that must be dropped: the sentinel is still there
            assert (e[s][:, out] != 0).all() and (e[s][:, ~out] == [ref.src(SEED, "buffer", s, j)[~out]
                                                                  for j in range(4)]).all()
        else:
            assert (e[s][:, out] == 0).all() and (e[s][:, ~out] != 0).any()


def test_cmpswap_rounds_hold_both_outcomes():
    a, b, cmp = ref.atomic_operands(SEED, "cmpswap", 0)
    assert all(x == c for x, c in zip(a, cmp))
    a, b, cmp = ref.atomic_operands(SEED, "cmpswap", 1)
    assert all(x != c for x, c in zip(a, cmp))
    e = ref.expected("atomic", SEED)[ref.ATOMIC_OPS.index("cmpswap")]
    assert (e[1] != e[0]).all() and (e[3] == e[2]).all()  # swapped, not swapped
    a, b, cmp = ref.atomic_operands(SEED, "cmpswap_x2")
    same = np.array([x == c for x, c in zip(a, cmp)])
    assert same.any() and not same.all()


def test_inc_and_dec_rounds_hold_both_wraps():
    for op in ("inc", "dec"):
        e = ref.expected("atomic", SEED)[ref.ATOMIC_OPS.index(op)].astype(np.int64)
        a, b, _ = ref.atomic_operands(SEED, op, 1)
        a, b = np.array(a), np.array(b)
        left = e[3]
        wrapped = left == (0 if op == "inc" else b)
        stepped = left == ((a + 1) if op == "inc" else (a - 1))
        assert wrapped.any() and stepped.any() and (wrapped | stepped).all()
        assert wrapped[::2].all() and stepped[1::2].all()
        # The hashed round has both as well.
        a, b, _ = ref.atomic_operands(SEED, op, 0)
        a, b = np.array(a), np.array(b)
        assert (a > b).any() and (a < b).any()


def test_integer_atomic_rules():
    f = ref.integer_atomic
    assert f("inc", 5, 5, 0, 32) == 0 and f("inc", 4, 5, 0, 32) == 5 and f("inc", 0xFFFFFFFF, 0xFFFFFFFF, 0, 32) == 0
    assert f("dec", 0, 9, 0, 32) == 9 and f("dec", 10, 9, 0, 32) == 9 and f("dec", 9, 9, 0, 32) == 8
    assert f("smin", 0xFFFFFFFF, 1, 0, 32) == 0xFFFFFFFF and f("umin", 0xFFFFFFFF, 1, 0, 32) == 1
    assert f("smax", 0x80000000, 1, 0, 32) == 1 and f("umax", 0x80000000, 1, 0, 32) == 0x80000000
    assert f("sub", 1, 2, 0, 32) == 0xFFFFFFFF and f("add", 1 << 63, 1 << 63, 0, 64) == 0
    assert f("smin", 1 << 63, 1, 0, 64) == 1 << 63
    assert f("cmpswap", 7, 9, 7, 32) == 9 and f("cmpswap", 7, 9, 6, 32) == 7


def test_float_atomic_operands_are_exact_normal_numbers():
    for op, kind, halves in (("add_f32", np.float32, 1), ("pk_add_f16", np.float16, 2)):
        for j in range(2):
            a, b, r = ref.atomic_operands(SEED, op, j)
            for h in range(halves):
                width = 32 // halves
                fa, fb, fr = ((v >> (width * h)) & ((1 << width) - 1) for v in (a, b, r))
                fa, fb, fr = (v.astype(f"uint{width}").view(kind).astype(np.float64) for v in (fa, fb, fr))
                assert (fa + fb == fr).all() and (fr == np.round(fr)).all() and (fr != 0).all()
                assert (np.abs(fr) >= np.finfo(kind).tiny).all() and np.isfinite(fr).all()
    a, b, r = ref.atomic_operands(SEED, "pk_add_bf16", 0)
    for h in range(2):
        fa, fb, fr = ((((v >> (16 * h)) & 0xFFFF) << 16).astype(np.uint32).view(np.float32).astype(np.float64)
                      for v in (a, b, r))
        assert (fa + fb == fr).all() and (fr < 256).all() and (fr >= 128).all()
    for op in ("add_f64", "min_f64", "max_f64"):
        a, b, r = (v.view(np.float64) for v in ref.atomic_operands(SEED, op))
        want = a + b if op == "add_f64" else np.minimum(a, b) if op == "min_f64" else np.maximum(a, b)
        assert (r == want).all() and np.isfinite(r).all() and (np.abs(r) >= 1).all()
        if op != "add_f64":
            assert (r == a).any() and (r == b).any() and (a < 0).any() and (a > 0).any()


def test_contended_words_do_not_depend_on_the_order():
    s = ref.ATOMIC_OPS.index("contended")
    e = ref.expected("atomic", SEED)[s].astype(np.int64)
    assert (e == e[:, :1]).all()
    ops = ref.contended_operands(SEED)
    init = [int(ref.aux(SEED, "atomic", s, j)[0]) for j in range(4)]
    assert e[0, 0] == (init[0] + 256) & ref.M32
    assert e[1, 0] == 0xFFFFFFFF  # 256 lanes set all 32 bits
    assert e[2, 0] == max(init[2], int(ops[2].max()))
    assert e[3, 0] == init[3] ^ int(np.bitwise_xor.reduce(ops[3]))


def test_scalar_offsets_are_uniform_aligned_and_in_the_table():
    for s in range(8):
        for off, size in zip(ref.scalar_offsets(SEED, s), ref.SCALAR_SIZES):
            assert (off % size == 0).all() and (off + size <= ref.TABLE_WORDS).all()
            assert all(len(np.unique(off[ref.WAVE == w])) == 1 for w in range(4))
    e = ref.expected("scalar", SEED)
    assert all((e[:, :, ref.WAVE == w] == e[:, :, 64 * w:64 * w + 1]).all() for w in range(4))
    assert len({tuple(e[:, :, 64 * w].ravel()) for w in range(4)}) == 4  # the waves read different places


def test_sub_dword_and_d16_rules_on_known_bytes():
    m = ref.Memory()
    m.store(ref.WORK, np.full(256, 0x80FF7F01), 4)
    assert int(m.load(ref.WORK + 1, 1, True)[0]) == 0x7F and int(m.load(ref.WORK + 2, 1, True)[0]) == 0xFFFFFFFF
    assert int(m.load(ref.WORK + 2, 2, True)[0]) == 0xFFFF80FF and int(m.load(ref.WORK + 2, 2)[0]) == 0x80FF
    assert int(ref.d16(0xAAAA5555, 0xFFFFFF80)) == 0x0000FF80 and int(ref.d16_hi(0xAAAA5555, 0x12)) == 0x00120000
    assert m.guards_intact()
    m.store(-4, np.zeros(256, np.int64), 4)
    assert not m.guards_intact()


def test_digest_of_the_injected_bit():
    for r in ("gwidth", "scalar"):
        first = int(ref.expected(r, SEED)[0, 0, 0])
        assert ref.digest(r, SEED, flip_first=True) == (ref.digest(r, SEED) - first + (first ^ 1)) & ref.M32
