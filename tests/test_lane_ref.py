"""Properties the lane sweep's design rests on, checked on the numpy reference
alone (tests/lane_sweep_ref.py): distinct values, maps that are bijections or
exactly the stated fan-out, rotations that cover the crossbar, offsets that
reach every LDS bank, transposed reads that cover the tile."""
import numpy as np
import pytest

import lane_sweep_ref as ref


def test_fmix32_is_the_murmur3_finaliser():
    # Known values of murmur3's fmix32.
    assert [int(v) for v in ref.fmix32(np.array([0, 1, 0xFFFFFFFF]))] == [0, 0x514E28B7, 0x81F16F39]
    x = np.arange(1 << 16, dtype=np.int64) * 65521
    assert len(np.unique(ref.fmix32(x))) == len(x)


@pytest.mark.parametrize("seed", ref.SEEDS)
def test_all_source_values_of_a_launch_are_distinct(seed):
    keys = ref.all_keys()
    assert len(np.unique(keys)) == len(keys)  # path, step, wave, word, lane and src/aux never collide
    values = ref.fmix32(seed ^ keys)
    assert len(np.unique(values)) == len(values)
    for h in range(2):  # the 16-bit tiles: all four waves and both strides of a launch
        tiles = np.stack([ref.tr_tile(seed, h, w) for w in range(4)])
        assert tiles.max() <= 0xFFFF and len(np.unique(tiles)) == tiles.size
    both = np.stack([ref.tr_tile(seed, h, w) for h in range(2) for w in range(4)])
    assert len(np.unique(both)) == both.size <= 65536


def test_shapes_and_step_counts():
    assert len(ref.dpp_steps()) == ref.SHAPES["dpp"][0] == 75
    assert 128 + len(ref.swizzle_steps()) == ref.SHAPES["bpermute"][0]
    assert 128 + len(ref.FIRST_LANES) == ref.SHAPES["readlane"][0]
    assert len(ref.ATOMIC_OPS) + 3 == ref.SHAPES["ldsatomic"][0]
    for f in ref.PATHS:
        steps, words = ref.SHAPES[f]
        assert steps < 4096 and words <= 4  # the key's step field and 4 * wave + word
        assert ref.expected(f, ref.SEEDS[0]).shape == (steps, words, 256)


def _fan_out(lanes):
    """How many destination lanes each source lane feeds, and the lanes with no source."""
    lanes = np.asarray(lanes)
    return np.bincount(lanes[lanes >= 0], minlength=64), np.flatnonzero(lanes < 0)


def test_every_dpp_map_is_a_bijection_or_the_stated_fan_out():
    l = np.arange(64)
    for name, lanes, rm, bm, bc in ref.dpp_steps():
        count, none = _fan_out(lanes)
        assert ((lanes < 64) & (lanes >= -1)).all(), name
        if name.startswith(("quad_perm", "row_ror", "row_mirror", "row_half_mirror", "wave_rol", "wave_ror")):
            assert (count == 1).all() and none.size == 0, name  # a permutation
            assert ((lanes >> 4) == (l >> 4)).all() or name.startswith("wave"), name  # inside the row
        elif name.startswith(("row_shl", "row_shr")):
            n = int(name.split(":")[1].split()[0])
            assert none.size == 4 * n and count.max() == 1 and count.sum() == 64 - 4 * n, name
            assert ((lanes[lanes >= 0] >> 4) == (l[lanes >= 0] >> 4)).all(), name
        elif name.startswith(("wave_shl", "wave_shr")):
            assert none.tolist() == ([63] if "shl" in name else [0]) and count.max() == 1, name
        elif name == "row_bcast15":  # lane 15 of a row to all of the next; row 0 reads itself
            assert none.size == 0 and (lanes[:16] == l[:16]).all(), name
            assert all((lanes[16 * r:16 * r + 16] == 16 * r - 1).all() for r in (1, 2, 3)), name
            assert count[15] == 17 and count[31] == 16 and count[47] == 16 and count.sum() == 64
        elif name == "row_bcast31":  # lane 31 to rows 2 and 3; rows 0 and 1 read themselves
            assert none.size == 0 and (lanes[:32] == l[:32]).all() and (lanes[32:] == 31).all(), name
            assert count[31] == 33 and count.sum() == 64
        else:
            n = int(name.split(":")[1])
            assert name.startswith("row_newbcast") and np.flatnonzero(count).tolist() == [n, 16 + n, 32 + n, 48 + n]
            assert set(count[count > 0]) == {16} and none.size == 0
    on = ref.dpp_enabled(0xA, 0x5)
    assert np.flatnonzero(on).tolist() == [16 * r + 4 * b + i for r in (1, 3) for b in (0, 2) for i in range(4)]
    assert ref.dpp_enabled(0xF, 0xF).all()


@pytest.mark.parametrize("seed", ref.SEEDS)
def test_dpp_lanes_without_a_source_keep_old_or_read_zero(seed):
    e = ref.expected("dpp", seed)
    names = [s[0] for s in ref.dpp_steps()]
    old = lambda s: ref.src(seed, "dpp", s, 0, aux=1)  # noqa: E731
    s = names.index("row_shl:5")
    assert (e[s, 0, ref.LANE % 16 >= 11] == old(s)[ref.LANE % 16 >= 11]).all()
    s = names.index("row_shr:3 bound_ctrl")
    assert (e[s, 0, ref.LANE % 16 < 3] == 0).all() and (e[s, 0, ref.LANE % 16 >= 3] != 0).all()
    s = names.index("row_ror:5 row_mask:0xa bank_mask:0x5")
    off = ~np.tile(ref.dpp_enabled(0xA, 0x5), 4)
    assert (e[s, 0, off] == old(s)[off]).all() and (e[s, 0, ~off] != old(s)[~off]).all()


@pytest.mark.parametrize("seed", ref.SEEDS)
def test_the_swaps_and_permutes_lose_and_duplicate_nothing(seed):
    for s in range(4):  # both outputs of a swap together are the inputs, rearranged
        e = ref.expected("permlane", seed)[s]
        ins = np.concatenate([ref.src(seed, "permlane", s, 0), ref.src(seed, "permlane", s, 1)])
        assert sorted(e.ravel().tolist()) == sorted(ins.tolist())
        assert (e[0] != ref.src(seed, "permlane", s, 0)).sum() == 128  # half of vdst was exchanged
    e = ref.expected("bpermute", seed)
    for s in list(range(133)) + [135, 136]:  # permutations; 133 and 134 are the fan-outs
        assert sorted(e[s, 0].tolist()) == sorted(ref.src(seed, "bpermute", s, 0).tolist()), s
    for s in range(64):  # ds_permute with rotation r undoes ds_bpermute with the same r on the same data
        x = ref.src(seed, "bpermute", s, 0)
        back = np.zeros(256, np.int64)
        back[(ref.T & ~63) | ((ref.LANE + s) % 64)] = ref.from_lane(x, (ref.LANE + s) % 64)
        assert (back == x).all()


def test_the_rotations_cover_all_4096_lane_pairs():
    pairs = {(int(l), int((l + s) % 64)) for s in range(64) for l in range(64)}
    assert len(pairs) == 4096
    for s in (0, 1, 63):
        assert sorted(((np.arange(64) + s) % 64).tolist()) == list(range(64))


def test_swizzle_maps():
    steps = dict(ref.swizzle_steps())
    l = np.arange(64)
    for x in (1, 2, 4, 8, 16):
        assert (steps[f"xor:{x}"] == (l ^ x)).all()
    assert sorted(set(steps["and:0x10"].tolist())) == [0, 16, 32, 48] and (steps["and:0x10"] == (l & 0x30)).all()
    assert (steps["or:3"] == (l | 3)).all()
    for name in ("quad:[3, 2, 1, 0]", "quad:[1, 2, 3, 0]"):
        assert sorted(steps[name].tolist()) == list(range(64)) and ((steps[name] >> 2) == (l >> 2)).all()


def test_ldswide_offsets_reach_all_64_banks_from_every_lane():
    banks = [set() for _ in range(64)]
    for rot in range(16):
        d = ref.ldswide_dwords(rot)
        assert sorted(d.ravel().tolist()) == list(range(256))  # the slots tile the wave's 1 KiB
        for lane in range(64):
            banks[lane] |= {int(b) % 64 for b in d[lane]}
    assert all(b == set(range(64)) for b in banks)
    # the strided read crosses into other lanes' slots and stays inside the tile
    for rot in range(16):
        d = (np.arange(64) + rot) % 64
        assert (d + 192).max() < 256


@pytest.mark.parametrize("seed", ref.SEEDS)
def test_ldswide_sign_extension_is_exercised(seed):
    e = ref.expected("ldswide", seed)
    for combo, words in ((4, (1, 2)), (5, (1, 2))):
        v = np.concatenate([e[7 * rot + combo, w] for rot in range(16) for w in words])
        assert (v >> 31).any() and not (v >> 31).all()  # negative and positive values both occur
        bits = 16 if combo == 4 else 8
        assert set((v[(v >> 31) == 1] >> bits).tolist()) == {0xFFFFFFFF >> bits}
    unsigned = np.concatenate([e[7 * rot + 4, w] for rot in range(16) for w in (0, 3)])
    assert unsigned.max() <= 0xFFFF


def test_every_block_of_the_ldstr_tile_is_read_by_every_lane_group():
    for half in (0, 16):
        for g in range(4):
            assert {ref.tr_block(half + k, g) for k in range(16)} == {(r, c) for r in range(4) for c in range(4)}
    for k in range(16):  # and the four groups read four different blocks in a step
        assert len({ref.tr_block(k, g) for g in range(4)}) == 4


@pytest.mark.parametrize("seed", ref.SEEDS)
def test_ldstr_delivers_the_transpose_of_each_block(seed):
    e = ref.expected("ldstr", seed)
    for s in (0, 7, 16, 31):
        for w in (0, 3):
            tile = ref.tr_tile(seed, s // 16, w)
            for g in range(4):
                br, bc = ref.tr_block(s, g)
                block = tile[4 * br:4 * br + 4, 16 * bc:16 * bc + 16]  # [row][col]
                lanes = slice(64 * w + 16 * g, 64 * w + 16 * g + 16)
                got = np.stack([e[s, 0, lanes] & 0xFFFF, e[s, 0, lanes] >> 16, e[s, 1, lanes] & 0xFFFF,
                                e[s, 1, lanes] >> 16])  # [row][lane = col]
                assert (got == block).all()


@pytest.mark.parametrize("seed", ref.SEEDS)
def test_ldsdma_sources_are_permuted_and_complete(seed):
    for s in range(6):
        q = ref.dma_perm(s)
        assert sorted(q.tolist()) == list(range(64)) and (q != np.arange(64)).any()
    e, g = ref.expected("ldsdma", seed), ref.dma_source(seed)
    assert len(np.unique(g)) == g.size
    for s in range(6):
        for w in range(4):
            assert sorted(e[s, :, 64 * w:64 * w + 64].ravel().tolist()) == sorted(g[s, w].ravel().tolist())


def test_digests_differ_between_seeds_and_paths():
    d = {(f, s): ref.digest(f, s) for f in ref.PATHS for s in ref.SEEDS}
    assert len(set(d.values())) == len(d) and 0 not in d.values()
