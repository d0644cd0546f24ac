"""The MFMA probes (csrc/hip/mfma_probe.hip) and the checksum health check
(xs_health_check in csrc/hip/hbm_probe.hip) on a real MI355X, against the plain
numpy reference of tests/mfma_probe_ref.py.

k_mfma_tile runs as the production check launches it (one wave) on operands
the test chose: the tile must be bit-equal to an int64 / float64 product where
every product and partial sum is exact, and inside the textbook accumulation
bound where it is not. k_mfma_peak runs as its checked instantiation: every
accumulator of every lane must be iters x the reference tile, and the
workgroups the kernel counts must be the ones that recorded a selected XCD.
The health pattern is held to numpy on a view inside sentinels, and the verdict
must fail on a single bit the test flips in its own tensor. Nothing here
provokes a fault: an injection is a bit flipped in the test's own data."""
import re

import numpy as np
import pytest

import mfma_probe_ref as ref

pytestmark = pytest.mark.gpu

BAD_ARGS, IDLE_XCD = -1000, -1002
SENT = 0x5EA7C0DE
PADW = 1024  # sentinel words to each side of a health buffer


@pytest.fixture(scope="module")
def env():
    import torch  # first: the probe library then binds to torch's HIP runtime

    assert torch.cuda.is_available()
    torch.cuda.init()
    from flex_gpu_scheduler_amd.ops.hip_probe import HipProbe

    return torch, HipProbe()


@pytest.fixture(scope="module")
def dev(env):
    """The XCDs this device shows, as a list and a mask, and its CU count."""
    _, pr = env
    hist = pr.xcd_census(0, 4096)["blocks_per_xcd"]
    present = [x for x in range(8) if hist[x]]
    return {"present": present, "mask": sum(1 << x for x in present), "cus": int(pr.props(0)["computeUnits"])}


@pytest.fixture(scope="module")
def peak_ref():
    """One workgroup's accumulators after one step, [256, 16] float64, and the
    iteration count below which iters x that is exact in fp32."""
    return {"one": ref.peak_accumulators(1), "limit": ref.peak_exact_iters_limit()}


def bits32(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def assert_tile_equal(got, want, what):
    """Bit-equal fp32 tiles; a mismatch lists (row, col, got, want) so that a
    wrong lane or register map names itself."""
    want32 = np.asarray(want, np.float64).astype(np.float32)
    assert np.array_equal(want32.astype(np.float64), np.asarray(want, np.float64)), f"{what}: reference not exact in fp32"
    bad = np.argwhere(bits32(got) != bits32(want32))
    assert len(bad) == 0, (what, len(bad), [(int(i), int(j), float(got[i, j]), float(want32[i, j])) for i, j in bad[:12]])


# ------------------------------------------------------------ k_mfma_tile
@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("k", [16, 32, 48, 256])
def test_tile_random_integers_are_exact(env, k, seed):
    """One instruction, one accumulate step, an odd step count and 16 steps,
    on integers in [-8, 8] x [-6, 6] (B not symmetric), against int64."""
    _, pr = env
    rng = np.random.default_rng(1000 * k + seed)
    a = rng.integers(-8, 9, (32, k))
    b = rng.integers(-6, 7, (k, 32))
    assert not np.array_equal(b[:16, :16], b[:16, :16].T)
    c = pr.mfma_tile(ref.bf16_exact(a), ref.bf16_exact(b))
    assert_tile_equal(c, ref.tile_int64(a, b), (k, seed))


@pytest.mark.parametrize("encode", ["row", "col"])
@pytest.mark.parametrize("identity", ["a", "b"])
def test_tile_identity_returns_the_other_operand(env, identity, encode):
    """A = I (K = 32) returns B and B = I returns A. The other operand's
    entries are integers up to 256 in magnitude (exact in bf16) that name their
    own row, or their own column, so that a wrong lane map or a wrong 8h + j
    shows in the listed (row, col, got, want) which index went astray."""
    _, pr = env
    i, j = np.indices((32, 32))
    sign = np.where((i + j) % 2 == 0, 1, -1)
    x = (sign * (8 * i + 8 if encode == "row" else 8 * j + 8)).astype(np.float64)  # 8 .. 256, mixed signs
    eye = np.eye(32)
    a, b = (eye, x) if identity == "a" else (x, eye)
    c = pr.mfma_tile(ref.bf16_exact(a), ref.bf16_exact(b))
    assert_tile_equal(c, x, (identity, encode))


def test_tile_full_significands_mixed_signs(env):
    """Every operand has all 8 significand bits in play (odd integers 129 ..
    255, both signs): products need 16 bits and the 32-term sums stay below
    2^24, so every partial sum in any order is an exact fp32 integer."""
    _, pr = env
    rng = np.random.default_rng(77)
    a = (2 * rng.integers(64, 128, (32, 32)) + 1) * rng.choice([-1, 1], (32, 32))
    b = (2 * rng.integers(64, 128, (32, 32)) + 1) * rng.choice([-1, 1], (32, 32))
    assert int(np.abs(a).min()) >= 129 and int((np.abs(a) @ np.abs(b)).max()) < 1 << 24
    c = pr.mfma_tile(ref.bf16_exact(a), ref.bf16_exact(b))
    assert_tile_equal(c, ref.tile_int64(a, b), "significands")


def test_tile_powers_of_two_across_the_exponent_range(env):
    """A[i][k] = +-2^(e_k + d_i) and B[k][j] = +-2^(c_j - e_k) with e, d, c in
    [-30, 30]: operands span 2^-60 .. 2^60, every product of element (i, j) is
    +-2^(d_i + c_j), so each partial sum is a small integer times that power:
    exact in any order."""
    _, pr = env
    rng = np.random.default_rng(5)
    e = rng.permutation(np.linspace(-30, 30, 32).round().astype(int))
    d = rng.permutation(np.linspace(-30, 30, 32).round().astype(int))
    cj = rng.permutation(np.linspace(-30, 30, 32).round().astype(int))
    a = rng.choice([-1.0, 1.0], (32, 32)) * 2.0 ** (e[None, :] + d[:, None])
    b = rng.choice([-1.0, 1.0], (32, 32)) * 2.0 ** (cj[None, :] - e[:, None])
    assert np.abs(a).max() == 2.0 ** 60 and np.abs(a).min() == 2.0 ** -60
    assert np.abs(b).max() == 2.0 ** 60 and np.abs(b).min() == 2.0 ** -60
    a_bits, b_bits = ref.bf16_exact(a), ref.bf16_exact(b)
    want = ref.tile_float64(a_bits, b_bits)
    n = want / 2.0 ** (d[:, None] + cj[None, :])
    assert np.array_equal(n, np.round(n)) and np.abs(n).max() <= 32 and len(np.unique(n)) > 8
    assert_tile_equal(pr.mfma_tile(a_bits, b_bits), want, "powers of two")


@pytest.mark.parametrize("special", ["+inf", "-inf", "nan", "inf and nan"])
def test_tile_inf_and_nan_stay_in_their_row(env, special):
    """One +-Inf and/or one NaN in A, small integers elsewhere. The Inf row of
    C is +-Inf with the sign of B's entry in that k-row, and NaN where that
    entry is 0; the NaN row of C is NaN throughout; every other row is exact.
    bf16 subnormals are left out of this file: nothing the kernels' guides say
    fixes whether the instruction keeps or flushes them."""
    _, pr = env
    rng = np.random.default_rng(11)
    k = 32
    a = rng.integers(-8, 9, (32, k)).astype(np.float64)
    b = rng.integers(-6, 7, (k, 32)).astype(np.float64)
    ri, ki, rn, kn = 5, 19, 22, 3
    b[ki, :] = np.resize(np.array([2.0, -3.0, 0.0, 1.0, -1.0, 0.0, 5.0]), 32)  # +, - and 0 under the Inf
    b[kn, ::4] = 0.0  # a NaN times 0 is still a NaN
    if "inf" in special:
        a[ri, ki] = -np.inf if special == "-inf" else np.inf
    if "nan" in special:
        a[rn, kn] = np.nan
    a_bits, b_bits = ref.bf16_encode(a), ref.bf16_encode(b)
    assert np.array_equal(ref.bf16_decode(a_bits), a, equal_nan=True)
    want = ref.tile_float64(a_bits, b_bits)
    c = pr.mfma_tile(a_bits, b_bits)
    # what the reference must itself look like
    rows_special = {ri} if "inf" in special else set()
    rows_special |= {rn} if "nan" in special else set()
    plain = [i for i in range(32) if i not in rows_special]
    assert np.isfinite(want[plain]).all()
    if "inf" in special:
        s = float(np.sign(a[ri, ki]))
        assert np.array_equal(np.isnan(want[ri]), b[ki] == 0)
        assert all(want[ri, j] == s * np.sign(b[ki, j]) * np.inf for j in range(32) if b[ki, j] != 0)
    if "nan" in special:
        assert np.isnan(want[rn]).all()
    # and the tile against it
    assert np.array_equal(np.isnan(c), np.isnan(want)), (special, np.argwhere(np.isnan(c) != np.isnan(want))[:12].tolist())
    ok = np.isnan(want) | (bits32(c) == bits32(want))
    assert ok.all(), (special, [(int(i), int(j), float(c[i, j]), float(want[i, j])) for i, j in np.argwhere(~ok)[:12]])


def test_tile_rounding_stays_inside_the_accumulation_bound(env):
    """Random normal bf16 operands, K = 256, against float64: per element
    |C - ref| <= K 2^-23 sum_k |a_ik||b_kj|, the textbook bound for K
    additions with unit round-off 2^-23 (any order, truncating adders
    included; the products of two bf16 are exact in fp32). A sequential fp32
    accumulation of such inputs uses about 0.2 % of it; the largest ratio seen
    is printed (profiles/mfma_probe_checks.md keeps the figure)."""
    _, pr = env
    k = 256
    rng = np.random.default_rng(2024)
    a_bits = ref.bf16_encode(rng.standard_normal((32, k)))
    b_bits = ref.bf16_encode(rng.standard_normal((k, 32)))
    a, b = ref.bf16_decode(a_bits), ref.bf16_decode(b_bits)
    assert np.isfinite(a).all() and np.abs(a[a != 0]).min() >= 2.0 ** -126  # no subnormal operand
    assert np.isfinite(b).all() and np.abs(b[b != 0]).min() >= 2.0 ** -126
    want = ref.tile_float64(a_bits, b_bits)
    bound = k * 2.0 ** -23 * ref.abs_product_sum(a_bits, b_bits)
    c = pr.mfma_tile(a_bits, b_bits).astype(np.float64)
    ratio = np.abs(c - want) / bound
    seq = np.zeros((32, 32), np.float32)
    for kk in range(k):
        seq += (a[:, kk:kk + 1] * b[kk:kk + 1, :]).astype(np.float32)
    print(f"mfma tile K={k}: max |C - ref| / bound = {ratio.max():.6f} "
          f"(sequential fp32 on the CPU: {(np.abs(seq - want) / bound).max():.6f})")
    assert np.isfinite(c).all()
    assert (ratio <= 1.0).all(), (float(ratio.max()), np.argwhere(ratio > 1.0)[:8].tolist())


# ----------------------------------------------------------- xs_mfma_check
def test_production_check_passes_and_is_the_pipeline_the_tests_drive(env):
    """mfma_check at K = 16, 64, 256, and its three stages by hand: the
    check's integers through k_mfma_tile satisfy the check's comparator, and
    one bit flipped in the host copy of C makes that comparator name it."""
    _, pr = env
    for k in (16, 64, 256):
        r = pr.mfma_check(0, k)
        assert r["healthy"] and r["mismatches"] == 0 and r["k"] == k, r
        a, b = pr.mfma_inputs(k)
        ra, rb = ref.check_inputs(k)
        assert np.array_equal(a, ra) and np.array_equal(b, rb)
        c = pr.mfma_tile(ref.bf16_exact(a), ref.bf16_exact(b))
        assert_tile_equal(c, ref.tile_int64(ra, rb), k)
        assert pr.mfma_compare(k, c) == (0, [])
        for at, bit in (((0, 0), 0), ((17, 9), 22), ((31, 31), 31)):
            flipped = c.copy()
            flipped.view(np.uint32)[at] ^= np.uint32(1 << bit)
            if c[at] == 0 and bit == 31:
                continue  # -0 equals 0: not a mismatch of values
            assert pr.mfma_compare(k, flipped) == (1, [32 * at[0] + at[1]]), (k, at, bit)
    assert pr.mfma_check(0)["k"] == 64


@pytest.mark.parametrize("k", [24, 0, -16, 8, 4096 + 16])
def test_production_check_refuses_a_k_it_cannot_run(env, k):
    from flex_gpu_scheduler_amd.ops.hip_probe import ProbeError

    _, pr = env
    with pytest.raises(ProbeError) as ei:
        pr.mfma_check(0, k)
    assert ei.value.rc == BAD_ARGS
    if k > 0:
        with pytest.raises(ProbeError) as ei:
            pr.mfma_tile(np.zeros((32, k), np.uint16), np.zeros((k, 32), np.uint16))
        assert ei.value.rc == BAD_ARGS


# ------------------------------------------ k_mfma_peak, checked instantiation
def check_peak_launch(r, peak_ref, selected):
    """Everything one checked launch must satisfy; returns the blocks that ran."""
    iters, acc, ran, xcd = r["iters"], r["acc"], r["ran"], r["xcd"]
    assert iters < peak_ref["limit"]  # iters x T exact in fp32 in any order
    want = (iters * peak_ref["one"]).astype(np.float32)
    assert np.array_equal(want.astype(np.float64), iters * peak_ref["one"])
    in_mask = np.array([(selected >> int(x)) & 1 == 1 for x in xcd])
    assert np.array_equal(ran, in_mask), (np.flatnonzero(ran != in_mask)[:8].tolist(), xcd[:16].tolist())
    bits = acc.view(np.uint32)
    assert (bits[~ran] == 0xFFFFFFFF).all(), "a workgroup that exited stored accumulators"
    got = bits[ran]  # [ran blocks, 256, kAcc, 16]
    if len(got):
        for n in range(1, got.shape[2]):
            assert np.array_equal(got[:, :, n], got[:, :, 0]), f"accumulator {n} differs from accumulator 0"
        bad = np.argwhere(got[:, :, 0] != want.view(np.uint32)[None])
        assert len(bad) == 0, (iters, len(bad), [(int(b), int(t), int(q), float(acc[ran][b, t, 0, q]), float(want[t, q]))
                                                  for b, t, q in bad[:8]])
    hist = [int(((xcd == x) & ran).sum()) for x in range(8)]
    assert r["active_per_xcd"] == hist, (r["active_per_xcd"], hist)
    assert sum(r["active_per_xcd"]) == int(ran.sum())
    return int(ran.sum())


@pytest.mark.parametrize("blocks", [1, 8])
@pytest.mark.parametrize("iters", [1, 3, 64, 257])
def test_peak_accumulators_are_iters_times_the_tile(env, dev, peak_ref, iters, blocks):
    _, pr = env
    r = pr.mfma_peak_op(0, dev["mask"], iters=iters, blocks=blocks)
    assert r["acc"].shape == (blocks, 256, 4, 16)
    assert check_peak_launch(r, peak_ref, dev["mask"]) == blocks


def test_peak_full_launch_every_lane_of_every_block(env, dev, peak_ref):
    """The production launch size, 8 workgroups per CU, once."""
    _, pr = env
    blocks = 8 * dev["cus"]
    r = pr.mfma_peak_op(0, dev["mask"], iters=3, blocks=0)
    assert r["acc"].shape[0] == blocks
    assert check_peak_launch(r, peak_ref, dev["mask"]) == blocks
    assert all(r["active_per_xcd"][x] > 0 for x in dev["present"])


@pytest.mark.parametrize("mask", [0x01, 0x80, 0xA5, 0x2A, 0xFF])
def test_peak_mask_selects_exactly_its_xcds(env, dev, peak_ref, mask):
    """A workgroup ran exactly when the XCD it recorded is in the mask, the
    per-XCD counters are the histogram of those records, and the timed
    instantiation counts the same way. Masks are cut down to the XCDs the
    census saw (a partitioned device: to all of them where none is left)."""
    _, pr = env
    m = (mask & dev["mask"]) or dev["mask"]
    blocks = 4 * dev["cus"]
    r = pr.mfma_peak_op(0, m, iters=2, blocks=blocks)
    n = check_peak_launch(r, peak_ref, m)
    assert all((r["active_per_xcd"][x] > 0) == bool(m >> x & 1) for x in range(8)), (hex(m), r["active_per_xcd"])
    assert 0 < n <= blocks and (n == blocks) == (m == dev["mask"])
    t = pr.mfma_peak(0, m, iters=16, blocks=blocks)
    assert all((t["active_per_xcd"][x] > 0) == bool(m >> x & 1) for x in range(8)), (hex(m), t["active_per_xcd"])
    assert t["active_blocks"] == sum(t["active_per_xcd"]) and 0 < t["active_blocks"] <= blocks
    assert t["flops"] == ref.peak_flops(t["active_blocks"], 16)


def test_peak_flop_count_is_the_formula(env, dev):
    """active x 4 waves x kAcc x iters x 32,768, with active the workgroups
    counted (all of them under a mask of every XCD), in xs_mfma_peak and in
    the line probe_kernels prints."""
    from flex_gpu_scheduler_amd.tools.probe_kernels import mfma_row

    _, pr = env
    for iters, blocks in ((64, 0), (5, 2 * dev["cus"])):
        t = pr.mfma_peak(0, dev["mask"], iters=iters, blocks=blocks)
        assert t["active_blocks"] == (blocks or 8 * dev["cus"]) and t["iters"] == iters
        assert t["flops"] == t["active_blocks"] * 4 * 4 * iters * 32768 == ref.peak_flops(t["active_blocks"], iters)
        assert t["ms"] > 0 and t["tflops"] == pytest.approx(t["flops"] / (t["ms"] * 1e-3) / 1e12, rel=1e-9)
        row = mfma_row(t)
        assert row["flops_per_dispatch"] == t["flops"] and row["mfma_insts_per_dispatch"] == t["active_blocks"] * 16 * iters


@pytest.mark.parametrize("mask", [0, 0x100, 0x1FF])
def test_peak_refuses_masks_outside_the_eight_xcds(env, mask):
    from flex_gpu_scheduler_amd.ops.hip_probe import ProbeError

    _, pr = env
    with pytest.raises(ProbeError) as ei:
        pr.mfma_peak(0, mask, iters=1, blocks=1)
    assert ei.value.rc == BAD_ARGS
    with pytest.raises(ProbeError) as ei:
        pr.mfma_peak_op(0, mask, iters=1, blocks=1)
    assert ei.value.rc == BAD_ARGS


def test_peak_fails_when_a_selected_xcd_stays_idle(env, dev):
    """One workgroup lands on one XCD: with every present XCD selected the
    others ran nothing, and the call must fail and name them, not report a
    rate. On a partitioned device a mask naming an XCD the census did not see
    does the same."""
    from flex_gpu_scheduler_amd.ops.hip_probe import ProbeError

    _, pr = env
    if len(dev["present"]) > 1:
        with pytest.raises(ProbeError) as ei:
            pr.mfma_peak(0, dev["mask"], iters=1, blocks=1)
        assert ei.value.rc == IDLE_XCD, ei.value
        named = re.search(r"XCD\(s\) ([\d,]+)", str(ei.value))
        assert named, ei.value
        idle = {int(x) for x in named.group(1).split(",")}
        assert idle < set(dev["present"]) and len(idle) == len(dev["present"]) - 1, (idle, dev["present"])
    absent = [x for x in range(8) if x not in dev["present"]]
    if absent:
        with pytest.raises(ProbeError) as ei:
            pr.mfma_peak(0, dev["mask"] | (1 << absent[0]), iters=1)
        assert ei.value.rc == IDLE_XCD, ei.value
        named = re.search(r"XCD\(s\) ([\d,]+)", str(ei.value))
        assert named and {int(x) for x in named.group(1).split(",")} == {absent[0]}, ei.value


# ---------------------------------------------------------- health pattern
def guarded_words(torch, n):
    """(whole, view): `view` holds n int32 words inside the sentinel-filled
    `whole`, starting 4 bytes past a 16-byte boundary."""
    whole = torch.full((n + 2 * PADW + 1,), SENT, dtype=torch.int32, device="cuda")
    view = whole[PADW + 1:PADW + 1 + n]
    assert view.data_ptr() % 16 == 4 and view.numel() == n
    return whole, view


def guards_intact(whole, n):
    return bool((whole[:PADW + 1] == SENT).all()) and bool((whole[PADW + 1 + n:] == SENT).all())


@pytest.mark.parametrize("n", [1, 255, 257, 65537, (1 << 20) + 3])
def test_health_pattern_and_verdict_on_a_caller_buffer(env, n):
    """k_pattern at the health check's grid writes exactly the numpy pattern
    and nothing beside it; the verdict over it is healthy with both sums the
    numpy sum; one flipped bit turns the verdict and moves the device's sum by
    exactly that power of two."""
    torch, pr = env
    want = ref.health_pattern(n)
    total = int(want.astype(np.uint64).sum())
    whole, view = guarded_words(torch, n)
    pr.pattern(view)
    got = view.cpu().numpy().view(np.uint32)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8].tolist()
    assert guards_intact(whole, n)
    v = pr.health_verify(view)
    assert v == {"healthy": True, "device_sum": total, "host_sum": total}
    for idx, bit in ((0, 0), (n // 2, 17), (n - 1, 31)):
        was_set = (int(want[idx]) >> bit) & 1
        flip = (1 << bit) - (1 << 32 if bit == 31 else 0)  # as an int32 bit pattern
        view[idx] ^= flip
        v = pr.health_verify(view)
        assert v["healthy"] is False and v["host_sum"] == total, (idx, bit, v)
        assert v["device_sum"] - total == (-(1 << bit) if was_set else (1 << bit)), (idx, bit, v)
        view[idx] ^= flip
    assert pr.health_verify(view)["healthy"] is True
    assert guards_intact(whole, n)


def test_health_ops_refuse_ragged_and_misaligned_buffers(env):
    from flex_gpu_scheduler_amd.ops.hip_probe import ProbeError

    torch, pr = env
    whole = torch.full((64,), 0x5A, dtype=torch.uint8, device="cuda")
    for view, rc in ((whole[16:19], BAD_ARGS), (whole[17:21], -1001), (whole[16:16], BAD_ARGS)):
        for op in (pr.pattern, pr.health_verify):
            with pytest.raises(ProbeError) as ei:
                op(view)
            assert ei.value.rc == rc, (op, view.shape)
    assert bool((whole == 0x5A).all())


def test_health_check_is_still_healthy(env):
    _, pr = env
    h = pr.health(0, 256 << 20)
    assert h["healthy"] and h["device_sum"] == h["host_sum"] > 0, h
    small = pr.health(0, 4 * 65537)
    assert small["healthy"] and small["host_sum"] == int(ref.health_pattern(65537).astype(np.uint64).sum()), small
