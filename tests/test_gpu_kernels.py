"""What the HIP/CDNA4 streaming probes (csrc/hip/hbm_probe.hip) move and
compute on a real MI355X. Each kernel runs on torch device tensors and is
compared with an independent reference of the same op: bit-exact for copy and
write, a per-element float64 bound for triad, the XOR of all words and the
count of 16-B loads for the read paths (their checked instantiations).

What the sizes reach. A persistent grid strides by CUs x workgroups-per-CU x
256 lanes (at least 32,768 lanes), so at ODD (65,539 lanes) the `*_variants`
tests run only the remainder loop of the U = 4 and U = 8 kernels, and the
large default-variant sizes (U = 1) have no separate body. The unrolled
bodies, the body/tail hand-over, the one-shot grid and the path where a grid
smaller than the buffer strides over the rest are reached with an explicit
small grid (`grid=`), and once at the production grid with a buffer of
U x stride + stride/2 + 3 lanes. Every destination there is a view into a
sentinel-filled tensor, so a store outside the buffer is seen, not suffered.
k_pinned is checked over non-contiguous XCD masks and ragged chunk counts,
and a launch that leaves a selected XCD's slice untouched must raise;
k_checksum and k_segments run on buffers the test owns."""
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    import torch  # first: the probe library then binds to torch's HIP runtime

    assert torch.cuda.is_available()
    torch.cuda.init()
    from flex_gpu_scheduler_amd.ops.hip_probe import HipProbe

    return torch, HipProbe()


# 1 MiB + 48 B: not a multiple of (blocks x 256 lanes x unroll), so every
# variant runs its remainder loop.
ODD = (1 << 20) + 48
VARIANTS = [(u, nt, b) for u in (1, 4, 8) for nt in (True, False) for b in (4, 8, 16)]


def _pattern(torch, n_vec4: int, seed: int):
    s = seed & 0xFFFFFFFF
    lane = [s, s ^ 0x55555555, (s + 1) & 0xFFFFFFFF, ~s & 0xFFFFFFFF]
    lane = [v - (1 << 32) if v >= (1 << 31) else v for v in lane]  # as int32 bit patterns
    return torch.tensor(lane, dtype=torch.int32, device="cuda").repeat(n_vec4)


@pytest.mark.parametrize("nbytes", [16, 4096, ODD, 64 << 20])
def test_copy_is_bit_exact(env, nbytes):
    torch, pr = env
    src = torch.randint(-(1 << 31), (1 << 31) - 1, (nbytes // 4,), dtype=torch.int32, device="cuda")
    dst = torch.zeros_like(src)
    pr.copy(dst, src)
    torch.cuda.synchronize()
    assert torch.equal(dst, src)


@pytest.mark.parametrize("u,nt,bpc", VARIANTS)
def test_copy_variants(env, u, nt, bpc):
    torch, pr = env
    src = torch.randint(-(1 << 31), (1 << 31) - 1, (ODD // 4,), dtype=torch.int32, device="cuda")
    dst = torch.full_like(src, -1)
    pr.copy(dst, src, variant=pr.variant(u, nt, bpc))
    assert torch.equal(dst, src)


@pytest.mark.parametrize("seed", [7, 0, 0xDEADBEEF])
@pytest.mark.parametrize("u,nt,bpc", [(1, False, 4), (4, True, 8), (8, True, 16)])
def test_write_pattern(env, seed, u, nt, bpc):
    torch, pr = env
    dst = torch.zeros(ODD // 4, dtype=torch.int32, device="cuda")
    pr.write_pattern(dst, seed=seed, variant=pr.variant(u, nt, bpc))
    assert torch.equal(dst, _pattern(torch, ODD // 16, seed))


def _assert_triad(torch, a, b, c, scale, what=None):
    """a = b + s*c within half an ulp of each rounding the kernel may make:
    |a - ref| <= 2^-24 (|s*c| + |ref|)(1 + 2^-20) + 2^-149 per element, against
    ref = b + float32(s)*c in float64. A fused multiply-add rounds once:
    at most 2^-24 |ref|. Multiply, then add, rounds twice: 2^-24 |s*c| for
    the product and 2^-24 |ref + that error| for the sum; the second-order
    term and the float64 reference's own rounding sit inside the 2^-20
    slack, and 2^-149 covers a product rounded in the subnormal range."""
    s32 = torch.tensor(scale, dtype=torch.float32).double().item()
    sc = s32 * c.double()
    ref = b.double() + sc
    bound = 2.0 ** -24 * (sc.abs() + ref.abs()) * (1 + 2.0 ** -20) + 2.0 ** -149
    err = (a.double() - ref).abs()
    bad = ~(err <= bound)  # a NaN is bad
    if bool(bad.any()):
        i = int(bad.nonzero()[0])
        raise AssertionError(f"triad {what}: {int(bad.sum())} of {a.numel()} elements outside the bound; first at {i}: "
                             f"a={a[i].item()!r} ref={ref[i].item()!r} err={err[i].item():.3e} "
                             f"bound={bound[i].item():.3e} b={b[i].item()!r} c={c[i].item()!r} s={s32!r}")


@pytest.mark.parametrize("nbytes", [4096, ODD, 256 << 20])
@pytest.mark.parametrize("scale", [3.0, -0.5])
def test_triad_matches_fp32_reference(env, nbytes, scale):
    torch, pr = env
    g = torch.Generator(device="cuda").manual_seed(nbytes)
    b = torch.randn(nbytes // 4, dtype=torch.float32, device="cuda", generator=g)
    c = torch.randn(nbytes // 4, dtype=torch.float32, device="cuda", generator=g)
    a = torch.full_like(b, float("nan"))
    pr.triad(a, b, c, scale=scale)
    _assert_triad(torch, a, b, c, scale, nbytes)
    assert not torch.isnan(a).any()


@pytest.mark.parametrize("u,nt,bpc", VARIANTS)
def test_triad_variants(env, u, nt, bpc):
    torch, pr = env
    b = torch.arange(ODD // 4, dtype=torch.float32, device="cuda")
    c = torch.full_like(b, 0.25)
    a = torch.zeros_like(b)
    pr.triad(a, b, c, scale=4.0, variant=pr.variant(u, nt, bpc))
    assert torch.equal(a, b + 1.0)  # exact in fp32 for these values


@pytest.mark.parametrize("mask", [0x01, 0x0F, 0xFF])
def test_xcd_pinned_copy_and_write(env, mask):
    torch, pr = env
    from flex_gpu_scheduler_amd.ops.hip_probe import probe as _  # noqa: F401 - same library

    if pr.xcd_census(0, 2048)["distinct_xcds"] < 8 and mask != 0x01:
        pytest.skip("device is partitioned")
    src = torch.randint(-(1 << 31), (1 << 31) - 1, ((8 << 20) // 4 + 12,), dtype=torch.int32, device="cuda")
    dst = torch.zeros_like(src)
    pr.pinned(dst, src, xcd_mask=mask)
    assert torch.equal(dst, src)
    pr.pinned(dst, None, xcd_mask=mask)
    assert torch.equal(dst, torch.tensor([1, 2, 3, 4], dtype=torch.int32, device="cuda").repeat(src.numel() // 4))


def test_rejects_misaligned_and_host_buffers(env):
    torch, pr = env
    x = torch.zeros(64, dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError):
        pr.copy(x[1:17], x[20:36])  # 4-byte offset
    with pytest.raises(ValueError):
        pr.copy(torch.zeros(16, dtype=torch.int32), torch.zeros(16, dtype=torch.int32))


# ----------------------------------------------------------------------------
# Explicit grids, checked reads, sentinels.

PAD = 4096  # bytes of sentinel on each side of every destination
SENT = 0x5EA7C0DE
CHUNK = 16384  # k_pinned hands out chunks of this many vec4 (256 KiB)
UNDRAINED = -1002
POLICIES = [(u, nt) for u in (1, 4, 8) for nt in (True, False)]
MODES = ["read", "write", "copy", "triad"]
SCALES = (3.0, -0.5, 7.123)
N_WORDS = 1 << 20  # shared random source: 4 MiB


def _guarded(torch, nbytes):
    """(whole, view): `view` is a 16-B-aligned int32 view of `nbytes` inside
    `whole`, which is filled with SENT and extends PAD bytes to each side."""
    assert nbytes % 16 == 0
    whole = torch.full(((nbytes + 2 * PAD) // 4,), SENT, dtype=torch.int32, device="cuda")
    view = whole[PAD // 4:(PAD + nbytes) // 4]
    assert view.data_ptr() % 16 == 0
    return whole, view


def _guards_intact(whole, nbytes):
    return bool((whole[:PAD // 4] == SENT).all()) and bool((whole[(PAD + nbytes) // 4:] == SENT).all())


def _xor(words):
    return int(np.bitwise_xor.reduce(words.reshape(-1))) if words.size else 0


@pytest.fixture(scope="module")
def data(env):
    """Random words on the host (numpy, for the references) and the same on
    the device; per triad scale, b and c with a quarter of b set to
    -s*c*(1 + 1e-6) so that b + s*c cancels to ~1e-6 of its operands."""
    torch, pr = env
    rng = np.random.default_rng(20240607)
    host = rng.integers(0, 1 << 32, N_WORDS, dtype=np.uint32)
    out = {"host": host, "dev": torch.from_numpy(host.view(np.int32)).cuda(), "triad": {}}
    nf = 1 << 16
    for s in SCALES:
        b = rng.standard_normal(nf).astype(np.float32)
        c = rng.standard_normal(nf).astype(np.float32)
        q = rng.permutation(nf)[:nf // 4]
        b[q] = (-float(np.float32(s)) * c[q].astype(np.float64) * (1 + 1e-6)).astype(np.float32)
        out["triad"][s] = (torch.from_numpy(b).cuda(), torch.from_numpy(c).cuda())
    out["props"] = pr.props(0)
    out["census"] = pr.xcd_census(0, 4096)
    return out


def _check_stream(torch, pr, data, mode, n, variant, grid):
    """One launch of `mode` over n vec4 with the given variant and grid,
    checked against its reference; destinations are guarded."""
    what = (mode, f"n={n}", f"variant={variant:#x}", f"grid={grid}")
    nbytes = 16 * n
    src = data["dev"][:4 * n]
    if mode == "read":
        assert pr.read_fold(src, variant=variant, grid=grid) == (_xor(data["host"][:4 * n]), n), what
        return
    if mode == "triad":
        for s in SCALES:
            b, c = (t[:4 * n] for t in data["triad"][s])
            whole, a = _guarded(torch, nbytes)
            pr.triad(a.view(torch.float32), b, c, scale=s, variant=variant, grid=grid)
            _assert_triad(torch, a.view(torch.float32), b, c, s, what)
            assert _guards_intact(whole, nbytes), what
        return
    whole, dst = _guarded(torch, nbytes)
    if mode == "copy":
        pr.copy(dst, src, variant=variant, grid=grid)
        assert torch.equal(dst, src), what
    else:
        pr.write_pattern(dst, seed=0xDEADBEEF, variant=variant, grid=grid)
        assert torch.equal(dst, _pattern(torch, n, 0xDEADBEEF)), what
    assert _guards_intact(whole, nbytes), what


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("u,nt", POLICIES)
def test_stream_explicit_grid_bodies_and_tails(env, data, u, nt, mode):
    """Grids of 1 and 3 workgroups (stride s = 256 g lanes): one lane; the
    second grid-stride step; one lane short of a full body row (that lane
    takes the tail, the rest the body); the body alone; two body iterations
    and a ragged tail."""
    torch, pr = env
    for g in (1, 3):
        s = 256 * g
        for n in (1, s + 1, u * s - 1, u * s, 2 * u * s + s + 5):
            _check_stream(torch, pr, data, mode, n, pr.variant(u, nt, 8), g)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("u,nt", POLICIES)
def test_stream_one_shot_and_capped_grid(env, data, u, nt, mode):
    """The one-shot grid as grid_for derives it (one workgroup per 256 U
    lanes, 4 here), and a grid smaller than that (as at the 2^22 cap): the
    kernel's grid stride must cover the rest."""
    torch, pr = env
    one_shot = pr.variant(u, nt, 0)
    _check_stream(torch, pr, data, mode, 256 * u * 3 + 5, one_shot, 0)
    _check_stream(torch, pr, data, mode, 256 * u * 5 + 7, one_shot, 2)


@pytest.mark.parametrize("mode", ["copy", "triad"])
@pytest.mark.parametrize("u,bpc", [(4, 8), (8, 16)])
def test_stream_production_grid_enters_the_body(env, data, u, bpc, mode):
    """grid_for's persistent grid with a buffer one body iteration, half a
    row and 3 lanes long (at most 136 MiB per array on an SPX device)."""
    torch, pr = env
    stride = data["props"]["computeUnits"] * bpc * 256
    n = u * stride + stride // 2 + 3
    g = torch.Generator(device="cuda").manual_seed(n)
    variant = pr.variant(u, True, bpc)
    if mode == "copy":
        src = torch.randint(-(1 << 31), (1 << 31) - 1, (4 * n,), dtype=torch.int32, device="cuda", generator=g)
        whole, dst = _guarded(torch, 16 * n)
        pr.copy(dst, src, variant=variant)
        assert torch.equal(dst, src)
    else:
        s = 7.123
        b = torch.randn(4 * n, dtype=torch.float32, device="cuda", generator=g)
        c = torch.randn(4 * n, dtype=torch.float32, device="cuda", generator=g)
        s32 = torch.tensor(s, dtype=torch.float32).double().item()
        b[1::4] = (-s32 * c[1::4].double() * (1 + 1e-6)).float()
        whole, a = _guarded(torch, 16 * n)
        pr.triad(a.view(torch.float32), b, c, scale=s, variant=variant)
        _assert_triad(torch, a.view(torch.float32), b, c, s, (u, bpc, n))
    assert _guards_intact(whole, 16 * n)


def test_triad_special_values(env):
    """+-0, +-inf, NaN, overflow of FLT_MAX and subnormal operands with s = 2.
    Every case has the same IEEE result fused or not, exactly representable
    (or NaN or inf), so NaN positions must agree and everything else is
    compared bit for bit with the float64 result rounded to fp32: signs of
    zero and inf, and subnormals kept (the library is built without a
    flush-to-zero flag)."""
    torch, pr = env
    inf, nan = np.inf, np.nan
    fmax = float(np.finfo(np.float32).max)
    t = 2.0 ** -149  # the smallest subnormal
    cases = [  # (b, c): a = b + 2c
        (0.0, 0.0), (0.0, -0.0), (-0.0, -0.0), (-0.0, 0.0), (1.5, -0.75), (-1.5, 0.75),
        (inf, 1.0), (1.0, -inf), (-inf, -inf), (inf, -inf), (nan, 1.0), (1.0, nan), (nan, inf),
        (0.0, fmax), (0.0, -fmax), (fmax, fmax), (-fmax, 0.0), (fmax, -fmax / 2),
        (t, t), (-t, 0.0), (0.0, t), (3 * t, -t), (2.0 ** -126, -2.0 ** -127), (2.0 ** -126, -2.0 ** -148),
        (2.0 ** -127, 2.0 ** -128), (-2.0 ** -127, -2.0 ** -128), (2.0 ** -130, -2.0 ** -131), (1.0, t),
    ]
    assert len(cases) % 4 == 0
    b0 = np.array([x for x, _ in cases], dtype=np.float32)
    c0 = np.array([y for _, y in cases], dtype=np.float32)
    assert b0[18] != 0 and c0[22] != 0  # the host kept the subnormals
    for u, grid in ((1, 0), (4, 1), (8, 1)):  # tail only; body and tail of the unrolled kernels
        nf = 4 * (256 * u + 3)
        bh, ch = np.resize(b0, nf), np.resize(c0, nf)
        with np.errstate(over="ignore", invalid="ignore"):
            exp = (bh.astype(np.float64) + 2.0 * ch.astype(np.float64)).astype(np.float32)
        whole, a = _guarded(torch, 4 * nf)
        pr.triad(a.view(torch.float32), torch.from_numpy(bh).cuda(), torch.from_numpy(ch).cuda(), scale=2.0,
                 variant=pr.variant(u, True, 8), grid=grid)
        got = a.cpu().numpy().view(np.float32)
        assert np.array_equal(np.isnan(got), np.isnan(exp)), (u, np.flatnonzero(np.isnan(got) != np.isnan(exp))[:8])
        ok = np.isnan(exp) | (got.view(np.uint32) == exp.view(np.uint32))
        i = np.flatnonzero(~ok)[:8]
        assert ok.all(), (u, [(int(j), float(bh[j]), float(ch[j]), float(got[j]), float(exp[j])) for j in i])
        assert _guards_intact(whole, 4 * nf)


# ------------------------------------------------------------------ k_pinned

@pytest.mark.parametrize("mask", [0x01, 0x80, 0xA5, 0x2A, 0x0F, 0xFF])
def test_pinned_masks_and_ragged_sizes(env, data, mask):
    """Less than one chunk (a single selected XCD has a slice); as many
    chunks as 4 XCDs; a chunk count that 3 or 4 XCDs do not divide, with a
    ragged last chunk; one chunk and 3 x 256 + 1 lanes (the edge of the inner
    4-way unrolled loop)."""
    torch, pr = env
    if data["census"]["distinct_xcds"] < 8:
        pytest.skip("needs the 8 XCDs of an unpartitioned device")
    fill = torch.tensor([1, 2, 3, 4], dtype=torch.int32, device="cuda")
    for n in (3, 4 * CHUNK, 5 * CHUNK + 12, CHUNK + 3 * 256 + 1):
        src = data["dev"][:4 * n]
        whole, dst = _guarded(torch, 16 * n)
        pr.pinned(dst, src, xcd_mask=mask)
        assert torch.equal(dst, src), n
        assert _guards_intact(whole, 16 * n), n
        whole, dst = _guarded(torch, 16 * n)
        pr.pinned(dst, None, xcd_mask=mask)
        assert torch.equal(dst, fill.repeat(n)), n
        assert _guards_intact(whole, 16 * n), n
        assert pr.pinned_read_fold(src, xcd_mask=mask) == (_xor(data["host"][:4 * n]), n), n


def test_pinned_refuses_xcds_the_gpu_does_not_have(env, data):
    from flex_gpu_scheduler_amd.ops.hip_probe import ProbeError

    torch, pr = env
    whole, dst = _guarded(torch, 64)
    for mask in (0x100, 0x1FF):
        with pytest.raises(ProbeError) as ei:
            pr.pinned(dst, data["dev"][:16], xcd_mask=mask)
        assert ei.value.rc == -1000
        with pytest.raises(ProbeError) as ei:
            pr.hbm_bandwidth_xcd(0, mask, 1 << 20, 1, "read")
        assert ei.value.rc == -1000
    assert bool((whole == SENT).all())


def test_pinned_undrained_launch_raises(env, data):
    """A selected XCD that receives no workgroup leaves its slice untouched:
    the call must fail, not return. One workgroup lands on one XCD, so with
    all 8 selected and 8 chunks exactly one eighth is copied. On a partitioned
    device a mask naming an XCD the census did not see does the same."""
    from flex_gpu_scheduler_amd.ops.hip_probe import ProbeError

    torch, pr = env
    n = 8 * CHUNK
    src = data["dev"][:4 * n]
    whole, dst = _guarded(torch, 16 * n)
    hist = data["census"]["blocks_per_xcd"]
    if data["census"]["distinct_xcds"] == 8:
        with pytest.raises(ProbeError) as ei:
            pr.pinned(dst, src, xcd_mask=0xFF, grid=1)
        assert ei.value.rc == UNDRAINED, ei.value
        rows, want = dst.view(8, -1), src.view(8, -1)
        done = [i for i in range(8) if torch.equal(rows[i], want[i])]
        assert len(done) == 1, done
        assert all(bool((rows[i] == SENT).all()) for i in range(8) if i not in done)
        named = re.search(r"XCD\(s\) ([\d,]+)", str(ei.value))  # slice i is XCD i's when all 8 are selected
        assert named and {int(x) for x in named.group(1).split(",")} == set(range(8)) - set(done), ei.value
    else:
        present = sum(1 << x for x in range(8) if hist[x])
        absent = next(x for x in range(8) if not hist[x])
        with pytest.raises(ProbeError) as ei:
            pr.pinned(dst, src, xcd_mask=present | (1 << absent))
        assert ei.value.rc == UNDRAINED, ei.value
    assert _guards_intact(whole, 16 * n)


# ------------------------------------------------- k_checksum and k_segments

@pytest.mark.parametrize("n", [1, 255, 257, 65537])
def test_checksum_of_a_known_buffer(env, data, n):
    """The health check's kernel on words the test chose (a 4-byte-aligned
    view, sizes off the 256-lane grid), and one flipped bit moves the sum by
    exactly that power of two."""
    torch, pr = env
    t = data["dev"][:n + 2].clone()[1:1 + n]  # a word before and one after that must not be summed
    assert t.data_ptr() % 16 == 4
    base = pr.checksum(t)
    assert base == int((t.to(torch.int64) & 0xFFFFFFFF).sum())
    assert base == int(data["host"][1:1 + n].astype(np.uint64).sum())
    for idx, bit in ((0, 0), (n // 2, 17), (n - 1, 31)):
        was_set = (int(data["host"][1 + idx]) >> bit) & 1
        flip = (1 << bit) - (1 << 32 if bit == 31 else 0)  # as an int32 bit pattern
        t[idx] ^= flip
        assert pr.checksum(t) - base == (-(1 << bit) if was_set else (1 << bit)), (idx, bit)
        t[idx] ^= flip


@pytest.mark.parametrize("nt", [False, True])
@pytest.mark.parametrize("seg,stride", [(16, 128), (16, 4096), (48, 128), (48, 4096), (1024, 4096)])
def test_segments_touch_exactly_their_bytes(env, data, seg, stride, nt):
    """Write mode fills the first `seg` bytes of every slot and nothing else;
    read mode loads exactly those lanes (count and XOR)."""
    torch, pr = env
    fill = torch.tensor([5, 6, 7, 8], dtype=torch.int32, device="cuda").repeat(seg // 16)
    for touches in (1, 7, 1000):
        nbytes = stride * touches
        whole, buf = _guarded(torch, nbytes)
        assert pr.segment_op(buf, "write", seg, stride, touches, nt) is None
        slots = buf.view(touches, stride // 4)
        assert bool((slots[:, :seg // 4] == fill).all()), touches
        assert bool((slots[:, seg // 4:] == SENT).all()), touches
        assert _guards_intact(whole, nbytes), touches
        words = data["host"][:nbytes // 4].reshape(touches, stride // 4)[:, :seg // 4]
        got = pr.segment_op(data["dev"][:nbytes // 4], "read", seg, stride, touches, nt)
        assert got == (_xor(words), touches * seg // 16), touches
