"""k_cu_sweep on the GPU (csrc/hip/cu_sweep.hip): every CU is reached and
identified, the three engines' digests match an independent numpy
reimplementation of the documented formulas, injected mis-compares are
localised to their CU and XCD, and bad arguments are refused."""
import numpy as np
import pytest

from flex_gpu_scheduler_amd.control.node_agent import GpuHealth, hip_health_fn
from flex_gpu_scheduler_amd.ops.hip_probe import ProbeError, probe, summarize_sweep

pytestmark = pytest.mark.gpu

M = 0xFFFFFFFF
CHAIN = 32768  # kSweepChain


@pytest.fixture(scope="module")
def p():
    return probe()


@pytest.fixture(scope="module")
def cus(p):
    return int(p.props(0)["computeUnits"])


@pytest.fixture(scope="module")
def clean(p):
    return p.cu_sweep(0)


def _keys(records):
    return {(r["xcd"], r["cu"]) for r in records}


# ------------------------------------------------- numpy reference digests
def ref_valu() -> int:
    t = np.arange(256, dtype=np.uint64)
    x = (((t + 1) * 0x9E3779B9) & M).astype(np.uint32)
    a, c = np.uint32(1664525), np.uint32(1013904223)
    with np.errstate(over="ignore"):
        for _ in range(CHAIN):
            x = x * a + c
            x ^= x >> np.uint32(15)
            x = (x << np.uint32(7)) | (x >> np.uint32(25))
    return int((x.astype(np.uint64) * (2 * t + 1)).sum() & M)


def ref_mfma(k: int) -> int:
    i, kk, j = np.arange(32)[:, None], np.arange(k), np.arange(32)[None, :]
    a = (i * 3 + kk[None, :] * 7) % 17 - 8
    b = (kk[:, None] * 5 + j * 11 + np.where(j > kk[:, None], 3, 0)) % 13 - 6
    c = a.astype(np.int64) @ b.astype(np.int64)
    w = 2 * (32 * np.arange(32)[:, None] + np.arange(32)[None, :]) + 1
    d = int(((c & M) * w).sum()) & M
    return (15 * d) & M  # four identical waves: sum_w D << w


def ref_lds(lds_bytes: int) -> int:
    i = np.arange(lds_bytes // 4, dtype=np.uint64)
    p0 = ((i * 2654435761) & M) ^ 0xA5A5A5A5
    d = [int(((v * (2 * i + 1)) & M).sum()) & M for v in (p0, p0 ^ M)]
    return d[0] ^ (((d[1] << 16) | (d[1] >> 16)) & M)


@pytest.fixture(scope="module")
def valu_digest():
    return ref_valu()


# ------------------------------------------------------------------- tests
def test_clean_sweep_covers_every_cu(p, cus, clean):
    s = clean["summary"]
    print("cu_sweep defaults:", {k: s[k] for k in ("rounds", "ms", "blocks", "covered", "uncovered")})
    print("simd masks:", sorted({r["simd_mask"] for r in clean["records"]}))
    xcds = cus // 32
    assert s["covered"]
    assert len(_keys(clean["records"])) == cus  # pins the HW_ID decoding
    assert len(s["xcds"]) == xcds
    for x, v in s["xcds"].items():
        assert v["cus_seen"] == cus // xcds == v["cus_expected"], (x, v)
    assert all(r["fail"] == 0 for r in clean["records"])
    assert s["bad_xcds"] == []


@pytest.mark.parametrize("k", [16, 64])
@pytest.mark.parametrize("lds", ["1KiB", "max"])
def test_digests_match_numpy_reference(p, valu_digest, k, lds):
    lds_bytes = 1024 if lds == "1KiB" else p.cu_sweep_max_lds(0)
    out = p.cu_sweep(0, k=k, lds_bytes=lds_bytes, max_rounds=1)
    want = (ref_mfma(k), valu_digest, ref_lds(lds_bytes))
    got = {(r["mfma"], r["valu"], r["lds"]) for r in out["records"]}
    print("digests", k, lds_bytes, [hex(v) for v in want], len(got))
    assert got == {want}
    assert all(r["fail"] == 0 for r in out["records"])


@pytest.mark.parametrize("bit", [1, 2, 4])
def test_injection_is_localised_to_one_cu(p, clean, bit):
    xcd, cu = sorted(_keys(clean["records"]))[len(clean["records"]) // 9]
    out = p.cu_sweep(0, inject=(xcd, cu, bit))
    s = out["summary"]
    hit = [r for r in out["records"] if (r["xcd"], r["cu"]) == (xcd, cu)]
    assert hit and all(r["fail"] == bit for r in hit)
    assert all(r["fail"] == 0 for r in out["records"] if (r["xcd"], r["cu"]) != (xcd, cu))
    assert s["bad_xcds"] == [xcd]
    assert s["xcds"][xcd]["failed_cus"] == [cu]
    assert s["xcds"][xcd]["fail_bits"] == bit


def test_injection_wildcard_flags_one_whole_xcd(p, clean):
    xcd = max(r["xcd"] for r in clean["records"])
    out = p.cu_sweep(0, inject=(xcd, None, 7))
    s = out["summary"]
    assert s["bad_xcds"] == [xcd]
    assert s["xcds"][xcd]["failed_cus"] == sorted(c for x, c in _keys(out["records"]) if x == xcd)
    assert s["xcds"][xcd]["fail_bits"] == 7
    assert all((r["fail"] == 7) == (r["xcd"] == xcd) for r in out["records"])
    assert all(r["fail"] in (0, 7) for r in out["records"])


def test_one_block_is_uncovered_not_failed(p, cus):
    out = p.cu_sweep(0, blocks=1)
    s = out["summary"]
    assert len(out["records"]) == 1 and s["rounds"] == 1
    assert not s["covered"]
    assert s["bad_xcds"] == [] and out["records"][0]["fail"] == 0
    assert summarize_sweep(out["records"], cus)["uncovered"] == s["uncovered"]
    verdict = hip_health_fn(sweep=True, sweep_args={"blocks": 1})(0)
    assert verdict.ok if isinstance(verdict, GpuHealth) else verdict is True


@pytest.mark.parametrize("kw", [{"k": 32}, {"lds_bytes": 1000}, {"lds_bytes": "above"}])
def test_bad_arguments_are_refused(p, kw):
    if kw.get("lds_bytes") == "above":
        kw = {"lds_bytes": p.cu_sweep_max_lds(0) + 1024}
    with pytest.raises(ProbeError) as e:
        p.cu_sweep(0, **kw)
    assert e.value.rc == -1000
