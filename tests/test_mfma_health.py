"""The MFMA and checksum health checks off the GPU: the host comparator of
xs_mfma_check (xs_mfma_compare) against a numpy product, the check's operands
(xs_mfma_inputs) against their formula, the numpy reference's own properties,
the flop count probe_kernels prints, and hip_health_fn withholding a GPU whose
MFMA or checksum check fails without consulting a sweep."""
import numpy as np
import pytest

import mfma_probe_ref as ref
from flex_gpu_scheduler_amd.control import LocalClient
from flex_gpu_scheduler_amd.control.node_agent import NodeAgent, hip_health_fn
from flex_gpu_scheduler_amd.gpu.discovery import fake_host
from flex_gpu_scheduler_amd.ops import hip_probe
from flex_gpu_scheduler_amd.tools.probe_kernels import mfma_row

KS = (16, 32, 48, 64, 256)


@pytest.fixture(scope="module")
def lib():
    try:
        return hip_probe.HipProbe()
    except (hip_probe.ProbeError, OSError) as e:
        pytest.skip(f"_hipprobe.so does not load here: {e}")


def product(k):
    a, b = ref.check_inputs(k)
    return ref.tile_int64(a, b).astype(np.float32)


# ------------------------------------------------------------ the reference
def test_reference_bf16_round_trip_and_rounding():
    bits = np.arange(1 << 16, dtype=np.uint16)
    v = ref.bf16_decode(bits)
    finite = np.isfinite(v)
    assert np.array_equal(ref.bf16_encode(v[finite]), bits[finite])
    assert np.isnan(ref.bf16_decode(ref.bf16_encode(np.array([np.nan])))).all()
    # 1 + 2^-8 is a tie (to even: 1.0); 1 + 3 * 2^-8 is a tie (to even: 1 + 2^-6); just above a tie rounds up
    assert ref.bf16_decode(ref.bf16_encode(np.array([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -20]))
                           ).tolist() == [1.0, 1 + 2.0 ** -6, 1 + 2.0 ** -7]
    with pytest.raises(AssertionError):
        ref.bf16_exact(np.array([257.0]))
    assert ref.bf16_decode(ref.bf16_exact(np.array([-256.0, 255.0, 2.0 ** -60, 2.0 ** 60]))).tolist() == [
        -256.0, 255.0, 2.0 ** -60, 2.0 ** 60]


def test_reference_maps_are_bijections():
    ops = {ref.operand_index(l, j) for l in range(64) for j in range(8)}
    assert ops == {(r, k) for r in range(32) for k in range(16)}
    cs = {ref.c_index(l, q) for l in range(64) for q in range(16)}
    assert cs == {(i, j) for i in range(32) for j in range(32)}
    assert ref.c_index(0, 4) == (8, 0) and ref.c_index(32, 0) == (4, 0) and ref.c_index(33, 5) == (13, 1)


def test_reference_peak_tile_is_exact_in_fp32_below_23045_iterations():
    t = ref.peak_tiles()
    assert float(t.max()) == 5.6875 and float(t.min()) >= 0.0
    assert np.array_equal(t * 128, np.round(t * 128))  # multiples of 2^-7
    assert all(np.array_equal(t[0], t[w]) for w in range(4))  # 64 = 0 mod 8 and 3 * 64 = 0 mod 16
    assert 23045 < ref.peak_exact_iters_limit() < 23046
    assert ref.peak_flops(2048, 8192) == 2048 * 4 * 4 * 8192 * 32768


def test_reference_check_inputs_are_small_and_b_is_not_symmetric():
    a, b = ref.check_inputs(64)
    assert a.min() == -8 and a.max() == 8 and b.min() == -6 and b.max() == 6
    assert not np.array_equal(b[:32], b[:32].T)


# ------------------------------------------------- the comparator, on the CPU
@pytest.mark.parametrize("k", KS)
def test_inputs_equal_the_formula(lib, k):
    a, b = lib.mfma_inputs(k)
    ra, rb = ref.check_inputs(k)
    assert np.array_equal(a, ra) and np.array_equal(b, rb)


@pytest.mark.parametrize("k", KS)
def test_compare_accepts_the_numpy_product(lib, k):
    assert lib.mfma_compare(k, product(k)) == (0, [])


@pytest.mark.parametrize("k", (16, 64))
@pytest.mark.parametrize("at", [(0, 0), (31, 31), (4, 0), (13, 1), (8, 17)])
def test_compare_names_one_element_off_by_one(lib, k, at):
    for delta in (1.0, -1.0):
        c = product(k)
        c[at] += delta
        assert lib.mfma_compare(k, c) == (1, [32 * at[0] + at[1]])


def test_compare_counts_the_transposed_product_as_numpy_does(lib):
    for k in (16, 64):
        c = product(k)
        want = np.flatnonzero((c.T != c).reshape(-1))
        assert len(want) > 900  # B is not symmetric: nearly every element moves
        n, first = lib.mfma_compare(k, c.T, cap=1024)
        assert n == len(want) and first == want.tolist()
        n, first = lib.mfma_compare(k, c.T, cap=4)
        assert n == len(want) and first == want[:4].tolist()
        assert lib.mfma_compare(k, c.T, cap=0) == (len(want), [])


def test_compare_counts_a_non_integer_and_a_nan(lib):
    c = product(64)
    c[5, 7] += 0.5
    assert c[5, 7] != np.round(c[5, 7])
    assert lib.mfma_compare(64, c) == (1, [5 * 32 + 7])
    c = product(64)
    c[30, 2] = np.nan
    c[0, 1] = np.inf
    assert lib.mfma_compare(64, c) == (2, [1, 30 * 32 + 2])


def test_compare_and_inputs_refuse_a_k_that_is_no_multiple_of_16(lib):
    c = product(16)
    for k in (0, -16, 8, 24, 65, lib.mfma_max_k() + 16):
        with pytest.raises(hip_probe.ProbeError) as ei:
            lib.mfma_compare(k, c)
        assert ei.value.rc == -1000
        with pytest.raises(hip_probe.ProbeError) as ei:
            lib.mfma_inputs(k)
        assert ei.value.rc == -1000
    assert lib.mfma_max_k() >= 256 and lib.mfma_max_k() % 16 == 0
    # another K's product is not this K's
    assert lib.mfma_compare(32, product(16))[0] > 900


# --------------------------------------------------------- probe_kernels row
def test_probe_kernels_prints_the_probes_own_flop_count():
    active, iters = 2048, 8192
    flops = ref.peak_flops(active, iters)
    row = mfma_row({"tflops": 2400.04, "ms": 1.83251, "active_blocks": active, "iters": iters, "flops": float(flops)})
    assert row["flops_per_dispatch"] == active * 4 * 4 * iters * 32768
    assert row["mfma_insts_per_dispatch"] == active * 4 * 4 * iters
    assert row["TFLOPs"] == 2400.0 and row["ms"] == 1.833 and row["kernel"] == "k_mfma_peak"


# ------------------------------------------------------------ hip_health_fn
class FakeProbe:
    def __init__(self, health_ok=True, mfma_ok=True, mfma_bad_devs=()):
        self.health_ok, self.mfma_ok, self.mfma_bad_devs = health_ok, mfma_ok, set(mfma_bad_devs)
        self.calls = []

    def props(self, dev):
        return {"computeUnits": 256}

    def health(self, dev):
        self.calls.append("health")
        return {"healthy": self.health_ok}

    def mfma_check(self, dev):
        self.calls.append("mfma_check")
        return {"healthy": self.mfma_ok and dev not in self.mfma_bad_devs, "mismatches": 0 if self.mfma_ok else 3}

    def _sweep(self, name):
        self.calls.append(name)
        raise AssertionError(f"{name} ran after a failed basic check")

    def cu_sweep(self, dev, **kw):
        self._sweep("cu_sweep")

    def matrix_sweep(self, dev, **kw):
        self._sweep("matrix_sweep")

    def regfile_sweep(self, dev, **kw):
        self._sweep("regfile_sweep")

    def hbm_sweep(self, dev, **kw):
        self._sweep("hbm_sweep")


ALL_SWEEPS = {"sweep": True, "matrix": True, "regfile": True, "hbm": True}


def test_health_fn_withholds_on_a_failed_mfma_check_without_a_sweep(monkeypatch):
    f = FakeProbe(mfma_ok=False)
    monkeypatch.setattr(hip_probe, "probe", lambda: f)
    assert hip_health_fn(**ALL_SWEEPS)(0) is False
    assert f.calls == ["health", "mfma_check"]
    assert hip_health_fn()(0) is False


def test_health_fn_withholds_on_a_failed_checksum_without_a_sweep(monkeypatch):
    f = FakeProbe(health_ok=False)
    monkeypatch.setattr(hip_probe, "probe", lambda: f)
    assert hip_health_fn(**ALL_SWEEPS)(0) is False
    assert f.calls == ["health"]  # the MFMA check is not reached either
    assert hip_health_fn()(0) is False


def test_agent_withholds_the_gpu_whose_mfma_check_fails(monkeypatch, store):
    f = FakeProbe(mfma_bad_devs={1})
    monkeypatch.setattr(hip_probe, "probe", lambda: f)
    agent = NodeAgent(LocalClient(store), "n", host_fn=lambda: fake_host(2, "SPX"), publish_metrics=False,
                      health_fn=hip_health_fn())
    agent.sync()
    assert agent.unhealthy == {1}
