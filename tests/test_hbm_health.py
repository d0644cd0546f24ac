"""The HBM sweep off the GPU: the pattern's properties, the host-side verdict
(summarize_hbm_sweep), hip_health_fn running the sweep under the sweeps' period,
the node agent withholding a GPU with an HBM fault as a whole and publishing
`hbmFaults`, and the node-agent flag."""
import json

import numpy as np
import pytest

from flex_gpu_scheduler_amd.cli import build_parser, health_fn_args
from flex_gpu_scheduler_amd.control import LocalClient
from flex_gpu_scheduler_amd.control.node_agent import GpuHealth, NodeAgent, hip_health_fn
from flex_gpu_scheduler_amd.gpu.discovery import fake_host
from flex_gpu_scheduler_amd.models import GPU, GPU_MEMORY, GPU_XCD, TOPOLOGY_ANNOTATION
from flex_gpu_scheduler_amd.ops import hip_probe
from flex_gpu_scheduler_amd.ops.hip_probe import HBM_UNSWEPT, ProbeError, summarize_hbm_sweep, summarize_sweep
from hbm_sweep_ref import SEED, pattern, pattern_of

GIB = 1 << 30


# ------------------------------------------------------------------ pattern
def test_every_bit_takes_both_values_in_every_4k_window():
    rng = np.random.default_rng(1)
    starts = np.concatenate([[0, 2 ** 32 - 256, 2 ** 32], rng.integers(0, 2 ** 35, 261) & ~np.int64(255)])
    for first in starts.tolist():
        w = pattern_of(np.uint64(first) + np.arange(256, dtype=np.uint64))  # 256 vectors = 4 KiB
        assert (np.bitwise_or.reduce(w, axis=0) == 0xFFFFFFFF).all(), first
        assert (np.bitwise_and.reduce(w, axis=0) == 0).all(), first


def test_one_flipped_index_bit_changes_all_four_words():
    v = np.random.default_rng(2).integers(0, 2 ** 35, 2000).astype(np.uint64)
    base = pattern_of(v)
    for bit in range(35):
        assert (pattern_of(v ^ np.uint64(1 << bit)) != base).all(), bit
    assert (pattern_of(v, inverted=True) == ~base).all()
    assert (pattern_of(v, seed=SEED ^ 1) != base).all()


@pytest.fixture(scope="module")
def lib():
    try:
        return hip_probe.HipProbe()
    except (ProbeError, OSError) as e:
        pytest.skip(f"_hipprobe.so does not load here: {e}")


@pytest.mark.parametrize("inverted", [False, True])
@pytest.mark.parametrize("first", [0, 2 ** 32 - 5, 2 ** 35 + 7])
def test_host_pattern_equals_the_formula(lib, first, inverted):
    got = lib.hbm_sweep_pattern(first, 64, inverted=inverted)
    assert got.dtype == np.uint32 and got.shape == (64, 4)
    assert np.array_equal(got, pattern(first, 64, inverted=inverted))
    assert np.array_equal(lib.hbm_sweep_pattern(first, 3, seed=99), pattern(first, 3, seed=99))


# ------------------------------------------------------ summarize_hbm_sweep
def raw(tested=4 * GIB, short=False, log=(), bad=None, bits=None, down=0, up=0, flip_or=(0, 0, 0, 0), xcd_mask=0,
        bad_chunks=None, ms=(1.0, 2.0, 1.0)):
    bad = len(log) if bad is None else bad
    return {"bytes_tested": tested, "short": short, "vectors_read": 2 * (tested // 16), "fold": [0, 0],
            "bad_vectors": bad, "bad_bits": down + up if bits is None else bits, "one_to_zero": down,
            "zero_to_one": up, "flip_or": list(flip_or), "reader_xcd_mask": xcd_mask,
            "bad_chunks": dict(bad_chunks or {}), "log": list(log), "ms": list(ms)}


def entry(v, word, mask, pass_=1, xcd=0, expected=(0x0F0F0F0F, 0x0F0F0F0F, 0x0F0F0F0F, 0x0F0F0F0F)):
    actual = list(expected)
    actual[word] ^= mask
    return {"v": v, "expected": list(expected), "actual": actual, "xcd": xcd, "pass": pass_}


def test_summarize_clean():
    s = summarize_hbm_sweep(raw())
    assert s["healthy"] and s["bad_vectors"] == 0 and s["faults"] == [] and s["bad_chunks"] == {}
    assert s["bytes_tested"] == 4 * GIB and not s["short"] and s["from_dram"]
    assert s["vectors_read"] == 2 * (4 * GIB // 16)
    assert s["flip_mask"] == "0" * 32 and s["reader_xcds"] == []
    # bytes moved over time; pass 1 reads and writes
    gbps = 4 * GIB / 1e-3 / 1e9
    assert s["ms"] == [1.0, 2.0, 1.0] and s["GBps"] == [round(gbps, 1), round(gbps, 1), round(gbps, 1)]
    assert summarize_hbm_sweep(raw(ms=(1.0, 1.0, 1.0)))["GBps"][1] == round(2 * gbps, 1)


def test_summarize_from_dram_starts_at_one_gib():
    assert summarize_hbm_sweep(raw(tested=GIB))["from_dram"] is True
    assert summarize_hbm_sweep(raw(tested=GIB - 16))["from_dram"] is False


def test_summarize_faults_are_sorted_and_decoded():
    log = [entry(900, 3, 0x80000001, pass_=2, xcd=5), entry(7, 0, 0x10, pass_=1, xcd=2)]
    s = summarize_hbm_sweep(raw(log=log, down=2, up=1, flip_or=(0x10, 0, 0, 0x80000001), xcd_mask=0b100100,
                                bad_chunks={3: 1, 0: 1}))
    assert not s["healthy"] and s["bad_vectors"] == 2 and s["bad_bits"] == 3
    assert (s["one_to_zero"], s["zero_to_one"]) == (2, 1)
    assert [f["v"] for f in s["faults"]] == [7, 900]
    a, b = s["faults"]
    assert a["offset"] == 7 * 16 and a["pass"] == 1 and a["xcd"] == 2
    assert a["bits"] == [4] and a["zero_to_one"] == [4] and a["one_to_zero"] == []  # 0x0F..: bit 4 was 0
    assert b["offset"] == 900 * 16 and b["bits"] == [96, 127]
    assert b["one_to_zero"] == [96] and b["zero_to_one"] == [127]
    assert int(s["flip_mask"], 16) == 0x10 | 0x80000001 << 96 and len(s["flip_mask"]) == 32
    assert s["reader_xcds"] == [2, 5]
    assert s["bad_chunks"] == {0: 1, 3: 1} and list(s["bad_chunks"]) == [0, 3]
    assert s["unlogged"] == 0


def test_summarize_short_is_not_a_fault():
    s = summarize_hbm_sweep(raw(tested=GIB // 2, short=True))
    assert s["short"] and s["healthy"] and not s["from_dram"] and s["bytes_tested"] == GIB // 2


def test_summarize_over_the_log_cap():
    log = [entry(10 * i, i % 4, 1 << i) for i in range(32)]
    s = summarize_hbm_sweep(raw(log=log, bad=40, bits=40, up=40, bad_chunks={0: 40}))
    assert not s["healthy"] and s["bad_vectors"] == 40 and len(s["faults"]) == 32 and s["unlogged"] == 8
    assert s["bad_chunks"] == {0: 40}


# ------------------------------------------------------------ hip_health_fn
def cu_records(xcds, fail=None):
    return [{"xcd": x, "cu": c, "simd_mask": 15, "fail": (fail or {}).get((x, c), 0)}
            for x in range(xcds) for c in range(32)]


class FakeProbe:
    """`hbm`: what hbm_sweep gives: a raw dict, or an exception to raise."""

    def __init__(self, cus=256, cu_bad=(), hbm=None):
        self.cus, self.cu_bad, self.hbm = cus, cu_bad, hbm if hbm is not None else raw()
        self.cu_calls, self.hbm_calls = 0, []

    def props(self, dev):
        return {"computeUnits": self.cus}

    def health(self, dev):
        return {"healthy": True}

    def mfma_check(self, dev):
        return {"healthy": True}

    def cu_sweep(self, dev, **kw):
        self.cu_calls += 1
        recs = cu_records(self.cus // 32, fail={(x, 0): 1 for x in self.cu_bad})
        s = summarize_sweep(recs, self.cus)
        s.update(rounds=1, ms=2.0, blocks=4 * self.cus)
        return {"records": recs, "summary": s}

    def hbm_sweep(self, dev, nbytes=0, **kw):
        self.hbm_calls.append((dev, nbytes, kw))
        if isinstance(self.hbm, Exception):
            raise self.hbm
        return {"raw": self.hbm, "summary": summarize_hbm_sweep(self.hbm)}


class NoHbmProbe(FakeProbe):
    hbm_sweep = None  # as the fake probes of the other sweeps' tests: calling it is an error


@pytest.fixture
def fake(monkeypatch):
    def install(cls=FakeProbe, **kw):
        f = cls(**kw)
        monkeypatch.setattr(hip_probe, "probe", lambda: f)
        return f
    return install


FAULT = raw(log=[entry(5, 1, 0x10, xcd=3)], up=1, flip_or=(0, 0x10, 0, 0), xcd_mask=1 << 3, bad_chunks={0: 1})


def test_health_fn_calls_the_sweep_only_when_asked(fake):
    fake(cls=NoHbmProbe)
    assert hip_health_fn()(0) is True
    v = hip_health_fn(sweep=True)(0)
    assert isinstance(v, GpuHealth) and v and "hbmSweep" not in v.detail and "hbmFaults" not in v.detail
    f = fake()
    v = hip_health_fn(hbm=True)(0)  # with neither of the other sweeps
    assert isinstance(v, GpuHealth) and v.ok and v
    assert v.detail["hbmFaults"] == {} and v.detail["hbmSweep"]["healthy"]
    assert f.hbm_calls == [(0, 0, {})] and f.cu_calls == 0
    f = fake()
    hip_health_fn(hbm=True, hbm_gib=64, hbm_args={"chunk_bytes": 1 << 28})(2)
    assert f.hbm_calls == [(2, 64 * GIB, {"chunk_bytes": 1 << 28})]
    f = fake()
    hip_health_fn(hbm=True, hbm_gib=0.5)(0)
    assert f.hbm_calls == [(0, GIB // 2, {})]


def test_health_fn_reuses_the_hbm_verdict_for_the_period(fake):
    f = fake(hbm=FAULT)
    fn = hip_health_fn(hbm=True, sweep=True, sweep_period_s=3600.0)
    first = fn(0)
    assert fn(0) is first and fn(0) is first
    assert len(f.hbm_calls) == 1 and f.cu_calls == 1
    fn(1)
    assert len(f.hbm_calls) == 2
    g = fake()
    fn = hip_health_fn(hbm=True, sweep_period_s=0.0)
    fn(0), fn(0)
    assert len(g.hbm_calls) == 2


def test_health_fn_fault_on_every_kind_of_device(fake):
    for cus in (256, 32):
        fake(cus=cus, hbm=FAULT)
        v = hip_health_fn(hbm=True)(0)
        assert isinstance(v, GpuHealth) and not v.ok and not v and v.bad_xcds == frozenset()
        assert v.detail["hbmFaults"] == {"badVectors": 1, "badBits": 1, "flipMask": f"{0x10 << 32:032x}",
                                         "oneToZero": 0, "zeroToOne": 1, "testedGiB": 4.0, "fromDram": True,
                                         "readerXcds": [3]}
        assert v.detail["hbmSweep"]["faults"][0]["v"] == 5
    fake(cus=32)  # clean on a partition device: the plain bool of the other sweeps
    assert hip_health_fn(hbm=True)(0) is True


def test_health_fn_keeps_the_bad_xcds_next_to_the_hbm_fault(fake):
    fake(cu_bad=(6,), hbm=FAULT)
    v = hip_health_fn(sweep=True, hbm=True)(0)
    assert isinstance(v, GpuHealth) and not v.ok
    assert v.bad_xcds == frozenset({6}) and v.detail["hbmFaults"]["badVectors"] == 1
    assert "sweep" in v.detail and "hbmSweep" in v.detail


def test_health_fn_unswept_and_short_do_not_fail_the_device(fake, caplog):
    e = ProbeError("hbm_sweep failed (-1003): unswept")
    e.rc = HBM_UNSWEPT
    fake(hbm=e)
    with caplog.at_level("WARNING"):
        v = hip_health_fn(hbm=True)(0)
    assert v and (v.ok if isinstance(v, GpuHealth) else v is True)
    assert "hbmFaults" not in v.detail and "unswept" in caplog.text
    caplog.clear()
    fake(hbm=raw(tested=GIB // 2, short=True))
    with caplog.at_level("WARNING"):
        v = hip_health_fn(hbm=True)(0)
    assert v and v.detail["hbmSweep"]["short"] and "short" in caplog.text
    other = ProbeError("hbm_sweep failed (-2): out of memory")  # any other error is the probe's failure
    other.rc = -2
    fake(hbm=other)
    with pytest.raises(ProbeError):
        hip_health_fn(hbm=True)(0)


# --------------------------------------------------------------- node agent
HBM_FAULTS = {"badVectors": 1, "badBits": 1, "flipMask": f"{0x10 << 32:032x}", "oneToZero": 0, "zeroToOne": 1,
              "testedGiB": 4.0, "fromDram": True, "readerXcds": [3]}


def agent_on(store, host, health_fn):
    agent = NodeAgent(LocalClient(store), "n", host_fn=lambda: host, publish_metrics=False, health_fn=health_fn)
    agent.sync()
    return agent


def topo_of(store) -> dict:
    return json.loads(store.get("nodes", "", "n")["metadata"]["annotations"][TOPOLOGY_ANNOTATION])


def alloc_of(store) -> dict:
    return store.get("nodes", "", "n")["status"]["allocatable"]


def test_agent_withholds_the_whole_gpu_of_an_hbm_fault(store):
    host = fake_host(2, "CPX")
    clean = agent_on(store, host, lambda dev: True)
    full = dict(alloc_of(store))
    assert clean.faults["hbmFaults"] == {} and "hbmFaults" not in topo_of(store)

    def health(dev):  # bad XCDs in the same verdict: still the whole GPU, not a partition
        return GpuHealth(False, {5}, {"hbmFaults": HBM_FAULTS}) if dev == 0 else True

    agent = agent_on(store, host, health)
    assert agent.unhealthy == {0} and agent.faults["hbmFaults"] == {0: HBM_FAULTS} and agent.unhealthy_xcds == {0: {5}}
    alloc = alloc_of(store)
    assert int(alloc[GPU_XCD]) == int(full[GPU_XCD]) - 8
    assert int(alloc[GPU_MEMORY]) == int(full[GPU_MEMORY]) - host.gpus[0].hbm_gib
    assert int(alloc[GPU]) == int(full[GPU]) - (1 if int(full[GPU]) else 0)
    topo = topo_of(store)
    assert topo["unhealthy"] == [0] and topo["hbmFaults"] == {"0": HBM_FAULTS}
    assert [g["index"] for g in topo["gpus"]] == [1]
    # the public shapes stay
    assert agent.probe_health(host) == ({0}, {0: {5}}) and agent.check_health(host) == {0}
    # an XCD fault alone still fences one partition of a CPX GPU
    agent = agent_on(store, host, lambda dev: GpuHealth(False, {5}) if dev == 0 else True)
    assert agent.unhealthy == set() and int(alloc_of(store)[GPU_XCD]) == int(full[GPU_XCD]) - 1


def test_agent_withholds_without_bad_xcds_and_on_spx(store):
    for mode in ("CPX", "SPX"):
        agent = agent_on(store, fake_host(2, mode), lambda dev: GpuHealth(False, (), {"hbmFaults": HBM_FAULTS})
                         if dev == 1 else True)
        assert agent.unhealthy == {1} and topo_of(store)["hbmFaults"] == {"1": HBM_FAULTS}


def test_agent_drops_the_key_when_the_fault_clears_and_resyncs_on_change(store):
    verdict = {"v": GpuHealth(False, (), {"hbmFaults": HBM_FAULTS})}
    agent = agent_on(store, fake_host(1, "CPX"), lambda dev: verdict["v"])
    assert topo_of(store)["hbmFaults"] == {"0": HBM_FAULTS}
    # only the counts change: the set of withheld GPUs is the same, the annotation follows
    worse = dict(HBM_FAULTS, badVectors=9, badBits=12)
    verdict["v"] = GpuHealth(False, (), {"hbmFaults": worse})
    agent._heartbeat_and_resync()
    assert topo_of(store)["hbmFaults"] == {"0": worse} and agent.faults["hbmFaults"] == {0: worse}
    verdict["v"] = GpuHealth(True, (), {"hbmFaults": {}})
    agent._heartbeat_and_resync()
    topo = topo_of(store)
    assert "hbmFaults" not in topo and topo["unhealthy"] == [] and agent.faults["hbmFaults"] == {}
    plain = NodeAgent(LocalClient(store), "n", host_fn=lambda: fake_host(1, "CPX"), publish_metrics=False)
    want = plain.build_node(fake_host(1, "CPX"))["metadata"]["annotations"][TOPOLOGY_ANNOTATION]
    assert store.get("nodes", "", "n")["metadata"]["annotations"][TOPOLOGY_ANNOTATION] == want


# ---------------------------------------------------------------------- CLI
def test_cli_parses_the_hbm_sweep_flag():
    ap = build_parser()
    none = ap.parse_args(["node-agent"])
    assert none.health_hbm_sweep is None
    assert health_fn_args(none) == {"sweep": False, "sweep_period_s": 600.0, "matrix": False,
                                    "matrix_formats": None}  # exactly the keys from before the flag
    bare = ap.parse_args(["node-agent", "--health-hbm-sweep"])
    assert health_fn_args(bare) == {"sweep": False, "sweep_period_s": 600.0, "matrix": False,
                                    "matrix_formats": None, "hbm": True, "hbm_gib": None}
    some = ap.parse_args(["node-agent", "--health-hbm-sweep", "64", "--health-sweep", "--health-sweep-period", "30"])
    assert health_fn_args(some) == {"sweep": True, "sweep_period_s": 30.0, "matrix": False, "matrix_formats": None,
                                    "hbm": True, "hbm_gib": 64.0}
    for bad in ("0", "-4", "lots"):
        with pytest.raises(SystemExit):
            ap.parse_args(["node-agent", "--health-hbm-sweep", bad])
