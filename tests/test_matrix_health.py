"""The matrix-format sweep off the GPU: its host-side verdict
(summarize_matrix_sweep), hip_health_fn merging it with the CU sweep, the node
agent publishing `matrixFaults` next to `xcdFaults`, the scheduler fencing
from such a node, and the node-agent flag."""
import json

import pytest

from flex_gpu_scheduler_amd.cli import build_parser, health_fn_args
from flex_gpu_scheduler_amd.control import LocalClient
from flex_gpu_scheduler_amd.control.node_agent import GpuHealth, NodeAgent, hip_health_fn
from flex_gpu_scheduler_amd.gpu.discovery import fake_host
from flex_gpu_scheduler_amd.models import GPU_XCD, TOPOLOGY_ANNOTATION
from flex_gpu_scheduler_amd.ops import hip_probe
from flex_gpu_scheduler_amd.ops.hip_probe import summarize_matrix_sweep, summarize_sweep
from helpers import FLEXGPU_PLUGINS, coscheduling_config, start

FORMATS = ["f16", "f32", "f64", "fp8", "bf8", "i8", "mxfp8", "mxbf8", "mxfp6", "mxbf6", "mxfp4"]


def bit(*names: str) -> int:
    return sum(1 << FORMATS.index(n) for n in names)


def records(xcds=8, cus=32, fail=None, skip=()):
    """One record per CU; `fail` maps (xcd, cu) to format bits."""
    return [{"xcd": x, "cu": c, "simd_mask": 15, "fail": (fail or {}).get((x, c), 0), "digests": {}}
            for x in range(xcds) for c in range(cus) if (x, c) not in skip]


# --------------------------------------------------- summarize_matrix_sweep
def test_summarize_clean():
    s = summarize_matrix_sweep(records(), 256, FORMATS)
    assert s["covered"] and s["bad_xcds"] == [] and s["failed_formats"] == []
    assert all(v["failed_formats"] == [] for v in s["xcds"].values())
    plain = summarize_sweep(records(), 256)
    assert {k: v for k, v in s.items() if k not in ("failed_formats", "xcds")} == \
        {k: v for k, v in plain.items() if k != "xcds"}


def test_summarize_names_formats_per_xcd_and_overall():
    recs = records(fail={(5, 17): bit("mxfp4"), (5, 3): bit("fp8", "mxfp4"), (2, 0): bit("f64")})
    s = summarize_matrix_sweep(recs, 256, FORMATS)
    assert s["bad_xcds"] == [2, 5]
    assert s["xcds"][5]["failed_formats"] == ["fp8", "mxfp4"] and s["xcds"][5]["failed_cus"] == [3, 17]
    assert s["xcds"][2]["failed_formats"] == ["f64"]
    assert s["xcds"][0]["failed_formats"] == []
    assert s["failed_formats"] == ["f64", "fp8", "mxfp4"]  # bit order
    assert s["covered"]


def test_summarize_uncovered_is_not_failed():
    s = summarize_matrix_sweep(records(skip={(6, 0), (6, 9)}), 256, FORMATS)
    assert not s["covered"] and s["uncovered"][6] == 2
    assert s["bad_xcds"] == [] and s["failed_formats"] == []


# ------------------------------------------------------------ hip_health_fn
class FakeProbe:
    def __init__(self, cus=256, cu_bad=(), matrix_fail=None, healthy=True):
        self.cus, self.cu_bad, self.matrix_fail, self.healthy = cus, cu_bad, matrix_fail or {}, healthy
        self.cu_calls, self.matrix_calls = 0, []

    def props(self, dev):
        return {"computeUnits": self.cus}

    def health(self, dev):
        return {"healthy": self.healthy}

    def mfma_check(self, dev):
        return {"healthy": True}

    def _xcds(self):
        return self.cus // 32

    def cu_sweep(self, dev, **kw):
        self.cu_calls += 1
        recs = records(self._xcds(), fail={(x, 0): 1 for x in self.cu_bad})
        s = summarize_sweep(recs, self.cus)
        s.update(rounds=1, ms=2.0, blocks=4 * self.cus)
        return {"records": recs, "summary": s}

    def matrix_sweep(self, dev, formats=None, **kw):
        self.matrix_calls.append((formats, kw))
        recs = records(self._xcds(), fail={(x, 1): bit(*f) for x, f in self.matrix_fail.items()})
        s = summarize_matrix_sweep(recs, self.cus, FORMATS)
        s.update(rounds=1, ms=0.1, blocks=4 * self.cus, formats=formats or FORMATS)
        return {"records": recs, "summary": s}


@pytest.fixture
def fake(monkeypatch):
    def install(**kw):
        f = FakeProbe(**kw)
        monkeypatch.setattr(hip_probe, "probe", lambda: f)
        return f
    return install


def test_health_fn_default_runs_no_sweep(fake):
    f = fake()
    assert hip_health_fn()(0) is True
    assert f.cu_calls == 0 and f.matrix_calls == []


def test_health_fn_unites_the_bad_xcds_of_both_sweeps(fake):
    f = fake(cu_bad=(1,), matrix_fail={6: ["mxfp4", "fp8"], 1: ["f64"]})
    v = hip_health_fn(sweep=True, matrix=True)(0)
    assert isinstance(v, GpuHealth) and not v.ok and not v
    assert v.bad_xcds == frozenset({1, 6})
    assert v.detail["matrixFaults"] == {1: ["f64"], 6: ["fp8", "mxfp4"]}
    assert "sweep" in v.detail and "matrixSweep" in v.detail
    assert f.cu_calls == 1 and len(f.matrix_calls) == 1


def test_health_fn_matrix_alone_and_its_arguments(fake):
    f = fake(matrix_fail={3: ["i8"]})
    v = hip_health_fn(matrix=True, matrix_formats=["i8", "f16"], matrix_args={"blocks": 64})(0)
    assert v.bad_xcds == frozenset({3}) and v.detail["matrixFaults"] == {3: ["i8"]}
    assert f.cu_calls == 0 and f.matrix_calls == [(["i8", "f16"], {"blocks": 64})]
    ok = fake()
    v = hip_health_fn(matrix=True)(0)
    assert isinstance(v, GpuHealth) and v.ok and v and v.detail["matrixFaults"] == {}
    assert ok.matrix_calls == [(None, {})]


def test_health_fn_reuses_the_verdict_for_the_period(fake):
    f = fake(matrix_fail={2: ["bf8"]})
    fn = hip_health_fn(sweep=True, matrix=True, sweep_period_s=3600.0)
    first = fn(0)
    assert fn(0) is first and fn(0) is first
    assert f.cu_calls == 1 and len(f.matrix_calls) == 1
    fn(1)  # another device has its own verdict
    assert f.cu_calls == 2 and len(f.matrix_calls) == 2
    g = fake(matrix_fail={2: ["bf8"]})
    fn = hip_health_fn(matrix=True, sweep_period_s=0.0)
    fn(0), fn(0)
    assert len(g.matrix_calls) == 2


def test_health_fn_on_a_partition_device_returns_a_bool(fake):
    fake(cus=64, matrix_fail={1: ["mxfp6"]})
    assert hip_health_fn(matrix=True)(0) is False
    fake(cus=64)
    assert hip_health_fn(matrix=True)(0) is True


def test_health_fn_skips_the_sweeps_when_the_basic_check_fails(fake):
    f = fake(healthy=False)
    assert hip_health_fn(sweep=True, matrix=True)(0) is False
    assert f.cu_calls == 0 and f.matrix_calls == []


# --------------------------------------------------------------- node agent
def agent_on(store, host, health_fn):
    agent = NodeAgent(LocalClient(store), "n", host_fn=lambda: host, publish_metrics=False, health_fn=health_fn)
    agent.sync()
    return agent


def topo_of(store) -> dict:
    return json.loads(store.get("nodes", "", "n")["metadata"]["annotations"][TOPOLOGY_ANNOTATION])


def test_agent_publishes_matrix_faults_next_to_xcd_faults(store):
    def health(dev):
        return GpuHealth(False, {5}, {"matrixFaults": {5: ["fp8", "mxfp4"]}}) if dev == 0 else True

    agent = agent_on(store, fake_host(2, "CPX"), health)
    topo = topo_of(store)
    assert topo["xcdFaults"] == {"0": [5]}
    assert topo["matrixFaults"] == {"0": {"5": ["fp8", "mxfp4"]}}
    assert agent.faults["matrixFaults"] == {0: {5: ["fp8", "mxfp4"]}} and agent.unhealthy_xcds == {0: {5}}
    assert store.get("nodes", "", "n")["status"]["allocatable"][GPU_XCD] == "15"


def test_agent_omits_the_key_when_there_is_none(store):
    agent = agent_on(store, fake_host(2, "CPX"), lambda dev: GpuHealth(False, {1}) if dev == 0 else True)
    assert "matrixFaults" not in topo_of(store) and topo_of(store)["xcdFaults"] == {"0": [1]}
    assert agent.faults["matrixFaults"] == {}
    agent = agent_on(store, fake_host(2, "CPX"), lambda dev: GpuHealth(True, (), {"matrixFaults": {}}))
    assert "matrixFaults" not in topo_of(store) and "xcdFaults" not in topo_of(store)
    plain = NodeAgent(LocalClient(store), "n", host_fn=lambda: fake_host(2, "CPX"), publish_metrics=False)
    want = plain.build_node(fake_host(2, "CPX"))["metadata"]["annotations"][TOPOLOGY_ANNOTATION]
    assert store.get("nodes", "", "n")["metadata"]["annotations"][TOPOLOGY_ANNOTATION] == want


def test_agent_resyncs_when_only_the_formats_change(store):
    verdict = {"v": GpuHealth(False, {5}, {"matrixFaults": {5: ["fp8"]}})}
    agent = agent_on(store, fake_host(1, "CPX"), lambda dev: verdict["v"])
    assert topo_of(store)["matrixFaults"] == {"0": {"5": ["fp8"]}}
    verdict["v"] = GpuHealth(False, {5}, {"matrixFaults": {5: ["fp8", "mxbf6"]}})
    agent._heartbeat_and_resync()
    assert topo_of(store)["matrixFaults"] == {"0": {"5": ["fp8", "mxbf6"]}}
    assert topo_of(store)["xcdFaults"] == {"0": [5]}


# ---------------------------------------------------------------- scheduler
def test_scheduler_fences_from_a_node_that_carries_matrix_faults(store):
    agent_on(store, fake_host(1, "CPX"), lambda dev: GpuHealth(False, {5}, {"matrixFaults": {5: ["mxfp4"]}}))
    assert "matrixFaults" in topo_of(store)
    s = start(store, coscheduling_config(FLEXGPU_PLUGINS))
    try:
        g = s.node_info("n")["gpu"]
        assert g["fenced"] == [[p == 5 for p in range(8)]] and g["free_xcds"] == 7
    finally:
        s.stop()


# ---------------------------------------------------------------------- CLI
def test_cli_parses_the_matrix_sweep_flag():
    ap = build_parser()
    none = ap.parse_args(["node-agent"])
    assert none.health_matrix_sweep is None and health_fn_args(none)["matrix"] is False
    bare = ap.parse_args(["node-agent", "--health-matrix-sweep"])
    assert health_fn_args(bare) == {"sweep": False, "sweep_period_s": 600.0, "matrix": True, "matrix_formats": None}
    some = ap.parse_args(["node-agent", "--health-matrix-sweep", "mxfp4,fp8", "--health-sweep",
                          "--health-sweep-period", "30"])
    assert health_fn_args(some) == {"sweep": True, "sweep_period_s": 30.0, "matrix": True,
                                    "matrix_formats": ["mxfp4", "fp8"]}
