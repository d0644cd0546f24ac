"""The lane sweep off the GPU: its host-side verdict (summarize_lane_sweep),
hip_health_fn merging it with the other sweeps, the node agent publishing
`laneFaults` next to `xcdFaults`, the scheduler fencing from such a node, and
the node-agent flag."""
import json

import pytest

import lane_sweep_ref as ref
from flex_gpu_scheduler_amd.cli import build_parser, health_fn_args
from flex_gpu_scheduler_amd.control import LocalClient
from flex_gpu_scheduler_amd.control.node_agent import GpuHealth, NodeAgent, hip_health_fn
from flex_gpu_scheduler_amd.gpu.discovery import fake_host
from flex_gpu_scheduler_amd.models import GPU, GPU_XCD, TOPOLOGY_ANNOTATION, make_pod
from flex_gpu_scheduler_amd.ops import hip_probe
from flex_gpu_scheduler_amd.ops.hip_probe import summarize_lane_sweep, summarize_regfile_sweep, summarize_sweep
from helpers import FLEXGPU_PLUGINS, annotations, coscheduling_config, create_all, start, wait_bound

PATHS = ref.PATHS


def bits(*names):
    return sum(1 << PATHS.index(n) for n in names)


def records(xcds=8, cus=32, fail=None, skip=()):
    """One record per CU; `fail` maps (xcd, cu) to the paths that failed there."""
    out = []
    for x in range(xcds):
        for c in range(cus):
            if (x, c) in skip:
                continue
            names = (fail or {}).get((x, c), ())
            out.append({"xcd": x, "cu": c, "simd_mask": 15, "fail": bits(*names),
                        "bad": {f: int(f in names) for f in PATHS}, "digests": {f: 0 for f in PATHS},
                        "bad_simds": 1 if names else 0})
    return out


# ---------------------------------------------------------- the host library
@pytest.fixture(scope="module")
def lib():
    try:
        return hip_probe.HipProbe()
    except (hip_probe.ProbeError, OSError) as e:
        pytest.skip(f"_hipprobe.so does not load here: {e}")


def test_host_names_and_shapes(lib):
    assert lib.lane_paths() == PATHS
    assert {f: tuple(lib.lane_shape(f).values()) for f in PATHS} == ref.SHAPES
    with pytest.raises(ValueError):
        lib._lane_mask(["dpp", "shfl"])
    assert lib._lane_mask(None) == 0xFF and lib._lane_mask("ldstr") == 1 << 5


@pytest.mark.parametrize("seed", ref.SEEDS + (0,))
def test_host_digests_equal_the_reference(lib, seed):
    assert lib.lane_sweep_expected(seed=seed) == {f: ref.digest(f, seed) for f in PATHS}
    assert lib.lane_sweep_expected(["ldsdma", "dpp"], seed) == {f: ref.digest(f, seed) for f in ("dpp", "ldsdma")}


# ------------------------------------------------------ summarize_lane_sweep
def test_summarize_clean():
    s = summarize_lane_sweep(records(), 256, PATHS)
    assert s["covered"] and s["bad_xcds"] == [] and s["failed_paths"] == []
    assert all(v["failed_paths"] == [] and v["failed_cus"] == [] for v in s["xcds"].values())
    plain = summarize_sweep(records(), 256)
    assert {k: v for k, v in s.items() if k not in ("failed_paths", "xcds")} == {k: v for k, v in plain.items()
                                                                                  if k != "xcds"}


def test_summarize_names_paths_per_xcd():
    s = summarize_lane_sweep(records(fail={(5, 17): ["ldstr"], (5, 3): ["dpp", "ldsdma"], (2, 0): ["permlane"]}),
                             256, PATHS)
    assert s["bad_xcds"] == [2, 5] and s["covered"]
    assert s["xcds"][5]["failed_cus"] == [3, 17] and s["xcds"][5]["failed_paths"] == ["dpp", "ldstr", "ldsdma"]
    assert s["xcds"][2]["failed_paths"] == ["permlane"] and s["xcds"][0]["failed_paths"] == []
    assert s["failed_paths"] == ["dpp", "permlane", "ldstr", "ldsdma"]


def test_summarize_uncovered_is_not_failed():
    s = summarize_lane_sweep(records(skip={(6, 0), (6, 9)}), 256, PATHS)
    assert not s["covered"] and s["uncovered"][6] == 2
    assert s["bad_xcds"] == [] and s["failed_paths"] == []


# ------------------------------------------------------------ hip_health_fn
class FakeProbe:
    def __init__(self, cus=256, cu_bad=(), regfile_fail=None, lane_fail=None, lane_skip=(), healthy=True):
        self.cus, self.cu_bad, self.healthy = cus, cu_bad, healthy
        self.regfile_fail, self.lane_fail, self.lane_skip = regfile_fail or {}, lane_fail or {}, lane_skip
        self.cu_calls, self.regfile_calls, self.lane_calls = 0, 0, []

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
        recs = [{"xcd": x, "cu": c, "fail": int(c == 0 and x in self.cu_bad)}
                for x in range(self._xcds()) for c in range(32)]
        s = summarize_sweep(recs, self.cus)
        s.update(rounds=1, ms=2.0, blocks=4 * self.cus)
        return {"records": recs, "summary": s}

    def regfile_sweep(self, dev, **kw):
        self.regfile_calls += 1
        recs = [{"xcd": x, "cu": c, "simd_mask": 15, "fail": int(c == 2 and x in self.regfile_fail), "bad_vgpr": 64,
                 "bad_agpr": 0, "first": 3, "flip": 1, "digest": 0, "bad_simds": 1}
                for x in range(self._xcds()) for c in range(32)]
        s = summarize_regfile_sweep(recs, self.cus)
        s.update(rounds=1, ms=0.3, blocks=4 * self.cus, seed=0)
        return {"records": recs, "summary": s}

    def lane_sweep(self, dev, paths=None, **kw):
        self.lane_calls.append({"paths": paths, **kw})
        recs = records(self._xcds(), fail={(x, 4): f for x, f in self.lane_fail.items()}, skip=self.lane_skip)
        s = summarize_lane_sweep(recs, self.cus, PATHS)
        s.update(rounds=1, ms=0.5, blocks=4 * self.cus, seed=0, paths=paths or PATHS)
        return {"records": recs, "summary": s}


@pytest.fixture
def fake(monkeypatch):
    def install(**kw):
        f = FakeProbe(**kw)
        monkeypatch.setattr(hip_probe, "probe", lambda: f)
        return f
    return install


def test_health_fn_default_runs_no_lane_sweep(fake):
    f = fake()
    assert hip_health_fn()(0) is True
    assert hip_health_fn(sweep=True, regfile=True)(0)
    assert f.lane_calls == []


def test_health_fn_unites_the_bad_xcds_of_the_sweeps(fake):
    f = fake(cu_bad=(1,), regfile_fail={6: 1}, lane_fail={3: ["ldstr"], 6: ["dpp", "permlane"]})
    v = hip_health_fn(sweep=True, regfile=True, lane=True)(0)
    assert isinstance(v, GpuHealth) and not v.ok and not v
    assert v.bad_xcds == frozenset({1, 3, 6})
    assert v.detail["laneFaults"] == {3: ["ldstr"], 6: ["dpp", "permlane"]}
    assert v.detail["laneSweep"]["bad_xcds"] == [3, 6] and sorted(v.detail["registerFaults"]) == [6]
    assert f.cu_calls == 1 and f.regfile_calls == 1 and len(f.lane_calls) == 1


def test_health_fn_lane_sweep_alone_and_its_arguments(fake):
    f = fake(lane_fail={3: ["ldsdma"]})
    v = hip_health_fn(lane=True, lane_paths=["ldsdma", "ldstr"], lane_args={"blocks": 64, "seed": 5})(0)
    assert v.bad_xcds == frozenset({3}) and v.detail["laneFaults"] == {3: ["ldsdma"]}
    assert f.cu_calls == 0 and f.regfile_calls == 0
    assert f.lane_calls == [{"paths": ["ldsdma", "ldstr"], "blocks": 64, "seed": 5}]
    ok = fake()
    v = hip_health_fn(lane=True)(0)
    assert isinstance(v, GpuHealth) and v.ok and v and v.detail["laneFaults"] == {}
    assert ok.lane_calls == [{"paths": None}]


def test_health_fn_uncovered_cus_do_not_fail_the_device(fake):
    fake(lane_skip={(4, 7)})
    v = hip_health_fn(lane=True)(0)
    assert isinstance(v, GpuHealth) and v.ok and v
    assert not v.detail["laneSweep"]["covered"] and v.detail["laneFaults"] == {}


def test_health_fn_reuses_the_verdict_for_the_period(fake):
    f = fake(lane_fail={2: ["bpermute"]})
    fn = hip_health_fn(sweep=True, lane=True, sweep_period_s=3600.0)
    first = fn(0)
    assert fn(0) is first and fn(0) is first
    assert f.cu_calls == 1 and len(f.lane_calls) == 1
    fn(1)  # another device has its own verdict
    assert f.cu_calls == 2 and len(f.lane_calls) == 2
    g = fake(lane_fail={2: ["bpermute"]})
    fn = hip_health_fn(lane=True, sweep_period_s=0.0)
    fn(0), fn(0)
    assert len(g.lane_calls) == 2


def test_health_fn_on_a_partition_device_returns_a_bool(fake):
    fake(cus=64, lane_fail={1: ["readlane"]})
    assert hip_health_fn(lane=True)(0) is False
    fake(cus=64)
    assert hip_health_fn(lane=True)(0) is True


def test_health_fn_skips_the_sweep_when_the_basic_check_fails(fake):
    f = fake(healthy=False)
    assert hip_health_fn(lane=True)(0) is False
    assert f.lane_calls == []


# --------------------------------------------------------------- node agent
def agent_on(store, host, health_fn):
    agent = NodeAgent(LocalClient(store), "n", host_fn=lambda: host, publish_metrics=False, health_fn=health_fn)
    agent.sync()
    return agent


def topo_of(store) -> dict:
    return json.loads(store.get("nodes", "", "n")["metadata"]["annotations"][TOPOLOGY_ANNOTATION])


def test_agent_publishes_lane_faults_and_fences_the_partition(store):
    def health(dev):
        return GpuHealth(False, {5}, {"laneFaults": {5: ["ldstr", "ldsdma"]}, "matrixFaults": {5: ["fp8"]}}) \
            if dev == 0 else True

    agent = agent_on(store, fake_host(2, "CPX"), health)
    topo = topo_of(store)
    assert topo["xcdFaults"] == {"0": [5]} and topo["unhealthy"] == []
    assert topo["laneFaults"] == {"0": {"5": ["ldstr", "ldsdma"]}}
    assert topo["matrixFaults"] == {"0": {"5": ["fp8"]}}
    assert agent.faults["laneFaults"] == {0: {5: ["ldstr", "ldsdma"]}} and agent.unhealthy_xcds == {0: {5}}
    alloc = store.get("nodes", "", "n")["status"]["allocatable"]
    assert alloc[GPU_XCD] == "15"  # only the partition that owns XCD 5 is fenced


def test_agent_fences_both_xcds_of_a_dpx_partition(store):
    agent_on(store, fake_host(1, "DPX"), lambda dev: GpuHealth(False, {6}, {"laneFaults": {6: ["dpp"]}}))
    assert topo_of(store)["laneFaults"] == {"0": {"6": ["dpp"]}}
    assert store.get("nodes", "", "n")["status"]["allocatable"][GPU_XCD] == "4"  # the partition of XCDs 4-7


def test_agent_withholds_an_spx_gpu_with_a_lane_fault(store):
    agent = agent_on(store, fake_host(2, "SPX"),
                     lambda dev: GpuHealth(False, {5}, {"laneFaults": {5: ["permlane"]}}) if dev == 1 else True)
    assert agent.unhealthy == {1} and topo_of(store)["unhealthy"] == [1]
    assert topo_of(store)["laneFaults"] == {"1": {"5": ["permlane"]}}
    assert store.get("nodes", "", "n")["status"]["allocatable"][GPU] == "1"


def test_agent_fails_a_partition_device_on_a_plain_bool(store):
    agent = agent_on(store, fake_host(2, "CPX"), lambda dev: dev != 1)  # what hip_health_fn returns there
    assert agent.unhealthy == {1} and agent.faults["laneFaults"] == {} and "laneFaults" not in topo_of(store)


def test_agent_omits_the_key_when_there_is_none(store):
    agent = agent_on(store, fake_host(2, "CPX"), lambda dev: GpuHealth(False, {1}) if dev == 0 else True)
    assert "laneFaults" not in topo_of(store) and topo_of(store)["xcdFaults"] == {"0": [1]}
    assert agent.faults["laneFaults"] == {}
    agent = agent_on(store, fake_host(2, "CPX"), lambda dev: GpuHealth(True, (), {"laneFaults": {}}))
    assert "laneFaults" not in topo_of(store) and "xcdFaults" not in topo_of(store)
    plain = NodeAgent(LocalClient(store), "n", host_fn=lambda: fake_host(2, "CPX"), publish_metrics=False)
    want = plain.build_node(fake_host(2, "CPX"))["metadata"]["annotations"][TOPOLOGY_ANNOTATION]
    assert store.get("nodes", "", "n")["metadata"]["annotations"][TOPOLOGY_ANNOTATION] == want


def test_agent_resyncs_when_only_the_lane_faults_change(store):
    verdict = {"v": GpuHealth(False, {5}, {"laneFaults": {5: ["ldstr"]}})}
    agent = agent_on(store, fake_host(1, "CPX"), lambda dev: verdict["v"])
    assert topo_of(store)["laneFaults"] == {"0": {"5": ["ldstr"]}}
    verdict["v"] = GpuHealth(False, {5}, {"laneFaults": {5: ["ldstr", "ldswide"]}})
    agent._heartbeat_and_resync()
    assert topo_of(store)["laneFaults"] == {"0": {"5": ["ldstr", "ldswide"]}}
    assert topo_of(store)["xcdFaults"] == {"0": [5]}


# ---------------------------------------------------------------- scheduler
def test_scheduler_never_places_xcd_work_on_the_fenced_partition(store):
    agent_on(store, fake_host(1, "CPX"), lambda dev: GpuHealth(False, {5}, {"laneFaults": {5: ["bpermute"]}}))
    assert "laneFaults" in topo_of(store)
    s = start(store, coscheduling_config(FLEXGPU_PLUGINS))
    try:
        g = s.node_info("n")["gpu"]
        assert g["fenced"] == [[p == 5 for p in range(8)]] and g["free_xcds"] == 7
        create_all(store, "pods", [make_pod(f"x{i}", limits={GPU_XCD: "1"}) for i in range(7)])
        wait_bound(s, 7)
        parts = sorted(annotations(store, f"x{i}")["amd.com/gpu-partitions"] for i in range(7))
        assert parts == [f"0:{p}" for p in range(8) if p != 5]
    finally:
        s.stop()


# ---------------------------------------------------------------------- CLI
def test_cli_parses_the_lane_sweep_flag():
    ap = build_parser()
    none = ap.parse_args(["node-agent"])
    assert none.health_lane_sweep is None
    assert "lane" not in health_fn_args(none) and "lane_paths" not in health_fn_args(none)
    base = {"sweep": False, "sweep_period_s": 600.0, "matrix": False, "matrix_formats": None}
    on = ap.parse_args(["node-agent", "--health-lane-sweep"])
    assert health_fn_args(on) == {**base, "lane": True, "lane_paths": None}
    some = ap.parse_args(["node-agent", "--health-lane-sweep", "ldstr, ldsdma"])
    assert health_fn_args(some) == {**base, "lane": True, "lane_paths": ["ldstr", "ldsdma"]}
    every = ap.parse_args(["node-agent", "--health-lane-sweep", "dpp", "--health-register-sweep", "--health-sweep",
                           "--health-matrix-sweep", "fp8", "--health-hbm-sweep", "4", "--health-sweep-period", "30"])
    assert health_fn_args(every) == {"sweep": True, "sweep_period_s": 30.0, "matrix": True, "matrix_formats": ["fp8"],
                                     "hbm": True, "hbm_gib": 4.0, "regfile": True, "lane": True, "lane_paths": ["dpp"]}
    hip_health_fn_keywords = hip_health_fn.__code__.co_varnames[:hip_health_fn.__code__.co_argcount]
    assert set(health_fn_args(every)) <= set(hip_health_fn_keywords)
