"""The VALU sweep off the GPU: its host-side verdict (summarize_valu_sweep),
hip_health_fn merging it with the other sweeps, the node agent publishing
`valuFaults` next to `xcdFaults`, the scheduler fencing from such a node, the
node-agent flag, and, where the library loads, the host's expected table
against the reference, bit for bit: the GPU trusts that table."""
import json

import numpy as np
import pytest

import valu_sweep_ref as ref
from flex_gpu_scheduler_amd.cli import build_parser, health_fn_args
from flex_gpu_scheduler_amd.control import LocalClient
from flex_gpu_scheduler_amd.control.node_agent import FAULT_KINDS, GpuHealth, NodeAgent, hip_health_fn
from flex_gpu_scheduler_amd.gpu.discovery import fake_host
from flex_gpu_scheduler_amd.models import GPU_XCD, TOPOLOGY_ANNOTATION, make_pod
from flex_gpu_scheduler_amd.ops import hip_probe
from flex_gpu_scheduler_amd.ops.hip_probe import summarize_lane_sweep, summarize_sweep, summarize_valu_sweep
from helpers import FLEXGPU_PLUGINS, annotations, coscheduling_config, create_all, start, wait_bound

UNITS = ref.UNITS
LANE_PATHS = ["dpp", "permlane", "readlane", "bpermute", "ldswide", "ldstr", "ldsatomic", "ldsdma"]


def bits(*names):
    return sum(1 << UNITS.index(n) for n in names)


def records(xcds=8, cus=32, fail=None, skip=()):
    """One record per CU; `fail` maps (xcd, cu) to {unit: [step, ...]} that failed there."""
    out = []
    for x in range(xcds):
        for c in range(cus):
            if (x, c) in skip:
                continue
            f = (fail or {}).get((x, c), {})
            out.append({"xcd": x, "cu": c, "simd_mask": 15, "fail": bits(*f),
                        "bad": {u: int(u in f) for u in UNITS}, "digests": {u: 0 for u in UNITS},
                        "bad_simds": 1 if f else 0, "bad_steps": [s for u in f for s in f[u]]})
    return out


# ---------------------------------------------------------- the host library
@pytest.fixture(scope="module")
def lib():
    try:
        return hip_probe.HipProbe()
    except (hip_probe.ProbeError, OSError) as e:
        pytest.skip(f"_hipprobe.so does not load here: {e}")


def test_host_names_and_shapes(lib):
    assert lib.valu_units() == UNITS
    assert {u: lib.valu_steps(u) for u in UNITS} == ref.STEPS
    assert lib.valu_steps() == [s for u in UNITS for s in ref.STEPS[u]]
    assert {u: tuple(lib.valu_shape(u).values()) for u in UNITS} == ref.SHAPES
    with pytest.raises(ValueError):
        lib._valu_mask(["f32", "f8"])
    assert lib._valu_mask(None) == 0xFF and lib._valu_mask("dot") == 1 << 5


@pytest.mark.parametrize("seed", ref.SEEDS)
@pytest.mark.parametrize("unit", UNITS)
def test_host_table_is_bit_equal_to_the_reference(lib, unit, seed):
    names = ref.row_names(unit)
    for rounds in (1, 2, 4):
        got, want = lib.valu_expected(unit, seed, rounds), ref.expected(unit, seed, rounds)
        assert got.shape == want.shape == (rounds, ref.SHAPES[unit][1], 256)
        bad = np.argwhere(got != want)
        assert not len(bad), [(names[row], int(r), int(t), hex(got[r, row, t]), hex(want[r, row, t]))
                              for r, row, t in bad[:12]]
        assert lib.valu_sweep_expected([unit], seed, rounds) == {unit: ref.digest(unit, seed, rounds)}


def test_host_digests_of_all_units_and_the_refusals(lib):
    seed = ref.SEEDS[0]
    assert lib.valu_sweep_expected(seed=seed, rounds=2) == {u: ref.digest(u, seed, 2) for u in UNITS}
    out8 = (hip_probe.ctypes.c_uint32 * 8)()
    assert lib.lib.xs_valu_sweep_expected(0, seed, 2, out8) == hip_probe.BAD_ARGS
    assert lib.lib.xs_valu_sweep_expected(0x100, seed, 2, out8) == hip_probe.BAD_ARGS
    assert lib.lib.xs_valu_sweep_expected(1, seed, 0, out8) == hip_probe.BAD_ARGS
    assert lib.lib.xs_valu_sweep_expected(1, seed, 65, out8) == hip_probe.BAD_ARGS
    assert lib.lib.xs_valu_sweep_expected(1, seed, 2, None) == hip_probe.BAD_ARGS
    buf = np.zeros(16, np.uint32)
    assert lib.lib.xs_valu_expected(0, seed, 1, buf.ctypes.data, buf.size) == hip_probe.BAD_ARGS  # the wrong size
    assert lib.lib.xs_valu_expected(8, seed, 1, buf.ctypes.data, buf.size) == hip_probe.BAD_ARGS
    assert lib.lib.xs_valu_steps(8) is None and lib.lib.xs_valu_steps(-1) is None
    for rounds in (0, 65):
        with pytest.raises(hip_probe.ProbeError) as e:
            lib.valu_expected("f32", seed, rounds)
        assert e.value.rc == hip_probe.BAD_ARGS


# ------------------------------------------------------ summarize_valu_sweep
def test_summarize_clean():
    s = summarize_valu_sweep(records(), 256, UNITS)
    assert s["covered"] and s["bad_xcds"] == [] and s["failed_units"] == [] and s["failed_steps"] == []
    assert all(v["failed_units"] == [] and v["failed_steps"] == [] and v["failed_cus"] == [] for v in s["xcds"].values())
    plain = summarize_sweep(records(), 256)
    assert {k: v for k, v in s.items() if k not in ("failed_units", "failed_steps", "xcds")} == \
        {k: v for k, v in plain.items() if k != "xcds"}


def test_summarize_names_units_and_steps_per_xcd():
    s = summarize_valu_sweep(records(fail={(5, 17): {"cvt": ["v_cvt_pk_fp8_f32"]},
                                           (5, 3): {"f32": ["v_fma_f32", "div_f32"], "trans": ["v_exp_f32"]},
                                           (2, 0): {"f64": ["v_fma_f64"]}}), 256, UNITS)
    assert s["bad_xcds"] == [2, 5] and s["covered"]
    assert s["xcds"][5]["failed_cus"] == [3, 17] and s["xcds"][5]["failed_units"] == ["f32", "cvt", "trans"]
    assert s["xcds"][5]["failed_steps"] == ["v_fma_f32", "div_f32", "v_exp_f32", "v_cvt_pk_fp8_f32"]
    assert s["xcds"][2]["failed_units"] == ["f64"] and s["xcds"][2]["failed_steps"] == ["v_fma_f64"]
    assert s["xcds"][0]["failed_units"] == [] and s["xcds"][0]["failed_steps"] == []
    assert s["failed_units"] == ["f32", "f64", "cvt", "trans"]
    assert s["failed_steps"] == ["v_fma_f64", "v_fma_f32", "div_f32", "v_exp_f32", "v_cvt_pk_fp8_f32"]


def test_summarize_uncovered_is_not_failed():
    s = summarize_valu_sweep(records(skip={(6, 0), (6, 9)}), 256, UNITS)
    assert not s["covered"] and s["uncovered"][6] == 2
    assert s["bad_xcds"] == [] and s["failed_units"] == []


# ------------------------------------------------------------ hip_health_fn
class FakeProbe:
    def __init__(self, cus=256, cu_bad=(), lane_fail=None, valu_fail=None, valu_skip=(), healthy=True):
        self.cus, self.cu_bad, self.healthy = cus, cu_bad, healthy
        self.lane_fail, self.valu_fail, self.valu_skip = lane_fail or {}, valu_fail or {}, valu_skip
        self.cu_calls, self.lane_calls, self.valu_calls = 0, 0, []

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

    def lane_sweep(self, dev, paths=None, **kw):
        self.lane_calls += 1
        recs = [{"xcd": x, "cu": c, "fail": sum(1 << LANE_PATHS.index(n) for n in self.lane_fail.get(x, ())) if c == 4 else 0}
                for x in range(self._xcds()) for c in range(32)]
        s = summarize_lane_sweep(recs, self.cus, LANE_PATHS)
        s.update(rounds=1, ms=0.5, blocks=4 * self.cus, seed=0, paths=paths or LANE_PATHS)
        return {"records": recs, "summary": s}

    def valu_sweep(self, dev, units=None, **kw):
        self.valu_calls.append({"units": units, **kw})
        recs = records(self._xcds(), fail={(x, 4): f for x, f in self.valu_fail.items()}, skip=self.valu_skip)
        s = summarize_valu_sweep(recs, self.cus, UNITS)
        s.update(rounds=1, ms=1.9, blocks=4 * self.cus, seed=0, units=units or UNITS, operand_rounds=2)
        return {"records": recs, "summary": s}


@pytest.fixture
def fake(monkeypatch):
    def install(**kw):
        f = FakeProbe(**kw)
        monkeypatch.setattr(hip_probe, "probe", lambda: f)
        return f
    return install


def test_fault_kind_is_registered_per_xcd():
    assert FAULT_KINDS["valuFaults"].per_xcd and not FAULT_KINDS["valuFaults"].withholds_gpu


def test_health_fn_default_runs_no_valu_sweep(fake):
    f = fake()
    assert hip_health_fn()(0) is True
    assert hip_health_fn(sweep=True, lane=True)(0)
    assert f.valu_calls == []


def test_health_fn_unites_the_bad_xcds_of_the_sweeps(fake):
    f = fake(cu_bad=(1,), lane_fail={6: ["dpp"]},
             valu_fail={3: {"f64": ["v_fma_f64"]}, 6: {"f32": ["v_fma_f32"], "cvt": ["v_cvt_f16_f32"]}})
    v = hip_health_fn(sweep=True, lane=True, valu=True)(0)
    assert isinstance(v, GpuHealth) and not v.ok and not v
    assert v.bad_xcds == frozenset({1, 3, 6})
    assert v.detail["valuFaults"] == {3: ["f64"], 6: ["f32", "cvt"]}
    assert v.detail["valuSweep"]["bad_xcds"] == [3, 6] and v.detail["laneFaults"] == {6: ["dpp"]}
    assert v.detail["valuSweep"]["xcds"][6]["failed_steps"] == ["v_fma_f32", "v_cvt_f16_f32"]
    assert f.cu_calls == 1 and f.lane_calls == 1 and len(f.valu_calls) == 1


def test_health_fn_valu_sweep_alone_and_its_arguments(fake):
    f = fake(valu_fail={3: {"dot": ["v_dot4_i32_i8"]}})
    v = hip_health_fn(valu=True, valu_units=["dot", "bit"], valu_args={"blocks": 64, "rounds": 4})(0)
    assert v.bad_xcds == frozenset({3}) and v.detail["valuFaults"] == {3: ["dot"]}
    assert f.cu_calls == 0 and f.lane_calls == 0
    assert f.valu_calls == [{"units": ["dot", "bit"], "blocks": 64, "rounds": 4}]
    ok = fake()
    v = hip_health_fn(valu=True)(0)
    assert isinstance(v, GpuHealth) and v.ok and v and v.detail["valuFaults"] == {}
    assert ok.valu_calls == [{"units": None}]


def test_health_fn_uncovered_cus_do_not_fail_the_device(fake):
    fake(valu_skip={(4, 7)})
    v = hip_health_fn(valu=True)(0)
    assert isinstance(v, GpuHealth) and v.ok and v
    assert not v.detail["valuSweep"]["covered"] and v.detail["valuFaults"] == {}


def test_health_fn_on_a_partition_device_returns_a_bool(fake):
    fake(cus=64, valu_fail={1: {"int": ["v_mad_u64_u32"]}})
    assert hip_health_fn(valu=True)(0) is False
    fake(cus=64)
    assert hip_health_fn(valu=True)(0) is True


def test_health_fn_skips_the_sweep_when_the_basic_check_fails(fake):
    f = fake(healthy=False)
    assert hip_health_fn(valu=True)(0) is False
    assert f.valu_calls == []


# --------------------------------------------------------------- node agent
def agent_on(store, host, health_fn):
    agent = NodeAgent(LocalClient(store), "n", host_fn=lambda: host, publish_metrics=False, health_fn=health_fn)
    agent.sync()
    return agent


def topo_of(store) -> dict:
    return json.loads(store.get("nodes", "", "n")["metadata"]["annotations"][TOPOLOGY_ANNOTATION])


def test_agent_publishes_valu_faults_and_fences_the_partition(store):
    def health(dev):
        return GpuHealth(False, {5}, {"valuFaults": {5: ["f64", "cvt"]}, "laneFaults": {5: ["dpp"]}}) \
            if dev == 0 else True

    agent = agent_on(store, fake_host(2, "CPX"), health)
    topo = topo_of(store)
    assert topo["xcdFaults"] == {"0": [5]} and topo["unhealthy"] == []
    assert topo["valuFaults"] == {"0": {"5": ["f64", "cvt"]}}
    assert topo["laneFaults"] == {"0": {"5": ["dpp"]}}
    assert agent.faults["valuFaults"] == {0: {5: ["f64", "cvt"]}} and agent.unhealthy_xcds == {0: {5}}
    assert store.get("nodes", "", "n")["status"]["allocatable"][GPU_XCD] == "15"  # only XCD 5's partition is fenced


def test_agent_omits_the_key_when_there_is_none(store):
    agent = agent_on(store, fake_host(2, "CPX"), lambda dev: GpuHealth(False, {1}) if dev == 0 else True)
    assert "valuFaults" not in topo_of(store) and topo_of(store)["xcdFaults"] == {"0": [1]}
    assert agent.faults["valuFaults"] == {}
    agent = agent_on(store, fake_host(2, "CPX"), lambda dev: GpuHealth(True, (), {"valuFaults": {}}))
    assert "valuFaults" not in topo_of(store) and "xcdFaults" not in topo_of(store)
    plain = NodeAgent(LocalClient(store), "n", host_fn=lambda: fake_host(2, "CPX"), publish_metrics=False)
    want = plain.build_node(fake_host(2, "CPX"))["metadata"]["annotations"][TOPOLOGY_ANNOTATION]
    assert store.get("nodes", "", "n")["metadata"]["annotations"][TOPOLOGY_ANNOTATION] == want


def test_agent_resyncs_when_only_the_valu_faults_change(store):
    verdict = {"v": GpuHealth(False, {5}, {"valuFaults": {5: ["f16"]}})}
    agent = agent_on(store, fake_host(1, "CPX"), lambda dev: verdict["v"])
    assert topo_of(store)["valuFaults"] == {"0": {"5": ["f16"]}}
    verdict["v"] = GpuHealth(False, {5}, {"valuFaults": {5: ["f16", "trans"]}})
    agent._heartbeat_and_resync()
    assert topo_of(store)["valuFaults"] == {"0": {"5": ["f16", "trans"]}}
    assert topo_of(store)["xcdFaults"] == {"0": [5]}


# ---------------------------------------------------------------- scheduler
def test_scheduler_never_places_xcd_work_on_the_fenced_partition(store):
    agent_on(store, fake_host(1, "CPX"), lambda dev: GpuHealth(False, {5}, {"valuFaults": {5: ["f32"]}}))
    assert "valuFaults" in topo_of(store)
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
def test_cli_parses_the_valu_sweep_flag():
    ap = build_parser()
    none = ap.parse_args(["node-agent"])
    assert none.health_valu_sweep is None
    assert "valu" not in health_fn_args(none) and "valu_units" not in health_fn_args(none)
    base = {"sweep": False, "sweep_period_s": 600.0, "matrix": False, "matrix_formats": None}
    on = ap.parse_args(["node-agent", "--health-valu-sweep"])
    assert health_fn_args(on) == {**base, "valu": True, "valu_units": None}
    some = ap.parse_args(["node-agent", "--health-valu-sweep", "f64, cvt"])
    assert health_fn_args(some) == {**base, "valu": True, "valu_units": ["f64", "cvt"]}
    every = ap.parse_args(["node-agent", "--health-valu-sweep", "dot", "--health-lane-sweep", "dpp",
                           "--health-register-sweep", "--health-sweep", "--health-sweep-period", "30"])
    assert health_fn_args(every) == {"sweep": True, "sweep_period_s": 30.0, "matrix": False, "matrix_formats": None,
                                     "regfile": True, "lane": True, "lane_paths": ["dpp"], "valu": True,
                                     "valu_units": ["dot"]}
    hip_health_fn_keywords = hip_health_fn.__code__.co_varnames[:hip_health_fn.__code__.co_argcount]
    assert set(health_fn_args(every)) <= set(hip_health_fn_keywords)
