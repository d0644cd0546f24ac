"""The memory-path sweep off the GPU: the host's digests against the numpy
reference, its verdict (summarize_mem_sweep, decode_part_record over the new
row), hip_health_fn merging it with the other sweeps and taking "unswept" for
what it is, the node agent publishing `memFaults` next to `xcdFaults`, and the
node-agent flag."""
import json

import pytest

import mem_sweep_ref as ref
from flex_gpu_scheduler_amd.cli import build_parser, health_fn_args, wants_health_fn
from flex_gpu_scheduler_amd.control import LocalClient
from flex_gpu_scheduler_amd.control.node_agent import (FAULT_KINDS, MEM_SWEEP_KIND, SWEEP_KINDS, GpuHealth, NodeAgent,
                                                       hip_health_fn)
from flex_gpu_scheduler_amd.gpu.discovery import fake_host
from flex_gpu_scheduler_amd.models import GPU_XCD, TOPOLOGY_ANNOTATION
from flex_gpu_scheduler_amd.ops import hip_probe
from flex_gpu_scheduler_amd.ops.hip_probe import (MEM_STRAY_STORE, MEM_SWEEP, MEM_UNSWEPT, PART_SWEEPS, ProbeError,
                                                  decode_part_record, summarize_lane_sweep, summarize_mem_sweep,
                                                  summarize_sweep)

ROUTES = ref.ROUTES


def bits(*names):
    return sum(1 << ROUTES.index(n) for n in names)


def records(xcds=8, cus=32, fail=None, skip=()):
    """One record per CU; `fail` maps (xcd, cu) to the routes that failed there."""
    out = []
    for x in range(xcds):
        for c in range(cus):
            if (x, c) in skip:
                continue
            names = (fail or {}).get((x, c), ())
            out.append({"xcd": x, "cu": c, "simd_mask": 15, "fail": bits(*names),
                        "bad": {f: int(f in names) for f in ROUTES}, "digests": {f: 0 for f in ROUTES},
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
    assert lib.mem_routes() == ROUTES == ["gwidth", "buffer", "flat", "atomic", "l1", "l2", "scalar"]
    assert {f: tuple(lib.mem_shape(f).values()) for f in ROUTES} == ref.SHAPES
    with pytest.raises(ValueError):
        lib.mem_shape("l3")
    with pytest.raises(ValueError):
        lib.mem_sweep_expected(["l1", "texture"])


@pytest.mark.parametrize("seed", ref.SEEDS)
def test_host_digests_equal_the_reference(lib, seed):
    assert lib.mem_sweep_expected(seed=seed) == {f: ref.digest(f, seed) for f in ROUTES}
    assert lib.mem_sweep_expected(["scalar", "buffer"], seed) == {f: ref.digest(f, seed) for f in ("buffer", "scalar")}
    assert lib.mem_sweep_expected("l2", seed) == {"l2": ref.digest("l2", seed)}


def test_the_library_exports_exactly_the_bound_symbols(lib):
    import re
    import shutil
    import subprocess

    nm = shutil.which("nm")
    if nm is None:
        pytest.skip("nm is not installed")
    out = subprocess.run([nm, "-D", "--defined-only", str(hip_probe._MEM_LIB)], capture_output=True, text=True, check=True)
    exported = {line.split()[-1] for line in out.stdout.splitlines() if line.split()}
    assert {name for name in exported if name.startswith("xs_")} == set(hip_probe.MEM_SYMBOLS)
    assert len(hip_probe.MEM_SYMBOLS) == 7
    # Every one is reachable where _call and _part_sweep look it up, and is the memory library's own.
    assert all(getattr(lib.lib, name) is getattr(lib.mem_lib, name) for name in hip_probe.MEM_SYMBOLS)
    main = subprocess.run([nm, "-D", "--defined-only", str(hip_probe._LIB)], capture_output=True, text=True, check=True)
    assert not re.search(r"\bxs_mem_", main.stdout)


def test_host_refuses_bad_masks(lib):
    import ctypes

    out = (ctypes.c_uint32 * 7)()
    assert lib.lib.xs_mem_sweep_expected(0, 0, out) == -1000
    assert lib.lib.xs_mem_sweep_expected(1 << 7, 0, out) == -1000
    assert lib.lib.xs_mem_sweep_expected(0x7F, 0, None) == -1000
    assert lib.lib.xs_mem_shape(7, (ctypes.c_int * 2)()) == -1000 and lib.lib.xs_mem_shape(-1, (ctypes.c_int * 2)()) == -1000


# ------------------------------------------------------- the PART_SWEEPS row
def test_the_row_and_its_codes():
    assert list(PART_SWEEPS) == ["matrix", "lane", "valu", "mem"] and PART_SWEEPS["mem"] is MEM_SWEEP
    assert (MEM_SWEEP.prefix, MEM_SWEEP.names_symbol, MEM_SWEEP.noun) == ("mem", "xs_mem_routes", "memory route")
    assert (MEM_SWEEP.summary_key, MEM_SWEEP.selection) == ("failed_routes", "routes")
    # PartRecordHead<7>: four words, seven counts, seven digests, bad_simds.
    assert (MEM_SWEEP.record_words, MEM_SWEEP.bad, MEM_SWEEP.digests, MEM_SWEEP.bad_simds) == (32, 4, 11, 18)
    assert (MEM_UNSWEPT, MEM_STRAY_STORE) == (-1003, -1004)
    assert MEM_UNSWEPT == hip_probe.HBM_UNSWEPT
    e = hip_probe._probe_error(lambda: b"", MEM_UNSWEPT, "mem_sweep", hip_probe.MEM_WORDING)
    assert e.rc == MEM_UNSWEPT and "no memory could be had" in str(e)
    e = hip_probe._probe_error(lambda: b"stray store: the guard band behind slab 3", MEM_STRAY_STORE, "mem_sweep",
                               hip_probe.MEM_WORDING)
    assert e.rc == MEM_STRAY_STORE and "stray store" in str(e) and "slab 3" in str(e)


def test_decode_part_record_over_the_row():
    w = [0] * 32
    w[0:4] = [5, 0x21, 0xF, 0]
    w[4:11] = [0, 0, 0, 3, 0, 0, 0]
    w[11:18] = [100 + i for i in range(7)]
    w[18] = 4
    expected = {f: 100 + i for i, f in enumerate(ROUTES)}
    r = decode_part_record(MEM_SWEEP, ROUTES, w, expected)
    assert (r["xcd"], r["cu"], r["simd_mask"], r["bad_simds"]) == (5, 0x21, 0xF, 4)
    assert r["bad"] == {f: 3 * (f == "atomic") for f in ROUTES} and r["digests"] == expected
    assert r["fail"] == 0 and "bad_steps" not in r
    # A digest off the host's fails the route even where the device passed it.
    r = decode_part_record(MEM_SWEEP, ROUTES, w, {**expected, "l2": 1})
    assert r["fail"] == bits("l2")
    # A sub-selection: the routes not selected carry digest 0.
    w[11:18] = [0, 0, 0, 0, 104, 0, 106]
    assert decode_part_record(MEM_SWEEP, ROUTES, w, {"l1": 104, "scalar": 106})["fail"] == 0
    assert decode_part_record(MEM_SWEEP, ROUTES, w, {"l1": 104})["fail"] == bits("scalar")


# ------------------------------------------------------- summarize_mem_sweep
def test_summarize_clean():
    s = summarize_mem_sweep(records(), 256, ROUTES)
    assert s["covered"] and s["bad_xcds"] == [] and s["failed_routes"] == []
    assert all(v["failed_routes"] == [] and v["failed_cus"] == [] for v in s["xcds"].values())
    plain = summarize_sweep(records(), 256)
    assert {k: v for k, v in s.items() if k not in ("failed_routes", "xcds")} == {k: v for k, v in plain.items()
                                                                                   if k != "xcds"}


def test_summarize_names_routes_per_xcd():
    s = summarize_mem_sweep(records(fail={(5, 17): ["l2"], (5, 3): ["gwidth", "scalar"], (2, 0): ["atomic"]}),
                            256, ROUTES)
    assert s["bad_xcds"] == [2, 5] and s["covered"]
    assert s["xcds"][5]["failed_cus"] == [3, 17] and s["xcds"][5]["failed_routes"] == ["gwidth", "l2", "scalar"]
    assert s["xcds"][2]["failed_routes"] == ["atomic"] and s["xcds"][0]["failed_routes"] == []
    assert s["failed_routes"] == ["gwidth", "atomic", "l2", "scalar"]


def test_summarize_uncovered_is_not_failed():
    s = summarize_mem_sweep(records(skip={(6, 0), (6, 9)}), 256, ROUTES)
    assert not s["covered"] and s["uncovered"][6] == 2
    assert s["bad_xcds"] == [] and s["failed_routes"] == []


# ------------------------------------------------------------ hip_health_fn
class FakeProbe:
    def __init__(self, cus=256, cu_bad=(), lane_fail=None, mem_fail=None, mem_skip=(), mem_error=None, healthy=True):
        self.cus, self.cu_bad, self.healthy = cus, cu_bad, healthy
        self.lane_fail, self.mem_fail, self.mem_skip, self.mem_error = lane_fail or {}, mem_fail or {}, mem_skip, mem_error
        self.cu_calls, self.lane_calls, self.mem_calls = 0, 0, []

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
        import lane_sweep_ref

        self.lane_calls += 1
        names = lane_sweep_ref.PATHS
        recs = [{"xcd": x, "cu": c, "simd_mask": 15,
                 "fail": sum(1 << names.index(n) for n in self.lane_fail.get(x, ())) if c == 4 else 0, "bad_simds": 0}
                for x in range(self._xcds()) for c in range(32)]
        s = summarize_lane_sweep(recs, self.cus, names)
        s.update(rounds=1, ms=0.5, blocks=4 * self.cus, seed=0, paths=paths or names)
        return {"records": recs, "summary": s}

    def mem_sweep(self, dev, routes=None, **kw):
        self.mem_calls.append({"routes": routes, **kw})
        if self.mem_error is not None:
            e = ProbeError(f"mem_sweep failed ({self.mem_error})")
            e.rc = self.mem_error
            raise e
        recs = records(self._xcds(), fail={(x, 4): f for x, f in self.mem_fail.items()}, skip=self.mem_skip)
        s = summarize_mem_sweep(recs, self.cus, ROUTES)
        s.update(rounds=1, ms=1.5, blocks=4 * self.cus, seed=0, routes=routes or ROUTES)
        return {"records": recs, "summary": s}


@pytest.fixture
def fake(monkeypatch):
    def install(**kw):
        f = FakeProbe(**kw)
        monkeypatch.setattr(hip_probe, "probe", lambda: f)
        return f
    return install


def test_the_sweep_kind_and_its_fault_kind():
    k = MEM_SWEEP_KIND
    assert k not in SWEEP_KINDS  # it can come back unswept, which the kinds of that table cannot
    assert (k.enabled_by, k.method, k.label, k.summary_key, k.selection, k.faults_key) == (
        "mem", "mem_sweep", "mem", "memSweep", "routes", "memFaults")
    assert k.fault_of({"failed_routes": ("l2",)}) == ["l2"]
    assert "memFaults" in FAULT_KINDS and not FAULT_KINDS["memFaults"].withholds_gpu


def test_health_fn_default_runs_no_mem_sweep(fake):
    f = fake()
    assert hip_health_fn()(0) is True
    assert hip_health_fn(sweep=True, lane=True)(0)
    assert f.mem_calls == []


def test_health_fn_mem_sweep_alone_and_its_arguments(fake):
    f = fake(mem_fail={3: ["l2"]})
    v = hip_health_fn(mem=True, mem_routes=["l2", "l1"], mem_args={"blocks": 64, "seed": 5})(0)
    assert isinstance(v, GpuHealth) and not v.ok
    assert v.bad_xcds == frozenset({3}) and v.detail["memFaults"] == {3: ["l2"]}
    assert v.detail["memSweep"]["routes"] == ["l2", "l1"]
    assert f.cu_calls == 0 and f.lane_calls == 0
    assert f.mem_calls == [{"routes": ["l2", "l1"], "blocks": 64, "seed": 5}]
    ok = fake()
    v = hip_health_fn(mem=True)(0)
    assert isinstance(v, GpuHealth) and v.ok and v and v.detail["memFaults"] == {}
    assert ok.mem_calls == [{"routes": None}]


def test_health_fn_unites_the_bad_xcds_of_the_sweeps(fake):
    f = fake(cu_bad=(1,), lane_fail={6: ["dpp"]}, mem_fail={3: ["scalar"], 6: ["gwidth", "atomic"]})
    v = hip_health_fn(sweep=True, lane=True, mem=True)(0)
    assert isinstance(v, GpuHealth) and not v.ok and not v
    assert v.bad_xcds == frozenset({1, 3, 6})
    assert v.detail["memFaults"] == {3: ["scalar"], 6: ["gwidth", "atomic"]}
    assert v.detail["laneFaults"] == {6: ["dpp"]} and v.detail["memSweep"]["bad_xcds"] == [3, 6]
    assert f.cu_calls == 1 and f.lane_calls == 1 and len(f.mem_calls) == 1


def test_health_fn_unswept_leaves_the_gpu_healthy_and_the_other_faults_intact(fake, caplog):
    fake(mem_error=MEM_UNSWEPT)
    with caplog.at_level("WARNING"):
        v = hip_health_fn(mem=True)(0)
    assert isinstance(v, GpuHealth) and v.ok and v and v.bad_xcds == frozenset()
    assert "memSweep" not in v.detail and "memFaults" not in v.detail
    assert "unswept, no memory could be had" in caplog.text
    f = fake(mem_error=MEM_UNSWEPT, cu_bad=(2,), lane_fail={5: ["ldstr"]})
    v = hip_health_fn(sweep=True, lane=True, mem=True)(0)
    assert not v.ok and v.bad_xcds == frozenset({2, 5}) and v.detail["laneFaults"] == {5: ["ldstr"]}
    assert "memFaults" not in v.detail and len(f.mem_calls) == 1


def test_health_fn_raises_every_other_error(fake):
    for rc in (MEM_STRAY_STORE, -1000, -2):
        fake(mem_error=rc)
        with pytest.raises(ProbeError) as e:
            hip_health_fn(mem=True)(0)
        assert e.value.rc == rc


def test_health_fn_uncovered_cus_do_not_fail_the_device(fake):
    fake(mem_skip={(4, 7)})
    v = hip_health_fn(mem=True)(0)
    assert isinstance(v, GpuHealth) and v.ok and v
    assert not v.detail["memSweep"]["covered"] and v.detail["memFaults"] == {}


def test_health_fn_on_a_partition_device_returns_a_bool(fake):
    fake(cus=64, mem_fail={1: ["flat"]})
    assert hip_health_fn(mem=True)(0) is False
    fake(cus=64)
    assert hip_health_fn(mem=True)(0) is True


# --------------------------------------------------------------- node agent
def agent_on(store, host, health_fn):
    agent = NodeAgent(LocalClient(store), "n", host_fn=lambda: host, publish_metrics=False, health_fn=health_fn)
    agent.sync()
    return agent


def topo_of(store) -> dict:
    return json.loads(store.get("nodes", "", "n")["metadata"]["annotations"][TOPOLOGY_ANNOTATION])


def test_agent_publishes_mem_faults_and_fences_the_partition(store):
    def health(dev):
        return GpuHealth(False, {5}, {"memFaults": {5: ["l2", "atomic"]}, "laneFaults": {5: ["dpp"]}}) \
            if dev == 0 else True

    agent = agent_on(store, fake_host(2, "CPX"), health)
    topo = topo_of(store)
    assert topo["xcdFaults"] == {"0": [5]} and topo["unhealthy"] == []
    assert topo["memFaults"] == {"0": {"5": ["l2", "atomic"]}}
    assert topo["laneFaults"] == {"0": {"5": ["dpp"]}}
    assert agent.faults["memFaults"] == {0: {5: ["l2", "atomic"]}} and agent.unhealthy_xcds == {0: {5}}
    assert store.get("nodes", "", "n")["status"]["allocatable"][GPU_XCD] == "15"  # only XCD 5's partition is fenced


def test_agent_fences_from_an_injected_fault_through_the_health_fn(store, fake):
    fake(mem_fail={6: ["l2"]})
    agent_on(store, fake_host(1, "DPX"), hip_health_fn(mem=True, mem_args={"inject": (6, None, ["l2"])}))
    assert topo_of(store)["memFaults"] == {"0": {"6": ["l2"]}} and topo_of(store)["xcdFaults"] == {"0": [6]}
    assert store.get("nodes", "", "n")["status"]["allocatable"][GPU_XCD] == "4"  # the partition of XCDs 4-7


def test_agent_omits_the_key_when_there_is_none(store, fake):
    agent = agent_on(store, fake_host(2, "CPX"), lambda dev: GpuHealth(False, {1}) if dev == 0 else True)
    assert "memFaults" not in topo_of(store) and topo_of(store)["xcdFaults"] == {"0": [1]}
    assert agent.faults["memFaults"] == {}
    fake()
    agent_on(store, fake_host(2, "CPX"), hip_health_fn(mem=True))  # a clean sweep: an empty fault dict
    assert "memFaults" not in topo_of(store) and "xcdFaults" not in topo_of(store)
    fake(mem_error=MEM_UNSWEPT)
    agent = agent_on(store, fake_host(2, "CPX"), hip_health_fn(mem=True))
    assert "memFaults" not in topo_of(store) and agent.unhealthy == set()


def test_agent_resyncs_when_only_the_mem_faults_change(store):
    verdict = {"v": GpuHealth(False, {5}, {"memFaults": {5: ["l1"]}})}
    agent = agent_on(store, fake_host(1, "CPX"), lambda dev: verdict["v"])
    assert topo_of(store)["memFaults"] == {"0": {"5": ["l1"]}}
    verdict["v"] = GpuHealth(False, {5}, {"memFaults": {5: ["l1", "l2"]}})
    agent._heartbeat_and_resync()
    assert topo_of(store)["memFaults"] == {"0": {"5": ["l1", "l2"]}}
    assert topo_of(store)["xcdFaults"] == {"0": [5]}


# ---------------------------------------------------------------------- CLI
def test_cli_parses_the_mem_sweep_flag():
    ap = build_parser()
    none = ap.parse_args(["node-agent"])
    assert none.health_mem_sweep is None and not wants_health_fn(none)
    assert "mem" not in health_fn_args(none) and "mem_routes" not in health_fn_args(none)
    base = {"sweep": False, "sweep_period_s": 600.0, "matrix": False, "matrix_formats": None}
    on = ap.parse_args(["node-agent", "--health-mem-sweep"])
    assert health_fn_args(on) == {**base, "mem": True, "mem_routes": None} and wants_health_fn(on)
    some = ap.parse_args(["node-agent", "--health-mem-sweep", "l2, scalar"])
    assert health_fn_args(some) == {**base, "mem": True, "mem_routes": ["l2", "scalar"]}
    every = ap.parse_args(["node-agent", "--health-mem-sweep", "l1", "--health-lane-sweep", "dpp", "--health-sweep",
                           "--health-valu-sweep", "--health-hbm-sweep", "4", "--health-sweep-period", "30"])
    assert health_fn_args(every) == {"sweep": True, "sweep_period_s": 30.0, "matrix": False, "matrix_formats": None,
                                     "hbm": True, "hbm_gib": 4.0, "lane": True, "lane_paths": ["dpp"], "valu": True,
                                     "valu_units": None, "mem": True, "mem_routes": ["l1"]}
    hip_health_fn_keywords = hip_health_fn.__code__.co_varnames[:hip_health_fn.__code__.co_argcount]
    assert set(health_fn_args(every)) <= set(hip_health_fn_keywords)
