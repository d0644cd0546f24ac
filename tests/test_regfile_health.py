"""The register-file sweep off the GPU: its host-side verdict
(summarize_regfile_sweep), hip_health_fn merging it with the CU and matrix
sweeps, the node agent publishing `registerFaults` next to `xcdFaults`, the
scheduler fencing from such a node, the node-agent flag, and the numpy
reference's own properties."""
import json

import numpy as np
import pytest

import regfile_sweep_ref as ref
from flex_gpu_scheduler_amd.cli import build_parser, health_fn_args
from flex_gpu_scheduler_amd.control import LocalClient
from flex_gpu_scheduler_amd.control.node_agent import GpuHealth, NodeAgent, hip_health_fn
from flex_gpu_scheduler_amd.gpu.discovery import fake_host
from flex_gpu_scheduler_amd.models import GPU_XCD, TOPOLOGY_ANNOTATION, make_pod
from flex_gpu_scheduler_amd.ops import hip_probe
from flex_gpu_scheduler_amd.ops.hip_probe import summarize_matrix_sweep, summarize_regfile_sweep, summarize_sweep
from helpers import FLEXGPU_PLUGINS, annotations, coscheduling_config, create_all, start, wait_bound

FORMATS = ["f16", "f32", "f64", "fp8", "bf8", "i8", "mxfp8", "mxbf8", "mxfp6", "mxbf6", "mxfp4"]
VGPR, AGPR = 1, 2


def records(xcds=8, cus=32, fail=None, skip=()):
    """One record per CU; `fail` maps (xcd, cu) to a dict of record fields."""
    out = []
    for x in range(xcds):
        for c in range(cus):
            if (x, c) in skip:
                continue
            r = {"xcd": x, "cu": c, "simd_mask": 15, "fail": 0, "bad_vgpr": 0, "bad_agpr": 0, "first": 0xFFFF,
                 "flip": 0, "digest": 0, "bad_simds": 0}
            r.update((fail or {}).get((x, c), {}))
            out.append(r)
    return out


# ------------------------------------------------------------ the reference
@pytest.mark.parametrize("seed", ref.SEEDS)
def test_reference_pattern_has_no_two_equal_cells(seed):
    for inverted in (False, True):
        p = ref.pattern(seed, inverted)
        assert p.shape == (512, 64) and int(p.max()) <= 0xFFFFFFFF
        assert len(np.unique(p)) == 512 * 64
    assert np.array_equal(ref.pattern(seed) ^ ref.pattern(seed, True), np.full((512, 64), 0xFFFFFFFF, np.uint64))


def test_reference_digests_differ_between_seeds():
    a, b = (ref.group_digest(s) for s in ref.SEEDS)
    assert a != b and a != 0 and b != 0
    assert ref.group_digest(ref.SEEDS[0]) == (15 * ref.wave_digest(ref.SEEDS[0])) & 0xFFFFFFFF


@pytest.fixture(scope="module")
def lib():
    try:
        return hip_probe.HipProbe()
    except (hip_probe.ProbeError, OSError) as e:
        pytest.skip(f"_hipprobe.so does not load here: {e}")


@pytest.mark.parametrize("seed", ref.SEEDS + (0, 1))
def test_host_digest_equals_the_reference(lib, seed):
    assert lib.regfile_sweep_expected(seed) == ref.group_digest(seed)


# -------------------------------------------------- summarize_regfile_sweep
def test_summarize_clean():
    s = summarize_regfile_sweep(records(), 256)
    assert s["covered"] and s["bad_xcds"] == [] and s["failed_files"] == []
    assert s["bad_cells"] == 0 and s["flip_mask"] == "0x00000000"
    for v in s["xcds"].values():
        assert v["failed_files"] == [] and v["bad_cells"] == 0 and v["bad_simds"] == {}
        assert v["flip_mask"] == "0x00000000"
    plain = summarize_sweep(records(), 256)
    extra = ("failed_files", "bad_cells", "flip_mask", "xcds")
    assert {k: v for k, v in s.items() if k not in extra} == {k: v for k, v in plain.items() if k != "xcds"}


def test_summarize_names_files_cells_and_simds_per_xcd():
    recs = records(fail={
        (5, 17): {"fail": AGPR, "bad_agpr": 64, "first": 456, "flip": 1 << 9, "bad_simds": 0b0100},
        (5, 3): {"fail": VGPR | AGPR, "bad_vgpr": 2, "bad_agpr": 1, "first": 12, "flip": 0x80000001,
                 "bad_simds": 0b1001},
        (2, 0): {"fail": VGPR, "bad_vgpr": 256, "first": 0, "flip": 1, "bad_simds": 0b1111},
    })
    s = summarize_regfile_sweep(recs, 256)
    assert s["bad_xcds"] == [2, 5] and s["covered"]
    x5, x2 = s["xcds"][5], s["xcds"][2]
    assert x5["failed_files"] == ["vgpr", "agpr"] and x5["failed_cus"] == [3, 17]
    assert x5["bad_cells"] == 67 and x5["flip_mask"] == "0x80000201"
    assert x5["bad_simds"] == {3: [0, 3], 17: [2]}
    assert x2["failed_files"] == ["vgpr"] and x2["bad_cells"] == 256 and x2["bad_simds"] == {0: [0, 1, 2, 3]}
    assert s["xcds"][0]["failed_files"] == [] and s["xcds"][0]["bad_simds"] == {}
    assert s["failed_files"] == ["vgpr", "agpr"] and s["bad_cells"] == 323 and s["flip_mask"] == "0x80000201"


def test_summarize_a_digest_only_failure_names_both_files():
    s = summarize_regfile_sweep(records(fail={(1, 1): {"fail": VGPR | AGPR}}), 256)
    assert s["bad_xcds"] == [1] and s["xcds"][1]["failed_files"] == ["vgpr", "agpr"]
    assert s["xcds"][1]["bad_cells"] == 0


def test_summarize_uncovered_is_not_failed():
    s = summarize_regfile_sweep(records(skip={(6, 0), (6, 9)}), 256)
    assert not s["covered"] and s["uncovered"][6] == 2
    assert s["bad_xcds"] == [] and s["failed_files"] == []


# ------------------------------------------------------------ hip_health_fn
class FakeProbe:
    def __init__(self, cus=256, cu_bad=(), matrix_fail=None, regfile_fail=None, regfile_skip=(), healthy=True):
        self.cus, self.cu_bad, self.matrix_fail, self.healthy = cus, cu_bad, matrix_fail or {}, healthy
        self.regfile_fail, self.regfile_skip = regfile_fail or {}, regfile_skip
        self.cu_calls, self.matrix_calls, self.regfile_calls = 0, 0, []

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

    def matrix_sweep(self, dev, formats=None, **kw):
        self.matrix_calls += 1
        recs = [{"xcd": x, "cu": c, "fail": sum(1 << FORMATS.index(f) for f in self.matrix_fail.get(x, ())) * (c == 1)}
                for x in range(self._xcds()) for c in range(32)]
        s = summarize_matrix_sweep(recs, self.cus, FORMATS)
        s.update(rounds=1, ms=0.1, blocks=4 * self.cus, formats=formats or FORMATS)
        return {"records": recs, "summary": s}

    def regfile_sweep(self, dev, **kw):
        self.regfile_calls.append(kw)
        recs = records(self._xcds(), fail={(x, 2): f for x, f in self.regfile_fail.items()}, skip=self.regfile_skip)
        s = summarize_regfile_sweep(recs, self.cus)
        s.update(rounds=1, ms=0.3, blocks=4 * self.cus, seed=0)
        return {"records": recs, "summary": s}


@pytest.fixture
def fake(monkeypatch):
    def install(**kw):
        f = FakeProbe(**kw)
        monkeypatch.setattr(hip_probe, "probe", lambda: f)
        return f
    return install


A200 = {"fail": AGPR, "bad_agpr": 64, "first": 456, "flip": 1 << 9, "bad_simds": 0b0100}
V8 = {"fail": VGPR, "bad_vgpr": 256, "first": 8, "flip": 1 << 31, "bad_simds": 0b1111}


def test_health_fn_default_runs_no_register_sweep(fake):
    f = fake()
    assert hip_health_fn()(0) is True
    assert hip_health_fn(sweep=True, matrix=True)(0)
    assert f.regfile_calls == []


def test_health_fn_unites_the_bad_xcds_of_the_three_sweeps(fake):
    f = fake(cu_bad=(1,), matrix_fail={6: ["mxfp4"]}, regfile_fail={3: A200, 6: V8})
    v = hip_health_fn(sweep=True, matrix=True, regfile=True)(0)
    assert isinstance(v, GpuHealth) and not v.ok and not v
    assert v.bad_xcds == frozenset({1, 3, 6})
    assert v.detail["matrixFaults"] == {6: ["mxfp4"]}
    assert v.detail["registerFaults"] == {
        3: {"files": ["agpr"], "cells": 64, "flipMask": "0x00000200", "simds": 1},
        6: {"files": ["vgpr"], "cells": 256, "flipMask": "0x80000000", "simds": 4}}
    assert v.detail["registerSweep"]["bad_xcds"] == [3, 6]
    assert "sweep" in v.detail and "matrixSweep" in v.detail
    assert f.cu_calls == 1 and f.matrix_calls == 1 and len(f.regfile_calls) == 1


def test_health_fn_register_sweep_alone_and_its_arguments(fake):
    f = fake(regfile_fail={3: A200})
    v = hip_health_fn(regfile=True, regfile_args={"blocks": 64, "seed": 5})(0)
    assert v.bad_xcds == frozenset({3}) and sorted(v.detail["registerFaults"]) == [3]
    assert f.cu_calls == 0 and f.matrix_calls == 0 and f.regfile_calls == [{"blocks": 64, "seed": 5}]
    ok = fake()
    v = hip_health_fn(regfile=True)(0)
    assert isinstance(v, GpuHealth) and v.ok and v and v.detail["registerFaults"] == {}
    assert ok.regfile_calls == [{}]


def test_health_fn_uncovered_cus_do_not_fail_the_device(fake):
    fake(regfile_skip={(4, 7)})
    v = hip_health_fn(regfile=True)(0)
    assert isinstance(v, GpuHealth) and v.ok and v
    assert not v.detail["registerSweep"]["covered"]


def test_health_fn_reuses_the_verdict_for_the_period(fake):
    f = fake(regfile_fail={2: V8})
    fn = hip_health_fn(sweep=True, regfile=True, sweep_period_s=3600.0)
    first = fn(0)
    assert fn(0) is first and fn(0) is first
    assert f.cu_calls == 1 and len(f.regfile_calls) == 1
    fn(1)  # another device has its own verdict
    assert f.cu_calls == 2 and len(f.regfile_calls) == 2
    g = fake(regfile_fail={2: V8})
    fn = hip_health_fn(regfile=True, sweep_period_s=0.0)
    fn(0), fn(0)
    assert len(g.regfile_calls) == 2


def test_health_fn_on_a_partition_device_returns_a_bool(fake):
    fake(cus=64, regfile_fail={1: A200})
    assert hip_health_fn(regfile=True)(0) is False
    fake(cus=64)
    assert hip_health_fn(regfile=True)(0) is True


def test_health_fn_skips_the_sweep_when_the_basic_check_fails(fake):
    f = fake(healthy=False)
    assert hip_health_fn(regfile=True)(0) is False
    assert f.regfile_calls == []


# --------------------------------------------------------------- node agent
def agent_on(store, host, health_fn):
    agent = NodeAgent(LocalClient(store), "n", host_fn=lambda: host, publish_metrics=False, health_fn=health_fn)
    agent.sync()
    return agent


def topo_of(store) -> dict:
    return json.loads(store.get("nodes", "", "n")["metadata"]["annotations"][TOPOLOGY_ANNOTATION])


FAULT = {"files": ["agpr"], "cells": 64, "flipMask": "0x00000200", "simds": 1}


def test_agent_publishes_register_faults_next_to_xcd_faults(store):
    def health(dev):
        return GpuHealth(False, {5}, {"registerFaults": {5: FAULT}, "matrixFaults": {5: ["fp8"]}}) if dev == 0 else True

    agent = agent_on(store, fake_host(2, "CPX"), health)
    topo = topo_of(store)
    assert topo["xcdFaults"] == {"0": [5]}
    assert topo["registerFaults"] == {"0": {"5": FAULT}}
    assert topo["matrixFaults"] == {"0": {"5": ["fp8"]}}
    assert agent.faults["registerFaults"] == {0: {5: FAULT}} and agent.unhealthy_xcds == {0: {5}}
    assert store.get("nodes", "", "n")["status"]["allocatable"][GPU_XCD] == "15"


def test_agent_withholds_an_spx_gpu_with_a_register_fault(store):
    agent = agent_on(store, fake_host(2, "SPX"),
                     lambda dev: GpuHealth(False, {5}, {"registerFaults": {5: FAULT}}) if dev == 1 else True)
    assert agent.unhealthy == {1} and topo_of(store)["unhealthy"] == [1]
    assert topo_of(store)["registerFaults"] == {"1": {"5": FAULT}}


def test_agent_omits_the_key_when_there_is_none(store):
    agent = agent_on(store, fake_host(2, "CPX"), lambda dev: GpuHealth(False, {1}) if dev == 0 else True)
    assert "registerFaults" not in topo_of(store) and topo_of(store)["xcdFaults"] == {"0": [1]}
    assert agent.faults["registerFaults"] == {}
    agent = agent_on(store, fake_host(2, "CPX"), lambda dev: GpuHealth(True, (), {"registerFaults": {}}))
    assert "registerFaults" not in topo_of(store) and "xcdFaults" not in topo_of(store)
    plain = NodeAgent(LocalClient(store), "n", host_fn=lambda: fake_host(2, "CPX"), publish_metrics=False)
    want = plain.build_node(fake_host(2, "CPX"))["metadata"]["annotations"][TOPOLOGY_ANNOTATION]
    assert store.get("nodes", "", "n")["metadata"]["annotations"][TOPOLOGY_ANNOTATION] == want


def test_agent_resyncs_when_only_the_register_faults_change(store):
    verdict = {"v": GpuHealth(False, {5}, {"registerFaults": {5: FAULT}})}
    agent = agent_on(store, fake_host(1, "CPX"), lambda dev: verdict["v"])
    assert topo_of(store)["registerFaults"] == {"0": {"5": FAULT}}
    worse = dict(FAULT, files=["vgpr", "agpr"], cells=65)
    verdict["v"] = GpuHealth(False, {5}, {"registerFaults": {5: worse}})
    agent._heartbeat_and_resync()
    assert topo_of(store)["registerFaults"] == {"0": {"5": worse}}
    assert topo_of(store)["xcdFaults"] == {"0": [5]}


# ---------------------------------------------------------------- scheduler
def test_scheduler_never_places_xcd_work_on_the_fenced_partition(store):
    agent_on(store, fake_host(1, "CPX"), lambda dev: GpuHealth(False, {5}, {"registerFaults": {5: FAULT}}))
    assert "registerFaults" in topo_of(store)
    s = start(store, coscheduling_config(FLEXGPU_PLUGINS))
    try:
        g = s.node_info("n")["gpu"]
        assert g["fenced"] == [[p == 5 for p in range(8)]] and g["free_xcds"] == 7
        create_all(store, "pods", [make_pod(f"x{i}", limits={GPU_XCD: "1"}) for i in range(7)])
        wait_bound(s, 7)
        parts = sorted(annotations(store, f"x{i}")["amd.com/gpu-partitions"] for i in range(7))
        assert parts == [f"0:{p}" for p in range(8) if p != 5]
        assert s.node_info("n")["gpu"]["free_xcds"] == 0
    finally:
        s.stop()


# ---------------------------------------------------------------------- CLI
def test_cli_parses_the_register_sweep_flag():
    ap = build_parser()
    none = ap.parse_args(["node-agent"])
    assert none.health_register_sweep is False and "regfile" not in health_fn_args(none)
    on = ap.parse_args(["node-agent", "--health-register-sweep"])
    assert health_fn_args(on) == {"sweep": False, "sweep_period_s": 600.0, "matrix": False, "matrix_formats": None,
                                  "regfile": True}
    both = ap.parse_args(["node-agent", "--health-register-sweep", "--health-sweep", "--health-matrix-sweep", "fp8",
                          "--health-sweep-period", "30"])
    assert health_fn_args(both) == {"sweep": True, "sweep_period_s": 30.0, "matrix": True, "matrix_formats": ["fp8"],
                                    "regfile": True}
