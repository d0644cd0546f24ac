"""The scalar sweep off the GPU: the host's digests against the numpy
reference, the library's C ABI, its verdict (summarize_scalar_sweep,
decode_part_record over the SCALAR_SWEEP row and the record's tail),
hip_health_fn merging it with the other sweeps in order, the node agent
publishing `scalarFaults` next to `xcdFaults`, and the node-agent flag."""
import json

import pytest

import scalar_sweep_ref as ref
from flex_gpu_scheduler_amd.cli import build_parser, health_fn_args, wants_health_fn
from flex_gpu_scheduler_amd.control import LocalClient
from flex_gpu_scheduler_amd.control.node_agent import (FAULT_KINDS, MEM_SWEEP_KIND, SCALAR_SWEEP_KIND, SWEEP_KINDS,
                                                       GpuHealth, NodeAgent, hip_health_fn)
from flex_gpu_scheduler_amd.gpu.discovery import fake_host
from flex_gpu_scheduler_amd.models import GPU_XCD, TOPOLOGY_ANNOTATION
from flex_gpu_scheduler_amd.ops import hip_probe
from flex_gpu_scheduler_amd.ops.hip_probe import (PART_SWEEPS, SCALAR_SWEEP, decode_part_record, scalar_record_tail,
                                                  summarize_mem_sweep, summarize_scalar_sweep, summarize_sweep,
                                                  summarize_valu_sweep)

PARTS = ref.PARTS


def bits(*names):
    return sum(1 << PARTS.index(n) for n in names)


def records(xcds=8, cus=32, fail=None, skip=()):
    """One record per CU; `fail` maps (xcd, cu) to the parts that failed there."""
    out = []
    for x in range(xcds):
        for c in range(cus):
            if (x, c) in skip:
                continue
            names = (fail or {}).get((x, c), ())
            out.append({"xcd": x, "cu": c, "simd_mask": 15, "fail": bits(*names),
                        "bad": {f: int(f in names) for f in PARTS}, "digests": {f: 0 for f in PARTS},
                        "bad_simds": 1 if names else 0})
    return out


# ---------------------------------------------------------- the host library
@pytest.fixture(scope="module")
def lib():
    # No skip: a _hipscalar.so that is missing or does not load is a failure of these tests.
    return hip_probe.HipProbe()


def test_host_names_and_shapes(lib):
    assert lib.scalar_parts() == PARTS == ["arith", "logic", "bits", "cmp", "branch", "mask", "movrel", "sgpr"]
    assert {f: tuple(lib.scalar_shape(f).values()) for f in PARTS} == ref.SHAPES
    with pytest.raises(ValueError):
        lib.scalar_shape("float")
    with pytest.raises(ValueError):
        lib.scalar_sweep_expected(["cmp", "trap"])


@pytest.mark.parametrize("seed", ref.SEEDS)
def test_host_digests_equal_the_reference(lib, seed):
    assert lib.scalar_sweep_expected(seed=seed) == {f: ref.digest(f, seed) for f in PARTS}
    assert lib.scalar_sweep_expected(["sgpr", "logic", "mask"], seed) == {f: ref.digest(f, seed)
                                                                          for f in ("logic", "mask", "sgpr")}
    assert lib.scalar_sweep_expected("movrel", seed) == {"movrel": ref.digest("movrel", seed)}


def test_the_library_exports_exactly_the_bound_symbols(lib):
    import re
    import shutil
    import subprocess

    nm = shutil.which("nm")
    if nm is None:
        pytest.skip("nm is not installed")

    def exported(path):
        out = subprocess.run([nm, "-D", "--defined-only", str(path)], capture_output=True, text=True, check=True)
        return {line.split()[-1] for line in out.stdout.splitlines() if line.split()}

    assert {n for n in exported(hip_probe._SCALAR_LIB) if n.startswith("xs_")} == set(hip_probe.SCALAR_SYMBOLS)
    assert hip_probe.SCALAR_SYMBOLS == ("xs_scalar_sweep_last_error", "xs_scalar_parts", "xs_scalar_shape",
                                        "xs_scalar_probe", "xs_scalar_sweep_expected", "xs_scalar_sweep_info",
                                        "xs_scalar_sweep")
    assert all(getattr(lib.lib, n) is getattr(lib.scalar_lib, n) for n in hip_probe.SCALAR_SYMBOLS)
    for other in (hip_probe._LIB, hip_probe._MEM_LIB):
        assert not any(re.match(r"xs_scalar_", n) for n in exported(other)), other


def test_host_refuses_bad_arguments(lib):
    import ctypes

    out = (ctypes.c_uint32 * 8)()
    assert lib.lib.xs_scalar_sweep_expected(0, 0, out) == -1000
    assert lib.lib.xs_scalar_sweep_expected(1 << 8, 0, out) == -1000
    assert lib.lib.xs_scalar_sweep_expected(0xFF, 0, None) == -1000
    two = (ctypes.c_int * 2)()
    assert lib.lib.xs_scalar_shape(8, two) == -1000 and lib.lib.xs_scalar_shape(-1, two) == -1000
    n, ms = ctypes.c_int(), ctypes.c_double()
    rec = (ctypes.c_uint32 * 32)()
    # Refused before anything touches a device: a bad mask, injected parts beyond the mask's range.
    assert lib.lib.xs_scalar_sweep(0, 1, 0, 0, -1, -1, 0, rec, ctypes.byref(n), ctypes.byref(ms)) == -1000
    assert lib.lib.xs_scalar_sweep(0, 1, 0x1FF, 0, -1, -1, 0, rec, ctypes.byref(n), ctypes.byref(ms)) == -1000
    assert lib.lib.xs_scalar_sweep(0, 1, 1, 0, -1, -1, 0x100, rec, ctypes.byref(n), ctypes.byref(ms)) == -1000
    assert lib.lib.xs_scalar_sweep(0, 1, 1, 0, -2, -1, 0, rec, ctypes.byref(n), ctypes.byref(ms)) == -1000
    assert lib.lib.xs_scalar_sweep(0, 1, 1, 0, -1, -2, 0, rec, ctypes.byref(n), ctypes.byref(ms)) == -1000
    assert lib.lib.xs_scalar_probe(0, 8, 0, rec, 32) == -1000 and lib.lib.xs_scalar_probe(0, 0, 0, rec, 32) == -1000


# ---------------------------------------------------------------- the row
def test_the_row_stands_beside_the_table():
    assert list(PART_SWEEPS) == ["matrix", "lane", "valu", "mem"] and SCALAR_SWEEP not in PART_SWEEPS.values()
    assert (SCALAR_SWEEP.prefix, SCALAR_SWEEP.names_symbol, SCALAR_SWEEP.noun) == ("scalar", "xs_scalar_parts",
                                                                                  "scalar part")
    assert (SCALAR_SWEEP.summary_key, SCALAR_SWEEP.selection) == ("failed_parts", "parts")
    # PartRecordHead<8>: four words, eight counts, eight digests, bad_simds; as the lane sweep's.
    assert (SCALAR_SWEEP.record_words, SCALAR_SWEEP.bad, SCALAR_SWEEP.digests, SCALAR_SWEEP.bad_simds) == (32, 4, 12, 20)
    assert SCALAR_SWEEP.step_mask is None
    assert (hip_probe.SCALAR_BLOCK, hip_probe.SCALAR_SEED, hip_probe.SCALAR_COVER_WORD) == (1024, ref.SEEDS[0], 22)


def test_decode_part_record_over_the_row_and_the_tail():
    w = [0] * 32
    w[0:4] = [5, 0x21, 0xF, 0]
    w[4:12] = [0, 0, 0, 3, 0, 0, 0, 0]
    w[12:20] = [100 + i for i in range(8)]
    w[20] = 4
    w[22:30] = [0x066060CC, ~0x060060C0 & 0xFFFFFFFF, 0, 0, 0x060060C0, ~0x060060C0 & 0xFFFFFFFF, 0, 0]
    expected = {f: 100 + i for i, f in enumerate(PARTS)}
    r = decode_part_record(SCALAR_SWEEP, PARTS, w, expected)
    assert (r["xcd"], r["cu"], r["simd_mask"], r["bad_simds"]) == (5, 0x21, 0xF, 4)
    assert r["bad"] == {f: 3 * (f == "cmp") for f in PARTS} and r["digests"] == expected
    assert r["fail"] == 0 and "bad_steps" not in r
    assert decode_part_record(SCALAR_SWEEP, PARTS, w, {**expected, "sgpr": 1})["fail"] == bits("sgpr")
    w2 = list(w)
    w2[12:20] = [0, 0, 0, 0, 104, 0, 0, 107]
    assert decode_part_record(SCALAR_SWEEP, PARTS, w2, {"branch": 104, "sgpr": 107})["fail"] == 0
    assert decode_part_record(SCALAR_SWEEP, PARTS, w2, {"branch": 104})["fail"] == bits("sgpr")
    # The tail: per SIMD the OR and the AND of the raw HW_REG_GPR_ALLOC words; a SIMD without a wave reads (0, all ones).
    tail = scalar_record_tail(w)
    assert tail == {"gpr_alloc": [(0x066060CC, 0x060060C0), (0, 0xFFFFFFFF), (0x060060C0, 0x060060C0), (0, 0xFFFFFFFF)]}


# -------------------------------------------------- summarize_scalar_sweep
def test_summarize_clean():
    s = summarize_scalar_sweep(records(), 256, PARTS)
    assert s["covered"] and s["bad_xcds"] == [] and s["failed_parts"] == []
    assert all(v["failed_parts"] == [] and v["failed_cus"] == [] for v in s["xcds"].values())
    plain = summarize_sweep(records(), 256)
    assert {k: v for k, v in s.items() if k not in ("failed_parts", "xcds")} == {k: v for k, v in plain.items()
                                                                                  if k != "xcds"}
    assert "sgpr_blocks" not in s  # no coverage figure: HW_REG_GPR_ALLOC is not laid out as assumed


def test_summarize_names_parts_per_xcd():
    s = summarize_scalar_sweep(records(fail={(5, 17): ["sgpr"], (5, 3): ["arith", "mask"], (2, 0): ["branch"]}),
                               256, PARTS)
    assert s["bad_xcds"] == [2, 5] and s["covered"]
    assert s["xcds"][5]["failed_cus"] == [3, 17] and s["xcds"][5]["failed_parts"] == ["arith", "mask", "sgpr"]
    assert s["xcds"][2]["failed_parts"] == ["branch"] and s["xcds"][0]["failed_parts"] == []
    assert s["failed_parts"] == ["arith", "branch", "mask", "sgpr"]


def test_summarize_uncovered_is_not_failed():
    s = summarize_scalar_sweep(records(skip={(6, 0), (6, 9)}), 256, PARTS)
    assert not s["covered"] and s["uncovered"][6] == 2
    assert s["bad_xcds"] == [] and s["failed_parts"] == []


# ------------------------------------------------------------ hip_health_fn
class FakeProbe:
    def __init__(self, cus=256, cu_bad=(), valu_fail=None, scalar_fail=None, scalar_skip=(), mem_fail=None):
        self.cus, self.cu_bad = cus, cu_bad
        self.valu_fail, self.scalar_fail, self.scalar_skip = valu_fail or {}, scalar_fail or {}, scalar_skip
        self.mem_fail = mem_fail or {}
        self.order, self.scalar_calls = [], []

    def props(self, dev):
        return {"computeUnits": self.cus}

    def health(self, dev):
        return {"healthy": True}

    def mfma_check(self, dev):
        return {"healthy": True}

    def _xcds(self):
        return self.cus // 32

    def cu_sweep(self, dev, **kw):
        self.order.append("cu")
        recs = [{"xcd": x, "cu": c, "fail": int(c == 0 and x in self.cu_bad)}
                for x in range(self._xcds()) for c in range(32)]
        s = summarize_sweep(recs, self.cus)
        s.update(rounds=1, ms=2.0, blocks=4 * self.cus)
        return {"records": recs, "summary": s}

    def valu_sweep(self, dev, units=None, **kw):
        import valu_sweep_ref

        self.order.append("valu")
        names = valu_sweep_ref.UNITS
        recs = [{"xcd": x, "cu": c, "simd_mask": 15, "bad_steps": [],
                 "fail": sum(1 << names.index(n) for n in self.valu_fail.get(x, ())) if c == 4 else 0}
                for x in range(self._xcds()) for c in range(32)]
        s = summarize_valu_sweep(recs, self.cus, names)
        s.update(rounds=1, ms=0.5, blocks=4 * self.cus, seed=0, units=units or names)
        return {"records": recs, "summary": s}

    def scalar_sweep(self, dev, parts=None, **kw):
        self.order.append("scalar")
        self.scalar_calls.append({"parts": parts, **kw})
        recs = records(self._xcds(), fail={(x, 4): f for x, f in self.scalar_fail.items()}, skip=self.scalar_skip)
        s = summarize_scalar_sweep(recs, self.cus, PARTS)
        s.update(rounds=1, ms=1.5, blocks=4 * self.cus, seed=0, parts=parts or PARTS)
        return {"records": recs, "summary": s}

    def mem_sweep(self, dev, routes=None, **kw):
        import mem_sweep_ref

        self.order.append("mem")
        names = mem_sweep_ref.ROUTES
        recs = [{"xcd": x, "cu": c, "simd_mask": 15,
                 "fail": sum(1 << names.index(n) for n in self.mem_fail.get(x, ())) if c == 4 else 0}
                for x in range(self._xcds()) for c in range(32)]
        s = summarize_mem_sweep(recs, self.cus, names)
        s.update(rounds=1, ms=1.5, blocks=4 * self.cus, seed=0, routes=routes or names)
        return {"records": recs, "summary": s}


@pytest.fixture
def fake(monkeypatch):
    def install(**kw):
        f = FakeProbe(**kw)
        monkeypatch.setattr(hip_probe, "probe", lambda: f)
        return f
    return install


def test_the_sweep_kind_and_its_fault_kind():
    k = SCALAR_SWEEP_KIND
    assert k not in SWEEP_KINDS and len(SWEEP_KINDS) == 5
    assert (k.enabled_by, k.method, k.label, k.summary_key, k.selection, k.faults_key) == (
        "scalar", "scalar_sweep", "scalar", "scalarSweep", "parts", "scalarFaults")
    assert k.fault_of({"failed_parts": ("sgpr",)}) == ["sgpr"]
    f = FAULT_KINDS["scalarFaults"]
    assert not f.per_xcd and not f.withholds_gpu
    assert sorted(n for n, v in FAULT_KINDS.items() if v.per_xcd) == ["laneFaults", "matrixFaults", "registerFaults",
                                                                     "valuFaults"]


def test_health_fn_default_runs_no_scalar_sweep(fake):
    f = fake()
    assert hip_health_fn()(0) is True
    assert hip_health_fn(sweep=True, valu=True)(0)
    assert f.scalar_calls == [] and f.order == ["cu", "valu"]


def test_health_fn_scalar_sweep_alone_and_its_arguments(fake):
    f = fake(scalar_fail={3: ["sgpr"]})
    v = hip_health_fn(scalar=True, scalar_parts=["sgpr", "cmp"], scalar_args={"blocks": 64, "seed": 5})(0)
    assert isinstance(v, GpuHealth) and not v.ok
    assert v.bad_xcds == frozenset({3}) and v.detail["scalarFaults"] == {3: ["sgpr"]}
    assert v.detail["scalarSweep"]["parts"] == ["sgpr", "cmp"]
    assert f.order == ["scalar"] and f.scalar_calls == [{"parts": ["sgpr", "cmp"], "blocks": 64, "seed": 5}]
    ok = fake()
    v = hip_health_fn(scalar=True)(0)
    assert isinstance(v, GpuHealth) and v.ok and v and v.detail["scalarFaults"] == {}
    assert ok.scalar_calls == [{"parts": None}]


def test_health_fn_runs_it_after_the_valu_sweep_and_before_the_memory_sweep(fake):
    f = fake(cu_bad=(1,), valu_fail={6: ["f64"]}, scalar_fail={3: ["arith"], 6: ["mask", "movrel"]},
             mem_fail={7: ["l2"]})
    v = hip_health_fn(mem=True, scalar=True, valu=True, sweep=True)(0)
    assert f.order == ["cu", "valu", "scalar", "mem"]
    assert isinstance(v, GpuHealth) and not v.ok and not v
    assert v.bad_xcds == frozenset({1, 3, 6, 7})
    assert v.detail["scalarFaults"] == {3: ["arith"], 6: ["mask", "movrel"]}
    assert v.detail["valuFaults"] == {6: ["f64"]} and v.detail["memFaults"] == {7: ["l2"]}
    assert v.detail["scalarSweep"]["bad_xcds"] == [3, 6]
    assert MEM_SWEEP_KIND is not SCALAR_SWEEP_KIND


def test_health_fn_uncovered_cus_do_not_fail_the_device(fake):
    fake(scalar_skip={(4, 7)})
    v = hip_health_fn(scalar=True)(0)
    assert isinstance(v, GpuHealth) and v.ok and v
    assert not v.detail["scalarSweep"]["covered"] and v.detail["scalarFaults"] == {}


def test_health_fn_on_a_partition_device_returns_a_bool(fake):
    fake(cus=64, scalar_fail={1: ["branch"]})
    assert hip_health_fn(scalar=True)(0) is False
    fake(cus=64)
    assert hip_health_fn(scalar=True)(0) is True


# --------------------------------------------------------------- node agent
def agent_on(store, host, health_fn):
    agent = NodeAgent(LocalClient(store), "n", host_fn=lambda: host, publish_metrics=False, health_fn=health_fn)
    agent.sync()
    return agent


def topo_of(store) -> dict:
    return json.loads(store.get("nodes", "", "n")["metadata"]["annotations"][TOPOLOGY_ANNOTATION])


def test_agent_publishes_scalar_faults_and_fences_the_partition(store):
    def health(dev):
        return GpuHealth(False, {5}, {"scalarFaults": {5: ["sgpr", "arith"]}, "valuFaults": {5: ["int"]}}) \
            if dev == 0 else True

    agent = agent_on(store, fake_host(2, "CPX"), health)
    topo = topo_of(store)
    assert topo["xcdFaults"] == {"0": [5]} and topo["unhealthy"] == []
    assert topo["scalarFaults"] == {"0": {"5": ["sgpr", "arith"]}}
    assert topo["valuFaults"] == {"0": {"5": ["int"]}}
    assert agent.faults["scalarFaults"] == {0: {5: ["sgpr", "arith"]}} and agent.unhealthy_xcds == {0: {5}}
    assert store.get("nodes", "", "n")["status"]["allocatable"][GPU_XCD] == "15"  # only XCD 5's partition is fenced


def test_agent_fences_from_an_injected_fault_through_the_health_fn(store, fake):
    fake(scalar_fail={6: ["mask"]})
    agent_on(store, fake_host(1, "DPX"), hip_health_fn(scalar=True, scalar_args={"inject": (6, None, ["mask"])}))
    assert topo_of(store)["scalarFaults"] == {"0": {"6": ["mask"]}} and topo_of(store)["xcdFaults"] == {"0": [6]}
    assert store.get("nodes", "", "n")["status"]["allocatable"][GPU_XCD] == "4"  # the partition of XCDs 4-7


def test_agent_omits_the_key_when_there_is_none_and_resyncs_when_it_changes(store, fake):
    fake()
    agent_on(store, fake_host(2, "CPX"), hip_health_fn(scalar=True))  # a clean sweep: an empty fault dict
    assert "scalarFaults" not in topo_of(store) and "xcdFaults" not in topo_of(store)
    verdict = {"v": GpuHealth(False, {5}, {"scalarFaults": {5: ["cmp"]}})}
    agent = agent_on(store, fake_host(1, "CPX"), lambda dev: verdict["v"])
    assert topo_of(store)["scalarFaults"] == {"0": {"5": ["cmp"]}}
    verdict["v"] = GpuHealth(False, {5}, {"scalarFaults": {5: ["cmp", "bits"]}})
    agent._heartbeat_and_resync()
    assert topo_of(store)["scalarFaults"] == {"0": {"5": ["cmp", "bits"]}}
    assert topo_of(store)["xcdFaults"] == {"0": [5]}


# ---------------------------------------------------------------------- CLI
def test_cli_parses_the_scalar_sweep_flag():
    ap = build_parser()
    none = ap.parse_args(["node-agent"])
    assert none.health_scalar_sweep is None and not wants_health_fn(none)
    assert "scalar" not in health_fn_args(none) and "scalar_parts" not in health_fn_args(none)
    base = {"sweep": False, "sweep_period_s": 600.0, "matrix": False, "matrix_formats": None}
    on = ap.parse_args(["node-agent", "--health-scalar-sweep"])
    assert health_fn_args(on) == {**base, "scalar": True, "scalar_parts": None} and wants_health_fn(on)
    some = ap.parse_args(["node-agent", "--health-scalar-sweep", "sgpr, mask"])
    assert health_fn_args(some) == {**base, "scalar": True, "scalar_parts": ["sgpr", "mask"]}
    every = ap.parse_args(["node-agent", "--health-scalar-sweep", "cmp", "--health-mem-sweep", "l1", "--health-sweep",
                           "--health-valu-sweep", "--health-sweep-period", "30"])
    assert health_fn_args(every) == {"sweep": True, "sweep_period_s": 30.0, "matrix": False, "matrix_formats": None,
                                     "valu": True, "valu_units": None, "scalar": True, "scalar_parts": ["cmp"],
                                     "mem": True, "mem_routes": ["l1"]}
    hip_health_fn_keywords = hip_health_fn.__code__.co_varnames[:hip_health_fn.__code__.co_argcount]
    assert set(health_fn_args(every)) <= set(hip_health_fn_keywords)
