"""The fetch sweep off the GPU: the host's digests against the independent
reference, the library's C ABI, its verdict (summarize_fetch_sweep,
decode_part_record over the FETCH_SWEEP row), hip_health_fn merging it with the
other sweeps in order, the node agent publishing `fetchFaults` next to
`xcdFaults`, and the node-agent flag."""
import json

import pytest

import fetch_sweep_ref as ref
from flex_gpu_scheduler_amd.cli import build_parser, health_fn_args, wants_health_fn
from flex_gpu_scheduler_amd.control import LocalClient
from flex_gpu_scheduler_amd.control.node_agent import (CONSENSUS_SWEEP_KIND, FAULT_KINDS, FETCH_SWEEP_KIND,
                                                       MEM_SWEEP_KIND, SWEEP_KINDS, GpuHealth, NodeAgent,
                                                       hip_health_fn)
from flex_gpu_scheduler_amd.gpu.discovery import fake_host
from flex_gpu_scheduler_amd.models import GPU_XCD, TOPOLOGY_ANNOTATION
from flex_gpu_scheduler_amd.ops import hip_probe
from flex_gpu_scheduler_amd.ops.hip_probe import (FETCH_SWEEP, PART_SWEEPS, decode_part_record, summarize_fetch_sweep,
                                                  summarize_mem_sweep, summarize_sweep)

PARTS = ref.PARTS
SEEDS = (hip_probe.FETCH_SEED, 0x9E3779B9)


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
                        "bad": {f: 0 for f in PARTS}, "digests": {f: 0 for f in PARTS}, "bad_simds": 0})
    return out


# ---------------------------------------------------------- the host library
@pytest.fixture(scope="module")
def lib():
    # No skip: a _hipfetch.so that is missing or does not load is a failure of these tests.
    return hip_probe.HipProbe()


def test_host_names_and_shapes(lib):
    assert lib.fetch_parts() == PARTS == ["stream", "loop", "call", "align", "refill"]
    for rounds in (1, 2, 5):
        assert {f: lib.fetch_shape(f, rounds)["rows"] for f in PARTS} == {f: ref.rows_of(f, rounds) for f in PARTS}
    assert lib.fetch_shape("loop") == {"fixed_rows": 0, "rows_per_round": 4, "rows": 4 * hip_probe.FETCH_ROUNDS}
    assert lib.fetch_shape("stream", 3) == {"fixed_rows": 32, "rows_per_round": 0, "rows": 32}
    with pytest.raises(ValueError):
        lib.fetch_shape("decode")
    with pytest.raises(ValueError):
        lib.fetch_sweep_expected(["call", "trap"])


@pytest.mark.parametrize("rounds", (1, 2))
@pytest.mark.parametrize("seed", SEEDS)
def test_host_digests_equal_the_reference(lib, seed, rounds):
    want = ref.digests(PARTS, seed, rounds)
    assert lib.fetch_sweep_expected(seed=seed, rounds=rounds) == want
    for f in PARTS:
        assert lib.fetch_sweep_expected(f, seed, rounds) == {f: want[f]}
    assert lib.fetch_sweep_expected(["refill", "stream"], seed, rounds) == {f: want[f] for f in ("stream", "refill")}
    assert len(set(want.values())) == len(PARTS)


def test_the_digests_depend_on_seed_and_rounds(lib):
    a, b = (lib.fetch_sweep_expected(seed=s, rounds=1) for s in SEEDS)
    assert all(a[f] != b[f] for f in PARTS)
    two = lib.fetch_sweep_expected(seed=SEEDS[0], rounds=2)
    assert all(a[f] != two[f] for f in ("loop", "call")) and all(a[f] == two[f] for f in ("stream", "align", "refill"))


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

    assert {n for n in exported(hip_probe._FETCH_LIB) if n.startswith("xs_")} == set(hip_probe.FETCH_SYMBOLS)
    assert hip_probe.FETCH_SYMBOLS == ("xs_fetch_sweep_last_error", "xs_fetch_parts", "xs_fetch_shape",
                                       "xs_fetch_probe", "xs_fetch_sweep_expected", "xs_fetch_sweep_info",
                                       "xs_fetch_sweep")
    assert all(getattr(lib.lib, n) is getattr(lib.fetch_lib, n) for n in hip_probe.FETCH_SYMBOLS)
    for other in (hip_probe._LIB, hip_probe._MEM_LIB, hip_probe._SCALAR_LIB, hip_probe._CONSENSUS_LIB):
        assert not any(re.match(r"xs_fetch_", n) for n in exported(other)), other


def test_host_refuses_bad_arguments(lib):
    import ctypes

    out = (ctypes.c_uint32 * 5)()
    assert lib.lib.xs_fetch_sweep_expected(0, 0, 1, out) == -1000
    assert lib.lib.xs_fetch_sweep_expected(1 << 5, 0, 1, out) == -1000
    assert lib.lib.xs_fetch_sweep_expected(0x1F, 0, 0, out) == -1000
    assert lib.lib.xs_fetch_sweep_expected(0x1F, 0, 65, out) == -1000
    assert lib.lib.xs_fetch_sweep_expected(0x1F, 0, 1, None) == -1000
    two = (ctypes.c_int * 2)()
    assert lib.lib.xs_fetch_shape(5, two) == -1000 and lib.lib.xs_fetch_shape(-1, two) == -1000
    n, ms = ctypes.c_int(), ctypes.c_double()
    rec = (ctypes.c_uint32 * 32)()
    # Refused before anything touches a device: a bad mask, bad rounds, injected parts beyond the mask's range.
    assert lib.lib.xs_fetch_sweep(0, 1, 0, 0, 1, -1, -1, 0, rec, ctypes.byref(n), ctypes.byref(ms)) == -1000
    assert lib.lib.xs_fetch_sweep(0, 1, 0x3F, 0, 1, -1, -1, 0, rec, ctypes.byref(n), ctypes.byref(ms)) == -1000
    assert lib.lib.xs_fetch_sweep(0, 1, 1, 0, 0, -1, -1, 0, rec, ctypes.byref(n), ctypes.byref(ms)) == -1000
    assert lib.lib.xs_fetch_sweep(0, 1, 1, 0, 1, -1, -1, 0x20, rec, ctypes.byref(n), ctypes.byref(ms)) == -1000
    assert lib.lib.xs_fetch_sweep(0, 1, 1, 0, 1, -2, -1, 0, rec, ctypes.byref(n), ctypes.byref(ms)) == -1000
    assert lib.lib.xs_fetch_sweep(0, 1, 1, 0, 1, -1, -2, 0, rec, ctypes.byref(n), ctypes.byref(ms)) == -1000
    # The probe: no part, a part beyond the five, the timing bit with a part, a size that is not the parts' rows.
    assert lib.lib.xs_fetch_probe(0, 0, 0, 1, rec, 32) == -1000
    assert lib.lib.xs_fetch_probe(0, 0x40, 0, 1, rec, 32) == -1000
    assert lib.lib.xs_fetch_probe(0, 0x21, 0, 1, rec, 32) == -1000
    assert lib.lib.xs_fetch_probe(0, 0x10, 0, 1, rec, 32) == -1000
    assert lib.lib.xs_fetch_probe(0, 0x10, 0, 0, rec, 512) == -1000


# ---------------------------------------------------------------- the row
def test_the_row_stands_beside_the_table():
    assert list(PART_SWEEPS) == ["matrix", "lane", "valu", "mem"] and FETCH_SWEEP not in PART_SWEEPS.values()
    assert (FETCH_SWEEP.prefix, FETCH_SWEEP.names_symbol, FETCH_SWEEP.noun) == ("fetch", "xs_fetch_parts", "fetch part")
    assert (FETCH_SWEEP.summary_key, FETCH_SWEEP.selection) == ("failed_parts", "parts")
    # PartRecordHead<5>: four words, five counts, five digests, bad_simds.
    assert (FETCH_SWEEP.record_words, FETCH_SWEEP.bad, FETCH_SWEEP.digests, FETCH_SWEEP.bad_simds) == (32, 4, 9, 14)
    assert FETCH_SWEEP.step_mask is None
    assert (hip_probe.FETCH_RECORD_WORDS, hip_probe.FETCH_BLOCK, hip_probe.FETCH_SEED) == (32, ref.BLOCK, SEEDS[0])
    assert hip_probe.FETCH_ROUNDS in (1, 2, 4, 8, 16, 32, 64)


def test_decode_part_record_over_the_row():
    w = [0] * 32
    w[0:4] = [5, 0x21, 0xF, 0]
    w[4:9] = [0, 0, 1, 0, 0]
    w[9:14] = [100 + i for i in range(5)]
    w[14] = 4
    expected = {f: 100 + i for i, f in enumerate(PARTS)}
    r = decode_part_record(FETCH_SWEEP, PARTS, w, expected)
    assert (r["xcd"], r["cu"], r["simd_mask"], r["bad_simds"]) == (5, 0x21, 0xF, 4)
    assert r["bad"] == {f: int(f == "call") for f in PARTS} and r["digests"] == expected
    assert r["fail"] == 0 and "bad_steps" not in r
    assert decode_part_record(FETCH_SWEEP, PARTS, w, {**expected, "refill": 1})["fail"] == bits("refill")
    w2 = list(w)
    w2[9:14] = [0, 101, 0, 0, 104]
    assert decode_part_record(FETCH_SWEEP, PARTS, w2, {"loop": 101, "refill": 104})["fail"] == 0
    assert decode_part_record(FETCH_SWEEP, PARTS, w2, {"loop": 101})["fail"] == bits("refill")
    w3 = list(w)
    w3[3] = bits("stream")  # the device's own verdict stays
    assert decode_part_record(FETCH_SWEEP, PARTS, w3, expected)["fail"] == bits("stream")


# --------------------------------------------------- summarize_fetch_sweep
def test_summarize_clean():
    s = summarize_fetch_sweep(records(), 256, PARTS)
    assert s["covered"] and s["bad_xcds"] == [] and s["failed_parts"] == []
    assert all(v["failed_parts"] == [] and v["failed_cus"] == [] for v in s["xcds"].values())
    plain = summarize_sweep(records(), 256)
    assert {k: v for k, v in s.items() if k not in ("failed_parts", "xcds")} == {k: v for k, v in plain.items()
                                                                                  if k != "xcds"}


def test_summarize_one_failed_part_on_one_xcd():
    s = summarize_fetch_sweep(records(fail={(5, 17): ["stream"]}), 256, PARTS)
    assert s["bad_xcds"] == [5] and s["covered"]
    assert s["xcds"][5]["failed_cus"] == [17] and s["xcds"][5]["failed_parts"] == ["stream"]
    assert all(v["failed_parts"] == [] for x, v in s["xcds"].items() if x != 5)
    assert s["failed_parts"] == ["stream"]
    s = summarize_fetch_sweep(records(fail={(5, 17): ["refill"], (5, 3): ["loop", "align"], (2, 0): ["call"]}),
                              256, PARTS)
    assert s["bad_xcds"] == [2, 5] and s["xcds"][5]["failed_parts"] == ["loop", "align", "refill"]
    assert s["failed_parts"] == ["loop", "call", "align", "refill"]


def test_summarize_uncovered_is_not_failed():
    s = summarize_fetch_sweep(records(skip={(6, 0), (6, 9)}), 256, PARTS)
    assert not s["covered"] and s["uncovered"][6] == 2 and s["cus_seen"] == 254
    assert s["bad_xcds"] == [] and s["failed_parts"] == []


# ------------------------------------------------------------ hip_health_fn
class FakeProbe:
    def __init__(self, cus=256, cu_bad=(), fetch_fail=None, fetch_skip=(), mem_fail=None, consensus_fail=None):
        self.cus, self.cu_bad = cus, cu_bad
        self.fetch_fail, self.fetch_skip = fetch_fail or {}, fetch_skip
        self.mem_fail, self.consensus_fail = mem_fail or {}, consensus_fail or {}
        self.order, self.fetch_calls = [], []

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

    def consensus_sweep(self, dev, parts=None, **kw):
        import consensus_sweep_ref

        self.order.append("consensus")
        names = consensus_sweep_ref.PARTS
        recs = [{"xcd": x, "cu": c, "simd_mask": 15,
                 "fail": sum(1 << names.index(n) for n in self.consensus_fail.get(x, ())) if c == 4 else 0}
                for x in range(self._xcds()) for c in range(32)]
        s = hip_probe._name_fail_bits(summarize_sweep(recs, self.cus), "failed_parts", names)
        s.update(rounds=1, ms=1.9, blocks=4 * self.cus, seed=0, parts=parts or names, undecided=[])
        return {"records": recs, "summary": s}

    def fetch_sweep(self, dev, parts=None, **kw):
        self.order.append("fetch")
        self.fetch_calls.append({"parts": parts, **kw})
        recs = records(self._xcds(), fail={(x, 4): f for x, f in self.fetch_fail.items()}, skip=self.fetch_skip)
        s = summarize_fetch_sweep(recs, self.cus, PARTS)
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
    k = FETCH_SWEEP_KIND
    assert k not in SWEEP_KINDS
    assert (k.enabled_by, k.method, k.label, k.summary_key, k.selection, k.faults_key) == (
        "fetch", "fetch_sweep", "fetch", "fetchSweep", "parts", "fetchFaults")
    assert k.fault_of({"failed_parts": ("stream",)}) == ["stream"]
    f = FAULT_KINDS["fetchFaults"]
    assert not f.per_xcd and not f.withholds_gpu


def test_health_fn_default_runs_no_fetch_sweep(fake):
    f = fake()
    assert hip_health_fn()(0) is True
    assert hip_health_fn(sweep=True)(0)
    assert f.fetch_calls == [] and f.order == ["cu"]


def test_health_fn_fetch_sweep_alone_and_its_arguments(fake):
    f = fake(fetch_fail={3: ["stream"]})
    v = hip_health_fn(fetch=True, fetch_parts=["stream", "call"], fetch_args={"blocks": 64, "rounds": 4})(0)
    assert isinstance(v, GpuHealth) and not v.ok
    assert v.bad_xcds == frozenset({3}) and v.detail["fetchFaults"] == {3: ["stream"]}
    assert v.detail["fetchSweep"]["parts"] == ["stream", "call"]
    assert f.order == ["fetch"] and f.fetch_calls == [{"parts": ["stream", "call"], "blocks": 64, "rounds": 4}]
    ok = fake()
    v = hip_health_fn(fetch=True)(0)
    assert isinstance(v, GpuHealth) and v.ok and v and v.detail["fetchFaults"] == {}
    assert ok.fetch_calls == [{"parts": None}]


def test_health_fn_runs_it_after_the_consensus_sweep_and_before_the_memory_sweep(fake):
    f = fake(cu_bad=(1,), consensus_fail={6: ["div"]}, fetch_fail={3: ["loop"], 6: ["align", "refill"]},
             mem_fail={7: ["l2"]})
    v = hip_health_fn(mem=True, fetch=True, consensus=True, sweep=True)(0)
    assert f.order == ["cu", "consensus", "fetch", "mem"]
    assert isinstance(v, GpuHealth) and not v.ok and not v
    assert v.bad_xcds == frozenset({1, 3, 6, 7})
    assert v.detail["fetchFaults"] == {3: ["loop"], 6: ["align", "refill"]}
    assert v.detail["consensusFaults"] == {6: ["div"]} and v.detail["memFaults"] == {7: ["l2"]}
    assert v.detail["fetchSweep"]["bad_xcds"] == [3, 6]
    assert len({MEM_SWEEP_KIND, CONSENSUS_SWEEP_KIND, FETCH_SWEEP_KIND}) == 3


def test_health_fn_uncovered_cus_do_not_fail_the_device(fake):
    fake(fetch_skip={(4, 7)})
    v = hip_health_fn(fetch=True)(0)
    assert isinstance(v, GpuHealth) and v.ok and v
    assert not v.detail["fetchSweep"]["covered"] and v.detail["fetchFaults"] == {}


def test_health_fn_on_a_partition_device_returns_a_bool(fake):
    fake(cus=64, fetch_fail={1: ["call"]})
    assert hip_health_fn(fetch=True)(0) is False
    fake(cus=64)
    assert hip_health_fn(fetch=True)(0) is True


# --------------------------------------------------------------- node agent
def agent_on(store, host, health_fn):
    agent = NodeAgent(LocalClient(store), "n", host_fn=lambda: host, publish_metrics=False, health_fn=health_fn)
    agent.sync()
    return agent


def topo_of(store) -> dict:
    return json.loads(store.get("nodes", "", "n")["metadata"]["annotations"][TOPOLOGY_ANNOTATION])


def test_agent_publishes_fetch_faults_and_fences_the_partition(store):
    def health(dev):
        return GpuHealth(False, {5}, {"fetchFaults": {5: ["stream", "refill"]}, "valuFaults": {5: ["int"]}}) \
            if dev == 0 else True

    agent = agent_on(store, fake_host(2, "CPX"), health)
    topo = topo_of(store)
    assert topo["xcdFaults"] == {"0": [5]} and topo["unhealthy"] == []
    assert topo["fetchFaults"] == {"0": {"5": ["stream", "refill"]}}
    assert topo["valuFaults"] == {"0": {"5": ["int"]}}
    assert agent.faults["fetchFaults"] == {0: {5: ["stream", "refill"]}} and agent.unhealthy_xcds == {0: {5}}
    assert store.get("nodes", "", "n")["status"]["allocatable"][GPU_XCD] == "15"  # only XCD 5's partition is fenced


def test_agent_fences_from_an_injected_fault_through_the_health_fn(store, fake):
    fake(fetch_fail={6: ["align"]})
    agent_on(store, fake_host(1, "DPX"), hip_health_fn(fetch=True, fetch_args={"inject": (6, None, ["align"])}))
    assert topo_of(store)["fetchFaults"] == {"0": {"6": ["align"]}} and topo_of(store)["xcdFaults"] == {"0": [6]}
    assert store.get("nodes", "", "n")["status"]["allocatable"][GPU_XCD] == "4"  # the partition of XCDs 4-7


def test_agent_omits_the_key_when_there_is_none_and_resyncs_when_it_changes(store, fake):
    fake()
    agent_on(store, fake_host(2, "CPX"), hip_health_fn(fetch=True))  # a clean sweep: an empty fault dict
    assert "fetchFaults" not in topo_of(store) and "xcdFaults" not in topo_of(store)
    verdict = {"v": GpuHealth(False, {5}, {"fetchFaults": {5: ["call"]}})}
    agent = agent_on(store, fake_host(1, "CPX"), lambda dev: verdict["v"])
    assert topo_of(store)["fetchFaults"] == {"0": {"5": ["call"]}}
    verdict["v"] = GpuHealth(False, {5}, {"fetchFaults": {5: ["call", "loop"]}})
    agent._heartbeat_and_resync()
    assert topo_of(store)["fetchFaults"] == {"0": {"5": ["call", "loop"]}}
    assert topo_of(store)["xcdFaults"] == {"0": [5]}


# ---------------------------------------------------------------------- CLI
def test_cli_parses_the_fetch_sweep_flag():
    ap = build_parser()
    none = ap.parse_args(["node-agent"])
    assert none.health_fetch_sweep is None and not wants_health_fn(none)
    assert "fetch" not in health_fn_args(none) and "fetch_parts" not in health_fn_args(none)
    base = {"sweep": False, "sweep_period_s": 600.0, "matrix": False, "matrix_formats": None}
    on = ap.parse_args(["node-agent", "--health-fetch-sweep"])
    assert health_fn_args(on) == {**base, "fetch": True, "fetch_parts": None} and wants_health_fn(on)
    every_part = ap.parse_args(["node-agent", "--health-fetch-sweep", "all"])
    assert health_fn_args(every_part) == {**base, "fetch": True, "fetch_parts": None}
    some = ap.parse_args(["node-agent", "--health-fetch-sweep", "stream, refill"])
    assert health_fn_args(some) == {**base, "fetch": True, "fetch_parts": ["stream", "refill"]}
    every = ap.parse_args(["node-agent", "--health-fetch-sweep", "call", "--health-mem-sweep", "l1", "--health-sweep",
                           "--health-consensus-sweep", "--health-sweep-period", "30"])
    assert health_fn_args(every) == {"sweep": True, "sweep_period_s": 30.0, "matrix": False, "matrix_formats": None,
                                     "consensus": True, "consensus_parts": None, "fetch": True, "fetch_parts": ["call"],
                                     "mem": True, "mem_routes": ["l1"]}
    hip_health_fn_keywords = hip_health_fn.__code__.co_varnames[:hip_health_fn.__code__.co_argcount]
    assert set(health_fn_args(every)) <= set(hip_health_fn_keywords)


def test_an_unknown_part_is_refused_where_the_sweep_reads_the_list(lib):
    some = build_parser().parse_args(["node-agent", "--health-fetch-sweep", "stream,decode"])
    assert health_fn_args(some)["fetch_parts"] == ["stream", "decode"]
    with pytest.raises(ValueError, match="unknown fetch part 'decode'"):
        lib.fetch_sweep(0, parts=health_fn_args(some)["fetch_parts"])  # refused before anything touches a device
