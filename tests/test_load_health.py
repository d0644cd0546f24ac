"""The load sweep off the GPU: the host's operands and digests against the
independent reference, the refusals of the C ABI, its verdict
(summarize_load_sweep, decode_part_record over the LOAD_SWEEP row) and the node
agent publishing `loadFaults` next to `xcdFaults`, with the node-agent flags."""
import ctypes
import json

import pytest

import load_sweep_ref as ref
from flex_gpu_scheduler_amd.cli import build_parser, health_fn_args, wants_health_fn
from flex_gpu_scheduler_amd.control import LocalClient
from flex_gpu_scheduler_amd.control.node_agent import FAULT_KINDS, LOAD_SWEEP_KIND, GpuHealth, NodeAgent, hip_health_fn
from flex_gpu_scheduler_amd.gpu.discovery import fake_host
from flex_gpu_scheduler_amd.models import GPU_XCD, TOPOLOGY_ANNOTATION
from flex_gpu_scheduler_amd.ops import hip_probe
from flex_gpu_scheduler_amd.ops.hip_probe import (LOAD_KSTEPS, LOAD_LAPS, LOAD_SETS, LOAD_SWEEP, decode_part_record,
                                                  load_record_tail, summarize_load_sweep)

PARTS = ref.PARTS
SEEDS = (hip_probe.LOAD_SEED, 0x9E3779B9)


@pytest.fixture(scope="module")
def lib():
    # No skip: a _hipload.so that is missing or does not load is a failure of these tests.
    return hip_probe.HipProbe()


@pytest.mark.parametrize("ksteps", (1, 3))
@pytest.mark.parametrize("set_", (0, 7))
@pytest.mark.parametrize("seed", SEEDS)
def test_operands_are_bit_equal_to_the_reference(lib, seed, set_, ksteps):
    a, bt = lib.load_operands(seed, set_, ksteps)
    want_a, want_bt = ref.operands(seed, set_, ksteps)
    assert a.shape == (128, 64 * ksteps) and bt.shape == (256, 64 * ksteps)
    assert (a == want_a).all() and (bt == want_bt).all()
    assert (bt == -128).any() and (bt == 127).any()  # the whole range of a byte is in use


@pytest.mark.parametrize("laps", (1, 9))
def test_host_digests_equal_the_reference_at_the_sweeps_shape(lib, laps):
    want = ref.digests(SEEDS[0], laps, LOAD_KSTEPS, LOAD_SETS)
    assert lib.load_parts() == PARTS and len(set(want.values())) == 4
    assert lib.load_sweep_expected(seed=SEEDS[0], laps=laps) == want
    assert lib.load_sweep_expected(["valu", "stage"], SEEDS[0], laps) == {f: want[f] for f in ("stage", "valu")}


def test_host_refuses_bad_arguments(lib):
    L = lib.lib
    out, two = (ctypes.c_uint32 * 4)(), (ctypes.c_int * 2)()
    rec, n, ms = (ctypes.c_uint32 * 32)(), ctypes.c_int(), ctypes.c_double()

    def sweep(mask=15, laps=1, blocks=1, ix=-1, ic=-1, im=0):
        return L.xs_load_sweep(0, blocks, mask, 0, laps, ix, ic, im, rec, ctypes.byref(n), ctypes.byref(ms))

    def probe(mask=15, laps=1, ksteps=1, sets=1, words=32768 + 1536):
        return L.xs_load_probe(0, mask, 0, laps, ksteps, sets, rec, words)

    # Every one is refused before anything touches a device or builds a set.
    cap = 16 * LOAD_LAPS
    refused = [sweep(mask=0), sweep(mask=16), sweep(laps=0), sweep(laps=cap + 1), sweep(im=16), sweep(ix=-2),
               sweep(ic=-2), sweep(blocks=-1), probe(mask=0), probe(laps=0), probe(laps=cap + 1), probe(ksteps=0),
               probe(ksteps=1025), probe(sets=0), probe(sets=65), probe(words=32768),
               L.xs_load_sweep_expected(0, 0, 1, out), L.xs_load_sweep_expected(15, 0, 0, out),
               L.xs_load_sweep_expected(15, 0, cap + 1, out), L.xs_load_sweep_expected(15, 0, 1, None),
               L.xs_load_shape(4, two), L.xs_load_shape(-1, two), L.xs_load_operands(0, 64, 1, rec, rec),
               L.xs_load_operands(0, 0, 1025, rec, rec), L.xs_load_operands(0, 0, 1, None, rec)]
    assert refused == [hip_probe.BAD_ARGS] * len(refused)
    assert lib.load_shape("gemm", 3) == {"fixed_words": 0, "words_per_lap": 32768, "words": 3 * 32768}
    assert lib.load_shape("lds") == {"fixed_words": 512, "words_per_lap": 0, "words": 512}


# ------------------------------------------------------- record and summary
def record_words(xcd, cu, fail=0, bad=(0, 0, 0, 0), digests=(100, 101, 102, 103), masks=(0, 0, 0)):
    w = [0] * 32
    w[0:4] = [xcd, cu, 0xF, fail]
    w[4:8], w[8:12], w[12] = list(bad), list(digests), 2 if any(bad) else 0
    w[14:17] = list(masks)
    return w


def decoded(w, expected=None):
    expected = expected or {f: 100 + i for i, f in enumerate(PARTS)}
    return {**decode_part_record(LOAD_SWEEP, PARTS, w, expected), **load_record_tail(w)}


def test_decode_part_record_over_the_row():
    assert (LOAD_SWEEP.prefix, LOAD_SWEEP.names_symbol, LOAD_SWEEP.summary_key) == ("load", "xs_load_parts", "failed_parts")
    r = decoded(record_words(5, 0x21, fail=4, bad=(0, 0, 3, 0), masks=(0x81, 0x4, 1 << 31)))
    assert (r["xcd"], r["cu"], r["simd_mask"], r["fail"], r["bad_simds"]) == (5, 0x21, 0xF, 4, 2)
    assert r["bad"] == {"stage": 0, "lds": 0, "gemm": 3, "valu": 0}
    assert (r["bad_subtiles"], r["bad_sets"], r["bad_spans"]) == (0x81, 0x4, 1 << 31)
    # A digest that is not the host's fails its part, whatever the device said.
    assert decoded(record_words(0, 0, digests=(100, 7, 102, 103)))["fail"] == 2
    assert decoded(record_words(0, 0, digests=(0, 0, 102, 0)), {"gemm": 102})["fail"] == 0


def test_summarize_names_the_parts_and_the_late_only_cus():
    recs = [decoded(record_words(x, c)) for x in range(8) for c in range(32)]
    s = summarize_load_sweep(recs, 256, PARTS)
    assert s["covered"] and s["bad_xcds"] == [] and s["failed_parts"] == [] and s["late_only"] == {}
    recs[3 * 32 + 4] = decoded(record_words(3, 4, fail=4, bad=(0, 0, 9, 0), masks=(1, 1, 0xC0000000)))  # late only
    recs[3 * 32 + 5] = decoded(record_words(3, 5, fail=6, bad=(0, 0, 1, 0), masks=(2, 2, 0x80000001)))  # early too
    recs[6 * 32] = decoded(record_words(6, 0, fail=1, bad=(1, 0, 0, 0)))  # no gemm mismatch: no span
    s = summarize_load_sweep(recs, 256, PARTS)
    assert s["bad_xcds"] == [3, 6] and s["xcds"][3]["failed_cus"] == [4, 5]
    assert s["xcds"][3]["failed_parts"] == ["lds", "gemm"] and s["xcds"][6]["failed_parts"] == ["stage"]
    assert s["failed_parts"] == ["stage", "lds", "gemm"] and s["late_only"] == {3: [4]}


# --------------------------------------------------------------- node agent
class FakeProbe:
    """hip_health_fn's probe with a load sweep and a memory sweep only."""

    def __init__(self, load_fail=None):
        self.load_fail, self.order, self.load_calls = load_fail or {}, [], []

    def props(self, dev):
        return {"computeUnits": 256}

    def health(self, dev):
        return {"healthy": True}

    mfma_check = health

    def _sweep(self, name, names, fail, summarize, **kw):
        self.order.append(name)
        recs = [{"xcd": x, "cu": c, "simd_mask": 15,
                 "fail": sum(1 << names.index(f) for f in fail.get(x, ())) if c == 4 else 0}
                for x in range(8) for c in range(32)]
        s = summarize(recs, 256, names)
        s.update(rounds=1, ms=40.0, blocks=1024, seed=0, **kw)
        return {"records": recs, "summary": s}

    def load_sweep(self, dev, parts=None, **kw):
        self.load_calls.append({"parts": parts, **kw})
        return self._sweep("load", PARTS, self.load_fail, summarize_load_sweep, parts=parts or PARTS)

    def mem_sweep(self, dev, routes=None, **kw):
        return self._sweep("mem", ["l1", "l2"], {}, hip_probe.summarize_mem_sweep, routes=routes or ["l1", "l2"])


@pytest.fixture
def fake(monkeypatch):
    def install(**kw):
        f = FakeProbe(**kw)
        monkeypatch.setattr(hip_probe, "probe", lambda: f)
        return f
    return install


def topo_of(store) -> dict:
    return json.loads(store.get("nodes", "", "n")["metadata"]["annotations"][TOPOLOGY_ANNOTATION])


def test_health_fn_runs_the_load_sweep_last_with_its_arguments(fake):
    k = LOAD_SWEEP_KIND
    assert (k.enabled_by, k.method, k.summary_key, k.selection, k.faults_key) == (
        "load", "load_sweep", "loadSweep", "parts", "loadFaults")
    assert not FAULT_KINDS["loadFaults"].per_xcd and not FAULT_KINDS["loadFaults"].withholds_gpu
    f = fake(load_fail={3: ["gemm"]})
    v = hip_health_fn(load=True, load_parts=["gemm", "valu"], load_args={"laps": 64}, mem=True)(0)
    assert f.order == ["mem", "load"] and f.load_calls == [{"parts": ["gemm", "valu"], "laps": 64}]
    assert isinstance(v, GpuHealth) and not v.ok and v.bad_xcds == frozenset({3})
    assert v.detail["loadFaults"] == {3: ["gemm"]} and v.detail["loadSweep"]["late_only"] == {}
    fake()
    v = hip_health_fn(load=True)(0)
    assert isinstance(v, GpuHealth) and v.ok and v.detail["loadFaults"] == {}


def test_agent_publishes_load_faults_and_fences_the_xcd(store, fake):
    fake(load_fail={6: ["lds", "gemm"]})
    agent = NodeAgent(LocalClient(store), "n", host_fn=lambda: fake_host(1, "DPX"), publish_metrics=False,
                      health_fn=hip_health_fn(load=True))
    agent.sync()
    topo = topo_of(store)
    assert topo["loadFaults"] == {"0": {"6": ["lds", "gemm"]}} and topo["xcdFaults"] == {"0": [6]}
    assert store.get("nodes", "", "n")["status"]["allocatable"][GPU_XCD] == "4"  # the partition of XCDs 4-7
    fake()
    agent = NodeAgent(LocalClient(store), "n", host_fn=lambda: fake_host(1, "DPX"), publish_metrics=False,
                      health_fn=hip_health_fn(load=True))
    agent.sync()
    assert "loadFaults" not in topo_of(store) and "xcdFaults" not in topo_of(store)


def test_cli_parses_the_load_sweep_flags():
    ap = build_parser()
    none = ap.parse_args(["node-agent", "--health-load-sweep-laps", "8"])
    assert not wants_health_fn(none) and "load" not in health_fn_args(none) and "load_args" not in health_fn_args(none)
    base = {"sweep": False, "sweep_period_s": 600.0, "matrix": False, "matrix_formats": None}
    on = ap.parse_args(["node-agent", "--health-load-sweep"])
    assert health_fn_args(on) == {**base, "load": True, "load_parts": None} and wants_health_fn(on)
    some = ap.parse_args(["node-agent", "--health-load-sweep", "gemm, lds", "--health-load-sweep-laps", "64"])
    assert health_fn_args(some) == {**base, "load": True, "load_parts": ["gemm", "lds"], "load_args": {"laps": 64}}
    keywords = hip_health_fn.__code__.co_varnames[:hip_health_fn.__code__.co_argcount]
    assert set(health_fn_args(some)) <= set(keywords)
