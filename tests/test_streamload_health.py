"""The stream load sweep off the GPU: the host's operands and digests against
the independent reference (tests/streamload_sweep_ref.py), the refusals of the
C ABI, and the node agent publishing `streamLoadFaults` behind the attention
load sweep."""
import ctypes
import json

import pytest

import streamload_sweep_ref as ref
from flex_gpu_scheduler_amd.cli import build_parser, health_fn_args
from flex_gpu_scheduler_amd.control import LocalClient
from flex_gpu_scheduler_amd.control.node_agent import NodeAgent, hip_health_fn
from flex_gpu_scheduler_amd.gpu.discovery import fake_host
from flex_gpu_scheduler_amd.models import TOPOLOGY_ANNOTATION
from flex_gpu_scheduler_amd.ops import hip_probe
from flex_gpu_scheduler_amd.ops.hip_probe import STREAMLOAD_DEPTH as D
from flex_gpu_scheduler_amd.ops.hip_probe import STREAMLOAD_LAPS, summarize_load_sweep

SEEDS = (hip_probe.STREAMLOAD_SEED, 0x9E3779B9)
# (ksteps, panels, laps) of the GPU test (tests/test_gpu_streamload_sweep.py).
GPU_SHAPES = ((1, 8, 1), (D - 1, 8, 2), (D + 1, 24, 7), (2 * D + 3, 16, 5), (64, 8, 1))


@pytest.fixture(scope="module")
def lib():
    # No skip: a _hipstreamload.so that is missing or does not load is a failure of these tests.
    return hip_probe.HipProbe()


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("ksteps,panels,laps", GPU_SHAPES)
def test_operands_and_digests_equal_the_reference(lib, ksteps, panels, laps, seed):
    for panel in (0, panels - 1):
        got, want = lib.streamload_operands(seed, panel, ksteps), ref.operands(seed, panel, ksteps)
        assert all(g.shape == (16, 64 * ksteps) and (g == w).all() for g, w in zip(got, want))
    want = ref.digests(seed, laps, ksteps, panels)
    assert lib.streamload_parts() == ref.PARTS and len(set(want.values())) == 3
    assert ref.digests(seed, laps, ksteps, panels, g=5) == want  # whichever workgroup: what the record's compare needs
    assert lib.streamload_sweep_expected(None, seed, laps, ksteps, panels) == want
    # A part outside the mask is not reported, and its word is 0.
    out = (ctypes.c_uint32 * 3)(7, 7, 7)
    assert lib.lib.xs_streamload_sweep_expected(4, seed, laps, ksteps, panels, out) == 0
    assert list(out) == [0, 0, want["gemm"]]


def test_the_hash_reaches_minus_128_and_every_byte(lib):
    wt, x = lib.streamload_operands(ksteps=64)
    assert set(wt.ravel()) == set(x.ravel()) == set(range(-128, 128))


def test_host_refuses_bad_arguments(lib):
    L = lib.lib
    out, two = (ctypes.c_uint32 * 3)(), (ctypes.c_int * 2)()
    rec, n, ms = (ctypes.c_uint32 * 32)(), ctypes.c_int(), ctypes.c_double()

    def sweep(mask=7, laps=1, ksteps=1, panels=8, blocks=1, ix=-1, ic=-1, im=0, records=rec):
        return L.xs_streamload_sweep(0, blocks, mask, 0, laps, ksteps, panels, ix, ic, im, records, ctypes.byref(n),
                                     ctypes.byref(ms))

    def probe(mask=7, laps=1, ksteps=1, panels=8, words=2048 + 1024, buf=rec):
        return L.xs_streamload_probe(0, mask, 0, laps, ksteps, panels, buf, words)

    def expected(mask=7, laps=1, ksteps=1, panels=8, buf=out):
        return L.xs_streamload_sweep_expected(mask, 0, laps, ksteps, panels, buf)

    # Every one is refused before anything touches a device or generates an arena.
    cap = 16 * STREAMLOAD_LAPS
    shapes = [dict(laps=0), dict(laps=cap + 1), dict(ksteps=0), dict(ksteps=65), dict(panels=0), dict(panels=4),
              dict(panels=12), dict(ksteps=64, panels=(1 << 14) + 8), dict(ksteps=1, panels=(1 << 20) + 8)]
    refused = [f(**kw) for kw in shapes + [dict(mask=0), dict(mask=8)] for f in (sweep, probe, expected)]
    refused += [sweep(im=8), sweep(ix=-2), sweep(ic=-2), sweep(blocks=-1), sweep(records=None), probe(words=2048),
                probe(buf=None), expected(buf=None), L.xs_streamload_shape(3, two), L.xs_streamload_shape(-1, two),
                L.xs_streamload_shape(0, None), L.xs_streamload_operands(0, 0, 0, rec, rec),
                L.xs_streamload_operands(0, 0, 65, rec, rec), L.xs_streamload_operands(0, 1 << 20, 1, rec, rec),
                L.xs_streamload_operands(0, 0, 1, rec, None)]
    assert refused == [hip_probe.BAD_ARGS] * len(refused)
    assert lib.streamload_shape("gemm", 3) == {"fixed_words": 0, "words_per_lap": 2048, "words": 3 * 2048}
    assert lib.streamload_shape("stage") == {"fixed_words": 512, "words_per_lap": 0, "words": 512}


class FakeProbe:
    """hip_health_fn's probe with the attention and stream load sweeps only; `bad_xcd` fails `gemm` of the latter."""

    def __init__(self, bad_xcd):
        self.order, self.bad_xcd = [], bad_xcd

    def props(self, dev):
        return {"computeUnits": 256}

    def health(self, dev):
        return {"healthy": True}

    mfma_check = health

    def _sweep(self, name, names, bad_xcd, **kw):
        self.order.append((name, kw))
        recs = [{"xcd": x, "cu": c, "simd_mask": 15, "fail": 4 if (x, c) == (bad_xcd, 4) else 0}
                for x in range(8) for c in range(32)]
        return {"records": recs, "summary": {**summarize_load_sweep(recs, 256, names), "rounds": 1, "ms": 40.0,
                                             "blocks": 1024, "seed": 0, "parts": names}}

    def attnload_sweep(self, dev, parts=None, **kw):
        return self._sweep("attnload", ["stage", "score", "stat", "transpose", "out"], None, **kw)

    def streamload_sweep(self, dev, parts=None, **kw):
        return self._sweep("streamload", ref.PARTS, self.bad_xcd, parts=parts, **kw)


def test_agent_runs_it_last_publishes_stream_load_faults_and_drops_them(store, monkeypatch):
    f = FakeProbe(5)
    monkeypatch.setattr(hip_probe, "probe", lambda: f)
    args = build_parser().parse_args(["node-agent", "--health-streamload-sweep", "gemm, stage", "--health-attnload-sweep",
                                      "--health-streamload-sweep-laps", "64", "--health-sweep-period", "0"])
    kw = health_fn_args(args)
    assert (kw["streamload"], kw["streamload_parts"], kw["streamload_args"]) == (True, ["gemm", "stage"], {"laps": 64})
    assert "streamload" not in health_fn_args(build_parser().parse_args(["node-agent"]))  # off by default
    agent = NodeAgent(LocalClient(store), "n", host_fn=lambda: fake_host(1, "DPX"), publish_metrics=False,
                      health_fn=hip_health_fn(**kw))

    def topology():
        agent.sync()
        return json.loads(store.get("nodes", "", "n")["metadata"]["annotations"][TOPOLOGY_ANNOTATION])

    topo = topology()
    assert f.order == [("attnload", {}), ("streamload", {"parts": ["gemm", "stage"], "laps": 64})]
    assert topo["streamLoadFaults"] == {"0": {"5": ["gemm"]}} and topo["xcdFaults"] == {"0": [5]}
    f.bad_xcd = None  # the fault clears
    topo = topology()
    assert "streamLoadFaults" not in topo and "xcdFaults" not in topo
