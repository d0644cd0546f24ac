"""The MX load sweep off the GPU: the host's operands and digests against the
independent reference (tests/mxload_sweep_ref.py), the refusals of the C ABI,
and the node agent publishing `mxLoadFaults` behind the load sweep."""
import ctypes
import json

import pytest

import mxload_sweep_ref as ref
from flex_gpu_scheduler_amd.cli import build_parser, health_fn_args
from flex_gpu_scheduler_amd.control import LocalClient
from flex_gpu_scheduler_amd.control.node_agent import NodeAgent, hip_health_fn
from flex_gpu_scheduler_amd.gpu.discovery import fake_host
from flex_gpu_scheduler_amd.models import TOPOLOGY_ANNOTATION
from flex_gpu_scheduler_amd.ops import hip_probe
from flex_gpu_scheduler_amd.ops.hip_probe import MXLOAD_KSTEPS, MXLOAD_LAPS, MXLOAD_SETS, summarize_load_sweep

SEEDS = (hip_probe.MXLOAD_SEED, 0x9E3779B9)


@pytest.fixture(scope="module")
def lib():
    # No skip: a _hipmxload.so that is missing or does not load is a failure of these tests.
    return hip_probe.HipProbe()


@pytest.mark.parametrize("ksteps", (1, 3))
@pytest.mark.parametrize("set_", (0, 2))
@pytest.mark.parametrize("seed", SEEDS)
def test_operands_are_bit_equal_to_the_reference(lib, seed, set_, ksteps):
    got, want = lib.mxload_operands(seed, set_, ksteps), ref.operands(seed, set_, ksteps)
    assert [g.shape for g in got] == [(128, 64 * ksteps), (256, 64 * ksteps), (128, 4 * ksteps), (256, 4 * ksteps)]
    assert all((g == w).all() for g, w in zip(got, want))
    assert set(got[2].ravel()) == {126, 127, 128, 129} and set(got[3].ravel()) == {127, 128}


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("laps", (1, 9))
def test_host_digests_equal_the_reference_at_the_sweeps_shape(lib, laps, seed):
    want = ref.digests(seed, laps, MXLOAD_KSTEPS, MXLOAD_SETS)
    assert lib.mxload_parts() == ref.PARTS and len(set(want.values())) == 3
    assert lib.mxload_sweep_expected(seed=seed, laps=laps) == want
    # A part outside the mask is not reported, and its word is 0.
    assert lib.mxload_sweep_expected(["gemm"], seed, laps) == {"gemm": want["gemm"]}
    out = (ctypes.c_uint32 * 3)(7, 7, 7)
    assert lib.lib.xs_mxload_sweep_expected(4, seed, laps, out) == 0 and list(out) == [0, 0, want["gemm"]]


def test_host_refuses_bad_arguments(lib):
    L = lib.lib
    out, two = (ctypes.c_uint32 * 3)(), (ctypes.c_int * 2)()
    rec, n, ms = (ctypes.c_uint32 * 32)(), ctypes.c_int(), ctypes.c_double()

    def sweep(mask=7, laps=1, blocks=1, ix=-1, ic=-1, im=0):
        return L.xs_mxload_sweep(0, blocks, mask, 0, laps, ix, ic, im, rec, ctypes.byref(n), ctypes.byref(ms))

    def probe(mask=7, laps=1, ksteps=1, sets=1, words=32768 + 1024):
        return L.xs_mxload_probe(0, mask, 0, laps, ksteps, sets, rec, words)

    # Every one is refused before anything touches a device or builds a set.
    cap = 16 * MXLOAD_LAPS
    refused = [sweep(mask=0), sweep(mask=8), sweep(laps=0), sweep(laps=cap + 1), sweep(im=8), sweep(ix=-2),
               sweep(ic=-2), sweep(blocks=-1), probe(mask=0), probe(laps=0), probe(laps=cap + 1), probe(ksteps=0),
               probe(ksteps=57), probe(sets=0), probe(sets=65), probe(words=32768),
               L.xs_mxload_sweep_expected(0, 0, 1, out), L.xs_mxload_sweep_expected(7, 0, 0, out),
               L.xs_mxload_sweep_expected(7, 0, cap + 1, out), L.xs_mxload_sweep_expected(7, 0, 1, None),
               L.xs_mxload_shape(3, two), L.xs_mxload_shape(-1, two), L.xs_mxload_operands(0, 64, 1, rec, rec, rec, rec),
               L.xs_mxload_operands(0, 0, 57, rec, rec, rec, rec), L.xs_mxload_operands(0, 0, 1, rec, rec, None, rec)]
    assert refused == [hip_probe.BAD_ARGS] * len(refused)
    assert lib.mxload_shape("gemm", 3) == {"fixed_words": 0, "words_per_lap": 32768, "words": 3 * 32768}
    assert lib.mxload_shape("scale") == {"fixed_words": 512, "words_per_lap": 0, "words": 512}


class FakeProbe:
    """hip_health_fn's probe with the two load sweeps only; XCD 6 fails `gemm` of the MX one."""

    def __init__(self):
        self.order = []

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

    def load_sweep(self, dev, parts=None, **kw):
        return self._sweep("load", ["stage", "lds", "gemm", "valu"], None, **kw)

    def mxload_sweep(self, dev, parts=None, **kw):
        return self._sweep("mxload", ref.PARTS, 6, parts=parts, **kw)


def test_agent_runs_it_last_and_publishes_mx_load_faults(store, monkeypatch):
    f = FakeProbe()
    monkeypatch.setattr(hip_probe, "probe", lambda: f)
    args = build_parser().parse_args(["node-agent", "--health-load-sweep", "--health-mxload-sweep", "gemm, scale",
                                      "--health-mxload-sweep-laps", "64"])
    kw = health_fn_args(args)
    assert (kw["mxload"], kw["mxload_parts"], kw["mxload_args"]) == (True, ["gemm", "scale"], {"laps": 64})
    assert "load_args" not in kw
    agent = NodeAgent(LocalClient(store), "n", host_fn=lambda: fake_host(1, "DPX"), publish_metrics=False,
                      health_fn=hip_health_fn(**kw))
    agent.sync()
    assert f.order == [("load", {}), ("mxload", {"parts": ["gemm", "scale"], "laps": 64})]
    topo = json.loads(store.get("nodes", "", "n")["metadata"]["annotations"][TOPOLOGY_ANNOTATION])
    assert topo["mxLoadFaults"] == {"0": {"6": ["gemm"]}} and topo["xcdFaults"] == {"0": [6]}
    assert "loadFaults" not in topo
