"""The bf16 load sweep off the GPU: the host's operands and digests against the
independent reference (tests/bfload_sweep_ref.py), the refusals of the C ABI,
and the node agent publishing `bfLoadFaults` behind the MX load sweep."""
import ctypes
import json

import pytest

import bfload_sweep_ref as ref
from flex_gpu_scheduler_amd.cli import build_parser, health_fn_args
from flex_gpu_scheduler_amd.control import LocalClient
from flex_gpu_scheduler_amd.control.node_agent import NodeAgent, hip_health_fn
from flex_gpu_scheduler_amd.gpu.discovery import fake_host
from flex_gpu_scheduler_amd.models import TOPOLOGY_ANNOTATION
from flex_gpu_scheduler_amd.ops import hip_probe
from flex_gpu_scheduler_amd.ops.hip_probe import BFLOAD_KSTEPS, BFLOAD_LAPS, BFLOAD_SETS, summarize_load_sweep

SEEDS = (hip_probe.BFLOAD_SEED, 0x9E3779B9)


@pytest.fixture(scope="module")
def lib():
    # No skip: a _hipbfload.so that is missing or does not load is a failure of these tests.
    return hip_probe.HipProbe()


@pytest.mark.parametrize("ksteps", (1, 3))
@pytest.mark.parametrize("set_", (0, 2))
@pytest.mark.parametrize("seed", SEEDS)
def test_operands_are_bit_equal_to_the_reference(lib, seed, set_, ksteps):
    got, want = lib.bfload_operands(seed, set_, ksteps), ref.operands(seed, set_, ksteps)
    assert [g.shape for g in got] == [(128, 32 * ksteps), (32 * ksteps, 256)]
    assert all((g == w).all() for g, w in zip(got, want))
    assert all((g & 0x7F80 == 0x3F80).all() for g in got)
    assert all(len(set((g & 0x807F).ravel())) == 256 for g in got)  # both signs, every mantissa


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("laps", (1, 33))
def test_host_digests_equal_the_reference_at_the_sweeps_shape(lib, laps, seed):
    assert (BFLOAD_KSTEPS, hip_probe.BFLOAD_MAX_KSTEPS, BFLOAD_SETS) == (8, 8, 32)
    want = ref.digests(seed, laps, BFLOAD_KSTEPS, BFLOAD_SETS)
    assert lib.bfload_parts() == ref.PARTS and len(set(want.values())) == 4
    assert lib.bfload_sweep_expected(seed=seed, laps=laps) == want
    # A part outside the mask is not reported, and its word is 0.
    assert lib.bfload_sweep_expected(["transpose"], seed, laps) == {"transpose": want["transpose"]}
    out = (ctypes.c_uint32 * 4)(7, 7, 7, 7)
    assert lib.lib.xs_bfload_sweep_expected(8, seed, laps, out) == 0 and list(out) == [0, 0, 0, want["gemm"]]


def test_host_refuses_bad_arguments(lib):
    L = lib.lib
    out, two = (ctypes.c_uint32 * 4)(), (ctypes.c_int * 2)()
    rec, n, ms = (ctypes.c_uint32 * 32)(), ctypes.c_int(), ctypes.c_double()

    def sweep(mask=15, laps=1, blocks=1, ix=-1, ic=-1, im=0):
        return L.xs_bfload_sweep(0, blocks, mask, 0, laps, ix, ic, im, rec, ctypes.byref(n), ctypes.byref(ms))

    def probe(mask=15, laps=1, ksteps=1, sets=1, words=32768 + 1536):
        return L.xs_bfload_probe(0, mask, 0, laps, ksteps, sets, rec, words)

    # Every one is refused before anything touches a device or builds a set.
    cap = 16 * BFLOAD_LAPS
    refused = [sweep(mask=0), sweep(mask=16), sweep(laps=0), sweep(laps=cap + 1), sweep(im=16), sweep(ix=-2),
               sweep(ic=-2), sweep(blocks=-1), probe(mask=0), probe(laps=0), probe(laps=cap + 1), probe(ksteps=0),
               probe(ksteps=9), probe(sets=0), probe(sets=65), probe(words=32768),
               L.xs_bfload_sweep_expected(0, 0, 1, out), L.xs_bfload_sweep_expected(15, 0, 0, out),
               L.xs_bfload_sweep_expected(15, 0, cap + 1, out), L.xs_bfload_sweep_expected(15, 0, 1, None),
               L.xs_bfload_shape(4, two), L.xs_bfload_shape(-1, two), L.xs_bfload_operands(0, 64, 1, rec, rec),
               L.xs_bfload_operands(0, 0, 9, rec, rec), L.xs_bfload_operands(0, 0, 1, rec, None)]
    assert refused == [hip_probe.BAD_ARGS] * len(refused)
    assert lib.bfload_shape("gemm", 3) == {"fixed_words": 0, "words_per_lap": 32768, "words": 3 * 32768}
    assert lib.bfload_shape("transpose") == {"fixed_words": 512, "words_per_lap": 0, "words": 512}


class FakeProbe:
    """hip_health_fn's probe with the MX and bf16 load sweeps only; XCD 5 fails `transpose` of the bf16 one."""

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

    def mxload_sweep(self, dev, parts=None, **kw):
        return self._sweep("mxload", ["operand", "scale", "gemm"], None, **kw)

    def bfload_sweep(self, dev, parts=None, **kw):
        return self._sweep("bfload", ref.PARTS, self.bad_xcd, parts=parts, **kw)


@pytest.mark.parametrize("bad_xcd", (5, None))
def test_agent_runs_it_last_and_publishes_bf_load_faults(store, monkeypatch, bad_xcd):
    f = FakeProbe(bad_xcd)
    monkeypatch.setattr(hip_probe, "probe", lambda: f)
    args = build_parser().parse_args(["node-agent", "--health-bfload-sweep", "gemm, transpose", "--health-mxload-sweep",
                                      "--health-bfload-sweep-laps", "64"])
    kw = health_fn_args(args)
    assert (kw["bfload"], kw["bfload_parts"], kw["bfload_args"]) == (True, ["gemm", "transpose"], {"laps": 64})
    assert "mxload_args" not in kw
    agent = NodeAgent(LocalClient(store), "n", host_fn=lambda: fake_host(1, "DPX"), publish_metrics=False,
                      health_fn=hip_health_fn(**kw))
    agent.sync()
    assert f.order == [("mxload", {}), ("bfload", {"parts": ["gemm", "transpose"], "laps": 64})]
    topo = json.loads(store.get("nodes", "", "n")["metadata"]["annotations"][TOPOLOGY_ANNOTATION])
    if bad_xcd is None:
        assert "bfLoadFaults" not in topo and "xcdFaults" not in topo
    else:
        assert topo["bfLoadFaults"] == {"0": {"5": ["transpose"]}} and topo["xcdFaults"] == {"0": [5]}
    assert "mxLoadFaults" not in topo
