"""The attention load sweep off the GPU: the host's operands and digests against
the independent reference (tests/attnload_sweep_ref.py), the refusals of the C
ABI, what the reference says of the test shapes, and the node agent publishing
`attnLoadFaults` behind the bf16 load sweep."""
import ctypes
import json

import numpy as np
import pytest

import attnload_sweep_ref as ref
from flex_gpu_scheduler_amd.cli import build_parser, health_fn_args
from flex_gpu_scheduler_amd.control import LocalClient
from flex_gpu_scheduler_amd.control.node_agent import NodeAgent, hip_health_fn
from flex_gpu_scheduler_amd.gpu.discovery import fake_host
from flex_gpu_scheduler_amd.models import TOPOLOGY_ANNOTATION
from flex_gpu_scheduler_amd.ops import hip_probe
from flex_gpu_scheduler_amd.ops.hip_probe import ATTNLOAD_KVSTEPS, ATTNLOAD_LAPS, ATTNLOAD_SETS, summarize_load_sweep

SEEDS = (hip_probe.ATTNLOAD_SEED, 0x9E3779B9)
# (kvsteps, sets, laps) of the GPU test (tests/test_gpu_attnload_sweep.py).
GPU_SHAPES = ((1, 1, 1), (2, 2, 3), (3, 2, 2), (16, 3, 9))


@pytest.fixture(scope="module")
def lib():
    # No skip: a _hipattnload.so that is missing or does not load is a failure of these tests.
    return hip_probe.HipProbe()


@pytest.mark.parametrize("kvsteps", (1, 3))
@pytest.mark.parametrize("set_", (0, 2))
@pytest.mark.parametrize("seed", SEEDS)
def test_operands_are_bit_equal_to_the_reference(lib, seed, set_, kvsteps):
    got, want = lib.attnload_operands(seed, set_, kvsteps), ref.operands(seed, set_, kvsteps)
    assert [g.shape for g in got] == [(256, 64), (64 * kvsteps, 64), (64 * kvsteps, 64)]
    assert all((g == w).all() for g, w in zip(got, want))
    q, k, v = got
    assert (q & 0x7F80 == 0x3D80).all() and (k & 0x7F80 == 0x3F80).all()
    assert all(len(set((g & 0x807F).ravel())) == 256 for g in (q, k))  # both signs, every mantissa
    assert set(ref.values(v).ravel()) == set(range(-127, 128))  # every integer the byte can hold


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("laps", (1, 33))
def test_host_digests_equal_the_reference_at_the_sweeps_shape(lib, laps, seed):
    assert (ATTNLOAD_KVSTEPS, hip_probe.ATTNLOAD_MAX_KVSTEPS, ATTNLOAD_SETS) == (8, 16, 32)
    want = ref.digests(seed, laps, ATTNLOAD_KVSTEPS, ATTNLOAD_SETS)
    assert lib.attnload_parts() == ref.PARTS and len(set(want.values())) == 5
    assert lib.attnload_sweep_expected(seed=seed, laps=laps) == want
    # A part outside the mask is not reported, and its word is 0.
    assert lib.attnload_sweep_expected(["stat"], seed, laps) == {"stat": want["stat"]}
    out = (ctypes.c_uint32 * 5)(7, 7, 7, 7, 7)
    assert lib.lib.xs_attnload_sweep_expected(16, seed, laps, out) == 0 and list(out) == [0, 0, 0, 0, want["out"]]


def test_host_refuses_bad_arguments(lib):
    L = lib.lib
    out, two = (ctypes.c_uint32 * 5)(), (ctypes.c_int * 2)()
    rec, n, ms = (ctypes.c_uint32 * 32)(), ctypes.c_int(), ctypes.c_double()

    def sweep(mask=31, laps=1, blocks=1, ix=-1, ic=-1, im=0, records=rec):
        return L.xs_attnload_sweep(0, blocks, mask, 0, laps, ix, ic, im, records, ctypes.byref(n), ctypes.byref(ms))

    def probe(mask=31, laps=1, kvsteps=1, sets=1, words=16896 + 1536, buf=rec):
        return L.xs_attnload_probe(0, mask, 0, laps, kvsteps, sets, buf, words)

    # Every one is refused before anything touches a device or builds a set.
    cap = 16 * ATTNLOAD_LAPS
    refused = [sweep(mask=0), sweep(mask=32), sweep(laps=0), sweep(laps=cap + 1), sweep(im=32), sweep(ix=-2),
               sweep(ic=-2), sweep(blocks=-1), sweep(records=None), probe(mask=0), probe(mask=32), probe(laps=0),
               probe(laps=cap + 1), probe(kvsteps=0), probe(kvsteps=17), probe(sets=0), probe(sets=65),
               probe(words=16896), probe(buf=None),
               L.xs_attnload_sweep_expected(0, 0, 1, out), L.xs_attnload_sweep_expected(31, 0, 0, out),
               L.xs_attnload_sweep_expected(31, 0, cap + 1, out), L.xs_attnload_sweep_expected(31, 0, 1, None),
               L.xs_attnload_shape(5, two), L.xs_attnload_shape(-1, two), L.xs_attnload_shape(0, None),
               L.xs_attnload_operands(0, 64, 1, rec, rec, rec), L.xs_attnload_operands(0, 0, 17, rec, rec, rec),
               L.xs_attnload_operands(0, 0, 0, rec, rec, rec), L.xs_attnload_operands(0, 0, 1, rec, rec, None)]
    assert refused == [hip_probe.BAD_ARGS] * len(refused)
    assert lib.attnload_shape("out", 3) == {"fixed_words": 0, "words_per_lap": 16384, "words": 3 * 16384}
    assert lib.attnload_shape("stat", 3) == {"fixed_words": 0, "words_per_lap": 512, "words": 3 * 512}
    assert lib.attnload_shape("score") == {"fixed_words": 512, "words_per_lap": 0, "words": 512}


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("kvsteps,sets", sorted({(k, s) for k, s, _ in GPU_SHAPES}))
def test_the_reference_rescales_and_meets_every_exponent_at_the_gpu_shapes(kvsteps, sets, seed):
    for s in range(sets):
        a = ref.attention(seed, s, kvsteps)
        assert set(np.unique(a["e"])) == set(range(-4, 4))
        assert kvsteps < 2 or (a["m"] > a["first_m"]).any()  # the rescale path runs on real factors


class FakeProbe:
    """hip_health_fn's probe with the bf16 and attention load sweeps only; `bad_xcd` fails `stat` of the latter."""

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

    def bfload_sweep(self, dev, parts=None, **kw):
        return self._sweep("bfload", ["stage", "operand", "transpose", "gemm"], None, **kw)

    def attnload_sweep(self, dev, parts=None, **kw):
        return self._sweep("attnload", ref.PARTS, self.bad_xcd, parts=parts, **kw)


def test_agent_runs_it_last_publishes_attn_load_faults_and_drops_them(store, monkeypatch):
    f = FakeProbe(5)
    monkeypatch.setattr(hip_probe, "probe", lambda: f)
    args = build_parser().parse_args(["node-agent", "--health-attnload-sweep", "out, stat", "--health-bfload-sweep",
                                      "--health-attnload-sweep-laps", "64", "--health-sweep-period", "0"])
    kw = health_fn_args(args)
    assert (kw["attnload"], kw["attnload_parts"], kw["attnload_args"]) == (True, ["out", "stat"], {"laps": 64})
    assert "bfload_args" not in kw
    assert "attnload" not in health_fn_args(build_parser().parse_args(["node-agent"]))  # off by default
    agent = NodeAgent(LocalClient(store), "n", host_fn=lambda: fake_host(1, "DPX"), publish_metrics=False,
                      health_fn=hip_health_fn(**kw))

    def topology():
        agent.sync()
        return json.loads(store.get("nodes", "", "n")["metadata"]["annotations"][TOPOLOGY_ANNOTATION])

    topo = topology()
    assert f.order == [("bfload", {}), ("attnload", {"parts": ["out", "stat"], "laps": 64})]
    assert topo["attnLoadFaults"] == {"0": {"5": ["stat"]}} and topo["xcdFaults"] == {"0": [5]}
    assert "bfLoadFaults" not in topo
    f.bad_xcd = None  # the fault clears
    topo = topology()
    assert "attnLoadFaults" not in topo and "xcdFaults" not in topo
