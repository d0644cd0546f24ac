"""The gradient load sweep off the GPU: the host's operands and digests against
the independent reference (tests/gradload_sweep_ref.py), the refusal of
anything past the bound that keeps every sum exact, record decoding and
summary, and the node agent publishing `gradLoadFaults` behind the stream load
sweep."""
import ctypes
import json

import pytest

import gradload_sweep_ref as ref
from flex_gpu_scheduler_amd.cli import build_parser, health_fn_args
from flex_gpu_scheduler_amd.control import LocalClient
from flex_gpu_scheduler_amd.control.node_agent import NodeAgent, hip_health_fn
from flex_gpu_scheduler_amd.gpu.discovery import fake_host
from flex_gpu_scheduler_amd.models import TOPOLOGY_ANNOTATION
from flex_gpu_scheduler_amd.ops import hip_probe
from flex_gpu_scheduler_amd.ops.hip_probe import (GRADLOAD_MASK_WORD, GRADLOAD_SWEEP, decode_part_record,
                                                   load_record_tail, summarize_load_sweep)

SEEDS = (hip_probe.GRADLOAD_SEED, 0x9E3779B9)
# (ksteps, epoch, laps) of the GPU test (tests/test_gpu_gradload_sweep.py), and one of whole rounds: 8 groups of 4.
SHAPES = ((1, 1, 1), (2, 1, 3), (3, 2, 5), (8, 32, 32), (1, 257, 257), (1, 4, 70))


@pytest.fixture(scope="module")
def lib():
    # No skip: a _hipgradload.so that is missing or does not load is a failure of these tests.
    return hip_probe.HipProbe()


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("ksteps,epoch,laps", SHAPES)
def test_operands_and_digests_equal_the_reference(lib, ksteps, epoch, laps, seed):
    for s in (0, ref.groups_of(epoch) * epoch - 1):
        got, want = lib.gradload_operands(seed, s, ksteps), ref.operands(seed, s, ksteps)
        assert all(g.shape == (32 * ksteps, 128) and (g == w).all() for g, w in zip(got, want))
    want = ref.digests(seed, laps, ksteps, epoch)
    # The digest is linear in fix, so the sums of an epoch carry the digest of their partials.
    assert lib.gradload_parts() == ref.PARTS and len(set(want.values())) == 3 and want["accum"] == want["gemm"]
    assert ref.digests(seed, laps, ksteps, epoch, g=5) == want  # whichever workgroup: what the record's compare needs
    assert lib.gradload_sweep_expected(None, seed, laps, ksteps, epoch, 1) == want
    # A part outside the mask is not reported, and its word is 0.
    out = (ctypes.c_uint32 * 4)(7, 7, 7, 7)
    assert lib.lib.xs_gradload_sweep_expected(8, seed, laps, ksteps, epoch, 2, out) == 0
    assert list(out) == [0, 0, 0, want["accum"]]


def test_the_largest_sum_of_an_epoch_is_an_exact_float(lib):
    x, dy = ref.values(hip_probe.GRADLOAD_SEED, 0, 8)
    assert {int(v) for v in abs(x).ravel()} == set(range(128, 256)) and {int(v) for v in dy.ravel()} == set(
        range(-8, 0)) | set(range(1, 9))
    assert hip_probe.GRADLOAD_MAX_TOKENS * 255 * 8 < 1 << 24 <= (hip_probe.GRADLOAD_MAX_TOKENS + 32) * 255 * 8


def test_host_refuses_what_leaves_the_bound_and_bad_arguments(lib):
    L = lib.lib
    out, two = (ctypes.c_uint32 * 4)(), (ctypes.c_int * 2)()
    rec, n, ms = (ctypes.c_uint32 * 32)(), ctypes.c_int(), ctypes.c_double()

    def sweep(mask=15, laps=1, ksteps=1, epoch=1, slabs=1, blocks=1, ix=-1, ic=-1, im=0, records=rec):
        return L.xs_gradload_sweep(0, blocks, mask, 0, laps, ksteps, epoch, slabs, ix, ic, im, records,
                                   ctypes.byref(n), ctypes.byref(ms))

    def probe(mask=15, laps=1, ksteps=1, epoch=1, slabs=1, words=3 * 16384 + 1024, buf=rec):
        return L.xs_gradload_probe(0, mask, 0, laps, ksteps, epoch, slabs, buf, words)

    def expected(mask=15, laps=1, ksteps=1, epoch=1, slabs=1, buf=out):
        return L.xs_gradload_sweep_expected(mask, 0, laps, ksteps, epoch, slabs, buf)

    # Every one is refused before anything touches a device: epoch x ksteps = 258 is past the bound, 257 is not.
    cap = 16 * hip_probe.GRADLOAD_LAPS
    shapes = [dict(ksteps=1, epoch=258), dict(ksteps=2, epoch=129), dict(ksteps=6, epoch=43), dict(ksteps=8, epoch=33),
              dict(laps=0), dict(laps=cap + 1), dict(ksteps=0), dict(ksteps=9), dict(epoch=0), dict(slabs=0),
              dict(slabs=17)]
    refused = [f(**kw) for kw in shapes + [dict(mask=0), dict(mask=16)] for f in (sweep, probe, expected)]
    refused += [sweep(im=16), sweep(ix=-2), sweep(ic=-2), sweep(blocks=-1), sweep(records=None), probe(words=16384),
                probe(buf=None), expected(buf=None), L.xs_gradload_shape(4, two), L.xs_gradload_shape(0, None),
                L.xs_gradload_operands(0, 0, 0, rec, rec), L.xs_gradload_operands(0, 0, 9, rec, rec),
                L.xs_gradload_operands(0, 1 << 10, 1, rec, rec), L.xs_gradload_operands(0, 0, 1, rec, None)]
    assert refused == [hip_probe.BAD_ARGS] * len(refused)
    assert [expected(ksteps=1, epoch=257), expected(ksteps=8, epoch=32)] == [0, 0]


def _record(xcd, cu, digests, fail=0, bad=(0, 0, 0, 0), masks=(0, 0, 0)):
    return [xcd, cu, 15, fail, *bad, *digests, 15 if any(bad) else 0, 0, *masks] + [0] * 15


def test_records_decode_and_an_injected_part_fails_its_xcd_alone():
    want = dict(zip(ref.PARTS, (11, 22, 33, 44)))
    words = [_record(x, c, want.values()) for x in range(8) for c in range(32)]
    words[5 * 32 + 4] = _record(5, 4, (11, 22, 33, 45), fail=8, bad=(0, 0, 0, 1), masks=(4, 2, 1))
    assert GRADLOAD_MASK_WORD == 14 and len(words[0]) == hip_probe.GRADLOAD_RECORD_WORDS
    recs = [{**decode_part_record(GRADLOAD_SWEEP, ref.PARTS, w, want, ()), **load_record_tail(w, GRADLOAD_MASK_WORD)}
            for w in words]
    hit = recs[5 * 32 + 4]
    assert hit["fail"] == 8 and hit["bad"]["accum"] == 1 and hit["digests"]["accum"] == 45
    assert (hit["bad_subtiles"], hit["bad_sets"], hit["bad_spans"]) == (4, 2, 1)
    s = summarize_load_sweep(recs, 256, ref.PARTS)
    assert s["covered"] and s["bad_xcds"] == [5] and s["failed_parts"] == ["accum"]
    assert s["xcds"][5]["failed_parts"] == ["accum"] and s["xcds"][4]["failed_parts"] == []
    # A digest that is not the host's fails the part even where the device's comparator passed it.
    lying = decode_part_record(GRADLOAD_SWEEP, ref.PARTS, _record(0, 0, (11, 22, 34, 44)), want, ())
    assert lying["fail"] == 4


class FakeProbe:
    """hip_health_fn's probe with the stream and gradient load sweeps only; `bad_xcd` fails `accum` of the latter,
    and `unswept` makes it find no memory."""

    def __init__(self, bad_xcd, unswept=False):
        self.order, self.bad_xcd, self.unswept = [], bad_xcd, unswept

    def props(self, dev):
        return {"computeUnits": 256}

    def health(self, dev):
        return {"healthy": True}

    mfma_check = health

    def _sweep(self, name, names, bad_xcd, **kw):
        self.order.append((name, kw))
        recs = [{"xcd": x, "cu": c, "simd_mask": 15, "fail": 8 if (x, c) == (bad_xcd, 4) else 0}
                for x in range(8) for c in range(32)]
        return {"records": recs, "summary": {**summarize_load_sweep(recs, 256, names), "rounds": 1, "ms": 40.0,
                                             "blocks": 1024, "seed": 0, "parts": names}}

    def streamload_sweep(self, dev, parts=None, **kw):
        return self._sweep("streamload", ["stage", "act", "gemm"], None, **kw)

    def gradload_sweep(self, dev, parts=None, **kw):
        if self.unswept:
            e = hip_probe.ProbeError("no memory could be had for the arena: nothing was swept")
            e.rc = hip_probe.GRADLOAD_UNSWEPT
            raise e
        return self._sweep("gradload", ref.PARTS, self.bad_xcd, parts=parts, **kw)


def test_agent_runs_it_last_publishes_grad_load_faults_and_drops_them(store, monkeypatch):
    f = FakeProbe(5)
    monkeypatch.setattr(hip_probe, "probe", lambda: f)
    args = build_parser().parse_args(["node-agent", "--health-gradload-sweep", "accum, gemm", "--health-streamload-sweep",
                                      "--health-gradload-sweep-laps", "64", "--health-sweep-period", "0"])
    kw = health_fn_args(args)
    assert (kw["gradload"], kw["gradload_parts"], kw["gradload_args"]) == (True, ["accum", "gemm"], {"laps": 64})
    assert "gradload" not in health_fn_args(build_parser().parse_args(["node-agent"]))  # off by default
    agent = NodeAgent(LocalClient(store), "n", host_fn=lambda: fake_host(1, "DPX"), publish_metrics=False,
                      health_fn=hip_health_fn(**kw))

    def topology():
        agent.sync()
        return json.loads(store.get("nodes", "", "n")["metadata"]["annotations"][TOPOLOGY_ANNOTATION])

    topo = topology()
    assert f.order == [("streamload", {}), ("gradload", {"parts": ["accum", "gemm"], "laps": 64})]
    assert topo["gradLoadFaults"] == {"0": {"5": ["accum"]}} and topo["xcdFaults"] == {"0": [5]}
    f.bad_xcd = None  # the fault clears
    topo = topology()
    assert "gradLoadFaults" not in topo and "xcdFaults" not in topo
    f.unswept = True  # no memory for the slabs: unswept, never failed
    topo = topology()
    assert "gradLoadFaults" not in topo and "xcdFaults" not in topo
