"""The FP8 load sweep off the GPU: the host's operands and digests against the
independent reference (tests/f8load_sweep_ref.py), the bound that keeps every
sum exact and the refusal of anything past it, record decoding and summary, and
the node agent publishing `f8LoadFaults` behind the gradient load sweep."""
import ctypes
import json

import numpy as np
import pytest

import f8load_sweep_ref as ref
from flex_gpu_scheduler_amd.cli import build_parser, health_fn_args
from flex_gpu_scheduler_amd.control import LocalClient
from flex_gpu_scheduler_amd.control.node_agent import NodeAgent, hip_health_fn
from flex_gpu_scheduler_amd.gpu.discovery import fake_host
from flex_gpu_scheduler_amd.models import TOPOLOGY_ANNOTATION
from flex_gpu_scheduler_amd.ops import hip_probe
from flex_gpu_scheduler_amd.ops.hip_probe import (F8LOAD_MASK_WORD, F8LOAD_SWEEP, decode_part_record, load_record_tail,
                                                   summarize_load_sweep)

SEEDS = (hip_probe.F8LOAD_SEED, 0x9E3779B9)
SHAPES = ((1, 1, 1), (2, 1, 3), (3, 2, 5), (18, 4, 6), (1, 3, 35))  # (ksteps, slots, laps) of the GPU test


@pytest.fixture(scope="module")
def lib():
    # No skip: a _hipf8load.so that is missing or does not load is a failure of these tests.
    return hip_probe.HipProbe()


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("ksteps,slots,laps", SHAPES)
def test_operands_and_digests_equal_the_reference(lib, ksteps, slots, laps, seed):
    for s in (0, ref.SETS - 1):
        got, want = lib.f8load_operands(seed, s, ksteps), ref.operands(seed, s, ksteps)
        assert all(g.shape == w.shape and g.dtype == w.dtype and (g == w).all() for g, w in zip(got, want))
        for panel in got[:2]:  # the four binades, and so never zero, subnormal or NaN
            assert set(np.unique(panel >> 3 & 15)) == {6, 7, 8, 9}
            assert 0.5 <= np.abs(ref.e4m3(panel)).min() and np.abs(ref.e4m3(panel)).max() <= 7.5
        assert set(got[2]) <= {0.25, 0.5, 1.0, 2.0} and set(got[3]) <= {1.0, 2.0}
    want = ref.digests(seed, laps, ksteps, slots)
    assert lib.f8load_parts() == ref.PARTS and want["store"] == want["round"] and len(set(want.values())) == 3
    assert ref.digests(seed, laps, ksteps, slots, g=5) == want  # whichever workgroup: what the record's compare needs
    assert lib.f8load_sweep_expected(None, seed, laps, ksteps, slots) == want
    # A part outside the mask is not reported, and its word is 0.
    out = (ctypes.c_uint32 * 4)(7, 7, 7, 7)
    assert lib.lib.xs_f8load_sweep_expected(0b1010, seed, laps, ksteps, slots, out) == 0
    assert list(out) == [0, want["gemm"], 0, want["store"]]


def test_the_largest_sum_is_an_exact_float():
    assert 18 * 64 * 14400 < 1 << 24 <= 19 * 64 * 14400 and hip_probe.F8LOAD_MAX_KSTEPS == 18
    a, bt, _, _ = ref.operands(hip_probe.F8LOAD_SEED, 0, 18)
    assert (np.abs(ref.e4m3(a)) @ np.abs(ref.e4m3(bt)).T).max() * 256 < 1 << 24
    assert {int(v) for v in np.unique(np.abs(ref.e4m3(a)) * 16)} == {(8 + m) << e for m in range(8) for e in range(4)}


def test_host_refuses_what_leaves_the_bound_and_bad_arguments(lib):
    L = lib.lib
    out, two = (ctypes.c_uint32 * 4)(), (ctypes.c_int * 2)()
    rec, n, ms = (ctypes.c_uint32 * 32)(), ctypes.c_int(), ctypes.c_double()

    def sweep(mask=15, laps=1, ksteps=1, slots=1, blocks=1, ix=-1, ic=-1, im=0, records=rec):
        return L.xs_f8load_sweep(0, blocks, mask, 0, laps, ksteps, slots, ix, ic, im, records, ctypes.byref(n),
                                 ctypes.byref(ms))

    def probe(mask=15, laps=1, ksteps=1, slots=1, words=49152 + 512, buf=rec):
        return L.xs_f8load_probe(0, mask, 0, laps, ksteps, slots, buf, words)

    def expected(mask=15, laps=1, ksteps=1, slots=1, buf=out):
        return L.xs_f8load_sweep_expected(mask, 0, laps, ksteps, slots, buf)

    # Every one is refused before anything touches a device.
    shapes = [dict(ksteps=0), dict(ksteps=19), dict(slots=0), dict(slots=17), dict(laps=0),
              dict(laps=16 * hip_probe.F8LOAD_LAPS + 1), dict(mask=0), dict(mask=16)]
    refused = [f(**kw) for kw in shapes for f in (sweep, probe, expected)]
    refused += [sweep(im=16), sweep(ix=-2), sweep(ic=-2), sweep(blocks=-1), sweep(records=None), probe(words=49152),
                probe(buf=None), expected(buf=None), L.xs_f8load_shape(4, two), L.xs_f8load_shape(0, None),
                L.xs_f8load_operands(0, 0, 0, rec, rec, rec, rec), L.xs_f8load_operands(0, 0, 19, rec, rec, rec, rec),
                L.xs_f8load_operands(0, 0, 1, rec, rec, rec, None)]
    assert refused == [hip_probe.BAD_ARGS] * len(refused)
    assert [expected(ksteps=18), expected(slots=16)] == [0, 0]


def _record(xcd, cu, digests, fail=0, bad=(0, 0, 0, 0), masks=(0, 0, 0)):
    return [xcd, cu, 15, fail, *bad, *digests, 15 if any(bad) else 0, 0, *masks] + [0] * 15


def test_records_decode_and_an_injected_part_fails_its_xcd_alone():
    want = dict(zip(ref.PARTS, (11, 22, 33, 33)))
    words = [_record(x, c, want.values()) for x in range(8) for c in range(32)]
    words[5 * 32 + 4] = _record(5, 4, (11, 22, 33, 32), fail=8, bad=(0, 0, 0, 1), masks=(4, 2, 1))
    assert F8LOAD_MASK_WORD == 14 and len(words[0]) == hip_probe.F8LOAD_RECORD_WORDS
    recs = [{**decode_part_record(F8LOAD_SWEEP, ref.PARTS, w, want, ()), **load_record_tail(w, F8LOAD_MASK_WORD)}
            for w in words]
    hit = recs[5 * 32 + 4]
    assert hit["fail"] == 8 and hit["bad"]["store"] == 1 and hit["digests"]["store"] == 32
    assert (hit["bad_subtiles"], hit["bad_sets"], hit["bad_spans"]) == (4, 2, 1)
    s = summarize_load_sweep(recs, 256, ref.PARTS)
    assert s["covered"] and s["bad_xcds"] == [5] and s["failed_parts"] == ["store"]
    assert s["xcds"][5]["failed_parts"] == ["store"] and s["xcds"][4]["failed_parts"] == []
    # A digest that is not the host's fails the part even where the device's comparator passed it.
    assert decode_part_record(F8LOAD_SWEEP, ref.PARTS, _record(0, 0, (11, 22, 34, 33)), want, ())["fail"] == 4


class FakeProbe:
    """hip_health_fn's probe with the gradient and FP8 load sweeps only; `bad_xcd` fails `store` of the latter, and
    `unswept` makes it find no memory."""

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

    def gradload_sweep(self, dev, parts=None, **kw):
        return self._sweep("gradload", ["stage", "transpose", "gemm", "accum"], None, **kw)

    def f8load_sweep(self, dev, parts=None, **kw):
        if self.unswept:
            e = hip_probe.ProbeError("no ring could be had: nothing was swept")
            e.rc = hip_probe.F8LOAD_UNSWEPT
            raise e
        return self._sweep("f8load", ref.PARTS, self.bad_xcd, parts=parts, **kw)


def test_agent_runs_it_last_publishes_f8_load_faults_and_drops_them(store, monkeypatch):
    f = FakeProbe(5)
    monkeypatch.setattr(hip_probe, "probe", lambda: f)
    args = build_parser().parse_args(["node-agent", "--health-f8load-sweep", "store, gemm", "--health-gradload-sweep",
                                      "--health-f8load-sweep-laps", "64", "--health-sweep-period", "0"])
    kw = health_fn_args(args)
    assert (kw["f8load"], kw["f8load_parts"], kw["f8load_args"]) == (True, ["store", "gemm"], {"laps": 64})
    assert "f8load" not in health_fn_args(build_parser().parse_args(["node-agent"]))  # off by default
    agent = NodeAgent(LocalClient(store), "n", host_fn=lambda: fake_host(1, "DPX"), publish_metrics=False,
                      health_fn=hip_health_fn(**kw))

    def topology():
        agent.sync()
        return json.loads(store.get("nodes", "", "n")["metadata"]["annotations"][TOPOLOGY_ANNOTATION])

    topo = topology()
    assert f.order == [("gradload", {}), ("f8load", {"parts": ["store", "gemm"], "laps": 64})]
    assert topo["f8LoadFaults"] == {"0": {"5": ["store"]}} and topo["xcdFaults"] == {"0": [5]}
    f.bad_xcd = None  # the fault clears
    topo = topology()
    assert "f8LoadFaults" not in topo and "xcdFaults" not in topo
    f.unswept = True  # no memory for the ring: unswept, never failed
    topo = topology()
    assert "f8LoadFaults" not in topo and "xcdFaults" not in topo
