"""The consensus sweep off the GPU: the vote (vote_consensus) on hand-built
records, the library's refusals, its operands against the Python reference,
hip_health_fn running it between the scalar and the memory sweep, the node
agent publishing `consensusFaults` next to `xcdFaults`, and the node-agent flag."""
import ctypes
import json
import logging

import numpy as np
import pytest

import consensus_sweep_ref as ref
from flex_gpu_scheduler_amd.cli import build_parser, health_fn_args, wants_health_fn
from flex_gpu_scheduler_amd.control import LocalClient
from flex_gpu_scheduler_amd.control.node_agent import (CONSENSUS_SWEEP_KIND, FAULT_KINDS, MEM_SWEEP_KIND,
                                                       SCALAR_SWEEP_KIND, SWEEP_KINDS, GpuHealth, NodeAgent,
                                                       hip_health_fn)
from flex_gpu_scheduler_amd.gpu.discovery import fake_host
from flex_gpu_scheduler_amd.models import GPU_XCD, TOPOLOGY_ANNOTATION
from flex_gpu_scheduler_amd.ops import hip_probe
from flex_gpu_scheduler_amd.ops.hip_probe import (CONSENSUS_SWEEP, PART_SWEEPS, summarize_consensus_sweep,
                                                  summarize_mem_sweep, summarize_scalar_sweep, summarize_sweep,
                                                  vote_consensus)

PARTS = ref.PARTS
GOOD = {f: 0x1000 + i for i, f in enumerate(PARTS)}


def bit(name):
    return 1 << PARTS.index(name)


def records(xcds=8, cus=32, per_cu=4, selected=PARTS, odd=None, skip=()):
    """`per_cu` records per CU holding GOOD (0 for a part not selected); `odd`
    maps (xcd, cu) to {part: digest}, or to a list of such dicts, one per record."""
    out = []
    for x in range(xcds):
        for c in range(cus):
            if (x, c) in skip:
                continue
            for i in range(per_cu):
                d = {f: (GOOD[f] if f in selected else 0) for f in PARTS}
                o = (odd or {}).get((x, c), {})
                d.update(o[i] if isinstance(o, list) else o)
                out.append({"xcd": x, "cu": c, "simd_mask": 15, "fail": 0, "digests": d})
    return out


def failed_cus(recs, fail):
    return {(r["xcd"], r["cu"]): f for r, f in zip(recs, fail) if f}


# ------------------------------------------------------------------ the vote
def test_all_cus_equal_is_clean_and_reports_the_consensus():
    recs = records()
    v = vote_consensus(recs, PARTS)
    assert not any(v["fail"]) and v["undecided"] == []
    assert v["consensus"] == {f: f"0x{GOOD[f]:08x}" for f in PARTS}
    assert all(r["fail"] == 0 for r in recs)  # nothing is changed in place
    s = summarize_consensus_sweep(recs, 256, PARTS)
    assert s["covered"] and s["bad_xcds"] == [] and s["failed_parts"] == [] and s["undecided"] == []
    assert s["consensus"] == v["consensus"] and s["cus_seen"] == 256


def test_one_cu_off_in_one_part_fails_exactly_that_cu_xcd_and_part():
    recs = records(odd={(5, 17): {"sr": 7}})
    v = vote_consensus(recs, PARTS)
    assert failed_cus(recs, v["fail"]) == {(5, 17): bit("sr")} and sum(map(bool, v["fail"])) == 4
    s = summarize_consensus_sweep(recs, 256, PARTS)
    assert s["bad_xcds"] == [5] and s["xcds"][5]["failed_cus"] == [17] and s["xcds"][5]["failed_parts"] == ["sr"]
    assert s["failed_parts"] == ["sr"] and s["undecided"] == [] and s["covered"]
    assert all(s["xcds"][x]["failed_parts"] == [] for x in range(8) if x != 5)
    assert [r["fail"] for r in recs if (r["xcd"], r["cu"]) == (5, 17)] == [bit("sr")] * 4


def test_a_cu_whose_own_records_disagree_fails_though_three_hold_the_consensus():
    recs = records(odd={(2, 9): [{}, {}, {"mfma": 1}, {}]})
    v = vote_consensus(recs, PARTS)
    assert failed_cus(recs, v["fail"]) == {(2, 9): bit("mfma")}
    assert sum(map(bool, v["fail"])) == 4  # each of its records, the three good ones too
    assert v["consensus"]["mfma"] == f"0x{GOOD['mfma']:08x}"


def test_a_whole_xcd_that_agrees_on_another_digest_is_bad():
    recs = records(odd={(3, c): {"ldsx": 0xBAD} for c in range(32)})
    s = summarize_consensus_sweep(recs, 256, PARTS)
    assert s["bad_xcds"] == [3] and len(s["xcds"][3]["failed_cus"]) == 32
    assert s["xcds"][3]["failed_parts"] == ["ldsx"] and s["consensus"]["ldsx"] == f"0x{GOOD['ldsx']:08x}"


def test_an_even_split_is_undecided_and_the_other_parts_are_still_judged():
    odd = {(x, c): {"trans": 9} for x in range(4) for c in range(32)}  # 128 against 128
    odd[(6, 1)] = {"div": 5}  # a clear majority in the same records
    recs = records(odd=odd)
    v = vote_consensus(recs, PARTS)
    assert v["undecided"] == ["trans"] and "trans" not in v["consensus"]
    assert failed_cus(recs, v["fail"]) == {(6, 1): bit("div")}
    s = summarize_consensus_sweep(recs, 256, PARTS)
    assert s["undecided"] == ["trans"] and s["bad_xcds"] == [6] and s["failed_parts"] == ["div"]


def test_129_against_127_fails_the_127():
    odd = {(x, c): {"edge": 9} for x in range(4) for c in range(32) if (x, c) != (0, 0)}  # 127
    recs = records(odd=odd)
    v = vote_consensus(recs, PARTS)
    assert v["undecided"] == [] and v["consensus"]["edge"] == f"0x{GOOD['edge']:08x}"
    assert failed_cus(recs, v["fail"]) == {k: bit("edge") for k in odd}


def test_two_cus_are_undecided_and_three_decide():
    two = records(xcds=1, cus=2)
    v = vote_consensus(two, PARTS)
    assert v["undecided"] == PARTS and v["consensus"] == {} and not any(v["fail"])
    v = vote_consensus(records(xcds=1, cus=2, odd={(0, 1): {"sr": 1}}), PARTS)
    assert v["undecided"] == PARTS and not any(v["fail"])
    three = records(xcds=1, cus=3, odd={(0, 2): {"sr": 1}})
    v = vote_consensus(three, PARTS)
    assert v["undecided"] == [] and failed_cus(three, v["fail"]) == {(0, 2): bit("sr")}


def test_a_cu_votes_once_however_many_records_it_left():
    recs = records(xcds=1, cus=1, per_cu=100, odd={(0, 0): {"smfmac": 0xAA}})
    recs += [{"xcd": 0, "cu": c, "simd_mask": 15, "fail": 0, "digests": dict(GOOD, smfmac=0xBB)} for c in (1, 2)]
    v = vote_consensus(recs, PARTS)
    assert v["consensus"]["smfmac"] == "0x000000bb"
    assert failed_cus(recs, v["fail"]) == {(0, 0): bit("smfmac")} and sum(map(bool, v["fail"])) == 100


def test_a_cu_without_a_vote_counts_in_the_denominator():
    # 4 CUs: two hold X, one holds Y, one disagrees with itself: 2 of 4 is no strict majority.
    recs = records(xcds=1, cus=4, per_cu=2, odd={(0, 2): {"div": 1}, (0, 3): [{"div": 2}, {}]})
    v = vote_consensus(recs, PARTS)
    assert "div" in v["undecided"] and not any(f & bit("div") for f in v["fail"])


def test_an_unselected_part_is_never_judged():
    sel = ["div", "mfma"]
    recs = records(selected=sel, odd={(1, 1): {"mfma": 3}})
    v = vote_consensus(recs, sel)
    assert set(v["consensus"]) == set(sel) and v["undecided"] == []
    assert failed_cus(recs, v["fail"]) == {(1, 1): bit("mfma")}
    # Even a record whose unselected digest is not 0 fails nothing for it.
    recs = records(selected=sel, odd={(1, 1): {"trans": 3}})
    assert not any(vote_consensus(recs, sel)["fail"])
    s = summarize_consensus_sweep(recs, 256, PARTS, sel)
    assert s["failed_parts"] == [] and set(s["consensus"]) == set(sel)


def test_uncovered_cus_are_not_failed():
    s = summarize_consensus_sweep(records(skip={(6, 0), (6, 9)}), 256, PARTS)
    assert not s["covered"] and s["uncovered"][6] == 2 and s["bad_xcds"] == [] and s["undecided"] == []


# ---------------------------------------------------------- the host library
@pytest.fixture(scope="module")
def lib():
    # No skip: a _hipconsensus.so that is missing or does not load is a failure of these tests.
    return hip_probe.HipProbe()


def test_host_names_and_shapes(lib):
    assert lib.consensus_parts() == PARTS
    assert {f: tuple(lib.consensus_shape(f).values()) for f in PARTS} == {f: ref.shape(f) for f in PARTS}
    with pytest.raises(ValueError):
        lib.consensus_shape("f32")


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

    assert {n for n in exported(hip_probe._CONSENSUS_LIB) if n.startswith("xs_")} == set(hip_probe.CONSENSUS_SYMBOLS)
    assert all(getattr(lib.lib, n) is getattr(lib.consensus_lib, n) for n in hip_probe.CONSENSUS_SYMBOLS)
    for other in (hip_probe._LIB, hip_probe._MEM_LIB, hip_probe._SCALAR_LIB):
        assert not any(re.match(r"xs_consensus_", n) for n in exported(other)), other


def test_host_refuses_bad_arguments_before_anything_touches_a_device(lib):
    n, ms = ctypes.c_int(), ctypes.c_double()
    rec = (ctypes.c_uint32 * 32)()
    sweep, tail = lib.lib.xs_consensus_sweep, (rec, ctypes.byref(n), ctypes.byref(ms))
    assert sweep(0, 1, 0, 0, 1, -1, -1, 0, *tail) == -1000  # a zero mask
    assert sweep(0, 1, 1 << 7, 0, 1, -1, -1, 0, *tail) == -1000  # a mask beyond the range
    assert sweep(0, 1, 1, 0, 1, -1, -1, 1 << 7, *tail) == -1000  # injected parts beyond the range
    assert sweep(0, 1, 1, 0, 1, -2, -1, 0, *tail) == -1000 and sweep(0, 1, 1, 0, 1, -1, -2, 0, *tail) == -1000
    assert sweep(0, 1, 1, 0, 0, -1, -1, 0, *tail) == -1000 and sweep(0, 1, 1, 0, 65, -1, -1, 0, *tail) == -1000
    three = (ctypes.c_int * 3)()
    assert lib.lib.xs_consensus_shape(7, three) == -1000 and lib.lib.xs_consensus_shape(-1, three) == -1000
    assert lib.lib.xs_consensus_probe(0, 7, 0, rec, 32) == -1000 and lib.lib.xs_consensus_probe(0, 0, 0, rec, 32) == -1000
    assert lib.lib.xs_consensus_operands(0, 0, rec, 32) == -1000 and lib.lib.xs_consensus_operands(7, 0, rec, 32) == -1000


@pytest.mark.parametrize("seed", ref.SEEDS)
@pytest.mark.parametrize("part", PARTS)
def test_host_operands_are_bit_equal_to_the_reference(lib, part, seed):
    got = lib.consensus_operands(part, seed, rounds=2)
    want = ref.operands(part, seed, 2)
    assert got.shape == want.shape
    bad = np.argwhere(got != want)
    for r, row, t in bad[:8]:
        print(f"{part}: round {r} operand row {row} thread {t}: got {got[r, row, t]:#010x}, want {want[r, row, t]:#010x}")
    assert len(bad) == 0
    assert got.any() and not np.array_equal(got[0], got[1])


@pytest.mark.parametrize("index", [i for i, s in enumerate(ref.steps_of("sr")) if s[1] != "v_prng_b32"])
def test_every_sr_form_has_256_operands_in_the_middle_of_the_gap_and_some_representable(index):
    _, name, _, ops = ref.steps_of("sr")[index]
    _, target, source, scaled = ops[0][0]
    middle = exact = 0
    for r in range(2):
        o = ref.step_operands("sr", index, ref.SEEDS[0], r)
        scale = ref.f32_of(o[2][0]) if scaled else 1.0
        x = ref.sr_values(target, source, o[0]) / scale
        lo, hi = ref.neighbours(target, x)
        ebits, mbits, bias = ref.FORMATS[target]
        assert (np.abs(x) >= 2.0 ** (1 - bias)).all() and np.isfinite(hi).all()  # in-range normals of the target
        gap = np.where(hi != lo, (x - lo) / np.where(hi != lo, hi - lo, 1.0), 0.0)
        middle += int(((gap >= 0.25) & (gap <= 0.75)).sum())
        exact += int((hi == lo).sum())
        assert (((gap >= 0.25) & (gap <= 0.75)) | (hi == lo)).all(), name
    assert middle >= 256 and exact > 0, (name, middle, exact)


# ------------------------------------------------------------------ the row
def test_the_row_stands_beside_the_table():
    assert list(PART_SWEEPS) == ["matrix", "lane", "valu", "mem"] and CONSENSUS_SWEEP not in PART_SWEEPS.values()
    assert (CONSENSUS_SWEEP.prefix, CONSENSUS_SWEEP.names_symbol) == ("consensus", "xs_consensus_parts")
    assert (CONSENSUS_SWEEP.summary_key, CONSENSUS_SWEEP.selection) == ("failed_parts", "parts")
    assert (CONSENSUS_SWEEP.record_words, CONSENSUS_SWEEP.digests, CONSENSUS_SWEEP.bad) == (32, 4, None)


# ------------------------------------------------------------ hip_health_fn
class FakeProbe:
    def __init__(self, cus=256, scalar_fail=None, odd=None, skip=(), mem_fail=None):
        self.cus, self.scalar_fail, self.odd, self.skip = cus, scalar_fail or {}, odd or {}, skip
        self.mem_fail = mem_fail or {}
        self.order, self.calls = [], []

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
        recs = [{"xcd": x, "cu": c, "fail": 0} for x in range(self._xcds()) for c in range(32)]
        s = summarize_sweep(recs, self.cus)
        s.update(rounds=1, ms=2.0, blocks=4 * self.cus)
        return {"records": recs, "summary": s}

    def scalar_sweep(self, dev, parts=None, **kw):
        import scalar_sweep_ref

        self.order.append("scalar")
        names = scalar_sweep_ref.PARTS
        recs = [{"xcd": x, "cu": c, "simd_mask": 15,
                 "fail": sum(1 << names.index(n) for n in self.scalar_fail.get(x, ())) if c == 4 else 0}
                for x in range(self._xcds()) for c in range(32)]
        s = summarize_scalar_sweep(recs, self.cus, names)
        s.update(rounds=1, ms=1.5, blocks=4 * self.cus, seed=0, parts=parts or names)
        return {"records": recs, "summary": s}

    def consensus_sweep(self, dev, parts=None, **kw):
        self.order.append("consensus")
        self.calls.append({"parts": parts, **kw})
        selected = parts or PARTS
        recs = records(self._xcds(), selected=selected, odd=self.odd, skip=self.skip)
        s = summarize_consensus_sweep(recs, self.cus, PARTS, selected)
        s.update(rounds=1, ms=1.0, blocks=4 * self.cus, seed=0, parts=selected, operand_rounds=2)
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
    k = CONSENSUS_SWEEP_KIND
    assert k not in SWEEP_KINDS and len(SWEEP_KINDS) == 5 and k is not SCALAR_SWEEP_KIND and k is not MEM_SWEEP_KIND
    assert (k.enabled_by, k.method, k.label, k.summary_key, k.selection, k.faults_key) == (
        "consensus", "consensus_sweep", "consensus", "consensusSweep", "parts", "consensusFaults")
    assert k.fault_of({"failed_parts": ("sr",)}) == ["sr"]
    f = FAULT_KINDS["consensusFaults"]
    assert not f.per_xcd and not f.withholds_gpu
    assert sorted(n for n, v in FAULT_KINDS.items() if v.per_xcd) == ["laneFaults", "matrixFaults", "registerFaults",
                                                                     "valuFaults"]


def test_health_fn_default_runs_no_consensus_sweep(fake):
    f = fake()
    assert hip_health_fn()(0) is True
    assert hip_health_fn(sweep=True, scalar=True, mem=True)(0)
    assert f.calls == [] and f.order == ["cu", "scalar", "mem"]


def test_health_fn_consensus_sweep_alone_and_its_arguments(fake):
    f = fake(odd={(3, 4): {"sr": 1}})
    v = hip_health_fn(consensus=True, consensus_parts=["sr", "div"], consensus_args={"blocks": 64, "seed": 5})(0)
    assert isinstance(v, GpuHealth) and not v.ok
    assert v.bad_xcds == frozenset({3}) and v.detail["consensusFaults"] == {3: ["sr"]}
    assert v.detail["consensusSweep"]["parts"] == ["sr", "div"] and set(v.detail["consensusSweep"]["consensus"]) == {"sr", "div"}
    assert f.order == ["consensus"] and f.calls == [{"parts": ["sr", "div"], "blocks": 64, "seed": 5}]
    ok = fake()
    v = hip_health_fn(consensus=True)(0)
    assert isinstance(v, GpuHealth) and v.ok and v and v.detail["consensusFaults"] == {}
    assert ok.calls == [{"parts": None}]


def test_health_fn_runs_it_after_the_scalar_sweep_and_before_the_memory_sweep(fake):
    f = fake(scalar_fail={6: ["mask"]}, odd={(2, 0): {"mfma": 1, "trans": 2}}, mem_fail={7: ["l2"]})
    v = hip_health_fn(mem=True, consensus=True, scalar=True, sweep=True)(0)
    assert f.order == ["cu", "scalar", "consensus", "mem"]
    assert isinstance(v, GpuHealth) and not v.ok and v.bad_xcds == frozenset({2, 6, 7})
    assert v.detail["consensusFaults"] == {2: ["trans", "mfma"]}
    assert v.detail["scalarFaults"] == {6: ["mask"]} and v.detail["memFaults"] == {7: ["l2"]}


def test_health_fn_undecided_parts_and_uncovered_cus_do_not_fail_the_device(fake, caplog):
    # 127 CUs against 127, one CU of either side not reached.
    fake(odd={(x, c): {"ldsx": 9} for x in range(4) for c in range(32)}, skip={(0, 7), (7, 7)})
    with caplog.at_level(logging.WARNING, logger="flex_gpu_scheduler_amd.control.node_agent"):
        v = hip_health_fn(consensus=True)(0)
    assert isinstance(v, GpuHealth) and v.ok and v and v.bad_xcds == frozenset()
    s = v.detail["consensusSweep"]
    assert s["undecided"] == ["ldsx"] and not s["covered"] and v.detail["consensusFaults"] == {}
    assert any(r.levelno == logging.WARNING and "undecided" in r.getMessage() and "ldsx" in r.getMessage()
               for r in caplog.records)


def test_health_fn_on_a_partition_device_returns_a_bool(fake):
    fake(cus=64, odd={(1, 3): {"edge": 1}})
    assert hip_health_fn(consensus=True)(0) is False
    fake(cus=64)
    assert hip_health_fn(consensus=True)(0) is True


# --------------------------------------------------------------- node agent
def agent_on(store, host, health_fn):
    agent = NodeAgent(LocalClient(store), "n", host_fn=lambda: host, publish_metrics=False, health_fn=health_fn)
    agent.sync()
    return agent


def topo_of(store) -> dict:
    return json.loads(store.get("nodes", "", "n")["metadata"]["annotations"][TOPOLOGY_ANNOTATION])


def test_agent_publishes_consensus_faults_and_fences_the_partition(store, fake):
    fake(odd={(5, 4): {"smfmac": 1, "sr": 2}})
    agent = agent_on(store, fake_host(2, "CPX"), hip_health_fn(consensus=True))
    topo = topo_of(store)
    assert topo["consensusFaults"] == {"0": {"5": ["sr", "smfmac"]}, "1": {"5": ["sr", "smfmac"]}}
    assert topo["xcdFaults"] == {"0": [5], "1": [5]} and topo["unhealthy"] == []
    assert agent.faults["consensusFaults"][0] == {5: ["sr", "smfmac"]}
    assert store.get("nodes", "", "n")["status"]["allocatable"][GPU_XCD] == "14"  # XCD 5's partition of either GPU


def test_agent_omits_the_key_when_there_is_no_fault(store, fake):
    fake()
    agent_on(store, fake_host(2, "CPX"), hip_health_fn(consensus=True))
    assert "consensusFaults" not in topo_of(store) and "xcdFaults" not in topo_of(store)
    verdict = GpuHealth(False, {1}, {"consensusFaults": {1: ["trans"]}})
    agent_on(store, fake_host(1, "CPX"), lambda dev: verdict)
    assert topo_of(store)["consensusFaults"] == {"0": {"1": ["trans"]}} and topo_of(store)["xcdFaults"] == {"0": [1]}


# ---------------------------------------------------------------------- CLI
def test_cli_parses_the_consensus_sweep_flag():
    ap = build_parser()
    none = ap.parse_args(["node-agent"])
    assert none.health_consensus_sweep is None and not wants_health_fn(none)
    assert "consensus" not in health_fn_args(none) and "consensus_parts" not in health_fn_args(none)
    base = {"sweep": False, "sweep_period_s": 600.0, "matrix": False, "matrix_formats": None}
    on = ap.parse_args(["node-agent", "--health-consensus-sweep"])
    assert health_fn_args(on) == {**base, "consensus": True, "consensus_parts": None} and wants_health_fn(on)
    every = ap.parse_args(["node-agent", "--health-consensus-sweep", "all"])
    assert health_fn_args(every) == {**base, "consensus": True, "consensus_parts": None}
    some = ap.parse_args(["node-agent", "--health-consensus-sweep", "sr, mfma", "--health-scalar-sweep", "cmp"])
    assert health_fn_args(some) == {**base, "scalar": True, "scalar_parts": ["cmp"], "consensus": True,
                                    "consensus_parts": ["sr", "mfma"]}
    keywords = hip_health_fn.__code__.co_varnames[:hip_health_fn.__code__.co_argcount]
    assert set(health_fn_args(some)) <= set(keywords)
