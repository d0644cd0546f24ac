"""The sweeps over named parts off the GPU and without the probe library: how
a workgroup's record is decoded from its words (the offsets are the C
records', written out here, not read from the table under test), the summary
of the three sweeps, and the node agent's table of sweep kinds."""
import struct

import pytest

from flex_gpu_scheduler_amd.control.node_agent import FAULT_KINDS, SWEEP_KINDS
from flex_gpu_scheduler_amd.ops.hip_probe import (PART_SWEEPS, decode_part_record, summarize_lane_sweep,
                                                  summarize_matrix_sweep, summarize_sweep, summarize_valu_sweep)

FORMATS = ["f16", "f32", "f64", "fp8", "bf8", "i8", "mxfp8", "mxbf8", "mxfp6", "mxbf6", "mxfp4"]
PATHS = ["dpp", "permlane", "readlane", "bpermute", "ldswide", "ldstr", "ldsatomic", "ldsdma"]
UNITS = ["f32", "f64", "f16", "int", "bit", "dot", "cvt", "trans"]
STEPS = [f"step{g}" for g in range(185)]


def words(n: int, fail: int, **at) -> tuple:
    """A record of n distinct words as the sweep's buffer is split: word i is
    0x1000 + i, word 3 is `fail`, `at` = {"w22": value} overrides others."""
    w = [0x1000 + i for i in range(n)]
    w[3] = fail
    for k, v in at.items():
        w[int(k[1:])] = v
    return struct.unpack(f"{n}I", struct.pack(f"{n}I", *w))


MATRIX_DIGESTS = {"f16": 0x1004, "f32": 0x1005, "f64": 0x1006, "fp8": 0x1007, "bf8": 0x1008, "i8": 0x1009,
                  "mxfp8": 0x100A, "mxbf8": 0x100B, "mxfp6": 0x100C, "mxbf6": 0x100D, "mxfp4": 0x100E}
LANE_BAD = {"dpp": 0x1004, "permlane": 0x1005, "readlane": 0x1006, "bpermute": 0x1007, "ldswide": 0x1008,
            "ldstr": 0x1009, "ldsatomic": 0x100A, "ldsdma": 0x100B}
LANE_DIGESTS = {"dpp": 0x100C, "permlane": 0x100D, "readlane": 0x100E, "bpermute": 0x100F, "ldswide": 0x1010,
                "ldstr": 0x1011, "ldsatomic": 0x1012, "ldsdma": 0x1013}
VALU_BAD = {"f32": 0x1004, "f64": 0x1005, "f16": 0x1006, "int": 0x1007, "bit": 0x1008, "dot": 0x1009,
            "cvt": 0x100A, "trans": 0x100B}
VALU_DIGESTS = {"f32": 0x100C, "f64": 0x100D, "f16": 0x100E, "int": 0x100F, "bit": 0x1010, "dot": 0x1011,
                "cvt": 0x1012, "trans": 0x1013}


# -------------------------------------------------------------------- decode
def test_matrix_record():
    rec = decode_part_record(PART_SWEEPS["matrix"], FORMATS, words(16, 0x402), dict(MATRIX_DIGESTS))
    assert rec == {"xcd": 0x1000, "cu": 0x1001, "simd_mask": 0x1002, "fail": 0x402, "digests": MATRIX_DIGESTS}


def test_lane_record():
    rec = decode_part_record(PART_SWEEPS["lane"], PATHS, words(32, 0x21), dict(LANE_DIGESTS))
    assert rec == {"xcd": 0x1000, "cu": 0x1001, "simd_mask": 0x1002, "fail": 0x21, "bad": LANE_BAD,
                   "digests": LANE_DIGESTS, "bad_simds": 0x1014}


def test_valu_record():
    # Word 22 = 0x1016 has bits 1, 2 and 4 among the first eight; its bit 12 names no step.
    rec = decode_part_record(PART_SWEEPS["valu"], UNITS, words(32, 0x80), dict(VALU_DIGESTS), STEPS[:8])
    assert rec == {"xcd": 0x1000, "cu": 0x1001, "simd_mask": 0x1002, "fail": 0x80, "bad": VALU_BAD,
                   "digests": VALU_DIGESTS, "bad_simds": 0x1014, "bad_steps": ["step1", "step2", "step4"]}


@pytest.mark.parametrize("kind, names, n, digests, part, bit", [
    ("matrix", FORMATS, 16, MATRIX_DIGESTS, "mxbf6", 9), ("lane", PATHS, 32, LANE_DIGESTS, "ldstr", 5),
    ("valu", UNITS, 32, VALU_DIGESTS, "f32", 0)])
def test_a_digest_that_differs_from_the_hosts_fails_the_part(kind, names, n, digests, part, bit):
    """The device's comparator, on the CU under test, passed the part: its fail bit is clear."""
    device_fail = 1 << 2
    host = {**digests, part: digests[part] ^ 1}
    rec = decode_part_record(PART_SWEEPS[kind], names, words(n, device_fail), host)
    assert rec["fail"] == device_fail | 1 << bit and rec["digests"] == digests
    # A part the host did not select must have left no digest.
    del host[part]
    assert decode_part_record(PART_SWEEPS[kind], names, words(n, device_fail), host)["fail"] == device_fail | 1 << bit
    same = decode_part_record(PART_SWEEPS[kind], names, words(n, device_fail), dict(digests))
    assert same["fail"] == device_fail


def test_valu_step_mask_names_the_steps_in_order():
    w = words(32, 1, w22=1 | 1 << 31, w23=1, w24=0, w25=0, w26=0, w27=1 << (184 - 160))
    rec = decode_part_record(PART_SWEEPS["valu"], UNITS, w, dict(VALU_DIGESTS), STEPS)
    assert rec["bad_steps"] == ["step0", "step31", "step32", "step184"]
    none = words(32, 0, w22=0, w23=0, w24=0, w25=0, w26=0, w27=0)
    assert decode_part_record(PART_SWEEPS["valu"], UNITS, none, dict(VALU_DIGESTS), STEPS)["bad_steps"] == []


# ------------------------------------------------------------------- summary
def records(names, fail):
    """One record per CU of 8 XCDs x 32 CUs; `fail` maps (xcd, cu) to the parts that failed there."""
    return [{"xcd": x, "cu": c, "simd_mask": 15, "fail": sum(1 << names.index(f) for f in fail.get((x, c), ())),
             "digests": {f: 0 for f in names}, "bad_steps": [f"{f}.s{c}" for f in fail.get((x, c), ())]}
            for x in range(8) for c in range(32)]


def named(summary: dict, key: str, names) -> dict:
    """`summary` (summarize_sweep's) with its fail bits named under `key`, per XCD and overall."""
    every = 0
    for v in summary["xcds"].values():
        v[key] = [f for b, f in enumerate(names) if v["fail_bits"] >> b & 1]
        every |= v["fail_bits"]
    summary[key] = [f for b, f in enumerate(names) if every >> b & 1]
    return summary


@pytest.mark.parametrize("summarize, key, names", [
    (summarize_matrix_sweep, "failed_formats", FORMATS), (summarize_lane_sweep, "failed_paths", PATHS)])
def test_summary_is_summarize_sweep_plus_the_named_fail_bits(summarize, key, names):
    fail = {(5, 17): [names[5]], (5, 3): [names[0], names[7]], (2, 0): [names[1]]}
    got = summarize(records(names, fail), 256, names)
    assert got == named(summarize_sweep(records(names, fail), 256), key, names)
    assert got["bad_xcds"] == [2, 5] and got[key] == [names[0], names[1], names[5], names[7]]
    assert got["xcds"][5][key] == [names[0], names[5], names[7]] and got["xcds"][0][key] == []


def test_valu_summary_adds_the_failed_steps():
    fail = {(5, 17): ["dot"], (5, 3): ["f32", "trans"], (2, 0): ["f64"]}
    got = summarize_valu_sweep(records(UNITS, fail), 256, UNITS)
    want = named(summarize_sweep(records(UNITS, fail), 256), "failed_units", UNITS)
    for x, v in want["xcds"].items():
        v["failed_steps"] = {2: ["f64.s0"], 5: ["f32.s3", "trans.s3", "dot.s17"]}.get(x, [])
    want["failed_steps"] = ["f64.s0", "f32.s3", "trans.s3", "dot.s17"]
    assert got == want and got["failed_units"] == ["f32", "f64", "dot", "trans"]


# --------------------------------------------------------------- agent table
def test_every_per_xcd_fault_kind_belongs_to_one_sweep_kind():
    per_xcd = [key for key, kind in FAULT_KINDS.items() if kind.per_xcd]
    assert sorted(per_xcd) == ["laneFaults", "matrixFaults", "registerFaults", "valuFaults"]
    for key in per_xcd:
        assert [k.faults_key for k in SWEEP_KINDS].count(key) == 1, key
    assert {k.faults_key for k in SWEEP_KINDS if k.faults_key} == set(per_xcd)
    assert [key for key, kind in FAULT_KINDS.items() if kind.withholds_gpu] == ["hbmFaults"]
    assert not FAULT_KINDS["hbmFaults"].per_xcd
