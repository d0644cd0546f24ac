"""The relaunch-until-covered policy of the four per-CU sweeps, driven through
their public methods over a fake C library: a device of 2 XCDs x 2 CUs, the
smallest on which "one CU unseen" and "the other XCD unaffected" differ."""
import json

import pytest

from flex_gpu_scheduler_amd.ops.hip_probe import HipProbe, ProbeError

CUS = 4
ALL = [(0, 0), (0, 1), (1, 0), (1, 1)]
FORMATS = "f16,f32,f64,fp8,bf8,i8,mxfp8,mxbf8,mxfp6,mxbf6,mxfp4".split(",")
PATHS = "dpp,permlane,readlane,bpermute,ldswide,ldstr,ldsatomic,ldsdma".split(",")
CU_EXPECTED = (11, 22, 33)  # mfma, valu, lds
MATRIX_EXPECTED = [100 + i for i in range(len(FORMATS))]
LANE_EXPECTED = [200 + i for i in range(len(PATHS))]
REGFILE_EXPECTED = 0xABC


def healthy(sweep: str, xcd: int, cu: int) -> list[int]:
    """The words a healthy CU leaves in its record."""
    head = [xcd, cu, 15, 0]
    if sweep == "cu":
        return head + list(CU_EXPECTED) + [0]
    if sweep == "matrix":
        return head + MATRIX_EXPECTED + [0]
    if sweep == "regfile":
        return head + [0, 0, 0xFFFF, 0, REGFILE_EXPECTED, 0] + [0] * 6
    return head + [0] * 8 + LANE_EXPECTED + [0] * 12


WORDS = {"cu": 8, "matrix": 16, "regfile": 16, "lane": 32}
# sweep -> (record word whose digest is spoilt, the fail bits the host must set, summary key, names of those bits)
SPOILT = {"cu": (5, 2, None, None), "matrix": (4 + 3, 1 << 3, "failed_formats", ["fp8"]),
          "regfile": (8, 3, "failed_files", ["vgpr", "agpr"]), "lane": (12 + 5, 1 << 5, "failed_paths", ["ldstr"])}


class FakeLib:
    """`rounds`: the records each launch returns, as lists of word lists;
    `ms` and `rcs` per launch. Every launch is noted in `launches`."""

    def __init__(self, sweep, rounds, ms=None, rcs=None):
        self.sweep, self.rounds = sweep, rounds
        self.ms = ms or [1.0] * len(rounds)
        self.rcs = rcs or [0] * len(rounds)
        self.launches: list[int] = []  # the `blocks` argument of each
        self.expected_calls = 0
        for name in ("cu", "matrix", "regfile", "lane"):
            setattr(self, f"xs_{name}_sweep", self._launch if name == sweep else self._other)
            setattr(self, f"xs_{name}_sweep_last_error", lambda name=name: f"boom from {name}".encode())

    def _other(self, *a):
        raise AssertionError("another sweep's launch was called")

    def xs_device_props(self, dev, buf, n):
        buf.value = json.dumps({"computeUnits": CUS}).encode()
        return 0

    def xs_cu_sweep_max_lds(self, dev):
        return 160 << 10

    def xs_matrix_formats(self):
        return ",".join(FORMATS).encode()

    def xs_lane_paths(self):
        return ",".join(PATHS).encode()

    def xs_cu_sweep_expected(self, k, lds_bytes, out):
        self.expected_calls += 1
        out[0], out[1], out[2] = CU_EXPECTED
        return 0

    def xs_matrix_sweep_expected(self, mask, out):
        self.expected_calls += 1
        for i, v in enumerate(MATRIX_EXPECTED):
            out[i] = v if mask >> i & 1 else 0
        return 0

    def xs_lane_sweep_expected(self, mask, seed, out):
        self.expected_calls += 1
        for i, v in enumerate(LANE_EXPECTED):
            out[i] = v if mask >> i & 1 else 0
        return 0

    def xs_regfile_sweep_expected(self, seed, out):
        self.expected_calls += 1
        out._obj.value = REGFILE_EXPECTED
        return 0

    def _launch(self, dev, blocks, *rest):
        buf, n, ms = rest[-3:]
        i = len(self.launches)
        assert i < len(self.rounds), "one launch too many"
        self.launches.append(blocks)
        if self.rcs[i]:
            return self.rcs[i]
        recs = self.rounds[i]
        assert len(recs) <= blocks and len(buf) >= WORDS[self.sweep] * blocks
        for r, words in enumerate(recs):
            assert len(words) == WORDS[self.sweep]
            for j, w in enumerate(words):
                buf[WORDS[self.sweep] * r + j] = w
        n._obj.value = len(recs)
        ms._obj.value = self.ms[i]
        return 0


def probe_over(lib) -> HipProbe:
    p = HipProbe.__new__(HipProbe)
    p.lib = lib
    return p


def run(lib, **kw):
    return getattr(probe_over(lib), f"{lib.sweep}_sweep")(0, **kw)


SWEEPS = list(WORDS)


@pytest.mark.parametrize("sweep", SWEEPS)
def test_second_round_covers_the_unseen_cu(sweep):
    lib = FakeLib(sweep, [[healthy(sweep, x, c) for x, c in ALL[:3]], [healthy(sweep, x, c) for x, c in ALL]],
                  ms=[1.5, 2.25])
    out = run(lib)
    s = out["summary"]
    assert lib.launches == [4 * CUS, 4 * CUS] and lib.expected_calls == 1
    assert [(r["xcd"], r["cu"]) for r in out["records"]] == ALL[:3] + ALL  # both rounds' records are kept
    assert s["covered"] and s["rounds"] == 2 and s["ms"] == 3.75 and s["blocks"] == 4 * CUS
    assert s["bad_xcds"] == [] and s["cus_seen"] == CUS and s["uncovered"] == {0: 0, 1: 0}


@pytest.mark.parametrize("sweep", SWEEPS)
def test_never_covered_stops_at_max_rounds(sweep):
    lib = FakeLib(sweep, [[healthy(sweep, x, c) for x, c in ALL[:3]]] * 3)
    s = run(lib, max_rounds=3)["summary"]
    assert len(lib.launches) == 3
    assert not s["covered"] and s["rounds"] == 3 and s["ms"] == 3.0
    assert s["uncovered"] == {0: 0, 1: 1} and s["bad_xcds"] == []  # unseen is not failed


@pytest.mark.parametrize("sweep", SWEEPS)
@pytest.mark.parametrize("max_rounds", [1, 4, 9])
def test_a_grid_that_cannot_cover_is_launched_once(sweep, max_rounds):
    lib = FakeLib(sweep, [[healthy(sweep, 1, 0)]])
    out = run(lib, blocks=1, max_rounds=max_rounds)
    assert lib.launches == [1]
    assert out["summary"]["rounds"] == 1 and not out["summary"]["covered"] and out["summary"]["blocks"] == 1
    assert len(out["records"]) == 1


@pytest.mark.parametrize("sweep", SWEEPS)
def test_host_digest_overrides_a_device_pass(sweep):
    word, bits, key, names = SPOILT[sweep]
    recs = [healthy(sweep, x, c) for x, c in ALL]
    recs[2][word] ^= 0x40  # XCD 1, CU 0: the device said fail == 0
    out = run(FakeLib(sweep, [recs]))
    s = out["summary"]
    assert [r["fail"] for r in out["records"]] == [0, 0, bits, 0]
    assert s["bad_xcds"] == [1] and s["xcds"][1]["failed_cus"] == [0] and s["xcds"][1]["fail_bits"] == bits
    assert s["xcds"][0]["fail_bits"] == 0 and s["covered"] and s["rounds"] == 1
    if key:
        assert s[key] == names and s["xcds"][1][key] == names and s["xcds"][0][key] == []


def test_regfile_digest_counts_only_when_no_cell_was_named():
    recs = [healthy("regfile", x, c) for x, c in ALL]
    recs[1][3], recs[1][4], recs[1][6], recs[1][7] = 1, 64, 7, 0x10  # a VGPR cell named by the device
    recs[1][8] ^= 0x40
    out = run(FakeLib("regfile", [recs]))
    assert [r["fail"] for r in out["records"]] == [0, 1, 0, 0]
    assert out["summary"]["failed_files"] == ["vgpr"] and out["summary"]["bad_cells"] == 64


@pytest.mark.parametrize("sweep", SWEEPS)
def test_an_error_on_the_second_launch_is_raised(sweep):
    lib = FakeLib(sweep, [[healthy(sweep, x, c) for x, c in ALL[:3]], []], rcs=[0, -7])
    with pytest.raises(ProbeError) as e:
        run(lib)
    assert e.value.rc == -7 and len(lib.launches) == 2
    assert str(e.value) == f"{sweep}_sweep failed (-7): boom from {sweep}"
    bad = FakeLib(sweep, [[]], rcs=[-1000])
    with pytest.raises(ProbeError) as e:
        run(bad)
    assert e.value.rc == -1000 and str(e.value) == f"{sweep}_sweep failed (-1000): bad arguments"
