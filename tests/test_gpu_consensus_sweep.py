"""k_consensus_sweep and k_consensus_probe on the GPU (csrc/hip/consensus_sweep.hip).

The sweep has no expected values, so nothing here is compared bit for bit with
a host table. A clean sweep must reach every CU, be unanimous and repeat
itself; an injected part must be localised to its CU, XCD and part by the vote;
and one workgroup's dump of every part is held to properties that do not depend
on the bits no document fixes (tests/consensus_sweep_ref.py): the stochastic
roundings land on a neighbour of the exact value, the transcendentals are
near numpy's, IEEE-754's classes hold on the edge operands, the full division
is correctly rounded, and the dump's digest is the record's. One workgroup of
256 threads and two rounds is the smallest shape at which every operand class
occurs (two rounds give each stochastic-rounding form more than 256 operands in
the middle of a gap); a sweep test is one launch at the default grid."""
import numpy as np
import pytest

import consensus_sweep_ref as ref
from flex_gpu_scheduler_amd.control.node_agent import GpuHealth, hip_health_fn
from flex_gpu_scheduler_amd.ops.hip_probe import CONSENSUS_ROUNDS, probe

pytestmark = pytest.mark.gpu
ROUNDS = 2  # of the probes

# The largest error of each raw transcendental over the probe's dumps at both
# seeds, measured on an MI355X (profiles/consensus_sweep_defaults.md): 1 ULP for
# the f32 forms, 2^-23 absolute for sin and cos, 0 for the f16 forms, and for
# the f64 forms, which are seeds of a refinement and not results, 220,167,674
# (rcp), 207,353,454 (rsq) and 157,855,731 (sqrt) ULP. The bound is the
# smallest power of two at or above twice the maximum. For the f16 forms twice
# the maximum is 0, below every power of two; an error in ULP of a rounded
# result is a whole number, so the bound there is the least error there is, 1,
# and it is strict: below 1 is 0, what was measured.
# It catches a wrong operand or register, which is off by far more; it does not
# grade the hardware.
TRANS_BOUNDS = {
    "v_exp_f32": 2.0, "v_log_f32": 2.0, "v_rcp_f32": 2.0, "v_rsq_f32": 2.0, "v_sqrt_f32": 2.0, "v_rcp_iflag_f32": 2.0,
    "v_sin_f32": 2.0 ** -22, "v_cos_f32": 2.0 ** -22,
    "v_rcp_f64": 2.0 ** 29, "v_rsq_f64": 2.0 ** 29, "v_sqrt_f64": 2.0 ** 29,
    "v_rcp_f16": 1.0, "v_rsq_f16": 1.0, "v_sqrt_f16": 1.0, "v_exp_f16": 1.0, "v_log_f16": 1.0,
}
STRICT = {k for k in TRANS_BOUNDS if k.endswith("_f16")}


@pytest.fixture(scope="module")
def p():
    return probe()


@pytest.fixture(scope="module")
def cus(p):
    return int(p.props(0)["computeUnits"])


@pytest.fixture(scope="module")
def clean(p):
    return {seed: p.consensus_sweep(0, seed=seed) for seed in ref.SEEDS}


@pytest.fixture(scope="module")
def dumps(p):
    """One workgroup's dump of every part at both seeds, taken once."""
    return {(part, seed): p.consensus_probe(0, part, seed, rounds=ROUNDS) for part in ref.PARTS for seed in ref.SEEDS}


@pytest.fixture(scope="module")
def target(clean):
    """(xcd, cu key) of one CU the clean sweep reached."""
    keys = sorted({(r["xcd"], r["cu"]) for r in clean[ref.SEEDS[0]]["records"]})
    return keys[len(keys) // 7]


# ------------------------------------------------------------------ sweeps
@pytest.mark.parametrize("seed", ref.SEEDS)
def test_a_default_sweep_reaches_every_cu_and_is_unanimous(clean, cus, seed):
    s = clean[seed]["summary"]
    assert s["covered"] and not any(s["uncovered"].values()) and s["cus_seen"] == cus
    assert s["undecided"] == [] and s["bad_xcds"] == [] and s["failed_parts"] == []
    assert s["parts"] == ref.PARTS and s["seed"] == seed and s["operand_rounds"] == CONSENSUS_ROUNDS
    assert set(s["consensus"]) == set(ref.PARTS)
    assert all(r["fail"] == 0 and r["simd_mask"] == 0xF for r in clean[seed]["records"])
    want = {f: int(s["consensus"][f], 16) for f in ref.PARTS}
    assert all(r["digests"] == want for r in clean[seed]["records"])


def test_two_launches_agree_and_two_seeds_differ_in_every_part(p, clean):
    a, b = (clean[seed]["summary"]["consensus"] for seed in ref.SEEDS)
    again = p.consensus_sweep(0, seed=ref.SEEDS[0])["summary"]
    assert again["consensus"] == a and again["undecided"] == [] and again["bad_xcds"] == []
    assert all(a[f] != b[f] for f in ref.PARTS), (a, b)


def test_an_injected_part_fails_exactly_its_cu_xcd_and_part(p, clean, target):
    xcd, cu = target
    out = p.consensus_sweep(0, inject=(xcd, cu), inject_parts=["sr"], max_rounds=1)
    hit = [r for r in out["records"] if (r["xcd"], r["cu"]) == (xcd, cu)]
    rest = [r for r in out["records"] if (r["xcd"], r["cu"]) != (xcd, cu)]
    assert hit and all(r["fail"] == 1 << ref.PARTS.index("sr") for r in hit)
    assert all(r["fail"] == 0 for r in rest)
    s = out["summary"]
    assert s["bad_xcds"] == [xcd] and s["xcds"][xcd]["failed_cus"] == [cu]
    assert s["xcds"][xcd]["failed_parts"] == ["sr"] and s["failed_parts"] == ["sr"] and s["undecided"] == []
    assert s["consensus"] == clean[ref.SEEDS[0]]["summary"]["consensus"]  # the majority is untouched
    v = hip_health_fn(consensus=True, consensus_args={"inject": (xcd, None, ["mfma", "trans"]), "max_rounds": 1})(0)
    assert isinstance(v, GpuHealth) and not v.ok and v.bad_xcds == frozenset({xcd})
    assert v.detail["consensusFaults"] == {xcd: ["trans", "mfma"]}


def test_a_subset_of_parts_leaves_the_others_digests_zero_and_unjudged(p, clean):
    seed = ref.SEEDS[1]
    out = p.consensus_sweep(0, parts=["ldsx", "div"], seed=seed, max_rounds=1)
    s = out["summary"]
    full = clean[seed]["summary"]["consensus"]
    assert s["parts"] == ["div", "ldsx"] and s["consensus"] == {"div": full["div"], "ldsx": full["ldsx"]}
    assert s["undecided"] == [] and s["bad_xcds"] == []
    want = {f: (int(full[f], 16) if f in ("div", "ldsx") else 0) for f in ref.PARTS}
    assert all(r["digests"] == want and r["fail"] == 0 for r in out["records"])


def test_the_runtime_reports_no_scratch_and_one_workgroup_per_cu(p):
    info = p.consensus_sweep_info(0)
    assert info["scratch_bytes"] == 0 and info["blocks_per_cu"] == 1
    assert info["lds_bytes"] > 80 << 10 and info["num_regs"] <= 512


# ------------------------------------------------------- one workgroup's dump
@pytest.mark.parametrize("part", ref.PARTS)
def test_the_dumps_digest_is_the_records(p, dumps, part):
    for seed in ref.SEEDS:
        d = dumps[part, seed]
        assert d.shape == (ROUNDS, ref.shape(part)[1], ref.BLOCK)
        out = p.consensus_sweep(0, parts=[part], blocks=1, seed=seed, rounds=ROUNDS, max_rounds=1)
        (rec,) = out["records"]
        assert rec["digests"] == {f: (ref.digest(d) if f == part else 0) for f in ref.PARTS}
        assert out["summary"]["undecided"] == [part]  # one CU is no vote


@pytest.mark.parametrize("part", ["ldsx", "mfma", "smfmac"])
def test_every_word_of_the_dump_is_written_and_the_seeds_differ(dumps, part):
    a, b = (dumps[part, seed] for seed in ref.SEEDS)
    assert (a != 0xFFFFFFFF).all() and (b != 0xFFFFFFFF).all()  # the poison the dump is launched with
    same_rows = [(r, row) for r in range(ROUNDS) for row in range(a.shape[1]) if np.array_equal(a[r, row], b[r, row])]
    assert same_rows == []
    assert not np.array_equal(a[0], a[1])  # nor do two rounds repeat each other


@pytest.mark.parametrize("seed", ref.SEEDS)
def test_smfmac_the_two_abid_encodings_give_the_same_tile(dumps, seed):
    """A step's result is two tiles, one per abid encoding, from the same
    operands. On the MI355X abid selects nothing at these shapes
    (profiles/consensus_sweep_defaults.md), so the tiles are equal: a CU on which
    they differ decodes the field differently from the rest."""
    d = dumps["smfmac", seed]
    for i, (_, name, words, _) in enumerate(ref.steps_of("smfmac")):
        row, n = ref.rows_of("smfmac", i)
        assert n == words and np.array_equal(d[:, row:row + n // 2], d[:, row + n // 2:row + n]), name


@pytest.mark.parametrize("seed", ref.SEEDS)
def test_sr_every_result_is_a_neighbour_of_the_exact_value_and_both_occur(dumps, seed):
    findings = ref.sr_findings(dumps["sr", seed], seed)
    for line in findings[:20]:
        print(line)
    assert findings == []


def test_trans_is_near_numpy(dumps):
    worst = {}
    for seed in ref.SEEDS:
        for name, err in ref.trans_errors(dumps["trans", seed], seed).items():
            worst[name] = max(worst.get(name, 0.0), err)
    print({k: (v, TRANS_BOUNDS[k]) for k, v in worst.items()})
    assert set(worst) == set(TRANS_BOUNDS)
    assert {k: v for k, v in worst.items() if not (v < TRANS_BOUNDS[k] if k in STRICT else v <= TRANS_BOUNDS[k])} == {}


@pytest.mark.parametrize("seed", ref.SEEDS)
def test_edge_keeps_the_classes_ieee_754_fixes(dumps, seed):
    findings = ref.edge_findings(dumps["edge", seed], seed)
    for line in findings[:20]:
        print(line)
    assert findings == []


@pytest.mark.parametrize("seed", ref.SEEDS)
def test_div_the_full_sequence_is_the_correctly_rounded_quotient(dumps, seed):
    findings = ref.div_findings(dumps["div", seed], seed)
    for line in findings[:20]:
        print(line)
    assert findings == []
