"""`Pod::from_json` (through `pod_summary`) held, field by field, to the plain
model in pod_decode_ref.py: on generated pods, and on a table of hostile ones
where the only other acceptable answer is a ValueError."""
import copy
import json

import pytest
from hypothesis import HealthCheck, given, settings
from hypothesis import strategies as st

from flex_gpu_scheduler_amd._native import native

import pod_decode_ref as ref

X = native()
# Deterministic, like the rest of the suite; a slow machine is no finding.
PROPERTY = dict(deadline=None, derandomize=True, database=None, suppress_health_check=[HealthCheck.too_slow])

RESOURCE_FIELDS = ("request", "nonzero_request", "limits")
# template_hash and spec_hash have no model: they are checked by invariants.
PLAIN_FIELDS = ("key", "uid", "resource_version", "pod_group", "priority", "node_name", "scheduler_name", "phase",
                "start_time", "scheduled_at", "qos", "host_ports", "gpus")


def check_against_model(pod, summary):
    want = ref.decode(pod)
    for f in PLAIN_FIELDS:
        assert summary[f] == want[f] and type(summary[f]) is type(want[f]), (f, summary[f], want[f])
    assert [tuple(p) for p in summary["partitions"]] == want["partitions"]
    assert dict(summary["labels"]) == want["labels"]
    assert dict(summary["annotations"]) == want["annotations"]
    for f in RESOURCE_FIELDS:
        got = {k: ref.summary_units(k, v) for k, v in summary[f].items()}
        assert got == want[f], (f, summary[f], want[f])


# Quantities in whole scheduler units (milli-cpu, bytes, devices), sorted, as
# strings with suffixes and as bare JSON numbers. A request is drawn at or
# below its limit, as validation demands.
POOL = {
    "cpu": ["0", "100m", 0.25, "0.5", 1, "1500m", 2.5, "4", "1e1", 64],
    "memory": [0, "1Ki", "128974848", "128Mi", 2.5e8, "1G", "1Gi", 3221225472, "4Gi", "1Ti"],
    ref.GPU: ["0", 1, "2", 4, "8"],
    ref.GPU_XCD: [0, "1", 2, "4", "8"],
    ref.GPU_MEMORY: ["0", 16, "36", 72.0, "144"],
}


@st.composite
def containers(draw, init=False):
    reqs, lims = {}, {}
    for name in draw(st.lists(st.sampled_from(list(POOL)), unique=True, max_size=4)):
        pool = POOL[name]
        hi = draw(st.integers(0, len(pool) - 1))
        shape = draw(st.sampled_from(["limit", "request", "both", "equal"]))
        if shape in ("limit", "both", "equal"):
            lims[name] = pool[hi]
        if shape == "request":
            reqs[name] = pool[hi]
        elif shape == "both":
            reqs[name] = pool[draw(st.integers(0, hi))]
        elif shape == "equal":
            reqs[name] = pool[hi]
    c = {"name": draw(st.sampled_from(["a", "b", "c"])), "image": "busybox", "resources": {}}
    if reqs or draw(st.booleans()):
        c["resources"]["requests"] = reqs
    if lims:
        c["resources"]["limits"] = lims
    if not init:
        ports = draw(st.lists(st.fixed_dictionaries(
            {"containerPort": st.integers(1, 65535)},
            optional={"hostPort": st.sampled_from([0, 80, 8080, 65535]), "protocol": st.sampled_from(["TCP", "UDP"])}),
            max_size=3))
        if ports:
            c["ports"] = ports
    return c


TIMES = ["2024-02-29T12:00:00Z", "1999-12-31T23:59:59.999999Z", "2024-02-29T13:00:00+01:00", "2030-01-01T00:00:00.5-08:00"]
small_text = st.text(st.sampled_from("ab-./_é\U0001F600 0"), max_size=6)


@st.composite
def pods(draw):
    md = {"name": draw(small_text), "namespace": draw(st.sampled_from(["default", "team-a", ""]))}
    if draw(st.booleans()):
        md["uid"] = draw(small_text)
    rv = draw(st.sampled_from([None, "0", "42", 42, "9223372036854775807", 7.0]))
    if rv is not None:
        md["resourceVersion"] = rv
    labels = draw(st.dictionaries(small_text, small_text, max_size=3))
    if draw(st.booleans()):
        labels[ref.POD_GROUP_LABEL] = draw(st.sampled_from(["pg", "gang-1", ""]))
    if labels or draw(st.booleans()):
        md["labels"] = labels
    ann = draw(st.dictionaries(small_text, small_text, max_size=2))
    if draw(st.booleans()):
        ann[ref.INDEX_ANNOTATION] = draw(st.sampled_from(["0", "3", "0,1,2,3,4,5,6,7", "7,0", "x", "1,x"]))
        if draw(st.booleans()):
            ann[ref.PARTITION_ANNOTATION] = draw(st.sampled_from(["3:4,3:5", "0:0", "1:7", "3", "a:b"]))
    if ann:
        md["annotations"] = ann
    spec = {"containers": draw(st.lists(containers(), max_size=3))}
    inits = draw(st.lists(containers(init=True), max_size=2))
    if inits:
        spec["initContainers"] = inits
    overhead = draw(st.dictionaries(st.sampled_from(["cpu", "memory"]), st.sampled_from(["100m", "1", 2, "64Mi", 1024]),
                                    max_size=2))
    if overhead:
        spec["overhead"] = overhead
    for key, values in (("priority", [0, -5, 1000, 2**31 - 1]), ("schedulerName", ["xsched", "default-scheduler"]),
                        ("nodeName", ["n1", ""])):
        if draw(st.booleans()):
            spec[key] = draw(st.sampled_from(values))
    pod = {"apiVersion": "v1", "kind": "Pod", "metadata": md, "spec": spec}
    if draw(st.booleans()):
        status = {}
        if draw(st.booleans()):
            status["phase"] = draw(st.sampled_from(["Pending", "Running", "Succeeded"]))
        if draw(st.booleans()):
            status["startTime"] = draw(st.sampled_from(TIMES))
        conds = draw(st.lists(st.fixed_dictionaries({"type": st.sampled_from(["PodScheduled", "Ready"]),
                                                     "status": st.sampled_from(["True", "False"]),
                                                     "lastTransitionTime": st.sampled_from(TIMES)}), max_size=2))
        if conds:
            status["conditions"] = conds
        pod["status"] = status
    return pod


# 250 examples: about two seconds.
@settings(max_examples=250, **PROPERTY)
@given(pods())
def test_generated_pods_decode_like_the_model(pod):
    check_against_model(pod, X.pod_summary(pod))
    # The same pod as JSON text takes the parser's path into the decoder.
    check_against_model(pod, X.pod_summary(json.dumps(pod)))


HOSTILE = ref.hostile_pods()


@pytest.mark.parametrize("label,pod", HOSTILE, ids=[label for label, _ in HOSTILE])
def test_hostile_pod_decodes_like_the_model_or_is_refused(label, pod):
    """Either the model's value in every field, or a ValueError; never a
    wrapped or truncated number, and never another kind of failure."""
    text = json.dumps(pod)
    try:
        summary = X.pod_summary(text)
    except ValueError:
        return
    check_against_model(pod, summary)


def test_named_hostile_values():
    """The cases the model decides, spelled out."""
    base = ref.base_pod()
    index = ("metadata", "annotations", ref.INDEX_ANNOTATION)
    parts = ("metadata", "annotations", ref.PARTITION_ANNOTATION)
    assert X.pod_summary(base)["gpus"] == [3]
    assert X.pod_summary(base)["partitions"] == [(3, 4), (3, 5)]
    for bad in ["4294967299", "-1", "", "1,,2", " 1"]:  # 4294967299 is 2^32 + 3
        assert X.pod_summary(ref.with_value(base, index, bad))["gpus"] == [], bad
    for bad in ["3:x", "99999999999:1", ":"]:
        s = X.pod_summary(ref.with_value(base, parts, bad))
        assert s["gpus"] == [3] and s["partitions"] == [], bad
    priority = ("spec", "priority")
    for v, want in [(1e300, 2**31 - 1), (-1e300, -2**31), (2**31, 2**31 - 1), (2.5, 2), (-2.5, -2)]:
        assert X.pod_summary(json.dumps(ref.with_value(base, priority, v)))["priority"] == want, v
    port = ("spec", "containers", 0, "ports", 0, "hostPort")
    for v, want in [(1e300, 1), (-1e300, 0), (2**31, 1), (2.5, 1), (0.5, 0)]:
        assert X.pod_summary(json.dumps(ref.with_value(base, port, v)))["host_ports"] == want, v
    rv = ("metadata", "resourceVersion")
    for v, want in [(1e300, 2**63 - 1), (-1e300, -2**63), ("9223372036854775808", 2**63 - 1), (42, 42), ("42", 42)]:
        assert X.pod_summary(json.dumps(ref.with_value(base, rv, v)))["resource_version"] == want, v
    cpu = ("spec", "overhead", "cpu")
    assert X.pod_summary(ref.with_value(base, cpu, 5e-7))["request"]["cpu"] == "2001m"  # 2 (init) + 1m, rounded up
    with pytest.raises(ValueError):
        X.pod_summary(ref.with_value(base, cpu, "abc"))


def test_spec_hash_ignores_node_name_and_nothing_else():
    base = ref.base_pod()
    a = X.pod_summary(base)
    moved = X.pod_summary(ref.with_value(base, ("spec", "nodeName"), "elsewhere"))
    unbound = copy.deepcopy(base)
    del unbound["spec"]["nodeName"]
    assert a["spec_hash"] == moved["spec_hash"] == X.pod_summary(unbound)["spec_hash"]
    assert X.pod_summary(ref.with_value(base, ("spec", "priority"), 6))["spec_hash"] != a["spec_hash"]
    # Only a pending pod has a template hash; it covers namespace and annotations too.
    assert a["template_hash"] == 0
    t = X.pod_summary(unbound)["template_hash"]
    assert t != 0
    assert X.pod_summary(ref.with_value(unbound, ("metadata", "namespace"), "other"))["template_hash"] != t


# 150 examples: about a second.
@settings(max_examples=150, **PROPERTY)
@given(pods())
def test_hashes_survive_a_store_round_trip(pod):
    """dump() writes 1.0 as 1 and parse() reads an Int: the same pod, so the
    same equivalence class."""
    pod = copy.deepcopy(pod)
    pod["spec"].pop("nodeName", None)  # pending, so that template_hash is set
    pod["spec"]["weights"] = [1.0, 2.5, -0.0, 1e3]
    before = X.pod_summary(pod)
    after = X.pod_summary(X.json_parse(X.json_dump(pod)))
    assert before["template_hash"] == after["template_hash"] != 0
    assert before["spec_hash"] == after["spec_hash"]
    check_against_model(pod, after)
