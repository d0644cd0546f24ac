"""What `Pod::from_json` promises, as a plain Python model written from the
Kubernetes rules (not from csrc/api/types.cc), and the hostile pods that
tests/test_pod_decode.py and the sanitizer driver feed it.

The decoder is lenient where the API server has already validated: a field
of the wrong JSON type reads as if it were missing. It is never sloppy with
numbers: an integer field saturates, an annotation that does not fit an int
is unparsable as a whole, and a quantity is exact.

- apiserver defaulting: a limit without a request is also the request.
- request (computePodResourceRequest): max(sum of containers, each init
  container), plus overhead. cpu counts in milli-units and everything else
  in units, each quantity rounded up once, when it is read.
- non-zero request (pkg/scheduler/util/non_zero.go): a container without a
  cpu (memory) request counts as 100m (200Mi); a pod without containers as 0.
- QoS (v1qos.GetPodQOS) over cpu and memory of containers and init
  containers, for pods that pass validation (request <= limit).
- resourceVersion is a decimal string or a number.
- The GPU index annotation counts only on a pod with a GPU limit
  (amd.com/gpu, else amd.com/gpu-xcd, else amd.com/gpu-memory); the partition
  annotation only next to a usable index annotation.
"""
from __future__ import annotations

import copy
import re
from datetime import datetime, timedelta, timezone
from fractions import Fraction

from flex_gpu_scheduler_amd.models import make_container, make_pod

INT64_MAX, INT64_MIN = 2**63 - 1, -2**63
INT32_MAX, INT32_MIN = 2**31 - 1, -2**31
POD_GROUP_LABEL = "pod-group.scheduling.sigs.k8s.io"
GPU, GPU_XCD, GPU_MEMORY = "amd.com/gpu", "amd.com/gpu-xcd", "amd.com/gpu-memory"
INDEX_ANNOTATION, PARTITION_ANNOTATION = "amd.com/gpu-index", "amd.com/gpu-partitions"

_SUFFIX = {"n": Fraction(1, 10**9), "u": Fraction(1, 10**6), "m": Fraction(1, 1000), "": Fraction(1),
           "k": Fraction(10**3), "M": Fraction(10**6), "G": Fraction(10**9), "T": Fraction(10**12),
           "P": Fraction(10**15), "E": Fraction(10**18),
           "Ki": Fraction(2**10), "Mi": Fraction(2**20), "Gi": Fraction(2**30), "Ti": Fraction(2**40),
           "Pi": Fraction(2**50), "Ei": Fraction(2**60)}
_QUANTITY = re.compile(r"([+-]?(?:\d+\.?\d*|\.\d+))(?:([eE][+-]?\d+)|([numkMGTPE]i?|[KMGTPE]i)?)")


def quantity(text: str) -> Fraction:
    """A resource.Quantity string as an exact number; ValueError otherwise."""
    m = _QUANTITY.fullmatch(text)
    if not m or (m.group(3) or "") not in _SUFFIX:
        raise ValueError(f"not a quantity: {text!r}")
    if m.group(2):
        return Fraction(m.group(1)) * Fraction(10) ** int(m.group(2)[1:])
    return Fraction(m.group(1)) * _SUFFIX[m.group(3) or ""]


def _ceil(f: Fraction) -> int:
    return -((-f.numerator) // f.denominator)


def _sat(v: int, lo: int = INT64_MIN, hi: int = INT64_MAX) -> int:
    return max(lo, min(hi, v))


def _obj(v) -> dict:
    return v if isinstance(v, dict) else {}


def _arr(v) -> list:
    return v if isinstance(v, list) else []


def _s(v, dflt: str = "") -> str:
    return v if isinstance(v, str) else dflt


def _is_num(v) -> bool:
    return isinstance(v, (int, float)) and not isinstance(v, bool)


def integer(v, dflt: int = 0, lo: int = INT64_MIN, hi: int = INT64_MAX) -> int:
    """A JSON number as an integer field: toward zero, saturating."""
    if not _is_num(v):
        return dflt
    if isinstance(v, float):
        if v != v:
            return 0
        v = hi if v == float("inf") else lo if v == float("-inf") else int(v)
    return _sat(v, lo, hi)


def resource_list(v) -> dict[str, int]:
    """{"cpu": "500m"} in scheduler units (milli-cpu, units of the rest).
    Strings are quantities, numbers are themselves (a float is the number its
    shortest spelling denotes); any other value is skipped."""
    out = {}
    for name, q in _obj(v).items():
        if isinstance(q, str):
            exact = quantity(q)
        elif _is_num(q):
            exact = Fraction(repr(q)) if isinstance(q, float) else Fraction(q)
        else:
            continue
        out[name] = _sat(_ceil(exact * 1000 if name == "cpu" else exact))
    return out


def _add(a: dict, b: dict) -> None:
    for k, v in b.items():
        a[k] = _sat(a.get(k, 0) + v)


def _max(a: dict, b: dict) -> None:
    for k, v in b.items():
        a[k] = v if k not in a else max(a[k], v)


_RFC3339 = re.compile(r"(\d{4})-(\d\d)-(\d\d)[Tt ](\d\d):(\d\d):(\d\d)(?:\.(\d+))?(?:[Zz]|([+-])(\d\d):(\d\d))?")


def micros(v) -> int:
    """An RFC 3339 timestamp in microseconds since the epoch; 0 when unset
    or not a timestamp."""
    m = _RFC3339.fullmatch(v) if isinstance(v, str) else None
    if not m:
        return 0
    y, mo, d, h, mi, s = (int(m.group(i)) for i in range(1, 7))
    t = datetime(y, mo, d, h, mi, s, tzinfo=timezone.utc)
    if m.group(8):
        off = timedelta(hours=int(m.group(9)), minutes=int(m.group(10)))
        t = t - off if m.group(8) == "+" else t + off
    whole = (t - datetime(1970, 1, 1, tzinfo=timezone.utc)) // timedelta(seconds=1)
    return whole * 1_000_000 + int((m.group(7) or "0")[:6].ljust(6, "0"))


def _int_list(text: str):
    """"0,3" as non-negative int32s, or None when any token is not one."""
    out = []
    for tok in text.split(","):
        if not re.fullmatch(r"-?\d+", tok) or not 0 <= int(tok) <= INT32_MAX:
            return None
        out.append(int(tok))
    return out


def _partition_list(text: str):
    out = []
    for tok in text.split(","):
        pair = tok.split(":")
        ints = _int_list(",".join(pair)) if len(pair) == 2 else None
        if ints is None:
            return None
        out.append((ints[0], ints[1]))
    return out


def decode(pod) -> dict:
    """The fields of `pod_summary` that follow from the rules above."""
    md, spec, status = _obj(_obj(pod).get("metadata")), _obj(_obj(pod).get("spec")), _obj(_obj(pod).get("status"))
    labels = {k: _s(v) for k, v in _obj(md.get("labels")).items()}
    annotations = {k: _s(v) for k, v in _obj(md.get("annotations")).items()}

    def container(c):
        res = _obj(_obj(c).get("resources"))
        limits, requests = resource_list(res.get("limits")), resource_list(res.get("requests"))
        for k, v in limits.items():
            requests.setdefault(k, v)
        ports = [integer(_obj(p).get("hostPort"), 0, INT32_MIN, INT32_MAX) for p in _arr(_obj(c).get("ports"))]
        return {"requests": requests, "limits": limits, "host_ports": sum(1 for p in ports if p > 0)}

    containers = [container(c) for c in _arr(spec.get("containers"))]
    inits = [container(c) for c in _arr(spec.get("initContainers"))]
    overhead = resource_list(spec.get("overhead"))

    def nonzero(c):
        return {"cpu": c["requests"].get("cpu") or 100, "memory": c["requests"].get("memory") or 200 * 2**20}

    request: dict = {}
    limits: dict = {}
    nz = {"cpu": 0, "memory": 0}
    for c in containers:
        _add(request, c["requests"])
        _add(limits, c["limits"])
        _add(nz, nonzero(c))
    for c in inits:
        _max(request, c["requests"])
        _max(nz, nonzero(c))
    _add(request, overhead)
    _add(nz, overhead)

    # v1qos.GetPodQOS, line by line: sums of the positive cpu and memory
    # requests and limits over all containers.
    q_requests: dict = {}
    q_limits: dict = {}
    guaranteed = True
    for c in containers + inits:
        for r in ("cpu", "memory"):
            if c["requests"].get(r, 0) > 0:
                q_requests[r] = q_requests.get(r, 0) + c["requests"][r]
        found = set()
        for r in ("cpu", "memory"):
            if c["limits"].get(r, 0) > 0:
                found.add(r)
                q_limits[r] = q_limits.get(r, 0) + c["limits"][r]
        if found != {"cpu", "memory"}:
            guaranteed = False
    if not q_requests and not q_limits:
        qos = "BestEffort"
    else:
        if guaranteed:
            guaranteed = all(r in q_limits and q_limits[r] == v for r, v in q_requests.items())
        qos = "Guaranteed" if guaranteed and len(q_requests) == len(q_limits) else "Burstable"

    gpus, partitions = [], []
    has_gpu_limit = limits.get(GPU, 0) > 0 or limits.get(GPU_XCD, 0) > 0 or GPU_MEMORY in limits
    if has_gpu_limit and INDEX_ANNOTATION in annotations:
        gpus = _int_list(annotations[INDEX_ANNOTATION]) or []
        if gpus and PARTITION_ANNOTATION in annotations:
            partitions = _partition_list(annotations[PARTITION_ANNOTATION]) or []

    rv = md.get("resourceVersion")
    if isinstance(rv, str):
        rv = _sat(int(rv)) if re.fullmatch(r"-?\d+", rv) else 0
    else:
        rv = integer(rv)

    scheduled_at = 0
    for c in _arr(status.get("conditions")):
        c = _obj(c)
        if c.get("type") == "PodScheduled" and c.get("status") == "True":
            scheduled_at = micros(c.get("lastTransitionTime"))

    return {
        "key": _s(md.get("namespace")) + "/" + _s(md.get("name")),
        "uid": _s(md.get("uid")),
        "resource_version": rv,
        "labels": labels,
        "annotations": annotations,
        "pod_group": labels.get(POD_GROUP_LABEL, ""),
        "priority": integer(spec.get("priority"), 0, INT32_MIN, INT32_MAX),
        "node_name": _s(spec.get("nodeName")),
        "scheduler_name": _s(spec.get("schedulerName"), "default-scheduler"),
        "phase": _s(status.get("phase"), "Pending"),
        "start_time": micros(status.get("startTime")),
        "scheduled_at": scheduled_at,
        "request": request,
        "nonzero_request": nz,
        "limits": limits,
        "qos": qos,
        "host_ports": sum(c["host_ports"] for c in containers),
        "gpus": gpus,
        "partitions": partitions,
    }


def summary_units(name: str, text: str) -> int:
    """A quantity string of `pod_summary` back in scheduler units."""
    v = quantity(text) * (1000 if name == "cpu" else 1)
    assert v.denominator == 1, (name, text)
    return int(v)


# ------------------------------------------------------------ hostile pods --
WRONG_TYPES = [None, True, 7, 2.5, "str", ["a"], {"a": "b"}]
HOSTILE_INTS = [1e300, -1e300, 2**31, -2**31 - 1, 2.5, -2.5, 2**63 - 1, -2**63]
HOSTILE_INDEX = ["4294967299", "-1", "", "1,,2", " 1", "1 ", "+1", "1,", ",1", "2147483648", "2147483647", "0x1", "1.0",
                 "99999999999999999999", "0,1,2"]
HOSTILE_PARTITIONS = ["3:x", "99999999999:1", ":", "3:4,", "3", "3:4:5", "-1:2", "3:-2", " 3:4", "3:4,3:4294967299",
                      "", "1:2147483647", "3:4,3:5"]
HOSTILE_QUANTITIES = ["abc", 5e-7, 1e300, "", "1.2.3", "5Xi", "1e", "--1", 0.1, 1e21, "9223372036854775807",
                      "1e40", 1e-300, "0.0000000001"]


def base_pod() -> dict:
    """A pod that uses every field the decoder reads."""
    pod = make_pod("p", namespace="ns", uid="u-1", priority=5, scheduler_name="xsched", node_name="n1",
                   labels={"app": "a", POD_GROUP_LABEL: "pg"},
                   annotations={INDEX_ANNOTATION: "3", PARTITION_ANNOTATION: "3:4,3:5"},
                   containers=[make_container("a", requests={"cpu": "500m"}, limits={"cpu": "1", "memory": "1Gi", GPU_XCD: "2"},
                                              ports=[{"containerPort": 80, "hostPort": 8080}, {"containerPort": 81}])],
                   init_containers=[make_container("i", requests={"cpu": "2", "memory": "512Mi"})],
                   overhead={"cpu": "100m"},
                   tolerations=[{"key": "k", "operator": "Exists", "tolerationSeconds": 30}],
                   affinity={"nodeAffinity": {"preferredDuringSchedulingIgnoredDuringExecution": [
                       {"weight": 10, "preference": {"matchExpressions": [{"key": "z", "operator": "In", "values": ["a"]}]}}]},
                       "podAffinity": {"preferredDuringSchedulingIgnoredDuringExecution": [
                           {"weight": 20, "podAffinityTerm": {"topologyKey": "zone",
                                                              "labelSelector": {"matchLabels": {"a": "b"}}}}]}})
    pod["metadata"]["resourceVersion"] = "42"
    pod["spec"]["topologySpreadConstraints"] = [{"maxSkew": 2, "topologyKey": "zone", "whenUnsatisfiable": "DoNotSchedule"}]
    pod["status"] = {"phase": "Running", "startTime": "2024-02-29T12:00:00Z",
                     "conditions": [{"type": "PodScheduled", "status": "True", "lastTransitionTime": "2024-02-29T11:59:58.25Z"}]}
    return pod


# Every place the decoder reads, as a path into base_pod().
FIELD_PATHS = [
    ("metadata",), ("metadata", "name"), ("metadata", "namespace"), ("metadata", "uid"), ("metadata", "resourceVersion"),
    ("metadata", "labels"), ("metadata", "labels", "app"), ("metadata", "labels", POD_GROUP_LABEL),
    ("metadata", "annotations"), ("metadata", "annotations", INDEX_ANNOTATION),
    ("metadata", "annotations", PARTITION_ANNOTATION),
    ("spec",), ("spec", "priority"), ("spec", "schedulerName"), ("spec", "nodeName"), ("spec", "overhead"),
    ("spec", "overhead", "cpu"), ("spec", "containers"), ("spec", "containers", 0), ("spec", "containers", 0, "resources"),
    ("spec", "containers", 0, "resources", "limits"), ("spec", "containers", 0, "resources", "limits", "cpu"),
    ("spec", "containers", 0, "resources", "limits", "memory"), ("spec", "containers", 0, "resources", "limits", GPU_XCD),
    ("spec", "containers", 0, "resources", "requests"), ("spec", "containers", 0, "resources", "requests", "cpu"),
    ("spec", "containers", 0, "ports"), ("spec", "containers", 0, "ports", 0),
    ("spec", "containers", 0, "ports", 0, "hostPort"), ("spec", "initContainers"), ("spec", "initContainers", 0),
    ("spec", "initContainers", 0, "resources", "requests", "memory"),
    ("spec", "tolerations"), ("spec", "tolerations", 0, "tolerationSeconds"), ("spec", "affinity"),
    ("spec", "topologySpreadConstraints"), ("spec", "topologySpreadConstraints", 0, "maxSkew"),
    ("status",), ("status", "phase"), ("status", "startTime"), ("status", "conditions"), ("status", "conditions", 0),
    ("status", "conditions", 0, "type"), ("status", "conditions", 0, "status"),
    ("status", "conditions", 0, "lastTransitionTime"),
]
INT_PATHS = [
    ("spec", "priority"), ("spec", "containers", 0, "ports", 0, "hostPort"),
    ("spec", "tolerations", 0, "tolerationSeconds"), ("spec", "topologySpreadConstraints", 0, "maxSkew"),
    ("spec", "affinity", "nodeAffinity", "preferredDuringSchedulingIgnoredDuringExecution", 0, "weight"),
    ("spec", "affinity", "podAffinity", "preferredDuringSchedulingIgnoredDuringExecution", 0, "weight"),
    ("metadata", "resourceVersion"),
]
QUANTITY_PATHS = [
    ("spec", "containers", 0, "resources", "limits", "cpu"), ("spec", "containers", 0, "resources", "limits", "memory"),
    ("spec", "containers", 0, "resources", "requests", "cpu"), ("spec", "overhead", "cpu"),
    ("spec", "initContainers", 0, "resources", "requests", "memory"),
]


def with_value(pod: dict, path: tuple, value) -> dict:
    out = copy.deepcopy(pod)
    at = out
    for k in path[:-1]:
        at = at[k]
    at[path[-1]] = value
    return out


def hostile_pods() -> list[tuple[str, dict]]:
    """(label, pod): every field with every wrong type, the integer fields
    with numbers that do not fit, the annotations and quantities with text
    and numbers that are not what they should be."""
    base = base_pod()
    out = []
    for path in FIELD_PATHS:
        for v in WRONG_TYPES:
            out.append((f"{'.'.join(map(str, path))}={v!r}", with_value(base, path, v)))
    for path in INT_PATHS:
        for v in HOSTILE_INTS:
            out.append((f"{'.'.join(map(str, path))}={v!r}", with_value(base, path, v)))
    for v in HOSTILE_INDEX:
        out.append((f"index={v!r}", with_value(base, ("metadata", "annotations", INDEX_ANNOTATION), v)))
    for v in HOSTILE_PARTITIONS:
        out.append((f"partitions={v!r}", with_value(base, ("metadata", "annotations", PARTITION_ANNOTATION), v)))
    for path in QUANTITY_PATHS:
        for v in HOSTILE_QUANTITIES:
            out.append((f"{'.'.join(map(str, path))}={v!r}", with_value(base, path, v)))
    for rv in ["9223372036854775808", "-9223372036854775809", "12abc", " 12", "", "1e3", "007"]:
        out.append((f"resourceVersion={rv!r}", with_value(base, ("metadata", "resourceVersion"), rv)))
    return out
