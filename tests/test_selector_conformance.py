"""Label and field selectors on both API servers held to an independent
reference (selector_ref.py: the grammar of k8s.io/apimachinery's pkg/labels
and pkg/fields): csrc/apiserver/selectors.cc through the bindings, its Python
twin control/selectors.py, and both over HTTP."""
import collections
import http.client
import json
from urllib.parse import quote

import pytest

from flex_gpu_scheduler_amd._native import native
from flex_gpu_scheduler_amd.control import ApiServer
from flex_gpu_scheduler_amd.control import selectors as py_selectors
from flex_gpu_scheduler_amd.models import make_pod

import selector_ref
from patch_selector_cases import (FIELD_OBJECTS, FIELD_STRINGS, FIELD_TABLE, L_OPERATORS, LABEL_OBJECTS, LABEL_STRINGS,
                                  LABEL_TABLE, REFUSED)

X = native()


def names(objects, match):
    return [o["metadata"]["name"] for o in objects if match(o)]


# --------------------------------------------- the four things under test --
def reference_labels(s):
    """(requirements, names of LABEL_OBJECTS that match) or REFUSED."""
    try:
        reqs = selector_ref.parse_labels(s)
    except selector_ref.Refused:
        return REFUSED
    return reqs, names(LABEL_OBJECTS, lambda o: selector_ref.labels_match(reqs, o))


def native_labels(s):
    try:
        reqs = X.parse_selector(s)
    except ValueError:
        return REFUSED
    return reqs, names(LABEL_OBJECTS, lambda o: X.labels_match(s, o))


def python_labels(s):
    try:
        reqs = [(r.key, r.op, list(r.values)) for r in py_selectors.parse_selector(s)]
        match = py_selectors.label_matcher(s) or (lambda o: True)
    except ValueError:
        return REFUSED
    return reqs, names(LABEL_OBJECTS, match)


def reference_fields(s):
    """Names of FIELD_OBJECTS that match, or REFUSED."""
    try:
        reqs = selector_ref.parse_fields(s)
    except selector_ref.Refused:
        return REFUSED
    return names(FIELD_OBJECTS, lambda o: selector_ref.fields_match(reqs, o))


def native_fields(s):
    try:
        return names(FIELD_OBJECTS, lambda o: X.fields_match(s, o))
    except ValueError:
        return REFUSED


def python_fields(s):
    try:
        match = py_selectors.field_matcher(s) or (lambda o: True)
    except ValueError:
        return REFUSED
    return names(FIELD_OBJECTS, match)


LABELS = {"native": native_labels, "python": python_labels}
FIELDS = {"native": native_fields, "python": python_fields}


def assert_labels_like_reference(parse, s):
    want, got = reference_labels(s), parse(s)
    if want is REFUSED:
        assert got is REFUSED, (s, "the reference refuses; got", got)
    else:
        assert got is not REFUSED, (s, "the reference gives", want)
        assert [tuple(r) for r in got[0]] == want[0] and got[1] == want[1], (s, got, want)


# ------------------------------------------------------------------ tables --
@pytest.mark.parametrize("s,reqs,matching", LABEL_TABLE, ids=[repr(r[0])[:40] for r in LABEL_TABLE])
def test_reference_reads_labels_as_the_table_says(s, reqs, matching):
    got = reference_labels(s)
    assert got is REFUSED if reqs is REFUSED else got == (reqs, matching), got


@pytest.mark.parametrize("s,reqs,matching", FIELD_TABLE, ids=[repr(r[0])[:40] for r in FIELD_TABLE])
def test_reference_reads_fields_as_the_table_says(s, reqs, matching):
    if reqs is REFUSED:
        with pytest.raises(selector_ref.Refused):
            selector_ref.parse_fields(s)
    else:
        assert selector_ref.parse_fields(s) == reqs and reference_fields(s) == matching


@pytest.mark.parametrize("impl", LABELS)
@pytest.mark.parametrize("s", [r[0] for r in LABEL_TABLE], ids=[repr(r[0])[:40] for r in LABEL_TABLE])
def test_label_table(impl, s):
    assert_labels_like_reference(LABELS[impl], s)


@pytest.mark.parametrize("impl", FIELDS)
@pytest.mark.parametrize("s", [r[0] for r in FIELD_TABLE], ids=[repr(r[0])[:40] for r in FIELD_TABLE])
def test_field_table(impl, s):
    assert FIELDS[impl](s) == reference_fields(s), s


def test_none_is_the_empty_selector():
    assert py_selectors.parse_selector(None) == [] and py_selectors.label_matcher(None) is None
    assert py_selectors.field_matcher(None) is None and py_selectors.field_matcher(",") is None


# --------------------------------------------------------------- generated --
def test_generated_selectors_land_on_both_sides():
    """Conditions on the generators, from the reference alone (seed 63, 2000
    label selectors: 1124 accepted, each operator in at least 203 of them;
    seed 64, 1000 field selectors: 768 accepted)."""
    accepted, spelled, verdicts = 0, collections.Counter(), collections.Counter()
    for s in LABEL_STRINGS:
        got = reference_labels(s)
        if got is REFUSED:
            continue
        accepted += 1
        # In an accepted selector a symbol of these is an operator; `in` and `notin` count where the parser read one.
        used = {lit for kind, lit in selector_ref.lex(s) if kind == "sym" and lit in L_OPERATORS} | \
            {op for _, op, _ in got[0] if op in ("in", "notin")}
        spelled.update(used)
        verdicts.update([len(got[1]) > 0])
    print(f"labels: accepted {accepted} of {len(LABEL_STRINGS)}; selectors per operator {dict(spelled)}; "
          f"matching something {verdicts[True]}, nothing {verdicts[False]}")
    assert accepted >= len(LABEL_STRINGS) // 4 and len(LABEL_STRINGS) - accepted >= len(LABEL_STRINGS) // 4
    for op in L_OPERATORS:
        assert spelled[op] >= 50, (op, spelled[op])
    assert verdicts[True] >= 100 and verdicts[False] >= 100
    ok = [reference_fields(s) for s in FIELD_STRINGS]
    accepted = sum(v is not REFUSED for v in ok)
    print(f"fields: accepted {accepted} of {len(FIELD_STRINGS)}")
    assert accepted >= len(ok) // 4 and len(ok) - accepted >= len(ok) // 5
    assert sum(1 for v in ok if v is not REFUSED and v) >= 100 and sum(1 for v in ok if v == []) >= 100


@pytest.mark.parametrize("impl", LABELS)
def test_generated_label_selectors(impl):
    for s in LABEL_STRINGS:
        assert_labels_like_reference(LABELS[impl], s)


@pytest.mark.parametrize("impl", FIELDS)
def test_generated_field_selectors(impl):
    for s in FIELD_STRINGS:
        assert FIELDS[impl](s) == reference_fields(s), s


# -------------------------------------------------------------------- HTTP --
@pytest.fixture(params=[True, False], ids=["native-http", "python-http"])
def server(request, store):
    srv = ApiServer(store, native_http=request.param).start()
    assert srv.native_http is request.param
    yield srv
    srv.stop()


def get(conn, query):
    conn.request("GET", "/api/v1/namespaces/default/pods?" + query)
    r = conn.getresponse()
    return r.status, r.getheader("Transfer-Encoding"), json.loads(r.read())


def test_http_label_selectors(server, store):
    """Every row of the table as a LIST: a refused one is 400 BadRequest,
    an accepted one returns the pods the table names."""
    pods = [o for o in LABEL_OBJECTS if o["metadata"].get("labels", {}) is not None]
    for o in pods:
        store.create("pods", make_pod(o["metadata"]["name"], labels=o["metadata"].get("labels")))
    conn = http.client.HTTPConnection(*server.address)
    wrong = []  # every row that goes wrong, not the first
    for s, reqs, matching in LABEL_TABLE:
        status, _, body = get(conn, "labelSelector=" + quote(s, safe=""))
        if reqs is REFUSED:
            if (status, body.get("kind"), body.get("reason")) != (400, "Status", "BadRequest"):
                wrong.append((s, "refused by the reference", status))
        elif status != 200:
            wrong.append((s, "accepted by the reference", status, body.get("reason")))
        elif sorted(p["metadata"]["name"] for p in body["items"]) != sorted(n for n in matching if n != "null"):
            wrong.append((s, [p["metadata"]["name"] for p in body["items"]], matching))
    assert not wrong, wrong


def test_http_watch_with_a_malformed_selector_is_refused_before_the_stream(server, store):
    store.create("pods", make_pod("p", labels={"a": "1"}))
    conn = http.client.HTTPConnection(*server.address)
    for query in ["labelSelector=" + quote("a in (1"), "labelSelector=a%2C", "fieldSelector=metadata.name",
                  "fieldSelector=" + quote("metadata.name=p\\q")]:
        status, chunked, body = get(conn, "watch=true&timeoutSeconds=1&" + query)
        assert (status, chunked, body["kind"], body["reason"]) == (400, None, "Status", "BadRequest"), query


def test_http_field_selectors(server, store):
    """A string, a bool, an integer, a null and a missing path, and the rows
    of the table that need no odd pod."""
    store.create("pods", {**make_pod("p"), "x": {"s": "n1", "b": True, "i": 7, "n": None, "neg": -3, "f": False}})
    store.create("pods", {**make_pod("p,q"), "x": "scalar"})
    store.create("pods", make_pod(" p"))
    conn = http.client.HTTPConnection(*server.address)
    rows = [("x.s=n1", ["p"]), ("x.s==n1", ["p"]), ("x.s!=n1", [" p", "p,q"]), ("x.b=true", ["p"]), ("x.b=True", []),
            ("x.f=false", ["p"]), ("x.i=7", ["p"]), ("x.neg=-3", ["p"]), ("x.n=", [" p", "p", "p,q"]),
            ("x.missing=", [" p", "p", "p,q"]), ("x.missing!=", []), ("x.s.deeper=", [" p", "p", "p,q"]), ("x=scalar", ["p,q"]),
            ("metadata.name= p", [" p"]), ("metadata.name=p ", []), ("metadata.name=p\\,q", ["p,q"]),
            ("metadata.name=p,x.i=7,,", ["p"]), ("metadata.name!=p,metadata.namespace=default", [" p", "p,q"]),
            ("metadata.name", None), ("metadata.name in (p)", None), ("metadata.name=p\\", None), ("metadata.name=p=q", None),
            ("metadata.name=p\\q", None)]
    wrong = []
    for s, matching in rows:
        assert (reference_fields(s) is REFUSED) == (matching is None), s
        status, _, body = get(conn, "fieldSelector=" + quote(s, safe=""))
        if matching is None:
            if (status, body.get("reason")) != (400, "BadRequest"):
                wrong.append((s, "refused by the reference", status))
        elif status != 200 or sorted(p["metadata"]["name"] for p in body["items"]) != matching:
            wrong.append((s, status, [p["metadata"]["name"] for p in body.get("items", [])], matching))
    assert not wrong, wrong
