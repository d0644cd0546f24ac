"""JSON patch on both API servers held to an independent reference
(json_patch_ref.py: RFC 6902 over RFC 6901), the way the JSON parser is held
to json_ref.py: csrc/apiserver/json_patch.cc through the bindings, its Python
twin control.apiserver.apply_json_patch, and both over HTTP. Documents compare
type-exact (json_ref.same); over HTTP, where 1.0 is written `1`, by value."""
import collections
import copy
import http.client
import json
import os
import subprocess

import pytest

from flex_gpu_scheduler_amd import build_ext
from flex_gpu_scheduler_amd._native import native
from flex_gpu_scheduler_amd.control import ApiServer
from flex_gpu_scheduler_amd.control import apiserver as py_apiserver
from flex_gpu_scheduler_amd.models import make_pod

import json_patch_ref
import patch_selector_cases as cases
from json_ref import same
from patch_selector_cases import PATCH_TABLE, REFUSED

X = native()
SEED, COUNT = 6902, 2000
GENERATED = cases.patch_cases(SEED, COUNT)


def reference(doc, patch):
    try:
        return json_patch_ref.apply(doc, patch)
    except json_patch_ref.Refused:
        return REFUSED


def native_patch(doc, patch):
    """Through JSON text: the bindings would read a bare str as text anyway.
    Only the 422 ApiError (a RuntimeError here) counts as a refusal."""
    try:
        return X.apply_json_patch(json.dumps(doc), json.dumps(patch))
    except X.JsonError:
        raise
    except RuntimeError:
        return REFUSED


def python_patch(doc, patch):
    try:
        return py_apiserver.apply_json_patch(doc, patch)
    except py_apiserver.ApiError as e:
        assert (e.code, e.reason) == (422, "Invalid")
        return REFUSED


IMPLEMENTATIONS = {"native": native_patch, "python": python_patch}


def assert_like_reference(apply, doc, patch):
    want = reference(doc, patch)
    before, patch_before = copy.deepcopy(doc), copy.deepcopy(patch)
    got = apply(doc, patch)
    assert same(doc, before) and same(patch, patch_before), "the arguments were changed"
    if want is REFUSED:
        assert got is REFUSED, (doc, patch, "the reference refuses; got", got)
    else:
        assert got is not REFUSED, (doc, patch, "the reference gives", want)
        assert same(got, want), (doc, patch, got, want)


# ------------------------------------------------------------------ table --
@pytest.mark.parametrize("name,doc,patch,want", PATCH_TABLE, ids=[r[0] for r in PATCH_TABLE])
def test_reference_gives_what_the_table_says(name, doc, patch, want):
    """RFC 6902 Appendix A and the rows of json_patch_ref's header, each with
    its answer written out by hand: what keeps the reference honest."""
    before = copy.deepcopy(doc)
    got = reference(doc, patch)
    assert same(doc, before)
    assert (got is REFUSED) == (want is REFUSED)
    if want is not REFUSED:
        assert same(got, want), got


@pytest.mark.parametrize("impl", IMPLEMENTATIONS)
@pytest.mark.parametrize("name,doc,patch,want", PATCH_TABLE, ids=[r[0] for r in PATCH_TABLE])
def test_table(impl, name, doc, patch, want):
    assert_like_reference(IMPLEMENTATIONS[impl], doc, patch)


def test_pointer_tokens_spelled_out():
    T = json_patch_ref.tokens
    assert T("") == [] and T("/") == [""] and T("//") == ["", ""] and T("/a/") == ["a", ""]
    assert T("/~01") == ["~1"] and T("/~10") == ["/0"] and T("/~0~1") == ["~/"] and T("/a~1b/~0") == ["a/b", "~"]
    for bad in ["a", "~", "/~", "/~2", "/a~", "/~~0", " /a"]:
        with pytest.raises(json_patch_ref.Refused):
            T(bad)


# -------------------------------------------------------------- generated --
def first_refused(doc, patch):
    """The name of the operation at which the reference refuses."""
    if isinstance(patch, list):
        for k, op in enumerate(patch):
            if not json_patch_ref.applies(doc, patch[:k + 1]):
                if isinstance(op, dict) and isinstance(op.get("op"), str) and op["op"] in json_patch_ref.OPS:
                    return op["op"]
                break
    return "malformed"


def test_generated_cases_land_on_both_sides():
    """Conditions on the generator, from the reference alone (seed 6902, 2000
    cases: 887 accepted; per op accepted/refused add 303/91, remove 278/176,
    replace 355/100, move 246/265, copy 356/87, test 307/162; 232 malformed)."""
    accepted, refused, n = collections.Counter(), collections.Counter(), 0
    for doc, patch in GENERATED:
        if reference(doc, patch) is REFUSED:
            refused[first_refused(doc, patch)] += 1
        else:
            n += 1
            accepted.update(op["op"] for op in patch)
    print(f"accepted {n} of {len(GENERATED)}; per op accepted {dict(accepted)}, refused {dict(refused)}")
    assert n >= len(GENERATED) // 4 and len(GENERATED) - n >= len(GENERATED) // 4
    for op in json_patch_ref.OPS:
        assert accepted[op] >= 50 and refused[op] >= 50, (op, accepted[op], refused[op])
    assert all(1 <= len(p) <= 4 for _, p in GENERATED if isinstance(p, list) and p and isinstance(p[0], dict))


@pytest.mark.parametrize("impl", IMPLEMENTATIONS)
def test_generated(impl):
    for doc, patch in GENERATED:
        assert_like_reference(IMPLEMENTATIONS[impl], doc, patch)


# ------------------------------------------------------------------- HTTP --
@pytest.fixture(params=[True, False], ids=["native-http", "python-http"])
def server(request, store):
    srv = ApiServer(store, native_http=request.param).start()
    assert srv.native_http is request.param
    yield srv
    srv.stop()


POD = "/api/v1/namespaces/default/pods/p"


def request(conn, method, path, body=None, ctype="application/json-patch+json"):
    conn.request(method, path, body, {"Content-Type": ctype} if body is not None else {})
    r = conn.getresponse()
    return r.status, r.read()


def http_cases():
    """(id, members added to the pod, patch): the table's rows whose document
    is an object, and a slice of the generated ones."""
    out = [(name, doc, patch) for name, doc, patch, _ in PATCH_TABLE if isinstance(doc, dict)]
    out += [(f"generated-{k}", doc, patch) for k, (doc, patch) in enumerate(GENERATED[:400]) if isinstance(doc, dict)]
    return out


def test_http_patch_is_all_or_nothing(server, store):
    """Each case on a pod that carries the case's document as extra members.
    What the reference refuses is 422 Invalid, and so is a result that is no
    object or has another name: never a 500, never a 404 for a pod that is
    there. After a refusal the pod reads back byte for byte as before, its
    resourceVersion included. Every case that goes wrong is listed."""
    conn = http.client.HTTPConnection(*server.address)
    refused, wrong = 0, []
    for name, members, patch in http_cases():
        store.delete_all("pods", "default")
        store.create("pods", {**make_pod("p"), **members})
        status, before = request(conn, "GET", POD)
        assert status == 200
        cur = json.loads(before)
        want = reference(cur, patch)
        if want is not REFUSED and not (isinstance(want, dict) and isinstance(want.get("metadata"), dict) and all(
                want["metadata"].get(k) == cur["metadata"][k] for k in ("name", "namespace"))):
            want = REFUSED
        status, body = request(conn, "PATCH", POD, json.dumps(patch))
        answer = json.loads(body)
        after = request(conn, "GET", POD)
        if want is REFUSED:
            refused += 1
            if (status, answer.get("kind"), answer.get("reason")) != (422, "Status", "Invalid"):
                wrong.append((name, "refused by the reference", status, answer.get("reason")))
            elif after != (200, before):
                wrong.append((name, "the pod changed", after))
        elif status != 200:
            wrong.append((name, "accepted by the reference", status, answer.get("reason")))
        else:
            rv = answer["metadata"]["resourceVersion"]
            want["metadata"]["resourceVersion"] = rv
            if int(rv) <= int(cur["metadata"]["resourceVersion"]) or not json_patch_ref.equal(answer, want) or \
                    after[0] != 200 or not json_patch_ref.equal(json.loads(after[1]), answer):
                wrong.append((name, answer, want))
    assert not wrong, wrong[:20]
    assert refused > 100


@pytest.mark.parametrize("body", [b"", b"null", b"{}", b"7", b'"x"', b'[{"op":"replace","path":"","value":null}]',
                                  b'[{"op":"replace","path":"","value":[]}]', b'[{"op":"replace","path":"","value":{}}]',
                                  b'[{"op":"remove","path":"/metadata"}]',
                                  b'[{"op":"replace","path":"/metadata/name","value":"q"}]',
                                  b'[{"op":"add","path":"/metadata/namespace","value":"other"}]',
                                  b'[{"op":"add","path":"/x","value":1,"op":"remove"}]'])
def test_http_patch_bodies_that_are_no_patch_of_this_pod(server, store, body):
    store.create("pods", make_pod("p"))
    conn = http.client.HTTPConnection(*server.address)
    before = request(conn, "GET", POD)
    status, out = request(conn, "PATCH", POD, body)
    assert (status, json.loads(out)["reason"]) == (422, "Invalid"), out
    assert request(conn, "GET", POD) == before


# -------------------------------------------------------------- sanitizers --
def test_sanitized_driver_runs_the_whole_corpus(tmp_path):
    """csrc/tests/patch_selector_main.cc, built with AddressSanitizer and
    UndefinedBehaviorSanitizer, applies every patch of this file and parses
    and matches every selector of test_selector_conformance.py. Any finding
    aborts it."""
    corpus = tmp_path / "corpus.bin"
    patches = [(doc, patch) for _, doc, patch, _ in PATCH_TABLE] + GENERATED
    n = cases.write_corpus(corpus, patches, cases.LABEL_OBJECTS + cases.FIELD_OBJECTS,
                           [row[0] for row in cases.LABEL_TABLE] + cases.LABEL_STRINGS,
                           [row[0] for row in cases.FIELD_TABLE] + cases.FIELD_STRINGS)
    exe = build_ext.build_patch_fuzz(verbose=False)
    r = subprocess.run([str(exe), str(corpus)], capture_output=True, text=True, timeout=300)
    if r.returncode != 0 and "LeakSanitizer has encountered a fatal error" in r.stderr:
        # The leak check at exit needs ptrace, which some sandboxes deny; every other check has run by then.
        r = subprocess.run([str(exe), str(corpus)], capture_output=True, text=True, timeout=300,
                           env={**os.environ, "ASAN_OPTIONS": "detect_leaks=0"})
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert f"{n} records" in r.stdout
