"""The cases of test_json_patch_conformance.py and
test_selector_conformance.py: hand-written tables with the expected answer
spelled out, and seeded generators. Nothing here imports the code under
test; the generators consult the references (json_patch_ref, selector_ref)
only to aim: a path is drawn from the document as the earlier operations of
the same patch have left it."""
from __future__ import annotations

import copy
import json
import random
import struct

import json_patch_ref

REFUSED = object()


def _op(op, path, **kw):
    kw = {("from" if k == "src" else k): v for k, v in kw.items()}
    return {"op": op, "path": path, **kw}


# --------------------------------------------------------------- patches --
# (id, document, patch, patched document or REFUSED)
RFC6902_APPENDIX_A = [
    ("A.1-add-member", {"foo": "bar"}, [_op("add", "/baz", value="qux")], {"baz": "qux", "foo": "bar"}),
    ("A.2-add-element", {"foo": ["bar", "baz"]}, [_op("add", "/foo/1", value="qux")], {"foo": ["bar", "qux", "baz"]}),
    ("A.3-remove-member", {"baz": "qux", "foo": "bar"}, [_op("remove", "/baz")], {"foo": "bar"}),
    ("A.4-remove-element", {"foo": ["bar", "qux", "baz"]}, [_op("remove", "/foo/1")], {"foo": ["bar", "baz"]}),
    ("A.5-replace", {"baz": "qux", "foo": "bar"}, [_op("replace", "/baz", value="boo")], {"baz": "boo", "foo": "bar"}),
    ("A.6-move-value", {"foo": {"bar": "baz", "waldo": "fred"}, "qux": {"corge": "grault"}},
     [_op("move", "/qux/thud", src="/foo/waldo")], {"foo": {"bar": "baz"}, "qux": {"corge": "grault", "thud": "fred"}}),
    ("A.7-move-element", {"foo": ["all", "grass", "cows", "eat"]}, [_op("move", "/foo/3", src="/foo/1")],
     {"foo": ["all", "cows", "eat", "grass"]}),
    ("A.8-test-passes", {"baz": "qux", "foo": ["a", 2, "c"]},
     [_op("test", "/baz", value="qux"), _op("test", "/foo/1", value=2)], {"baz": "qux", "foo": ["a", 2, "c"]}),
    ("A.9-test-fails", {"baz": "qux"}, [_op("test", "/baz", value="bar")], REFUSED),
    ("A.10-add-nested", {"foo": "bar"}, [_op("add", "/child", value={"grandchild": {}})],
     {"foo": "bar", "child": {"grandchild": {}}}),
    ("A.11-unknown-member-ignored", {"foo": "bar"}, [_op("add", "/baz", value="qux", xyz=123)], {"foo": "bar", "baz": "qux"}),
    ("A.12-add-below-missing", {"foo": "bar"}, [_op("add", "/baz/bat", value="qux")], REFUSED),
    # A.13 has two "op" members. Which one a parser keeps is the parser's
    # business (test_json_conformance.py: the last); that leaves this patch.
    ("A.13-duplicate-op", {"foo": "bar"}, [_op("remove", "/baz", value="qux")], REFUSED),
    ("A.14-tilde-order", {"/": 9, "~1": 10}, [_op("test", "/~01", value=10)], {"/": 9, "~1": 10}),
    ("A.15-string-is-no-number", {"/": 9, "~1": 10}, [_op("test", "/~01", value="10")], REFUSED),
    ("A.16-add-array-value", {"foo": ["bar"]}, [_op("add", "/foo/-", value=["abc", "def"])], {"foo": ["bar", ["abc", "def"]]}),
]

A3 = {"a": [1, 2, 3]}
# The rows of the issue that brought these tests, then the rest of json_patch_ref's header.
PATCH_ROWS = [
    ("remove-root", {"a": 1}, [_op("remove", "")], REFUSED),
    ("op-is-a-number", {"a": 1}, [1], REFUSED),
    ("no-path", {"a": 1}, [{"op": "add", "value": {"x": 1}}], REFUSED),
    ("unknown-op-at-root", {"a": 1}, [_op("bogus", "", value=7)], REFUSED),
    ("add-without-value", {"a": 1}, [_op("add", "/b")], REFUSED),
    ("test-without-value", {"a": None}, [_op("test", "/a")], REFUSED),
    ("index-leading-zero", A3, [_op("replace", "/a/01", value=9)], REFUSED),
    ("index-negative", A3, [_op("remove", "/a/-1")], REFUSED),
    ("index-plus-sign", A3, [_op("replace", "/a/+1", value=9)], REFUSED),
    ("add-past-the-end", A3, [_op("add", "/a/9", value=9)], REFUSED),
    ("test-bool-against-number", {"a": True}, [_op("test", "/a", value=1)], REFUSED),
    ("tilde-2", {"a~2b": 1}, [_op("remove", "/a~2b")], REFUSED),
    ("tilde-at-the-end", {"a~": 1}, [_op("remove", "/a~")], REFUSED),
    ("patch-is-an-object", {"a": 1}, {"op": "remove", "path": "/a"}, REFUSED),
    ("patch-is-null", {"a": 1}, None, REFUSED),
    ("empty-patch", {"a": 1}, [], {"a": 1}),
    ("op-is-null", {"a": 1}, [{"op": None, "path": "/a"}], REFUSED),
    ("op-in-capitals", {"a": 1}, [_op("REMOVE", "/a")], REFUSED),
    ("path-is-a-number", {"a": 1}, [{"op": "remove", "path": 0}], REFUSED),
    ("path-without-slash", {"a": 1}, [_op("remove", "a")], REFUSED),
    ("from-is-missing", {"a": 1}, [_op("move", "/b")], REFUSED),
    ("from-is-a-number", {"a": 1}, [_op("copy", "/b", src=1)], REFUSED),
    ("from-with-tilde-2", {"a": 1}, [_op("copy", "/b", src="/~2")], REFUSED),
    ("add-null", {"a": 1}, [_op("add", "/b", value=None)], {"a": 1, "b": None}),
    ("test-null", {"a": None}, [_op("test", "/a", value=None)], {"a": None}),
    ("test-null-against-false", {"a": None}, [_op("test", "/a", value=False)], REFUSED),
    ("test-zero-against-false", {"a": 0}, [_op("test", "/a", value=False)], REFUSED),
    ("test-int-against-double", {"a": 1}, [_op("test", "/a", value=1.0)], {"a": 1}),
    ("test-double-against-int", {"a": [1.0, {"b": 2}]}, [_op("test", "/a", value=[1, {"b": 2.0}])], {"a": [1.0, {"b": 2}]}),
    ("test-members-unordered", {"a": {"x": 1, "y": 2}}, [_op("test", "/a", value={"y": 2, "x": 1})], {"a": {"x": 1, "y": 2}}),
    ("test-root", {"a": 1}, [_op("test", "", value={"a": 1})], {"a": 1}),
    ("test-missing", {"a": 1}, [_op("test", "/b", value=None)], REFUSED),
    ("add-replaces-a-member", {"a": 1}, [_op("add", "/a", value=2)], {"a": 2}),
    ("add-at-root", {"a": 1}, [_op("add", "", value={"b": 2})], {"b": 2}),
    ("replace-at-root", {"a": 1}, [_op("replace", "", value=[1])], [1]),
    ("replace-missing", {"a": 1}, [_op("replace", "/b", value=2)], REFUSED),
    ("remove-missing", {"a": 1}, [_op("remove", "/b")], REFUSED),
    ("add-at-the-length", A3, [_op("add", "/a/3", value=4)], {"a": [1, 2, 3, 4]}),
    ("add-at-zero", A3, [_op("add", "/a/0", value=0)], {"a": [0, 1, 2, 3]}),
    ("replace-at-the-length", A3, [_op("replace", "/a/3", value=4)], REFUSED),
    ("remove-dash", A3, [_op("remove", "/a/-")], REFUSED),
    ("replace-dash", A3, [_op("replace", "/a/-", value=4)], REFUSED),
    ("test-dash", A3, [_op("test", "/a/-", value=3)], REFUSED),
    ("dash-in-the-middle", {"a": [{"b": 1}]}, [_op("add", "/a/-/b", value=2)], REFUSED),
    ("index-blank", A3, [_op("remove", "/a/ 1")], REFUSED),
    ("index-empty", A3, [_op("remove", "/a/")], REFUSED),
    ("index-twenty-digits", A3, [_op("remove", "/a/18446744073709551616")], REFUSED),
    ("remove-from-empty-array", {"a": []}, [_op("remove", "/a/0")], REFUSED),
    ("add-to-empty-array", {"a": []}, [_op("add", "/a/0", value=1)], {"a": [1]}),
    ("members-named-like-indexes", {"0": 1, "-": 2, "01": 3}, [_op("remove", "/0"), _op("replace", "/-", value=4),
                                                             _op("test", "/01", value=3)], {"-": 4, "01": 3}),
    ("empty-member-name", {"": {"": 1}}, [_op("replace", "//", value=2)], {"": {"": 2}}),
    ("below-a-scalar", {"a": 1}, [_op("add", "/a/b", value=2)], REFUSED),
    ("move-into-own-child", {"a": {"b": 1}}, [_op("move", "/a/b/c", src="/a")], REFUSED),
    ("move-root-into-member", {"a": 1}, [_op("move", "/b", src="")], REFUSED),
    ("move-to-a-name-that-only-starts-alike", {"a": 1, "ab": {}}, [_op("move", "/ab/c", src="/a")], {"ab": {"c": 1}}),
    ("move-onto-itself", {"a": 1}, [_op("move", "/a", src="/a")], {"a": 1}),
    ("move-root-onto-itself", {"a": 1}, [_op("move", "", src="")], {"a": 1}),
    ("move-missing-onto-itself", {"a": 1}, [_op("move", "/b", src="/b")], REFUSED),
    ("move-to-own-parent", {"a": {"b": 1}}, [_op("move", "/a", src="/a/b")], {"a": 1}),
    ("move-within-array", A3, [_op("move", "/a/-", src="/a/0")], {"a": [2, 3, 1]}),
    ("move-past-the-shortened-array", A3, [_op("move", "/a/3", src="/a/0")], REFUSED),
    ("copy-root-into-member", {"a": 1}, [_op("copy", "/b", src="")], {"a": 1, "b": {"a": 1}}),
    ("copy-is-a-copy", {"a": [1]}, [_op("copy", "/b", src="/a"), _op("add", "/b/-", value=2)], {"a": [1], "b": [1, 2]}),
    ("copy-missing", {"a": 1}, [_op("copy", "/b", src="/c")], REFUSED),
    ("copy-from-dash", A3, [_op("copy", "/b", src="/a/-")], REFUSED),
    ("second-op-fails", {"a": 1}, [_op("add", "/b", value=2), _op("remove", "/c")], REFUSED),
    ("later-op-is-malformed", {"a": 1}, [_op("add", "/b", value=2), {"op": "add"}], REFUSED),
]
PATCH_TABLE = RFC6902_APPENDIX_A + PATCH_ROWS

NAMES = ["", "a", "0", "01", "-", "~", "/", "a/b", "~1"]
SCALARS = [None, True, False, 0, 1, 1.0, 1.5, -1, 2, "", "x", "1"]


def _value(rng, depth):
    r = rng.random()
    if depth <= 0 or r < 0.4:
        return rng.choice(SCALARS)
    if r < 0.7:
        return [_value(rng, depth - 1) for _ in range(rng.randint(0, 3))]
    return {rng.choice(NAMES): _value(rng, depth - 1) for _ in range(rng.randint(0, 3))}


def _escape(token):
    return token.replace("~", "~0").replace("/", "~1")


def _walk(doc, prefix=()):
    """Every location of the document as (tokens, value), the root first."""
    yield prefix, doc
    if isinstance(doc, list):
        for i, v in enumerate(doc):
            yield from _walk(v, prefix + (str(i),))
    elif isinstance(doc, dict):
        for k, v in doc.items():
            yield from _walk(v, prefix + (k,))


def _pointer(tokens):
    return "".join("/" + _escape(t) for t in tokens)


def _respell(rng, v):
    """A value that is equal, or looks equal and is not."""
    swaps = {1: [1.0, True, "1"], 0: [False, 0.0, None, ""], 1.0: [1, True], True: [1], False: [0, None], None: [False, 0]}
    if not isinstance(v, (list, dict)) and v in swaps:
        for k, alts in swaps.items():
            if type(k) is type(v) and k == v:
                return rng.choice(alts)
    if isinstance(v, dict) and v:
        return dict(reversed(list(v.items())))
    return _value(rng, 1)


def _target(rng, doc, putting):
    """Tokens of a location: one that exists, or for `putting` often a new one."""
    toks, value = rng.choice(list(_walk(doc)))
    if putting and rng.random() < 0.6 and isinstance(value, (list, dict)):
        if isinstance(value, list):
            return toks + (rng.choice(["-", str(len(value)), str(rng.randint(0, len(value)))]),)
        return toks + (rng.choice(NAMES),)
    return toks


def _mutate_tokens(rng, toks):
    toks = list(toks)
    how = rng.randrange(7)
    if not toks:
        return toks
    last = toks[-1]
    if how == 0 and last.isdigit():
        toks[-1] = str(int(last) + rng.choice([1, 2]))
    elif how == 1 and last.isdigit():
        toks[-1] = rng.choice(["0" + last, "+" + last, "-" + last, " " + last, last + " ", "-1", ""])
    elif how == 2:
        toks[-1] = "-"
    elif how == 3:
        toks[-1] = rng.choice(NAMES)
    elif how == 4:
        toks.append(rng.choice(["0", "-", "a", ""]))
    elif how == 5 and len(toks) > 1:
        toks.pop(rng.randrange(len(toks) - 1))
    return toks


def _one_op(rng, doc):
    kind = rng.choice(json_patch_ref.OPS)
    op = {"op": kind}
    toks = _target(rng, doc, putting=kind in ("add", "move", "copy"))
    if kind in ("remove", "replace") and not toks and rng.random() < 0.8:
        toks = _target(rng, doc, False)
    if kind in ("move", "copy"):
        src = _target(rng, doc, False)
        if rng.random() < 0.12:
            src = _mutate_tokens(rng, src)
        op["from"] = _pointer(src)
        if rng.random() < 0.05:
            toks = tuple(src) + tuple(toks[-1:])  # into or onto the source
    if kind in ("add", "replace"):
        op["value"] = _value(rng, 2)
    if kind == "test":
        try:
            there = copy.deepcopy(json_patch_ref.resolve(doc, list(toks)))
        except json_patch_ref.Refused:
            there = _value(rng, 1)
        op["value"] = there if rng.random() < 0.75 else _respell(rng, there)
    if rng.random() < (0.35 if kind == "add" else 0.2):
        toks = _mutate_tokens(rng, toks)
    op["path"] = _pointer(toks)
    r = rng.random()
    if r < 0.03:
        op["path"] = rng.choice([op["path"][1:], op["path"] + "~", op["path"] + "~2", "/a~", None, 3, ["a"]])
    elif r < 0.06 and "value" in op:
        del op["value"]
    elif r < 0.08:
        op["op"] = rng.choice([None, 7, kind.upper(), "bogus", "", [kind]])
    elif r < 0.10 and "from" in op:
        op["from"] = rng.choice([None, 0, op["from"][1:] or "a", op["from"] + "~x"])
    elif r < 0.11:
        op.pop(rng.choice(["op", "path"]))
    elif r < 0.12:
        return rng.choice([1, None, "add", [op]])
    return op


def patch_cases(seed, count):
    """[(document, patch)]: 1 to 4 operations, each aimed at the document as
    the reference says the operations before it have left it."""
    rng = random.Random(seed)
    out = []
    for _ in range(count):
        doc = _value(rng, 3)
        if not isinstance(doc, (list, dict)) or rng.random() < 0.3:
            doc = {rng.choice(NAMES): _value(rng, 2) for _ in range(rng.randint(1, 4))}
        patch, now = [], doc
        for _ in range(rng.randint(1, 4)):
            patch.append(_one_op(rng, now))
            try:
                now = json_patch_ref.apply(doc, patch)
            except json_patch_ref.Refused:
                now = doc
        out.append((doc, patch if rng.random() > 0.01 else rng.choice([None, {}, 1, "x", patch[0]])))
    return out


# ------------------------------------------------------------- selectors --
LABEL_OBJECTS = [
    {"metadata": {"name": "none"}},
    {"metadata": {"name": "null", "labels": None}},
    {"metadata": {"name": "empty", "labels": {"e": "", "a": ""}}},
    {"metadata": {"name": "one", "labels": {"a": "1"}}},
    {"metadata": {"name": "web", "labels": {"a": "x", "b": "05", "n": "7", "app.kubernetes.io/name": "web"}}},
    {"metadata": {"name": "neg", "labels": {"n": "-5", "in": "1", "notin": "x"}}},
    {"metadata": {"name": "big", "labels": {"n": "9223372036854775807", "a": "1", "b": "y"}}},
    {"metadata": {"name": "odd", "labels": {"n": "+3", "a": "A_b.c", "e": "x"}}},
    {"metadata": {"name": "nan", "labels": {"n": "7x", "b": " 5"}}},
]

# (selector, [(key, op, [values])] or REFUSED, names of LABEL_OBJECTS that match)
LABEL_TABLE = [
    ("", [], [o["metadata"]["name"] for o in LABEL_OBJECTS]),
    (" \t", [], [o["metadata"]["name"] for o in LABEL_OBJECTS]),
    ("a in (1", REFUSED, None),
    ("a > 0", [("a", ">", ["0"])], ["one", "big"]),
    ("a > x", REFUSED, None),
    ("a > 1 2", REFUSED, None),
    ("n<9223372036854775808", REFUSED, None),
    ("!a in (1)", REFUSED, None),
    ("=1", REFUSED, None),
    ("a,,e", REFUSED, None),
    ("a,", REFUSED, None),
    (",a", REFUSED, None),
    ("a=1=2", REFUSED, None),
    ("a in (1 2)", REFUSED, None),
    ("e in ()", [("e", "in", [""])], ["empty"]),
    ("e in (x,)", [("e", "in", ["", "x"])], ["empty", "odd"]),
    ("e in (,x)", [("e", "in", ["", "x"])], ["empty", "odd"]),
    ("e in (y,,x)", [("e", "in", ["", "x", "y"])], ["empty", "odd"]),
    ("e notin ()", [("e", "notin", [""])], ["none", "null", "one", "web", "neg", "big", "odd", "nan"]),
    ("a in (x, 1 ,1)", [("a", "in", ["1", "x"])], ["one", "web", "big"]),
    ("a=", [("a", "=", [""])], ["empty"]),
    ("a= ,e", [("a", "=", [""]), ("e", "exists", [])], ["empty"]),
    ("a==1", [("a", "=", ["1"])], ["one", "big"]),
    ("a = 1", [("a", "=", ["1"])], ["one", "big"]),
    ("a!=1", [("a", "!=", ["1"])], ["none", "null", "empty", "web", "neg", "odd", "nan"]),
    ("a! =1", REFUSED, None),
    ("a=!b", REFUSED, None),
    ("a", [("a", "exists", [])], ["empty", "one", "web", "big", "odd"]),
    ("!a", [("a", "!exists", [])], ["none", "null", "neg", "nan"]),
    ("! a", [("a", "!exists", [])], ["none", "null", "neg", "nan"]),
    ("!!a", REFUSED, None),
    ("!a=1", REFUSED, None),
    ("!", REFUSED, None),
    ("a b", REFUSED, None),
    ("in", [("in", "exists", [])], ["neg"]),
    ("in in (in,notin)", [("in", "in", ["in", "notin"])], []),
    ("notin notin (x),in=1", [("notin", "notin", ["x"]), ("in", "=", ["1"])], []),
    ("a in(1)", [("a", "in", ["1"])], ["one", "big"]),
    ("a in", REFUSED, None),
    ("a in 1", REFUSED, None),
    ("a in (1))", REFUSED, None),
    ("a in ((1)", REFUSED, None),
    ("a in (1),", REFUSED, None),
    ("a in (=)", REFUSED, None),
    ("a IN (1)", REFUSED, None),
    ("n>6", [("n", ">", ["6"])], ["web", "big"]),
    ("n<7", [("n", "<", ["7"])], ["neg", "odd"]),
    ("n > 007", [("n", ">", ["007"])], ["big"]),
    ("n<-1", REFUSED, None),  # -1 is no label value
    ("n>", REFUSED, None),
    ("n>=1", REFUSED, None),
    ("app.kubernetes.io/name=web", [("app.kubernetes.io/name", "=", ["web"])], ["web"]),
    ("App.io/name", REFUSED, None),  # a DNS subdomain is lower case
    ("/name", REFUSED, None),
    ("a/b/c", REFUSED, None),
    ("a/", REFUSED, None),
    ("-a", REFUSED, None),
    ("a.", REFUSED, None),
    ("a$b", REFUSED, None),
    ("a=-x", REFUSED, None),
    ("a=x y", REFUSED, None),
    ("a in (x_)", REFUSED, None),
    ("k" * 63, [("k" * 63, "exists", [])], []),
    ("k" * 64, REFUSED, None),
    ("a=" + "v" * 63, [("a", "=", ["v" * 63])], []),
    ("a=" + "v" * 64, REFUSED, None),
    ("p" * 253 + "/a", [("p" * 253 + "/a", "exists", [])], []),  # a subdomain's labels have no limit of their own
    ("p" * 254 + "/a", REFUSED, None),
    ("a=A_b.c", [("a", "=", ["A_b.c"])], ["odd"]),
    ("a\n=\r1", [("a", "=", ["1"])], ["one", "big"]),
    ("a\x0b=1", REFUSED, None),  # a vertical tab is no blank: part of the key
]

FIELD_OBJECTS = [
    {"metadata": {"name": "p", "namespace": "default"}, "spec": {"nodeName": "n1", "flag": True, "count": 7, "none": None}},
    {"metadata": {"name": "p,q", "namespace": "default"}, "spec": {"nodeName": "", "flag": False, "count": -3}},
    {"metadata": {"name": "p=q", "namespace": "default"}, "spec": {"nodeName": "a\\b", "count": 0}},
    {"metadata": {"name": " p", "namespace": "default"}, "spec": "scalar"},
    {"metadata": {"name": "q"}, "": "root", "spec": {"nodeName": "true", "flag": "7", "count": "n1"}},
]
_ALL = [o["metadata"]["name"] for o in FIELD_OBJECTS]

# (selector, [(path, op, value)] or REFUSED, names of FIELD_OBJECTS that match)
FIELD_TABLE = [
    ("", [], _ALL),
    (",,", [], _ALL),
    ("metadata.name", REFUSED, None),
    ("metadata.name in (p)", REFUSED, None),
    ("metadata.name= p", [("metadata.name", "=", " p")], [" p"]),
    ("metadata.name=p\\,q", [("metadata.name", "=", "p,q")], ["p,q"]),
    ("metadata.name=p\\=q", [("metadata.name", "=", "p=q")], ["p=q"]),
    ("metadata.name=p=q", REFUSED, None),
    ("spec.nodeName=a\\\\b", [("spec.nodeName", "=", "a\\b")], ["p=q"]),
    ("spec.nodeName=a\\b", REFUSED, None),
    ("spec.nodeName=a\\", REFUSED, None),
    ("metadata.name=p", [("metadata.name", "=", "p")], ["p"]),
    ("metadata.name==p", [("metadata.name", "=", "p")], ["p"]),
    ("metadata.name!=p", [("metadata.name", "!=", "p")], ["p,q", "p=q", " p", "q"]),
    ("metadata.name =p", [("metadata.name ", "=", "p")], []),
    (",metadata.name=p,,spec.count=7,", [("metadata.name", "=", "p"), ("spec.count", "=", "7")], ["p"]),
    ("spec.flag=true", [("spec.flag", "=", "true")], ["p"]),
    ("spec.flag=false", [("spec.flag", "=", "false")], ["p,q"]),
    ("spec.flag=True", [("spec.flag", "=", "True")], []),
    ("spec.count=7", [("spec.count", "=", "7")], ["p"]),
    ("spec.count=-3", [("spec.count", "=", "-3")], ["p,q"]),
    ("spec.none=", [("spec.none", "=", "")], ["p", "p,q", "p=q", " p", "q"]),
    ("spec.missing=", [("spec.missing", "=", "")], _ALL),
    ("spec.missing!=", [("spec.missing", "!=", "")], []),
    ("spec.nodeName.x=", [("spec.nodeName.x", "=", "")], _ALL),
    ("spec.nodeName=", [("spec.nodeName", "=", "")], ["p,q", " p"]),
    ("=root", [("", "=", "root")], ["q"]),
    ("a!b=c", [("a!b", "=", "c")], []),
    ("a=!b", [("a", "=", "!b")], []),
    ("a!==b", REFUSED, None),  # != then a bare =
    ("spec.nodeName!=n1,spec.count!=0", [("spec.nodeName", "!=", "n1"), ("spec.count", "!=", "0")], ["p,q", " p", "q"]),
]

L_KEYS = ["a", "b", "e", "n", "in", "notin", "app.kubernetes.io/name", "a/b/c", "-a", "A_b.c", "k" * 64, "Up/x"]
L_VALUES = ["1", "x", "05", "7", "0", "-5", "9223372036854775807", "9223372036854775808", "v" * 64, "A_b.c", "in", "y_"]
L_OPERATORS = ["=", "==", "!=", ">", "<", "in", "notin"]
L_BLANKS = ["", "", " ", "  ", "\t"]


def _requirement(rng):
    """The tokens of one well-formed requirement (its key and values may
    still be invalid names)."""
    key = rng.choice(L_KEYS[:7] if rng.random() < 0.9 else L_KEYS)
    value = lambda: rng.choice(L_VALUES[:5] if rng.random() < 0.9 else L_VALUES)
    form = rng.randrange(9)
    if form == 7:
        return [key]
    if form == 8:
        return ["!", key]
    op = L_OPERATORS[form]
    if op in ("in", "notin"):
        inside = []
        for _ in range(rng.randint(0, 3)):
            inside += [value(), ","]
        if inside and rng.random() < 0.7:
            inside.pop()
        if rng.random() < 0.15:
            inside.insert(rng.randint(0, len(inside)), ",")
        return [key, op, "(", *inside, ")"]
    if op in (">", "<"):
        return [key, op, rng.choice(["0", "6", "05", "7", "9223372036854775807"]) if rng.random() < 0.85 else value()]
    return [key, op] + ([value()] if rng.random() < 0.85 else [])


def label_selectors(seed, count):
    rng = random.Random(seed)
    pool = L_KEYS + L_VALUES + L_OPERATORS + ["(", ")", ",", "!", " "]
    out = []
    for _ in range(count):
        if rng.random() < 0.1:
            toks = [rng.choice(pool) for _ in range(rng.randint(1, 8))]
        else:
            toks = []
            for k in range(rng.randint(1, 3)):
                toks += ([","] if k else []) + _requirement(rng)
            if rng.random() < 0.4:
                for _ in range(rng.randint(1, 2)):
                    at = rng.randrange(len(toks) + 1)
                    how = rng.randrange(3)
                    if how == 0:
                        toks.insert(at, rng.choice(pool))
                    elif how == 1 and toks:
                        toks.pop(min(at, len(toks) - 1))
                    elif toks:
                        toks[min(at, len(toks) - 1)] = rng.choice(pool)
        s = ""
        for i, t in enumerate(toks):
            # Two identifiers need a blank between them; elsewhere blanks are optional.
            glue = rng.choice(L_BLANKS)
            if i and not glue and t[0] not in "=!(),<> " and toks[i - 1][-1] not in "=!(),<> ":
                glue = " "
            s += glue + t
        out.append(s + rng.choice(L_BLANKS))
    return out


F_KEYS = ["metadata.name", "spec.nodeName", "spec.flag", "spec.count", "spec.none", "spec.missing", "spec.nodeName.x", "",
          "metadata.namespace"]
F_VALUES = ["p", "p\\,q", "p\\=q", "a\\\\b", "n1", "true", "false", "7", "-3", "0", "", " p", "q", "root", "p=q", "a\\b", "p\\",
            "True", "p ", "\\\\", "!b"]


def field_selectors(seed, count):
    rng = random.Random(seed)
    out = []
    for _ in range(count):
        terms = []
        for _ in range(rng.randint(1, 3)):
            r = rng.random()
            if r < 0.06:
                terms.append("")
            elif r < 0.12:
                terms.append(rng.choice(F_KEYS) + rng.choice(["", " in (p)", " ", ">1"]))
            else:
                value = rng.choice(F_VALUES[:15] if rng.random() < 0.8 else F_VALUES)
                key = rng.choice(F_KEYS[:7] if rng.random() < 0.9 else F_KEYS)
                terms.append(key + rng.choice(["=", "=", "==", "!="]) + value)
        out.append(",".join(terms))
    return out


# The generated selectors of test_selector_conformance.py (the sanitizer driver's test reads them too).
LABEL_STRINGS = label_selectors(seed=63, count=2000)
FIELD_STRINGS = field_selectors(seed=64, count=1000)


# ------------------------------------------------ corpus for the driver --
def write_corpus(path, patches, objects, label_strings, field_strings):
    """Records of <one byte kind><u32 little-endian length><payload>:
    P {"doc":..,"patch":..}   O an object to match against
    L a label selector        F a field selector"""
    with open(path, "wb") as f:
        def record(kind, payload):
            data = payload if isinstance(payload, bytes) else payload.encode()
            f.write(kind + struct.pack("<I", len(data)) + data)

        for doc, patch in patches:
            record(b"P", json.dumps({"doc": doc, "patch": patch}))
        for o in objects:
            record(b"O", json.dumps(o))
        for s in label_strings:
            record(b"L", s)
        for s in field_strings:
            record(b"F", s)
    return len(patches) + len(objects) + len(label_strings) + len(field_strings)
