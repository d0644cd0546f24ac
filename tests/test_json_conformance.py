"""The JSON parser, writer, hash and merge patch of csrc/common/json.cc held
to an independent reference (json_ref.py: Python's json.loads made strict),
the way the HIP kernels are held to numpy. Every comparison is type-exact
(an int is not a float) and bit-exact for floats."""
import json
import os
import struct
import subprocess

import pytest
from hypothesis import HealthCheck, given, settings
from hypothesis import strategies as st

from flex_gpu_scheduler_amd import build_ext
from flex_gpu_scheduler_amd._native import native

import json_corpus
import json_ref
import pod_decode_ref
from json_ref import same

X = native()
# Deterministic, like the rest of the suite; a slow machine is no finding.
PROPERTY = dict(deadline=None, derandomize=True, database=None, suppress_health_check=[HealthCheck.too_slow])


def native_parse(text, parse=None):
    """(True, value) or (False, None). Only JsonError counts as a refusal:
    any other exception propagates and fails the test."""
    try:
        return True, (parse or X.json_parse)(text)
    except X.JsonError:
        return False, None


def reference_parse(text):
    try:
        return True, json_ref.loads(text)
    except json_ref.Rejected:
        return False, None


def assert_like_reference(text):
    want_ok, want = reference_parse(text)
    got_ok, got = native_parse(text)
    assert got_ok == want_ok, (text[:80], "reference accepts" if want_ok else "reference rejects")
    if want_ok:
        assert same(got, want, ordered=True), (text[:80], got, want)


# ------------------------------------------------------------------ table --
@pytest.mark.parametrize("name,text,accepted", json_corpus.TABLE, ids=[n for n, _, _ in json_corpus.TABLE])
def test_table(name, text, accepted):
    assert json_ref.accepts(text) == accepted, "the reference disagrees with the table"
    assert_like_reference(text)
    if accepted:  # and what was parsed is written as text that reads back the same
        v = json_ref.loads(text)
        assert same(json.loads(X.json_dump(X.json_parse(text))), v, int_float=True)


def test_table_values_spelled_out():
    """The reference's answers for the cases the table is there for, so that
    a reference that drifted would be noticed too."""
    P = X.json_parse
    bits = lambda f: struct.pack("<d", f)
    assert P(b'"\\ud800\\u0041"') == "\ufffdA"
    assert P(b'"\\ud800"') == P(b'"\\udc00"') == "\ufffd"
    assert P(b'"\\ud800\\ud800"') == "\ufffd\ufffd"
    assert P(b'"\\ud800\\ud83d\\ude00"') == "\ufffd\U0001F600"
    assert P(b'"\\ud83d\\ude00"') == P("\"\U0001F600\"".encode()) == "\U0001F600"
    assert P(b'"a\\u0000b"') == "a\x00b"
    assert P(b'"\\"\\\\\\/\\b\\f\\n\\r\\t"') == "\"\\/\b\f\n\r\t"
    assert list(P(b'{"a":1,"b":2,"a":3}').items()) == [("a", 3), ("b", 2)]
    assert P(b'{"\\ud800":1,"\\udc00":2}') == {"\ufffd": 2}
    for text, want in [(b"9223372036854775807", 2**63 - 1), (b"-9223372036854775808", -2**63), (b"9007199254740993", 2**53 + 1),
                       (b"-0", 0), (b"0", 0)]:
        assert type(P(text)) is int and P(text) == want
    for text, want in [(b"9223372036854775808", 2.0**63), (b"-9223372036854775809", -2.0**63), (b"1.0", 1.0), (b"-0.0", -0.0),
                       (b"5e-324", 5e-324), (b"2e-324", 0.0), (b"1e-999", 0.0), (b"0.1", 0.1),
                       (b"1.7976931348623157e308", 1.7976931348623157e308), (b"9007199254740993.0", 9007199254740992.0)]:
        assert type(P(text)) is float and bits(P(text)) == bits(want), text
    assert X.json_dump([1.0, -0.0, 0.1, 5e-324, 1.7976931348623157e308, 2**53 + 1, -2**63]) == \
        b"[1,-0,0.10000000000000001,4.9406564584124654e-324,1.7976931348623157e+308,9007199254740993,-9223372036854775808]"


# ----------------------------------------------------------- differential --
EDGE_INTS = [0, -1, 1, 2**31, -2**31, 2**53 - 1, 2**53, 2**53 + 1, -(2**53) - 1, 2**63 - 1, -2**63]
BIG_INTS = [2**63, -2**63 - 1, 2**64, 10**30, -10**400 + 1]  # no int64: the DOM reads these as doubles (or refuses)
EDGE_FLOATS = [0.0, -0.0, 1.0, -1.0, 0.1, 5e-324, 2.2250738585072014e-308, 1.7976931348623157e308, 2.0**53, 2.0**63, -2.0**63,
               1e15, 1e16, 1e22, 123456789.0, 2.5, 1 / 3]
ODD_CHARS = "\x00\x01\x1f \"\\/\x7f\x80\u07ff\u0800\u2028\ud7ff\ue000\ufeff\ufffd\uffff\U00010000\U0001F600\U0010ffff"
texts = st.one_of(st.text(max_size=8),  # all planes; hypothesis leaves surrogates out by default
                  st.text(st.sampled_from(ODD_CHARS), max_size=6))
ints64 = st.one_of(st.sampled_from(EDGE_INTS), st.integers(-2**63, 2**63 - 1))
floats = st.one_of(st.sampled_from(EDGE_FLOATS), st.floats(allow_nan=False, allow_infinity=False))


def values(ints):
    scalars = st.one_of(st.none(), st.booleans(), ints, floats, texts)
    return st.recursive(scalars, lambda kids: st.one_of(st.lists(kids, max_size=4), st.dictionaries(texts, kids, max_size=4)),
                        max_leaves=12)


spellings = st.fixed_dictionaries({"ensure_ascii": st.booleans(), "indent": st.sampled_from([None, 0, 2, "\t"]),
                                   "separators": st.sampled_from([None, (",", ":"), (" ,\n", "\t: ")])})


# 400 examples: about two seconds.
@settings(max_examples=400, **PROPERTY)
@given(values(st.one_of(ints64, st.sampled_from(BIG_INTS))), spellings)
def test_parse_agrees_with_reference_on_generated_text(v, spelling):
    """json_parse(text) is json.loads(text), except that an integer outside
    int64 is the nearest double (json_ref) where Python keeps a big int."""
    text = json.dumps(v, ensure_ascii=spelling["ensure_ascii"], indent=spelling["indent"], separators=spelling["separators"])
    assert_like_reference(text.encode())
    if isinstance(v, list) and json_ref.accepts(text):
        assert same(X.json_parse_array_stream(text), json_ref.loads(text), ordered=True)


# 400 examples: about two seconds.
@settings(max_examples=400, **PROPERTY)
@given(values(ints64))
def test_dump_reads_back_and_keeps_the_hash(v):
    text = X.json_dump(v)
    # Type-exact and bit-exact, except that an integral Double may come back
    # as an Int of the same value (1.0 is written "1").
    assert same(json.loads(text), v, int_float=True), text
    assert same(json_ref.loads(text), X.json_parse(text), ordered=True)
    assert X.json_hash([X.json_parse(text)]) == X.json_hash([v])  # in a list: a bare str would be taken for text
    assert X.json_hash(b"[" + text + b"]") == X.json_hash([v])


def native_equal(a, b):
    # diff_merge_patch leaves out exactly the members that compare equal.
    return X.diff_merge_patch({"k": a}, {"k": b}) == {}


def respell(v, draw):
    """v with some of its numbers in the other spelling, Int for Double and
    Double for Int, wherever that is the same number."""
    if isinstance(v, bool):
        return v
    if isinstance(v, int) and float(v) == v and -2**63 <= float(v) < 2**63 and draw(st.booleans()):
        return float(v)
    if isinstance(v, float) and v == int(v) and -2**63 <= v < 2**63 and draw(st.booleans()):
        return int(v)
    if isinstance(v, list):
        return [respell(x, draw) for x in v]
    if isinstance(v, dict):
        return {k: respell(x, draw) for k, x in v.items()}
    return v


# 300 examples: about a second.
@settings(max_examples=300, **PROPERTY)
@given(values(ints64), st.data())
def test_equal_values_hash_equal(v, data):
    w = respell(v, data.draw)
    assert native_equal(v, w) and native_equal(w, v)
    assert X.json_hash([v]) == X.json_hash([w])


def test_int_and_double_compare_exactly():
    assert native_equal(1, 1.0) and native_equal(0, -0.0) and native_equal(2**53, 2.0**53)
    assert native_equal(-2**63, -2.0**63)
    for i, d in [(2**53 + 1, 2.0**53), (2**63 - 1, 2.0**63), (1, 1.5), (0, 5e-324), (-2**53 - 1, -2.0**53)]:
        assert not native_equal(i, d) and not native_equal(d, i), (i, d)
        assert X.diff_merge_patch({"k": i}, {"k": d}) == {"k": d}
    assert X.json_hash(1) == X.json_hash(1.0) != X.json_hash(1.5)
    assert X.json_hash(2**53 + 1) != X.json_hash(2.0**53)


# ------------------------------------------------------- accept iff accept --
FUZZ = [(name, doc) for name, doc in json_corpus.fuzz_documents()]


@pytest.mark.parametrize("name,doc", FUZZ, ids=[n for n, _ in FUZZ])
def test_every_prefix(name, doc):
    assert json_ref.accepts(doc)
    for text in json_corpus.prefixes(doc):
        assert_like_reference(text)


@pytest.mark.parametrize("k,name,doc", [(k, n, d) for k, (n, d) in enumerate(FUZZ)], ids=[n for n, _ in FUZZ])
def test_single_byte_mutations(k, name, doc):
    muts = json_corpus.mutations(doc, seed=1000 + k, count=json_corpus.MUTATIONS)  # 300 per document
    verdicts = [json_ref.accepts(t) for t in muts]
    assert 10 < sum(verdicts) < len(muts) - 10, "the mutations should land on both sides"
    for text in muts:
        assert_like_reference(text)


# ----------------------------------------------------------- stream parity --
def test_array_stream_agrees_with_parse_on_the_whole_corpus():
    """Elements equal, malformed input refused alike, and the depth limit at
    the same document. Text whose value is no array is refused by the stream."""
    arrays = 0
    for text in json_corpus.all_documents():
        ok, want = reference_parse(text)
        ok = ok and isinstance(want, list)
        got_ok, got = native_parse(text, X.json_parse_array_stream)
        assert got_ok == ok, text[:80]
        if ok:
            arrays += 1
            assert same(got, want, ordered=True), text[:80]
            assert same(got, X.json_parse(text), ordered=True)
    assert arrays > 20


# ------------------------------------------------------------ merge patch --
def rfc7386(target, patch):
    """RFC 7386 section 2, as written there."""
    if isinstance(patch, dict):
        if not isinstance(target, dict):
            target = {}
        target = dict(target)
        for name, value in patch.items():
            if value is None:
                target.pop(name, None)
            else:
                target[name] = rfc7386(target.get(name), value)
        return target
    return patch


keys = st.sampled_from(["a", "b", "c", "é", ""])
leaves = st.one_of(st.none(), st.booleans(), st.sampled_from(EDGE_INTS), st.sampled_from(EDGE_FLOATS),
                   st.sampled_from(["", "x", "é"]))
documents = st.recursive(leaves, lambda kids: st.one_of(st.lists(kids, max_size=3), st.dictionaries(keys, kids, max_size=4)),
                         max_leaves=10)
objects = st.dictionaries(keys, documents, max_size=4)
# The bindings read a top-level str as JSON text, so no bare string here.
not_text = documents.filter(lambda v: not isinstance(v, str))


# 400 examples: about a second.
@settings(max_examples=400, **PROPERTY)
@given(st.one_of(objects, not_text), st.one_of(objects, objects, not_text))
def test_merge_patch_is_rfc7386(target, patch):
    assert same(X.merge_patch(target, patch), rfc7386(target, patch))


def without_null_members(v):
    if isinstance(v, dict):
        return {k: without_null_members(x) for k, x in v.items() if x is not None}
    return v  # an array is replaced whole: nulls inside it are data


# 400 examples: about a second.
@settings(max_examples=400, **PROPERTY)
@given(objects, objects)
def test_diff_then_merge_gives_the_target(a, b):
    """merge_patch(a, diff_merge_patch(a, b)) == b, for b without null
    members: a merge patch cannot say "set this member to null", null means
    "remove". A number may keep a's spelling where b's is the same value."""
    b = without_null_members(b)
    patch = X.diff_merge_patch(a, b)
    assert same(X.merge_patch(a, patch), b, int_float=True), patch
    assert same(rfc7386(a, patch), b, int_float=True), patch
    if same(a, b):
        assert patch == {}


# -------------------------------------------------------------- sanitizers --
def test_sanitized_driver_runs_the_whole_corpus(tmp_path):
    """csrc/tests/json_fuzz_main.cc, built with AddressSanitizer and
    UndefinedBehaviorSanitizer (float-cast-overflow included), takes every
    document of this file and every hostile pod through parse, dump, parse,
    hash and Pod::from_json. Any finding aborts it."""
    docs = json_corpus.all_documents() + [json.dumps(p).encode() for _, p in pod_decode_ref.hostile_pods()]
    corpus = tmp_path / "corpus.bin"
    with open(corpus, "wb") as f:
        for d in docs:
            f.write(struct.pack("<I", len(d)) + d)
    exe = build_ext.build_json_fuzz(verbose=False)
    r = subprocess.run([str(exe), str(corpus)], capture_output=True, text=True, timeout=300)
    if r.returncode != 0 and "LeakSanitizer has encountered a fatal error" in r.stderr:
        # The leak check at exit needs ptrace, which some sandboxes deny; every other check has run by then.
        r = subprocess.run([str(exe), str(corpus)], capture_output=True, text=True, timeout=300,
                           env={**os.environ, "ASAN_OPTIONS": "detect_leaks=0"})
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert f"{len(docs)} documents" in r.stdout
