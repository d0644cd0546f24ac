"""The documents the JSON conformance tests and the sanitizer driver share:
a hand-written table (text, accepted?) and three small documents with their
prefixes and seeded single-byte mutations."""
from __future__ import annotations

import json
import random

from flex_gpu_scheduler_amd.models import make_container, make_pod

from json_ref import MAX_DEPTH

OK, NO = True, False


def _nest(open_, close, n, inner=b""):
    return open_ * n + inner + close * n


# (name, text, accepted). What an accepted text is worth comes from
# json_ref.loads; a few values are also spelled out in the test itself.
TABLE: list[tuple[str, bytes, bool]] = [
    # --- whitespace, framing ---
    ("empty", b"", NO),
    ("spaces only", b" \t\r\n ", NO),
    ("ws around", b" \t\r\n1 \t\r\n", OK),
    ("bom", b"\xef\xbb\xbf1", NO),
    ("bom alone", b"\xef\xbb\xbf", NO),
    ("vtab ws", b"\v1", NO),
    ("formfeed ws", b"1\f", NO),
    ("nbsp ws", b"\xc2\xa01", NO),
    ("two values", b"1 2", NO),
    ("trailing comma array", b"[1,]", NO),
    ("trailing comma object", b'{"a":1,}', NO),
    ("lone comma", b"[,]", NO),
    ("missing comma", b"[1 2]", NO),
    ("missing colon", b'{"a" 1}', NO),
    ("unquoted key", b"{a:1}", NO),
    ("single quotes", b"'a'", NO),
    ("comment", b"1 // x", NO),
    ("unclosed array", b"[1", NO),
    ("unclosed object", b'{"a":1', NO),
    ("mismatched close", b"[1}", NO),
    ("empty containers", b'[{},[],{"a":[]}]', OK),
    # --- literals ---
    ("true", b"true", OK), ("false", b"false", OK), ("null", b"null", OK),
    ("True", b"True", NO), ("nul", b"nul", NO), ("nulll", b"nulll", NO), ("truefalse", b"truefalse", NO),
    ("NaN", b"NaN", NO), ("Infinity", b"Infinity", NO), ("-Infinity", b"-Infinity", NO),
    ("[NaN]", b"[NaN]", NO), ("nan", b"nan", NO),
    # --- number grammar ---
    ("+1", b"+1", NO), ("01", b"01", NO), ("-01", b"-01", NO), ("1.", b"1.", NO), (".5", b".5", NO),
    ("-.5", b"-.5", NO), ("-", b"-", NO), ("--1", b"--1", NO), ("1e", b"1e", NO), ("1e+", b"1e+", NO),
    ("1ee5", b"1ee5", NO), ("1e5.5", b"1e5.5", NO), ("0x10", b"0x10", NO), ("1.2.3", b"1.2.3", NO),
    ("1_000", b"1_000", NO), ("1 in array +", b"[+1]", NO), ("[01]", b"[01]", NO), ("[1.]", b"[1.]", NO),
    ("[.5]", b"[.5]", NO), ("1.e5", b"1.e5", NO), ("00", b"00", NO), ("0.0", b"0.0", OK), ("0e0", b"0e0", OK),
    ("1E5", b"1E5", OK), ("1e+5", b"1e+5", OK), ("1e-5", b"1e-5", OK), ("1e05", b"1e05", OK),
    ("0", b"0", OK), ("-0", b"-0", OK), ("-0.0", b"-0.0", OK), ("-0e0", b"-0e0", OK),
    ("1.0", b"1.0", OK), ("0.1", b"0.1", OK), ("5e-324", b"5e-324", OK), ("2e-324 rounds to 0", b"2e-324", OK),
    ("1e-999", b"1e-999", OK), ("dbl max", b"1.7976931348623157e308", OK),
    ("just over dbl max, rounds down", b"1.7976931348623158e308", OK),
    ("1.8e308", b"1.8e308", NO), ("1e999", b"1e999", NO), ("[-1e999]", b"[-1e999]", NO),
    ("400 digit int", b"1" + b"0" * 400, NO), ("5000 digit int", b"-1" + b"0" * 5000, NO),
    ("long fraction", b"0." + b"3" * 400, OK),
    ("int64 max", b"9223372036854775807", OK), ("int64 min", b"-9223372036854775808", OK),
    ("2^63", b"9223372036854775808", OK), ("-2^63-1", b"-9223372036854775809", OK),
    ("2^64", b"18446744073709551616", OK), ("2^64-1", b"18446744073709551615", OK),
    ("20 digits", b"99999999999999999999", OK),
    ("2^53-1", b"9007199254740991", OK), ("2^53", b"9007199254740992", OK), ("2^53+1", b"9007199254740993", OK),
    ("2^53+1 as float", b"9007199254740993.0", OK), ("-(2^53+1)", b"-9007199254740993", OK),
    # --- escapes ---
    ("two-char escapes", b'"\\"\\\\\\/\\b\\f\\n\\r\\t"', OK),
    ("escape a", b'"\\a"', NO), ("escape v", b'"\\v"', NO), ("escape 0", b'"\\0"', NO), ("escape x", b'"\\x41"', NO),
    ("escape '", b'"\\\'"', NO), ("escape U", b'"\\U0041"', NO), ("escape at end", b'"\\', NO),
    ("escape quote then end", b'"\\"', NO),
    ("u0000", b'"a\\u0000b"', OK), ("u0000 key", b'{"\\u0000":1}', OK),
    ("u upper hex", b'"\\u00E9\\u00e9"', OK), ("u short", b'"\\u12"', NO), ("u bad hex", b'"\\u12G4"', NO),
    ("u sign", b'"\\u+123"', NO), ("u space", b'"\\u 123"', NO), ("u 0x", b'"\\u0x12"', NO),
    ("u7f raw", b'"\x7f"', OK),
    # --- surrogates ---
    ("pair escaped", b'"\\ud83d\\ude00"', OK), ("pair raw", "\"\U0001F600\"".encode(), OK),
    ("pair both", b'"\\ud83d\\ude00' + "\U0001F600".encode() + b'"', OK),
    ("max code point", b'"\\udbff\\udfff' + "\U0010FFFF".encode() + b'"', OK),
    ("lone high", b'"\\ud800"', OK), ("lone low", b'"\\udc00"', OK),
    ("high then A", b'"\\ud800\\u0041"', OK), ("high high", b'"\\ud800\\ud800"', OK),
    ("low high", b'"\\udc00\\ud800"', OK), ("high then text", b'"\\ud800abc"', OK),
    ("high high low", b'"\\ud800\\ud83d\\ude00"', OK), ("high then escape n", b'"\\ud800\\n"', OK),
    ("high then short u", b'"\\ud800\\u12"', NO), ("high then bad u", b'"\\ud800\\uZZZZ"', NO),
    ("high at end", b'"\\ud800', NO),
    ("lone surrogate keys collide", b'{"\\ud800":1,"\\udc00":2}', OK),
    # --- raw bytes in strings ---
    ("raw tab", b'"a\tb"', NO), ("raw lf", b'"a\nb"', NO), ("raw cr", b'"a\rb"', NO), ("raw nul", b'"a\x00b"', NO),
    ("raw 1f", b'"\x1f"', NO), ("raw nul key", b'{"\x00":1}', NO), ("nul between tokens", b"[1,\x002]", NO),
    ("ff fe", b'"\xff\xfe"', NO), ("lone continuation", b'"\x80"', NO), ("c0 overlong", b'"\xc0\xaf"', NO),
    ("c1 overlong", b'"\xc1\xbf"', NO), ("e0 overlong", b'"\xe0\x9f\xbf"', NO), ("f0 overlong", b'"\xf0\x8f\xbf\xbf"', NO),
    ("raw surrogate d800", b'"\xed\xa0\x80"', NO), ("raw surrogate dfff", b'"\xed\xbf\xbf"', NO),
    ("above 10ffff", b'"\xf4\x90\x80\x80"', NO), ("f5", b'"\xf5\x80\x80\x80"', NO),
    ("f8 five-byte", b'"\xf8\x88\x80\x80\x80"', NO),
    ("truncated 2", b'"\xc3"', NO), ("truncated 3", b'"\xe2\x82"', NO), ("truncated 4", b'"\xf0\x9f\x98"', NO),
    ("truncated at end of text", b'"\xe2\x82', NO), ("bad second continuation", b'"\xe2\x82\x41"', NO),
    ("bad third continuation", b'"\xf0\x9f\x98\x41"', NO), ("invalid in key", b'{"\xff":1}', NO),
    ("boundaries ok", "\"\x7f\u0080\u07ff\u0800\ud7ff\ue000\uffff\U00010000\U0010ffff\"".encode(), OK),
    ("bytes outside string", b"[\xc3\xa9]", NO),
    # --- objects ---
    ("duplicate keys", b'{"a":1,"b":2,"a":3}', OK), ("duplicate nested", b'{"a":{"x":1},"a":{"y":2}}', OK),
    ("empty key", b'{"":0}', OK), ("non-string key", b"{1:2}", NO),
    # --- depth ---
    ("arrays at limit, scalar inside", _nest(b"[", b"]", MAX_DEPTH, b"1"), OK),
    ("arrays past limit, scalar inside", _nest(b"[", b"]", MAX_DEPTH + 1, b"1"), NO),
    ("arrays at limit, empty inside", _nest(b"[", b"]", MAX_DEPTH + 1), OK),
    ("arrays past limit, empty inside", _nest(b"[", b"]", MAX_DEPTH + 2), NO),
    ("objects at limit", _nest(b'{"a":', b"}", MAX_DEPTH, b"1"), OK),
    ("objects past limit", _nest(b'{"a":', b"}", MAX_DEPTH + 1, b"1"), NO),
    ("objects at limit, empty inside", _nest(b'{"a":', b"}", MAX_DEPTH, b"{}"), OK),
    ("objects past limit, empty inside", _nest(b'{"a":', b"}", MAX_DEPTH + 1, b"{}"), NO),
    ("too deep under a duplicate key", b'{"a":' + _nest(b"[", b"]", MAX_DEPTH, b"1") + b',"a":0}', NO),
    ("very deep", b"[" * 5000, NO),
]


def fuzz_documents() -> list[tuple[str, bytes]]:
    pod = make_pod("fuzz-0", namespace="team-a", labels={"app": "fuzz", "tier": "é"},
                   annotations={"amd.com/gpu-index": "0,3"}, priority=7,
                   containers=[make_container("a", requests={"cpu": "500m", "memory": "1Gi"},
                                              limits={"amd.com/gpu": 2})])
    deep = [[[[[[[[1, [2.5, [-3e-7, [True, [None, ["x", [{}, [[]]]]]]]]]]]]]]], 0, -0.0, 1e21, 2**63 - 1]
    strings = {"plain": "abc", "esc": "q\"b\\s/\b\f\n\r\t\x00\x1f\x7f", "bmp": "é€\u07ff\u0800\uffff",
               "astral": "\U0001F600\U0010FFFF", "": "", "kéy": ["\u2028\u2029", "\ud7ff\ue000"]}
    return [
        ("pod", json.dumps(pod, separators=(",", ":")).encode()),
        ("deep", json.dumps(deep).encode()),
        # ensure_ascii=False and True halves: raw multi-byte text and escapes.
        ("strings", (json.dumps(strings, ensure_ascii=False)[:-1] + ", \"esc2\": " +
                     json.dumps(strings, ensure_ascii=True) + "}").encode()),
    ]


def prefixes(doc: bytes) -> list[bytes]:
    return [doc[:n] for n in range(len(doc))]


def mutations(doc: bytes, seed: int, count: int) -> list[bytes]:
    """`count` seeded single-byte flips, inserts and deletes of `doc`."""
    rng = random.Random(seed)
    # Bytes that matter to a JSON scanner, and any byte at all.
    hot = b'"\\{}[]:,-+.eE0123456789tfnu \t\n\x00\x1f\x7f\x80\xbf\xc0\xc3\xe2\xed\xf0\xf4\xff'
    out = []
    for k in range(count):
        at = rng.randrange(len(doc))
        b = hot[rng.randrange(len(hot))] if rng.random() < 0.7 else rng.randrange(256)
        op = k % 3
        if op == 0:
            out.append(doc[:at] + bytes([b]) + doc[at + 1:])
        elif op == 1:
            out.append(doc[:at] + bytes([b]) + doc[at:])
        else:
            out.append(doc[:at] + doc[at + 1:])
    return out


def all_documents() -> list[bytes]:
    """Every text the conformance tests feed the parser."""
    docs = [t for _, t, _ in TABLE]
    for i, (_, d) in enumerate(fuzz_documents()):
        docs += prefixes(d) + mutations(d, seed=1000 + i, count=MUTATIONS)
    return docs


MUTATIONS = 300  # per fuzz document
