"""What the native JSON parser must accept, and as what: Python's
`json.loads` made strict. It shares nothing with csrc/common/json.cc; the
rules are the ones the header of csrc/common/json.h lists.

- The text is UTF-8, decoded with errors="strict": overlong forms, encoded
  surrogates, truncated sequences and code points above U+10FFFF are refused.
  A byte-order mark is not whitespace, so a document that starts with one is
  refused like any other stray character.
- `NaN`, `Infinity` and `-Infinity` are refused.
- An integer literal within int64 is an `int`. The DOM has no wider integer:
  a longer literal is read the way a literal with a fraction or an exponent
  is, as the nearest `float`. A number whose float is infinite is refused.
- A value may stand inside at most MAX_DEPTH arrays and objects.
- A surrogate escape that is not half of a valid pair becomes U+FFFD, as in
  Go's encoding/json (`loads` has already combined the valid pairs).
- Duplicate keys: the last value, at the first key's position (a dict).
"""
from __future__ import annotations

import json
import struct

MAX_DEPTH = 256  # csrc/common/json.h: "inside at most 256 arrays and objects"
INT64_MIN, INT64_MAX = -2**63, 2**63 - 1


class Rejected(ValueError):
    """The reference refuses this document."""


def _int(s: str):
    # At most 19 digits can fit int64; never hand a huge literal to int().
    if len(s) <= 20:
        v = int(s)
        if INT64_MIN <= v <= INT64_MAX:
            return v
    return _float(s)


def _float(s: str) -> float:
    v = float(s)
    if v in (float("inf"), float("-inf")):
        raise Rejected(f"number overflows a double: {s[:40]}")
    return v


def _constant(s: str):
    raise Rejected(f"not JSON: {s}")


class _Obj(dict):
    """A decoded object that remembers how deep its text nested, the values
    of dropped duplicate keys included (the parser read those too)."""
    height = 0


def _height(v) -> int:
    # Levels of container below v that hold something: a scalar and an empty
    # container both stand at their own depth only.
    if isinstance(v, _Obj):
        return v.height
    if isinstance(v, list) and v:
        return 1 + max(_height(x) for x in v)
    return 0


def _pairs(pairs):
    o = _Obj(pairs)
    if pairs:
        o.height = 1 + max(_height(v) for _, v in pairs)
        if o.height > MAX_DEPTH + 1:  # cheap early stop; loads() checks the root
            raise Rejected("nested too deep")
    return o


def _fix_str(s: str) -> str:
    if s.isascii():
        return s
    return "".join("\ufffd" if 0xD800 <= ord(c) <= 0xDFFF else c for c in s)


def _finish(v):
    """Plain dicts and lists, lone surrogates replaced."""
    if isinstance(v, str):
        return _fix_str(v)
    if isinstance(v, list):
        return [_finish(x) for x in v]
    if isinstance(v, dict):
        out = {}
        for k, x in v.items():
            out[_fix_str(k)] = _finish(x)  # two keys may meet after replacement: last wins
        return out
    return v


def loads(text: bytes | str):
    """The value of `text`, or Rejected."""
    if isinstance(text, (bytes, bytearray)):
        try:
            text = bytes(text).decode("utf-8", errors="strict")
        except UnicodeDecodeError as e:
            raise Rejected(str(e)) from None
    try:
        v = json.loads(text, parse_int=_int, parse_float=_float, parse_constant=_constant,
                       object_pairs_hook=_pairs)
    except Rejected:
        raise
    except (ValueError, RecursionError) as e:  # JSONDecodeError is a ValueError
        raise Rejected(str(e)) from None
    try:
        if _height(v) > MAX_DEPTH:
            raise Rejected("nested too deep")
        return _finish(v)
    except RecursionError:
        raise Rejected("nested too deep") from None


def accepts(text: bytes | str) -> bool:
    try:
        loads(text)
        return True
    except Rejected:
        return False


def same(a, b, int_float: bool = False, ordered: bool = False) -> bool:
    """Type-exact equality: an int is no float and no bool, floats compare by
    their bits, dicts by key and value (with `ordered`, by key order too).
    With `int_float`, an int and a float of exactly the same value count as
    the same."""
    if isinstance(a, bool) or isinstance(b, bool):
        return isinstance(a, bool) and isinstance(b, bool) and a == b
    if int_float and isinstance(a, (int, float)) and isinstance(b, (int, float)) and type(a) is not type(b):
        return a == b  # Python compares int with float exactly
    if type(a) is not type(b):
        return False
    if isinstance(a, float):
        return struct.pack("<d", a) == struct.pack("<d", b)
    if isinstance(a, list):
        return len(a) == len(b) and all(same(x, y, int_float, ordered) for x, y in zip(a, b))
    if isinstance(a, dict):
        if a.keys() != b.keys() or (ordered and list(a) != list(b)):
            return False
        return all(same(a[k], b[k], int_float, ordered) for k in a)
    return a == b
