"""What a JSON patch must do to a document: RFC 6902 over the JSON pointers
of RFC 6901, on plain Python values. It shares nothing with
csrc/apiserver/json_patch.cc or control/apiserver.py; the rules are the
RFCs', with the few choices the RFCs leave open written out here.

- The patch is an array of objects. Each has a string `op` (add, remove,
  replace, move, copy, test) and a string `path`; add, replace and test need
  a `value` member (null is a value); move and copy need a string `from`.
  Members an operation does not use are ignored (RFC 6902 section 4).
- A pointer is "" or starts with "/". In a token `~` is followed by 0 or 1;
  `~1` is decoded before `~0`, so `~01` is the two characters `~1`.
- An array index is `0` or `[1-9][0-9]*`: no sign, no leading zero, no blank.
  It is below the array's length; where a value is put (add, and the `path`
  of move and copy) it may equal the length, or be `-`, which means the
  same. In an object, `0` and `-` are member names like any other.
- add on an existing member replaces it; remove and replace need their
  target to exist; add and replace at "" give the value as the document.
- remove at "" is refused: the RFC names no result, and a document that
  has become null is not an object any more.
- move is refused when `from` is a proper prefix of `path`; with `from`
  equal to `path` (which must exist) it changes nothing. copy has no such
  rule: the whole document may be copied into one of its members.
- test is deep equality: object members unordered, numbers by value (1 is
  1.0), a bool never equal to a number, null equal to null only.
- Negative indexes, an extension of some libraries, are refused.
- All or nothing: `apply` returns a new document or raises `Refused`, and
  never changes its arguments.
"""
from __future__ import annotations

import copy
import re

OPS = ("add", "remove", "replace", "move", "copy", "test")
_INDEX = re.compile(r"\A(0|[1-9][0-9]*)\Z", re.ASCII)
_MISSING = object()


class Refused(ValueError):
    """The reference refuses this patch for this document."""


def tokens(pointer: str) -> list[str]:
    """RFC 6901 section 3 and 4: the reference tokens of a pointer."""
    if pointer == "":
        return []
    if pointer[0] != "/":
        raise Refused(f"pointer {pointer!r} does not start with /")
    out = []
    for raw in pointer[1:].split("/"):
        if re.search(r"~(?![01])", raw):
            raise Refused(f"pointer {pointer!r}: ~ not followed by 0 or 1")
        out.append(raw.replace("~1", "/").replace("~0", "~"))
    return out


def _index(token: str, length: int, putting: bool = False) -> int:
    """The position `token` names in an array of `length` elements."""
    if putting and token == "-":
        return length
    if not _INDEX.match(token):
        raise Refused(f"bad array index {token!r}")
    i = int(token)
    if i > length or (i == length and not putting):
        raise Refused(f"array index {token} out of range")
    return i


def _step(node, token: str):
    if isinstance(node, list):
        return node[_index(token, len(node))]
    if isinstance(node, dict):
        if token not in node:
            raise Refused(f"no member {token!r}")
        return node[token]
    raise Refused(f"cannot descend into a scalar at {token!r}")


def resolve(doc, toks: list[str]):
    for t in toks:
        doc = _step(doc, t)
    return doc


def _put(doc, toks: list[str], value):
    """The add operation (RFC 6902 section 4.1); returns the document."""
    if not toks:
        return value
    parent = resolve(doc, toks[:-1])
    if isinstance(parent, list):
        parent.insert(_index(toks[-1], len(parent), putting=True), value)
    elif isinstance(parent, dict):
        parent[toks[-1]] = value
    else:
        raise Refused("the parent of the target is a scalar")
    return doc


def _take(doc, toks: list[str]):
    """The remove operation (section 4.2) below the root; returns the value."""
    parent = resolve(doc, toks[:-1])
    if isinstance(parent, list):
        return parent.pop(_index(toks[-1], len(parent)))
    if isinstance(parent, dict):
        if toks[-1] not in parent:
            raise Refused(f"no member {toks[-1]!r}")
        return parent.pop(toks[-1])
    raise Refused("the parent of the target is a scalar")


def equal(a, b) -> bool:
    """JSON equality as RFC 6902 section 4.6 defines it."""
    if isinstance(a, bool) or isinstance(b, bool):
        return isinstance(a, bool) and isinstance(b, bool) and a == b
    if isinstance(a, (int, float)) and isinstance(b, (int, float)):
        return a == b  # Python compares an int with a float exactly
    if type(a) is not type(b):
        return False
    if isinstance(a, list):
        return len(a) == len(b) and all(equal(x, y) for x, y in zip(a, b))
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(equal(a[k], b[k]) for k in a)
    return a == b  # str, None


def check(patch) -> list[tuple]:
    """The patch document's shape, before any document is looked at:
    [(op, path tokens, from tokens or None, value or _MISSING)]."""
    if not isinstance(patch, list):
        raise Refused("a patch is an array")
    out = []
    for op in patch:
        if not isinstance(op, dict):
            raise Refused("an operation is an object")
        kind, path = op.get("op"), op.get("path")
        if not isinstance(kind, str) or kind not in OPS:
            raise Refused(f"unknown op {kind!r}")
        if not isinstance(path, str):
            raise Refused("path must be a string")
        src, value = None, _MISSING
        if kind in ("add", "replace", "test"):
            if "value" not in op:
                raise Refused(f"{kind} needs a value")
            value = op["value"]
        if kind in ("move", "copy"):
            if not isinstance(op.get("from"), str):
                raise Refused(f"{kind} needs a string from")
            src = tokens(op["from"])
        out.append((kind, tokens(path), src, value))
    return out


def apply(doc, patch):
    """The patched document, or Refused. `doc` and `patch` are left alone."""
    steps = check(patch)
    doc = copy.deepcopy(doc)
    for kind, path, src, value in steps:
        value = copy.deepcopy(value)
        if kind == "add":
            doc = _put(doc, path, value)
        elif kind == "remove":
            if not path:
                raise Refused("remove of the whole document")
            _take(doc, path)
        elif kind == "replace":
            resolve(doc, path)  # must exist
            if not path:
                doc = value
                continue
            parent = resolve(doc, path[:-1])
            parent[_index(path[-1], len(parent)) if isinstance(parent, list) else path[-1]] = value
        elif kind == "move":
            if len(src) < len(path) and path[:len(src)] == src:
                raise Refused("move into one of the value's own children")
            if src == path:
                resolve(doc, src)
                continue
            doc = _put(doc, path, _take(doc, src))
        elif kind == "copy":
            doc = _put(doc, path, copy.deepcopy(resolve(doc, src)))
        elif not equal(resolve(doc, path), value):
            raise Refused("test failed")
    return doc


def applies(doc, patch) -> bool:
    try:
        apply(doc, patch)
        return True
    except Refused:
        return False
