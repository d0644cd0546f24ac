"""What a label selector and a field selector mean: the string syntax of
k8s.io/apimachinery/pkg/labels and pkg/fields, on plain Python values. It
shares nothing with csrc/apiserver/selectors.cc or control/selectors.py.

Label selectors
- Tokens: blanks (space, TAB, CR, LF) separate; the symbols are
  `= ! ( ) , > <`, of which `==` and `!=` are read as one (longest match);
  an identifier is a maximal run of anything else. `in` and `notin` are
  operators only where an operator is expected: as a key or a value they
  are identifiers.
- A selector is empty, or requirements joined by single commas; a comma is
  followed by a requirement. A requirement is `KEY`, `!KEY` (then a comma or
  the end), `KEY op VALUE` for `= == != > <` where VALUE is one identifier or
  nothing before a comma or the end, or `KEY in|notin ( list )`. The list is
  identifiers and commas, no two identifiers without a comma between them;
  every empty position is the value "", so `()`, `(,x)`, `(x,)` and `(x,,y)`
  hold "". A requirement's values are a set: sorted, each once.
- A key is a qualified name: an optional prefix (a DNS subdomain of RFC 1123,
  at most 253 characters) and `/`, then a name of 1 to 63 characters,
  `[A-Za-z0-9]([-A-Za-z0-9_.]*[A-Za-z0-9])?`. A value is empty or such a
  name. `>` and `<` take one value that is a decimal int64.
- `=`, `==`, `in`: the label is there and its value in the set. `!=`,
  `notin`: the label is absent or its value not in the set. `>`, `<`: the
  label is there, reads as a decimal int64 (a sign allowed, as
  strconv.ParseInt reads it) and compares so.

Field selectors
- Terms are split at commas that no odd run of backslashes precedes; empty
  terms are skipped. In a term the leftmost of `!=`, `==`, `=` parts key and
  value; a term without one is an error. Nothing is trimmed.
- In the value `\\\\`, `\\,` and `\\=` stand for the second character; any other
  backslash sequence and a backslash at the end are errors, and so is a bare
  `=` (fields.UnescapeValue: a `=` in a value is written `\\=`).
- A requirement compares the string of the field at the dotted path: the
  string itself, `true` or `false`, a decimal integer, and "" for null, for
  a missing member and for a path through something that is no object.
"""
from __future__ import annotations

import re

BLANKS = " \t\r\n"
SYMBOLS = "=!(),><"
#                 spelling -> the name control/selectors.py uses
OPERATORS = {"=": "=", "==": "=", "!=": "!=", ">": ">", "<": "<", "in": "in", "notin": "notin"}
_NAME = re.compile(r"\A[A-Za-z0-9]([-A-Za-z0-9_.]*[A-Za-z0-9])?\Z", re.ASCII)
_SUBDOMAIN = re.compile(r"\A[a-z0-9]([-a-z0-9]*[a-z0-9])?(\.[a-z0-9]([-a-z0-9]*[a-z0-9])?)*\Z", re.ASCII)
_INT = re.compile(r"\A[+-]?[0-9]+\Z", re.ASCII)
END = ("end", "")


class Refused(ValueError):
    """The reference refuses this selector."""


# ------------------------------------------------------------------ labels --
def lex(s: str) -> list[tuple[str, str]]:
    """[("sym", "=="), ("id", "app"), ...]"""
    out, i = [], 0
    while i < len(s):
        c = s[i]
        if c in BLANKS:
            i += 1
        elif c in SYMBOLS:
            lit = s[i:i + 2] if s[i:i + 2] in ("==", "!=") else c
            out.append(("sym", lit))
            i += len(lit)
        else:
            j = i
            while j < len(s) and s[j] not in BLANKS and s[j] not in SYMBOLS:
                j += 1
            out.append(("id", s[i:j]))
            i = j
    return out


def _int64(s: str):
    if not _INT.match(s) or len(s) > 40:
        return None
    v = int(s)
    return v if -2**63 <= v < 2**63 else None


def _check_key(key: str) -> None:
    parts = key.split("/")
    if len(parts) > 2:
        raise Refused(f"key {key!r}: more than one /")
    if len(parts) == 2 and (not parts[0] or len(parts[0]) > 253 or not _SUBDOMAIN.match(parts[0])):
        raise Refused(f"key {key!r}: the prefix is no DNS subdomain")
    if not 1 <= len(parts[-1]) <= 63 or not _NAME.match(parts[-1]):
        raise Refused(f"key {key!r}: bad name")


def _check_value(v: str) -> None:
    if v and (len(v) > 63 or not _NAME.match(v)):
        raise Refused(f"bad label value {v!r}")


def parse_labels(s: str) -> list[tuple[str, str, list[str]]]:
    """[(key, op, [values])], op one of = != in notin exists !exists > <."""
    toks = lex(s) + [END]
    at = 0

    def take():
        nonlocal at
        at += 1
        return toks[at - 1]

    def ends_requirement(t):
        return t == END or t == ("sym", ",")

    reqs = []
    while toks[at] != END:
        negated = toks[at] == ("sym", "!")
        if negated:
            take()
        kind, key = take()
        if kind != "id":
            raise Refused(f"expected a key, found {key!r}")
        _check_key(key)
        if ends_requirement(toks[at]):
            reqs.append((key, "!exists" if negated else "exists", []))
        elif negated:
            raise Refused(f"!{key} is followed by {toks[at][1]!r}")
        else:
            spelling = take()[1]  # `in` as an identifier and `=` as a symbol alike
            if spelling not in OPERATORS:
                raise Refused(f"expected an operator, found {spelling!r}")
            op = OPERATORS[spelling]
            if op in ("in", "notin"):
                if take() != ("sym", "("):
                    raise Refused(f"{spelling} is not followed by (")
                values, here = set(), 0  # here: identifiers since the last comma
                while toks[at] != ("sym", ")"):
                    kind, lit = take()
                    if kind == "id" and here == 0:
                        values.add(lit)
                        here = 1
                    elif (kind, lit) == ("sym", ","):
                        if here == 0:
                            values.add("")
                        here = 0
                    else:
                        raise Refused(f"in a value list: {lit!r}")
                if here == 0:
                    values.add("")
                take()
            elif ends_requirement(toks[at]):
                values = {""}
            else:
                kind, lit = take()
                if kind != "id":
                    raise Refused(f"expected a value, found {lit!r}")
                values = {lit}
            for v in values:
                _check_value(v)
            if op in (">", "<") and any(_int64(v) is None for v in values):
                raise Refused(f"{op} needs an integer")
            reqs.append((key, op, sorted(values)))
        if toks[at] == END:
            break
        if take() != ("sym", ","):
            raise Refused(f"expected a comma or the end, found {toks[at - 1][1]!r}")
        if toks[at][0] != "id" and toks[at] != ("sym", "!"):
            raise Refused("a comma is followed by a requirement")
    return reqs


def labels_match(reqs, obj) -> bool:
    labels = ((obj.get("metadata") or {}).get("labels") or {}) if isinstance(obj, dict) else {}
    for key, op, values in reqs:
        has = key in labels
        if op == "exists":
            ok = has
        elif op == "!exists":
            ok = not has
        elif op in ("=", "in"):
            ok = has and labels[key] in values
        elif op in ("!=", "notin"):
            ok = not has or labels[key] not in values
        else:
            have = _int64(labels[key]) if has else None
            want = _int64(values[0])
            ok = have is not None and (have > want if op == ">" else have < want)
        if not ok:
            return False
    return True


# ------------------------------------------------------------------ fields --
def parse_fields(s: str) -> list[tuple[str, str, str]]:
    """[(dotted path, "=" or "!=", value)]"""
    terms, cur, escaped = [], "", False
    for c in s:
        if escaped:
            escaped = False
        elif c == "\\":
            escaped = True
        elif c == ",":
            terms.append(cur)
            cur = ""
            continue
        cur += c
    terms.append(cur)
    reqs = []
    for term in terms:
        if term == "":
            continue
        for i in range(len(term)):
            spelling = next((o for o in ("!=", "==", "=") if term.startswith(o, i)), None)
            if spelling:
                break
        else:
            raise Refused(f"term {term!r} has no operator")
        raw, value, escaped = term[i + len(spelling):], "", False
        for c in raw:
            if escaped:
                if c not in "\\,=":
                    raise Refused(f"bad escape \\{c}")
                value += c
                escaped = False
            elif c == "\\":
                escaped = True
            elif c == "=":
                raise Refused("a bare = in a value")
            else:
                value += c
        if escaped:
            raise Refused("a backslash at the end")
        reqs.append((term[:i], "!=" if spelling == "!=" else "=", value))
    return reqs


def field_string(obj, path: str) -> str:
    for part in path.split("."):
        if not isinstance(obj, dict) or part not in obj:
            return ""
        obj = obj[part]
    if obj is None:
        return ""
    if isinstance(obj, bool):
        return "true" if obj else "false"
    if isinstance(obj, (str, int)):
        return str(obj)
    raise NotImplementedError("containers and floating-point fields are out of scope")


def fields_match(reqs, obj) -> bool:
    return all((field_string(obj, path) == value) == (op == "=") for path, op, value in reqs)
