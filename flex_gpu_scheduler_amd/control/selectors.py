"""Label and field selectors: the string syntax of k8s.io/apimachinery's
pkg/labels (`a=b`, `a==b`, `a!=b`, `a>1`, `a<1`, `a in (x,y)`, `a notin (x)`,
`a`, `!a`, joined by commas) and pkg/fields (`path=value`, `path==value`,
`path!=value`). Used by the API server's list/watch filtering and by
controllers (the PodGroup controller lists pods by the
`pod-group.scheduling.sigs.k8s.io` label, pkg/controller/podgroup.go:209-210).

tests/selector_ref.py writes the grammar out, and
tests/test_selector_conformance.py holds this module and its native twin
(csrc/apiserver/selectors.cc) to it. A malformed selector is a ValueError.
"""
from __future__ import annotations

import re
from dataclasses import dataclass
from typing import Callable, Mapping

# One token: == and != before their first characters; an identifier is a run of anything else.
_TOKEN_RE = re.compile(r"[ \t\r\n]*(==|!=|[=!(),><]|[^ \t\r\n=!(),><]+)")
_NAME_RE = re.compile(r"[A-Za-z0-9]([-A-Za-z0-9_.]*[A-Za-z0-9])?", re.ASCII)
_SUBDOMAIN_RE = re.compile(r"[a-z0-9]([-a-z0-9]*[a-z0-9])?(\.[a-z0-9]([-a-z0-9]*[a-z0-9])?)*", re.ASCII)
_INT_RE = re.compile(r"[+-]?[0-9]+", re.ASCII)
_OPS = {"=": "=", "==": "=", "!=": "!=", ">": ">", "<": "<", "in": "in", "notin": "notin"}
_SYMBOLS = {"=", "==", "!=", "!", "(", ")", ",", ">", "<"}
_END = ""  # no token is empty


def _int64(s: str) -> int | None:
    """strconv.ParseInt(s, 10, 64)."""
    if not _INT_RE.fullmatch(s) or len(s.lstrip("+-").lstrip("0")) > 19:
        return None
    v = int(s)
    return v if -2**63 <= v < 2**63 else None


@dataclass(frozen=True)
class Requirement:
    key: str
    op: str                 # "=", "!=", "in", "notin", "exists", "!exists", ">", "<"
    values: tuple[str, ...] = ()   # sorted, each once

    def matches(self, labels: Mapping[str, str]) -> bool:
        has = self.key in labels
        if self.op == "exists":
            return has
        if self.op == "!exists":
            return not has
        if self.op in ("=", "in"):
            return has and labels[self.key] in self.values
        if self.op in (">", "<"):
            have = _int64(labels[self.key]) if has and isinstance(labels[self.key], str) else None
            want = _int64(self.values[0])
            return have is not None and (have > want if self.op == ">" else have < want)
        # "!=" / "notin": true when the key is absent (apimachinery semantics)
        return not has or labels[self.key] not in self.values


def _is_name(s: str) -> bool:
    return 1 <= len(s) <= 63 and _NAME_RE.fullmatch(s) is not None


def _check_key(key: str) -> None:
    prefix, slash, name = key.rpartition("/")
    if slash and not (len(prefix) <= 253 and _SUBDOMAIN_RE.fullmatch(prefix)) or not _is_name(name):
        raise ValueError(f"invalid selector: {key!r} is no qualified name")


def parse_selector(s: str | None) -> list[Requirement]:
    """The requirements of a label selector."""
    toks = _TOKEN_RE.findall(s or "") + [_END]
    at = 0

    def bad(what: str):
        return ValueError(f"invalid selector {s!r}: {what}, found {toks[at]!r}")

    reqs = []
    while toks[at] != _END:
        negated = toks[at] == "!"
        at += negated
        key = toks[at]
        if key in _SYMBOLS or key == _END:
            raise bad("expected a key")
        _check_key(key)
        at += 1
        if toks[at] in (",", _END):
            reqs.append(Requirement(key, "!exists" if negated else "exists"))
        elif negated:
            raise bad(f"!{key} stands alone")
        else:
            # `in` and `notin` are operators here only: as a key or a value they are identifiers.
            op = _OPS.get(toks[at])
            if op is None:
                raise bad("expected an operator")
            at += 1
            if op in ("in", "notin"):
                if toks[at] != "(":
                    raise bad(f"expected ( after {op}")
                at += 1
                # Identifiers and commas; every empty position is the value "".
                values, filled = set(), False
                while toks[at] != ")":
                    if toks[at] == ",":
                        if not filled:
                            values.add("")
                        filled = False
                    elif toks[at] in _SYMBOLS or toks[at] == _END or filled:
                        raise bad("expected a comma or )")
                    else:
                        values.add(toks[at])
                        filled = True
                    at += 1
                if not filled:
                    values.add("")
                at += 1
            elif toks[at] in (",", _END):
                values = {""}
            elif toks[at] in _SYMBOLS:
                raise bad("expected a value")
            else:
                values = {toks[at]}
                at += 1
            for v in values:
                if v and not _is_name(v):
                    raise ValueError(f"invalid selector {s!r}: {v!r} is no label value")
            if op in (">", "<") and any(_int64(v) is None for v in values):
                raise ValueError(f"invalid selector {s!r}: {op} needs an integer")
            reqs.append(Requirement(key, op, tuple(sorted(values))))
        if toks[at] == _END:
            break
        if toks[at] != ",":
            raise bad("expected a comma or the end")
        at += 1
        if toks[at] == _END or (toks[at] in _SYMBOLS and toks[at] != "!"):
            raise bad("a comma is followed by a requirement")
    return reqs


def label_matcher(s: str | None) -> Callable[[dict], bool] | None:
    reqs = parse_selector(s)
    if not reqs:
        return None

    def match(obj: dict) -> bool:
        labels = (obj.get("metadata") or {}).get("labels") or {}
        return all(r.matches(labels) for r in reqs)
    return match


_FIELD_TERM_RE = re.compile(r"((?:[^\\,]|\\.)*\\?)(?:,|\Z)", re.DOTALL)   # up to a comma no backslash escapes
_FIELD_OP_RE = re.compile(r"!=|==|=")
_FIELD_VALUE_RE = re.compile(r"(?:[^\\=]|\\[\\,=])*", re.DOTALL)


def parse_field_selector(s: str | None) -> list[Requirement]:
    """The requirements of a field selector: ops "=" and "!=", one value
    each. Nothing is trimmed; in a value `\\\\`, `\\,` and `\\=` stand for
    their second character."""
    reqs = []
    at, s = 0, s or ""
    while at < len(s):
        m = _FIELD_TERM_RE.match(s, at)
        term, at = m.group(1), max(m.end(), at + 1)
        if not term:
            continue
        op = _FIELD_OP_RE.search(term)
        if op is None:
            raise ValueError(f"invalid field selector {s!r}: {term!r} has no operator")
        raw = term[op.end():]
        if not _FIELD_VALUE_RE.fullmatch(raw):
            raise ValueError(f"invalid field selector {s!r}: bad escape or bare = in {raw!r}")
        reqs.append(Requirement(term[:op.start()], "!=" if op.group() == "!=" else "=", (re.sub(r"\\(.)", r"\1", raw),)))
    return reqs


def _field(obj: dict, path: str) -> str:
    cur = obj
    for part in path.split("."):
        if not isinstance(cur, dict):
            return ""
        cur = cur.get(part)
    if isinstance(cur, bool):
        return "true" if cur else "false"
    return "" if cur is None else str(cur)


def field_matcher(s: str | None) -> Callable[[dict], bool] | None:
    """Field selectors support = / == / != on any dotted path (the API server
    restricts keys per kind; we accept any path, e.g. spec.nodeName)."""
    reqs = parse_field_selector(s)
    if not reqs:
        return None

    def match(obj: dict) -> bool:
        for r in reqs:
            if (_field(obj, r.key) == r.values[0]) != (r.op == "="):
                return False
        return True
    return match


def combine(*ms: Callable[[dict], bool] | None) -> Callable[[dict], bool] | None:
    live = [m for m in ms if m is not None]
    if not live:
        return None
    if len(live) == 1:
        return live[0]
    return lambda o: all(m(o) for m in live)
