// RFC 6902 JSON patch over the Json DOM (apiserver.h: apply_json_patch).
//
// The rules, choices the RFCs leave open included, are those of
// tests/json_patch_ref.py, and tests/test_json_patch_conformance.py holds
// this file to them: every operation's shape is checked before the document
// is touched; an array index is 0 or [1-9][0-9]* and in range; `~` in a
// pointer is followed by 0 or 1; remove at "" is refused.
#include <algorithm>
#include <stdexcept>
#include <string>
#include <vector>

#include "apiserver/api_error.h"
#include "apiserver/apiserver.h"

namespace xsched::apiserver {

namespace {

using Pointer = std::vector<std::string>;

// Why an operation cannot be applied; apply_json_patch makes it the 422.
struct Refused : std::runtime_error {
  using std::runtime_error::runtime_error;
};

Pointer split_pointer(const std::string& ptr) {
  Pointer out;
  if (ptr.empty()) return out;
  if (ptr[0] != '/') throw Refused("JSON pointer \"" + ptr + "\" does not start with /");
  out.emplace_back();
  for (size_t k = 1; k < ptr.size(); ++k) {
    if (ptr[k] == '/') {
      out.emplace_back();
    } else if (ptr[k] == '~') {
      char n = k + 1 < ptr.size() ? ptr[k + 1] : '\0';
      if (n != '0' && n != '1') throw Refused("JSON pointer \"" + ptr + "\": ~ is followed by 0 or 1");
      out.back().push_back(n == '0' ? '~' : '/');
      ++k;
    } else {
      out.back().push_back(ptr[k]);
    }
  }
  return out;
}

// The position `s` names in an array of `size` elements: below `size`, or
// with `putting` (where a value is inserted) up to it, `-` meaning `size`.
size_t array_index(const std::string& s, size_t size, bool putting = false) {
  if (putting && s == "-") return size;
  bool ok = !s.empty() && s.size() <= 9 && (s.size() == 1 || s[0] != '0');
  for (char c : s) ok = ok && c >= '0' && c <= '9';
  if (!ok) throw Refused("bad array index \"" + s + "\"");
  size_t i = std::stoul(s);
  if (i > size || (i == size && !putting)) throw Refused("array index " + s + " out of range");
  return i;
}

Json* child(Json* cur, const std::string& seg) {
  if (cur->is_array()) {
    auto& a = cur->items_mut();
    return &a[array_index(seg, a.size())];
  }
  if (cur->is_object()) {
    Json* n = cur->get_mut(seg);
    if (!n) throw Refused("missing member \"" + seg + "\"");
    return n;
  }
  throw Refused("cannot descend into a scalar at \"" + seg + "\"");
}

Json* walk(Json& doc, const Pointer& parts, size_t n) {
  Json* cur = &doc;
  for (size_t i = 0; i < n; ++i) cur = child(cur, parts[i]);
  return cur;
}

void add(Json& doc, const Pointer& path, Json value) {
  if (path.empty()) {
    doc = std::move(value);
    return;
  }
  Json* par = walk(doc, path, path.size() - 1);
  if (par->is_array()) {
    auto& a = par->items_mut();
    a.insert(a.begin() + static_cast<long>(array_index(path.back(), a.size(), /*putting=*/true)), std::move(value));
  } else if (par->is_object()) {
    par->set(path.back(), std::move(value));
  } else {
    throw Refused("the parent of the target is a scalar");
  }
}

// Below the root; returns what was there.
Json remove(Json& doc, const Pointer& path) {
  Json* par = walk(doc, path, path.size() - 1);
  Json old = *child(par, path.back());
  if (par->is_array()) {
    auto& a = par->items_mut();
    a.erase(a.begin() + static_cast<long>(array_index(path.back(), a.size())));
  } else {
    par->erase(path.back());
  }
  return old;
}

struct Op {
  enum Kind { Add, Remove, Replace, Move, Copy, Test } kind;
  Pointer path, from;
  const Json* value = nullptr;
};

// The shape of one operation (RFC 6902 section 4), before any document is looked at.
Op check(const Json& op) {
  static const char* const kNames[] = {"add", "remove", "replace", "move", "copy", "test"};
  if (!op.is_object()) throw Refused("an operation is an object");
  const Json* kind = op.get("op");
  const Json* path = op.get("path");
  Op out;
  size_t k = 0;
  while (k < 6 && !(kind && kind->is_string() && kind->as_string() == kNames[k])) ++k;
  if (k == 6) throw Refused("unknown json-patch op " + (kind ? kind->dump() : "(none)"));
  out.kind = static_cast<Op::Kind>(k);
  if (!path || !path->is_string()) throw Refused("path must be a string");
  out.path = split_pointer(path->as_string());
  if (out.kind == Op::Add || out.kind == Op::Replace || out.kind == Op::Test) {
    out.value = op.get("value");
    if (!out.value) throw Refused(std::string(kNames[k]) + " needs a value");
  }
  if (out.kind == Op::Move || out.kind == Op::Copy) {
    const Json* from = op.get("from");
    if (!from || !from->is_string()) throw Refused(std::string(kNames[k]) + " needs a string from");
    out.from = split_pointer(from->as_string());
  }
  return out;
}

void apply(Json& doc, const Op& op) {
  switch (op.kind) {
    case Op::Add: add(doc, op.path, *op.value); break;
    case Op::Remove:
      if (op.path.empty()) throw Refused("cannot remove the whole document");
      remove(doc, op.path);
      break;
    case Op::Replace: *walk(doc, op.path, op.path.size()) = *op.value; break;
    case Op::Move: {
      bool inside = op.from.size() < op.path.size() && std::equal(op.from.begin(), op.from.end(), op.path.begin());
      if (inside) throw Refused("cannot move a value into one of its own children");
      if (op.from == op.path) {
        walk(doc, op.from, op.from.size());  // must exist
        break;
      }
      add(doc, op.path, remove(doc, op.from));
      break;
    }
    case Op::Copy: add(doc, op.path, Json(*walk(doc, op.from, op.from.size()))); break;
    case Op::Test:
      if (*walk(doc, op.path, op.path.size()) != *op.value) throw Refused("test failed");
      break;
  }
}

}  // namespace

Json apply_json_patch(const Json& in, const Json& ops) {
  if (!ops.is_array()) throw ApiError(422, "Invalid", "json patch body must be an array");
  std::vector<Op> checked;
  checked.reserve(ops.size());
  const Json* at = nullptr;
  try {
    for (const auto& op : ops.items()) checked.push_back(check(*(at = &op)));
    Json doc = in;
    for (size_t i = 0; i < checked.size(); ++i) {
      at = &ops.items()[i];
      apply(doc, checked[i]);
    }
    return doc;
  } catch (const Refused& e) {
    throw ApiError(422, "Invalid", "json patch " + at->dump() + ": " + e.what());
  }
}

}  // namespace xsched::apiserver
