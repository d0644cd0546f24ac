// RFC 6902 JSON patch over the Json DOM (apiserver.h: apply_json_patch).
#include <algorithm>
#include <cctype>
#include <stdexcept>

#include "apiserver/api_error.h"
#include "apiserver/apiserver.h"

namespace xsched::apiserver {

namespace {

std::vector<std::string> split_pointer(const std::string& ptr) {
  std::vector<std::string> out;
  if (ptr.empty()) return out;
  if (ptr[0] != '/') throw ApiError(422, "Invalid", "bad JSON pointer \"" + ptr + "\"");
  size_t i = 1;
  for (;;) {
    size_t j = ptr.find('/', i);
    std::string seg = ptr.substr(i, j == std::string::npos ? std::string::npos : j - i);
    std::string d;
    for (size_t k = 0; k < seg.size(); ++k) {
      if (seg[k] == '~' && k + 1 < seg.size() && (seg[k + 1] == '0' || seg[k + 1] == '1')) {
        d.push_back(seg[k + 1] == '0' ? '~' : '/');
        ++k;
      } else {
        d.push_back(seg[k]);
      }
    }
    out.push_back(std::move(d));
    if (j == std::string::npos) break;
    i = j + 1;
  }
  return out;
}

size_t array_index(const std::string& s, size_t limit) {
  if (s.empty() || s.size() > 9 || !std::all_of(s.begin(), s.end(), [](char c) { return std::isdigit(c); }))
    throw std::out_of_range("bad array index " + s);
  size_t i = std::stoul(s);
  if (i > limit) throw std::out_of_range("array index " + s + " out of range");
  return i;
}

Json* child(Json* cur, const std::string& seg) {
  if (cur->is_array()) {
    auto& a = cur->items_mut();
    size_t i = array_index(seg, a.empty() ? 0 : a.size() - 1);
    if (i >= a.size()) throw std::out_of_range("array index out of range");
    return &a[i];
  }
  if (cur->is_object()) {
    Json* n = cur->get_mut(seg);
    if (!n) throw std::out_of_range("missing member " + seg);
    return n;
  }
  throw std::out_of_range("cannot descend into a scalar at " + seg);
}

Json* walk(Json& doc, const std::vector<std::string>& parts, size_t n) {
  Json* cur = &doc;
  for (size_t i = 0; i < n; ++i) cur = child(cur, parts[i]);
  return cur;
}

}  // namespace

Json apply_json_patch(const Json& in, const Json& ops) {
  Json doc = in;
  if (!ops.is_array()) throw ApiError(422, "Invalid", "json patch body must be an array");
  for (const auto& op0 : ops.items()) {
    Json op = op0;
    std::string kind = op["op"].as_string();
    try {
      auto parts = split_pointer(op["path"].as_string());
      if (kind == "test") {
        const Json* cur = walk(doc, parts, parts.size());
        if (*cur != op["value"]) throw ApiError(422, "Invalid", "test failed at " + op["path"].as_string());
        continue;
      }
      if (kind == "move" || kind == "copy") {
        auto src = split_pointer(op["from"].as_string());
        if (src.empty()) throw std::out_of_range("cannot move/copy the document root");
        Json* sp = walk(doc, src, src.size() - 1);
        Json val = *child(sp, src.back());
        if (kind == "move") {
          if (sp->is_array()) {
            auto& a = sp->items_mut();
            a.erase(a.begin() + static_cast<long>(array_index(src.back(), a.size() - 1)));
          } else {
            sp->erase(src.back());
          }
        }
        kind = "add";
        op = Json::object();
        op.set("value", std::move(val));
      }
      if (parts.empty()) {
        doc = op["value"];
        continue;
      }
      Json* par = walk(doc, parts, parts.size() - 1);
      const std::string& last = parts.back();
      if (kind == "add") {
        if (par->is_array()) {
          auto& a = par->items_mut();
          size_t i = last == "-" ? a.size() : array_index(last, a.size());
          a.insert(a.begin() + static_cast<long>(i), op["value"]);
        } else if (par->is_object()) {
          par->set(last, op["value"]);
        } else {
          throw std::out_of_range("parent is not a container");
        }
      } else if (kind == "remove") {
        if (par->is_array()) {
          auto& a = par->items_mut();
          if (a.empty()) throw std::out_of_range("remove from an empty array");
          a.erase(a.begin() + static_cast<long>(array_index(last, a.size() - 1)));
        } else if (!par->is_object() || !par->erase(last)) {
          throw std::out_of_range("missing member " + last);
        }
      } else if (kind == "replace") {
        *child(par, last) = op["value"];
      } else {
        throw ApiError(422, "Invalid", "unknown json-patch op \"" + kind + "\"");
      }
    } catch (const std::out_of_range& e) {
      throw ApiError(422, "Invalid", "json patch " + op0.dump() + ": " + e.what());
    }
  }
  return doc;
}

}  // namespace xsched::apiserver
