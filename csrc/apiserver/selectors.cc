// Label and field selectors: the k8s.io/apimachinery string syntax, parsed and matched (apiserver.h).
#include <algorithm>
#include <cctype>
#include <stdexcept>

#include "apiserver/apiserver.h"
#include "common/strings.h"

namespace xsched::apiserver {

namespace {

bool valid_key_char(char c) {
  return std::isalnum(static_cast<unsigned char>(c)) || c == '_' || c == '.' || c == '/' || c == '-';
}

std::string field_string(const Json& obj, std::string_view path) {
  const Json* cur = &obj;
  size_t i = 0;
  while (i <= path.size()) {
    size_t j = path.find('.', i);
    if (j == std::string_view::npos) j = path.size();
    if (!cur->is_object()) return "";
    cur = cur->get(path.substr(i, j - i));
    if (!cur) return "";
    i = j + 1;
  }
  switch (cur->type()) {
    case Json::Type::Null: return "";
    case Json::Type::String: return cur->as_string();
    case Json::Type::Bool: return cur->as_bool() ? "true" : "false";
    case Json::Type::Int: return std::to_string(cur->as_int());
    default: return cur->dump();
  }
}

}  // namespace

std::vector<Requirement> parse_selector(std::string_view s) {
  std::vector<Requirement> out;
  std::vector<std::string_view> terms;
  int depth = 0;
  size_t start = 0;
  for (size_t i = 0; i <= s.size(); ++i) {
    char c = i < s.size() ? s[i] : ',';
    if (c == '(') ++depth;
    if (c == ')') --depth;
    if (c == ',' && depth <= 0) {
      auto t = trim(s.substr(start, i - start));
      if (!t.empty()) terms.push_back(t);
      start = i + 1;
    }
  }
  for (auto term : terms) {
    Requirement r;
    size_t p;
    if ((p = term.find("!=")) != std::string_view::npos) {
      r.op = Requirement::Ne;
      r.key = std::string(trim(term.substr(0, p)));
      r.values = {std::string(trim(term.substr(p + 2)))};
    } else if ((p = term.find("==")) != std::string_view::npos) {
      r.op = Requirement::Eq;
      r.key = std::string(trim(term.substr(0, p)));
      r.values = {std::string(trim(term.substr(p + 2)))};
    } else if ((p = term.find('=')) != std::string_view::npos && term.find('(') == std::string_view::npos) {
      r.op = Requirement::Eq;
      r.key = std::string(trim(term.substr(0, p)));
      r.values = {std::string(trim(term.substr(p + 1)))};
    } else {
      std::string_view t = term;
      bool neg = false;
      if (!t.empty() && t[0] == '!') {
        neg = true;
        t = trim(t.substr(1));
      }
      size_t k = 0;
      while (k < t.size() && valid_key_char(t[k])) ++k;
      r.key = std::string(t.substr(0, k));
      std::string_view rest = trim(t.substr(k));
      if (rest.empty()) {
        r.op = neg ? Requirement::NotExists : Requirement::Exists;
      } else {
        bool notin = rest.substr(0, 5) == "notin", in = !notin && rest.substr(0, 2) == "in";
        if (neg || (!notin && !in) || k == t.size() || !std::isspace(static_cast<unsigned char>(t[k])))
          throw std::invalid_argument("invalid selector term \"" + std::string(term) + "\"");
        rest = trim(rest.substr(notin ? 5 : 2));
        if (rest.size() < 2 || rest.front() != '(' || rest.back() != ')')
          throw std::invalid_argument("invalid selector term \"" + std::string(term) + "\"");
        r.op = notin ? Requirement::NotIn : Requirement::In;
        std::string_view vals = rest.substr(1, rest.size() - 2);
        size_t a = 0;
        for (size_t i = 0; i <= vals.size(); ++i) {
          if (i == vals.size() || vals[i] == ',') {
            auto v = trim(vals.substr(a, i - a));
            if (!v.empty()) r.values.emplace_back(v);
            a = i + 1;
          }
        }
      }
    }
    if (r.key.empty()) throw std::invalid_argument("invalid selector term \"" + std::string(term) + "\"");
    out.push_back(std::move(r));
  }
  return out;
}

bool labels_match(const std::vector<Requirement>& reqs, const Json& obj) {
  const Json& labels = obj["metadata"]["labels"];
  for (const auto& r : reqs) {
    const Json* v = labels.get(r.key);
    bool has = v != nullptr;
    const std::string& val = has ? v->as_string() : json_null().as_string();
    bool in_values = has && std::find(r.values.begin(), r.values.end(), val) != r.values.end();
    bool ok;
    switch (r.op) {
      case Requirement::Exists: ok = has; break;
      case Requirement::NotExists: ok = !has; break;
      case Requirement::Eq:
      case Requirement::In: ok = in_values; break;
      default: ok = !in_values; break;  // != / notin: true when the key is absent
    }
    if (!ok) return false;
  }
  return true;
}

bool fields_match(const std::vector<Requirement>& reqs, const Json& obj) {
  for (const auto& r : reqs) {
    if (r.op != Requirement::Eq && r.op != Requirement::Ne)
      throw std::invalid_argument("field selector supports only = and !=");
    bool eq = field_string(obj, r.key) == r.values.at(0);
    if (eq != (r.op == Requirement::Eq)) return false;
  }
  return true;
}

}  // namespace xsched::apiserver
