// Label and field selectors: the string syntax of k8s.io/apimachinery's
// pkg/labels and pkg/fields, parsed and matched (apiserver.h). The grammar is
// written out in tests/selector_ref.py, and
// tests/test_selector_conformance.py holds this file to it.
#include <algorithm>
#include <cstdint>
#include <stdexcept>

#include "apiserver/apiserver.h"

namespace xsched::apiserver {

namespace {

[[noreturn]] void refuse(const std::string& why) { throw std::invalid_argument("invalid selector: " + why); }

// ---------------------------------------------------------------- labels --
bool is_blank(char c) { return c == ' ' || c == '\t' || c == '\r' || c == '\n'; }
bool is_symbol(char c) { return std::string_view("=!(),><").find(c) != std::string_view::npos; }
bool is_alnum(char c) { return (c >= '0' && c <= '9') || (c >= 'a' && c <= 'z') || (c >= 'A' && c <= 'Z'); }

struct Token {
  enum Kind { Id, Symbol, End } kind;
  std::string_view text;
  bool is(std::string_view symbol) const { return kind == Symbol && text == symbol; }
  bool ends_requirement() const { return kind == End || is(","); }
};

// Blanks separate; == and != are one symbol; an identifier is a maximal run of anything else.
std::vector<Token> lex(std::string_view s) {
  std::vector<Token> out;
  size_t i = 0;
  while (i < s.size()) {
    if (is_blank(s[i])) {
      ++i;
    } else if (is_symbol(s[i])) {
      size_t n = (s[i] == '=' || s[i] == '!') && i + 1 < s.size() && s[i + 1] == '=' ? 2 : 1;
      out.push_back({Token::Symbol, s.substr(i, n)});
      i += n;
    } else {
      size_t j = i;
      while (j < s.size() && !is_blank(s[j]) && !is_symbol(s[j])) ++j;
      out.push_back({Token::Id, s.substr(i, j - i)});
      i = j;
    }
  }
  out.push_back({Token::End, {}});
  return out;
}

// [A-Za-z0-9]([-A-Za-z0-9_.]*[A-Za-z0-9])?, 1 to 63 characters.
bool is_name(std::string_view s) {
  if (s.empty() || s.size() > 63 || !is_alnum(s.front()) || !is_alnum(s.back())) return false;
  return std::all_of(s.begin(), s.end(), [](char c) { return is_alnum(c) || c == '-' || c == '_' || c == '.'; });
}

// RFC 1123: lower-case labels of letters, digits and inner dashes, joined by dots; at most 253 characters.
bool is_dns_subdomain(std::string_view s) {
  if (s.empty() || s.size() > 253) return false;
  auto lower = [](char c) { return (c >= '0' && c <= '9') || (c >= 'a' && c <= 'z'); };
  for (size_t i = 0; i < s.size(); ++i) {
    bool edge = i == 0 || i + 1 == s.size() || s[i - 1] == '.' || s[i + 1] == '.';
    if (!(lower(s[i]) || (!edge && (s[i] == '-' || s[i] == '.')))) return false;
  }
  return true;
}

void check_key(std::string_view key) {
  size_t slash = key.find('/');
  bool ok = slash == std::string_view::npos
                ? is_name(key)
                : is_dns_subdomain(key.substr(0, slash)) && is_name(key.substr(slash + 1));
  if (!ok) refuse("\"" + std::string(key) + "\" is no qualified name");
}

// A decimal int64 as strconv.ParseInt reads it: an optional sign, then digits.
bool parse_int64(std::string_view s, int64_t* out) {
  bool neg = !s.empty() && s[0] == '-';
  if (!s.empty() && (s[0] == '-' || s[0] == '+')) s.remove_prefix(1);
  if (s.empty()) return false;
  uint64_t v = 0;
  const uint64_t limit = neg ? uint64_t{1} << 63 : (uint64_t{1} << 63) - 1;
  for (char c : s) {
    if (c < '0' || c > '9') return false;
    uint64_t d = static_cast<uint64_t>(c - '0');
    if (v > (limit - d) / 10) return false;
    v = v * 10 + d;
  }
  *out = neg ? static_cast<int64_t>(~v + 1) : static_cast<int64_t>(v);
  return true;
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
  const std::vector<Token> toks = lex(s);
  std::vector<Requirement> out;
  size_t at = 0;
  while (toks[at].kind != Token::End) {
    Requirement r;
    bool negated = toks[at].is("!");
    if (negated) ++at;
    if (toks[at].kind != Token::Id) refuse("expected a key, found \"" + std::string(toks[at].text) + "\"");
    r.key = std::string(toks[at++].text);
    check_key(r.key);
    if (toks[at].ends_requirement()) {
      r.op = negated ? Requirement::NotExists : Requirement::Exists;
    } else if (negated) {
      refuse("!" + r.key + " is followed by \"" + std::string(toks[at].text) + "\"");
    } else {
      // `in` and `notin` are operators here only: as a key or a value they are identifiers.
      std::string_view op = toks[at++].text;
      if (op == "=" || op == "==") r.op = Requirement::Eq;
      else if (op == "!=") r.op = Requirement::Ne;
      else if (op == ">") r.op = Requirement::Gt;
      else if (op == "<") r.op = Requirement::Lt;
      else if (op == "in") r.op = Requirement::In;
      else if (op == "notin") r.op = Requirement::NotIn;
      else refuse("expected an operator, found \"" + std::string(op) + "\"");
      if (r.op == Requirement::In || r.op == Requirement::NotIn) {
        if (!toks[at++].is("(")) refuse(std::string(op) + " is not followed by (");
        // Identifiers and commas; every empty position is the value "".
        bool filled = false;  // an identifier since the last comma
        for (; !toks[at].is(")"); ++at) {
          if (toks[at].kind == Token::Id && !filled) {
            r.values.emplace_back(toks[at].text);
            filled = true;
          } else if (toks[at].is(",")) {
            if (!filled) r.values.emplace_back();
            filled = false;
          } else {
            refuse("in a value list: \"" + std::string(toks[at].text) + "\"");
          }
        }
        if (!filled) r.values.emplace_back();
        ++at;
      } else if (toks[at].ends_requirement()) {
        r.values.emplace_back();
      } else if (toks[at].kind == Token::Id) {
        r.values.emplace_back(toks[at++].text);
      } else {
        refuse("expected a value, found \"" + std::string(toks[at].text) + "\"");
      }
      // A set, as in apimachinery: sorted, each value once.
      std::sort(r.values.begin(), r.values.end());
      r.values.erase(std::unique(r.values.begin(), r.values.end()), r.values.end());
      for (const auto& v : r.values)
        if (!v.empty() && !is_name(v)) refuse("\"" + v + "\" is no label value");
      int64_t n;
      if ((r.op == Requirement::Gt || r.op == Requirement::Lt) && !parse_int64(r.values[0], &n))
        refuse(std::string(op) + " needs an integer");
    }
    out.push_back(std::move(r));
    if (toks[at].kind == Token::End) break;
    if (!toks[at].is(",")) refuse("expected a comma or the end, found \"" + std::string(toks[at].text) + "\"");
    ++at;
    if (toks[at].kind != Token::Id && !toks[at].is("!")) refuse("a comma is followed by a requirement");
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
      case Requirement::Gt:
      case Requirement::Lt: {
        int64_t have, want;
        ok = has && parse_int64(val, &have) && parse_int64(r.values.at(0), &want) &&
             (r.op == Requirement::Gt ? have > want : have < want);
        break;
      }
      default: ok = !in_values; break;  // != / notin: true when the key is absent
    }
    if (!ok) return false;
  }
  return true;
}

// ---------------------------------------------------------------- fields --
std::vector<Requirement> parse_field_selector(std::string_view s) {
  std::vector<Requirement> out;
  // Terms end at a comma that no backslash escapes; empty ones are skipped.
  size_t start = 0;
  bool escaped = false;
  for (size_t i = 0; i <= s.size(); ++i) {
    if (i < s.size() && (escaped || s[i] != ',')) {
      escaped = !escaped && s[i] == '\\';
      continue;
    }
    std::string_view term = s.substr(start, i - start);
    start = i + 1;
    if (term.empty()) continue;
    // The leftmost of != == = parts key and value; nothing is trimmed.
    size_t p = term.find_first_of("!=");
    while (p != std::string_view::npos && term[p] == '!' && term.substr(p, 2) != "!=") p = term.find_first_of("!=", p + 1);
    if (p == std::string_view::npos) refuse("\"" + std::string(term) + "\" has no operator");
    Requirement r;
    r.op = term[p] == '!' ? Requirement::Ne : Requirement::Eq;
    r.key = std::string(term.substr(0, p));
    std::string_view raw = term.substr(p + (term[p] == '!' || term.substr(p, 2) == "==" ? 2 : 1));
    std::string value;
    for (size_t k = 0; k < raw.size(); ++k) {
      if (raw[k] == '\\') {
        char n = k + 1 < raw.size() ? raw[k + 1] : '\0';
        if (n != '\\' && n != ',' && n != '=') refuse("bad escape in \"" + std::string(term) + "\"");
        value.push_back(n);
        ++k;
      } else if (raw[k] == '=') {
        refuse("a = in a value is written \\=: \"" + std::string(term) + "\"");
      } else {
        value.push_back(raw[k]);
      }
    }
    r.values.push_back(std::move(value));
    out.push_back(std::move(r));
  }
  return out;
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
