#include "common/json.h"

#include <array>
#include <cerrno>
#include <charconv>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>

namespace xsched {

namespace {
const std::string kEmptyString;
const Json::Array kEmptyArray;
const Json::Object kEmptyObject;

class Parser {
 public:
  explicit Parser(std::string_view s) : p_(s.data()), end_(s.data() + s.size()) {}

  Json parse_document() {
    ws();
    Json v = value(0);
    ws();
    if (p_ != end_) fail("trailing characters");
    return v;
  }

  // Top-level array, one element at a time (bulk creates pipeline parsing
  // with store inserts and informer hand-off).
  void parse_array_stream(const std::function<void(Json&&)>& fn) {
    ws();
    if (p_ >= end_ || *p_ != '[') fail("expected a JSON array");
    ++p_;
    ws();
    if (p_ < end_ && *p_ == ']') {
      ++p_;
    } else {
      for (;;) {
        ws();
        fn(value(1));
        ws();
        if (p_ < end_ && *p_ == ',') { ++p_; continue; }
        if (p_ < end_ && *p_ == ']') { ++p_; break; }
        fail("expected ',' or ']'");
      }
    }
    ws();
    if (p_ != end_) fail("trailing characters");
  }

 private:
  const char* p_;
  const char* end_;

  [[noreturn]] void fail(const char* what) {
    throw JsonError(std::string("json parse error: ") + what);
  }
  void ws() {
    while (p_ < end_ && (*p_ == ' ' || *p_ == '\n' || *p_ == '\r' || *p_ == '\t')) ++p_;
  }
  bool lit(const char* l, size_t n) {
    if (static_cast<size_t>(end_ - p_) >= n && std::memcmp(p_, l, n) == 0) {
      p_ += n;
      return true;
    }
    return false;
  }

  Json value(int depth) {
    if (depth > 256) fail("nesting too deep");
    if (p_ >= end_) fail("unexpected end");
    switch (*p_) {
      case '{': return object(depth);
      case '[': return array(depth);
      case '"': return Json(string());
      case 't': if (lit("true", 4)) return Json(true); fail("bad literal");
      case 'f': if (lit("false", 5)) return Json(false); fail("bad literal");
      case 'n': if (lit("null", 4)) return Json(); fail("bad literal");
      default: return number();
    }
  }

  Json object(int depth) {
    ++p_;
    Json o = Json::object();
    auto& m = o.members_mut();
    ws();
    if (p_ < end_ && *p_ == '}') { ++p_; return o; }
    for (;;) {
      ws();
      if (p_ >= end_ || *p_ != '"') fail("expected key");
      std::string k = string();
      ws();
      if (p_ >= end_ || *p_ != ':') fail("expected ':'");
      ++p_;
      ws();
      Json v = value(depth + 1);
      // Duplicate keys: last one wins (encoding/json semantics).
      bool replaced = false;
      for (auto& kv : m) {
        if (kv.first == k) { kv.second = std::move(v); replaced = true; break; }
      }
      if (!replaced) m.emplace_back(std::move(k), std::move(v));
      ws();
      if (p_ < end_ && *p_ == ',') { ++p_; continue; }
      if (p_ < end_ && *p_ == '}') { ++p_; return o; }
      fail("expected ',' or '}'");
    }
  }

  Json array(int depth) {
    ++p_;
    Json a = Json::array();
    auto& items = a.items_mut();
    ws();
    if (p_ < end_ && *p_ == ']') { ++p_; return a; }
    for (;;) {
      ws();
      items.push_back(value(depth + 1));
      ws();
      if (p_ < end_ && *p_ == ',') { ++p_; continue; }
      if (p_ < end_ && *p_ == ']') { ++p_; return a; }
      fail("expected ',' or ']'");
    }
  }

  static void put_utf8(std::string& out, uint32_t cp) {
    if (cp < 0x80) {
      out.push_back(static_cast<char>(cp));
    } else if (cp < 0x800) {
      out.push_back(static_cast<char>(0xC0 | (cp >> 6)));
      out.push_back(static_cast<char>(0x80 | (cp & 0x3F)));
    } else if (cp < 0x10000) {
      out.push_back(static_cast<char>(0xE0 | (cp >> 12)));
      out.push_back(static_cast<char>(0x80 | ((cp >> 6) & 0x3F)));
      out.push_back(static_cast<char>(0x80 | (cp & 0x3F)));
    } else {
      out.push_back(static_cast<char>(0xF0 | (cp >> 18)));
      out.push_back(static_cast<char>(0x80 | ((cp >> 12) & 0x3F)));
      out.push_back(static_cast<char>(0x80 | ((cp >> 6) & 0x3F)));
      out.push_back(static_cast<char>(0x80 | (cp & 0x3F)));
    }
  }

  uint32_t hex4() {
    if (end_ - p_ < 4) fail("bad \\u escape");
    uint32_t v = 0;
    for (int i = 0; i < 4; ++i) {
      char c = *p_++;
      v <<= 4;
      if (c >= '0' && c <= '9') v |= c - '0';
      else if (c >= 'a' && c <= 'f') v |= c - 'a' + 10;
      else if (c >= 'A' && c <= 'F') v |= c - 'A' + 10;
      else fail("bad hex digit");
    }
    return v;
  }

  // 1 for the bytes that end a run of plain string bytes: the quote, the
  // backslash, the control bytes (refused) and every byte of a multi-byte
  // UTF-8 sequence (validated).
  static constexpr auto kStop = [] {
    std::array<uint8_t, 256> t{};
    for (int c = 0; c < 0x20; ++c) t[c] = 1;
    for (int c = 0x80; c < 0x100; ++c) t[c] = 1;
    t['"'] = 1;
    t['\\'] = 1;
    return t;
  }();

  // One well-formed multi-byte sequence (Unicode 15, table 3-7): no overlong
  // form, no surrogate, nothing above U+10FFFF.
  void utf8_sequence() {
    auto cont = [&](int k, unsigned lo, unsigned hi) {
      if (end_ - p_ <= k) fail("truncated UTF-8 sequence");
      unsigned char c = static_cast<unsigned char>(p_[k]);
      if (c < lo || c > hi) fail("invalid UTF-8 sequence");
    };
    unsigned char c = static_cast<unsigned char>(*p_);
    if (c >= 0xC2 && c <= 0xDF) {
      cont(1, 0x80, 0xBF);
      p_ += 2;
    } else if (c >= 0xE0 && c <= 0xEF) {
      cont(1, c == 0xE0 ? 0xA0 : 0x80, c == 0xED ? 0x9F : 0xBF);
      cont(2, 0x80, 0xBF);
      p_ += 3;
    } else if (c >= 0xF0 && c <= 0xF4) {
      cont(1, c == 0xF0 ? 0x90 : 0x80, c == 0xF4 ? 0x8F : 0xBF);
      cont(2, 0x80, 0xBF);
      cont(3, 0x80, 0xBF);
      p_ += 4;
    } else {
      fail("invalid UTF-8 byte");
    }
  }

  std::string string() {
    ++p_;  // opening quote
    std::string out;
    const char* run = p_;
    while (p_ < end_) {
      unsigned char c = static_cast<unsigned char>(*p_);
      if (!kStop[c]) {
        ++p_;
        continue;
      }
      if (c == '"') {
        out.append(run, p_);
        ++p_;
        return out;
      }
      if (c >= 0x80) {
        utf8_sequence();
        continue;
      }
      if (c < 0x20) fail("control character in string");
      // c == '\\'
      out.append(run, p_);
      ++p_;
      if (p_ >= end_) fail("bad escape");
      char e = *p_++;
      switch (e) {
        case '"': out.push_back('"'); break;
        case '\\': out.push_back('\\'); break;
        case '/': out.push_back('/'); break;
        case 'b': out.push_back('\b'); break;
        case 'f': out.push_back('\f'); break;
        case 'n': out.push_back('\n'); break;
        case 'r': out.push_back('\r'); break;
        case 't': out.push_back('\t'); break;
        case 'u': {
          // A high surrogate directly followed by a low one is one code
          // point; any other surrogate escape stands alone and becomes
          // U+FFFD (encoding/json), and what followed it is read afresh.
          uint32_t cp = hex4();
          if (cp >= 0xD800 && cp <= 0xDBFF) {
            const char* after = p_;
            uint32_t lo = 0;
            if (end_ - p_ >= 6 && p_[0] == '\\' && p_[1] == 'u') {
              p_ += 2;
              lo = hex4();
            }
            if (lo >= 0xDC00 && lo <= 0xDFFF) {
              cp = 0x10000 + ((cp - 0xD800) << 10) + (lo - 0xDC00);
            } else {
              p_ = after;
              cp = 0xFFFD;
            }
          } else if (cp >= 0xDC00 && cp <= 0xDFFF) {
            cp = 0xFFFD;
          }
          put_utf8(out, cp);
          break;
        }
        default: fail("bad escape");
      }
      run = p_;
    }
    fail("unterminated string");
  }

  // RFC 8259 section 6: -? (0 | [1-9][0-9]*) (. [0-9]+)? ([eE] [+-]? [0-9]+)?
  // Without fraction and exponent, and within int64, the value is an Int; any
  // other number is the nearest double, and one that overflows is refused.
  Json number() {
    const char* start = p_;
    auto digit = [&] { return p_ < end_ && *p_ >= '0' && *p_ <= '9'; };
    bool neg = false;
    if (p_ < end_ && *p_ == '-') { neg = true; ++p_; }
    if (!digit()) fail(p_ == start ? "unexpected character" : "bad number");
    uint64_t mag = 0;
    bool fits = true;  // mag holds the digits so far
    if (*p_ == '0') {
      ++p_;
    } else {
      while (digit()) {
        unsigned d = static_cast<unsigned>(*p_++ - '0');
        if (mag > (UINT64_MAX - d) / 10) fits = false;
        else mag = mag * 10 + d;
      }
    }
    bool is_float = false;
    if (p_ < end_ && *p_ == '.') {
      is_float = true;
      ++p_;
      if (!digit()) fail("bad number");
      while (digit()) ++p_;
    }
    if (p_ < end_ && (*p_ == 'e' || *p_ == 'E')) {
      is_float = true;
      ++p_;
      if (p_ < end_ && (*p_ == '+' || *p_ == '-')) ++p_;
      if (!digit()) fail("bad number");
      while (digit()) ++p_;
    }
    if (!is_float && fits) {
      constexpr uint64_t kMax = static_cast<uint64_t>(std::numeric_limits<int64_t>::max());
      if (!neg && mag <= kMax) return Json(static_cast<int64_t>(mag));
      if (neg && mag <= kMax + 1) return Json(static_cast<int64_t>(0 - mag));
    }
    double d = 0.0;
    auto r = std::from_chars(start, p_, d);
    if (r.ec == std::errc::result_out_of_range) {
      // Too large, or too small to tell from zero: strtod tells which.
      d = std::strtod(std::string(start, p_).c_str(), nullptr);
    } else if (r.ec != std::errc() || r.ptr != p_) {
      fail("bad number");
    }
    if (!std::isfinite(d)) fail("number out of range");
    return Json(d);
  }
};

void dump_string(std::string& out, const std::string& s) {
  out.push_back('"');
  for (unsigned char c : s) {
    switch (c) {
      case '"': out += "\\\""; break;
      case '\\': out += "\\\\"; break;
      case '\n': out += "\\n"; break;
      case '\r': out += "\\r"; break;
      case '\t': out += "\\t"; break;
      case '\b': out += "\\b"; break;
      case '\f': out += "\\f"; break;
      default:
        if (c < 0x20) {
          char buf[8];
          std::snprintf(buf, sizeof buf, "\\u%04x", c);
          out += buf;
        } else {
          out.push_back(static_cast<char>(c));
        }
    }
  }
  out.push_back('"');
}
}  // namespace

const std::string& Json::as_string() const { return t_ == Type::String ? h_.s : kEmptyString; }
const Json::Array& Json::items() const { return t_ == Type::Array ? h_.a : kEmptyArray; }
Json::Array& Json::items_mut() {
  if (t_ != Type::Array) { *this = array(); }
  return h_.a;
}
const Json::Object& Json::members() const { return t_ == Type::Object ? h_.o : kEmptyObject; }
Json::Object& Json::members_mut() {
  if (t_ != Type::Object) { *this = object(); }
  return h_.o;
}

const Json* Json::get(std::string_view key) const {
  if (t_ != Type::Object) return nullptr;
  for (const auto& kv : h_.o)
    if (kv.first == key) return &kv.second;
  return nullptr;
}

Json* Json::get_mut(std::string_view key) {
  if (t_ != Type::Object) return nullptr;
  for (auto& kv : h_.o)
    if (kv.first == key) return &kv.second;
  return nullptr;
}

const Json* Json::path(std::initializer_list<std::string_view> keys) const {
  const Json* cur = this;
  for (auto k : keys) {
    cur = cur->get(k);
    if (!cur) return nullptr;
  }
  return cur;
}

const Json& Json::operator[](std::string_view key) const {
  const Json* v = get(key);
  return v ? *v : json_null();
}

Json& Json::set(std::string_view key, Json v) {
  auto& m = members_mut();
  for (auto& kv : m) {
    if (kv.first == key) {
      kv.second = std::move(v);
      return kv.second;
    }
  }
  m.emplace_back(std::string(key), std::move(v));
  return m.back().second;
}

Json& Json::at_or_create(std::string_view key) {
  auto& m = members_mut();
  for (auto& kv : m)
    if (kv.first == key) {
      if (!kv.second.is_object()) kv.second = object();
      return kv.second;
    }
  m.emplace_back(std::string(key), object());
  return m.back().second;
}

bool Json::erase(std::string_view key) {
  if (t_ != Type::Object) return false;
  for (auto it = h_.o.begin(); it != h_.o.end(); ++it) {
    if (it->first == key) {
      h_.o.erase(it);
      return true;
    }
  }
  return false;
}

void Json::push_back(Json v) { items_mut().push_back(std::move(v)); }

namespace {
// True, with the value, for a double that is integral and within int64.
inline bool double_is_int64(double d, int64_t* out) {
  if (!(d >= -9223372036854775808.0 && d < 9223372036854775808.0) || d != std::trunc(d)) return false;
  *out = static_cast<int64_t>(d);
  return true;
}
}  // namespace

bool Json::operator==(const Json& o) const {
  if (is_number() && o.is_number()) {
    if (t_ == o.t_) return t_ == Type::Int ? i_ == o.i_ : d_ == o.d_;
    // Int against Double, exactly: through double, 2^53 + 1 equals 2^53.
    int64_t as_i;
    return t_ == Type::Int ? double_is_int64(o.d_, &as_i) && as_i == i_ : double_is_int64(d_, &as_i) && as_i == o.i_;
  }
  if (t_ != o.t_) return false;
  switch (t_) {
    case Type::Null: return true;
    case Type::Bool: return i_ == o.i_;
    case Type::String: return h_.s == o.h_.s;
    case Type::Array: return h_.a == o.h_.a;
    case Type::Object: {
      if (h_.o.size() != o.h_.o.size()) return false;
      for (const auto& kv : h_.o) {
        const Json* other = o.get(kv.first);
        if (!other || !(*other == kv.second)) return false;
      }
      return true;
    }
    default: return false;
  }
}

void Json::dump_to(std::string& out) const {
  switch (t_) {
    case Type::Null: out += "null"; break;
    case Type::Bool: out += i_ ? "true" : "false"; break;
    case Type::Int: out += std::to_string(i_); break;
    case Type::Double: {
      if (!std::isfinite(d_)) { out += "null"; break; }
      char buf[32];
      std::snprintf(buf, sizeof buf, "%.17g", d_);
      out += buf;
      break;
    }
    case Type::String: dump_string(out, h_.s); break;
    case Type::Array: {
      out.push_back('[');
      bool first = true;
      for (const auto& v : h_.a) {
        if (!first) out.push_back(',');
        first = false;
        v.dump_to(out);
      }
      out.push_back(']');
      break;
    }
    case Type::Object: {
      out.push_back('{');
      bool first = true;
      for (const auto& kv : h_.o) {
        if (!first) out.push_back(',');
        first = false;
        dump_string(out, kv.first);
        out.push_back(':');
        kv.second.dump_to(out);
      }
      out.push_back('}');
      break;
    }
  }
}

std::string Json::dump() const {
  std::string out;
  out.reserve(256);
  dump_to(out);
  return out;
}

Json Json::parse(std::string_view text) { return Parser(text).parse_document(); }

void Json::parse_array_stream(std::string_view text, const std::function<void(Json&&)>& fn) {
  Parser(text).parse_array_stream(fn);
}

void Json::merge_patch(const Json& patch) {
  if (!patch.is_object()) {
    *this = patch;
    return;
  }
  if (!is_object()) *this = object();
  for (const auto& kv : patch.h_.o) {
    if (kv.second.is_null()) {
      erase(kv.first);
    } else if (kv.second.is_object()) {
      Json* cur = get_mut(kv.first);
      if (cur && cur->is_object()) {
        cur->merge_patch(kv.second);
      } else {
        Json fresh = object();
        fresh.merge_patch(kv.second);
        set(kv.first, std::move(fresh));
      }
    } else {
      set(kv.first, kv.second);
    }
  }
}

Json Json::diff_merge_patch(const Json& from, const Json& to) {
  if (!from.is_object() || !to.is_object()) return to;
  Json patch = object();
  for (const auto& kv : from.h_.o) {
    if (!to.get(kv.first)) patch.set(kv.first, Json());
  }
  for (const auto& kv : to.h_.o) {
    const Json* old = from.get(kv.first);
    if (!old) {
      patch.set(kv.first, kv.second);
    } else if (!(*old == kv.second)) {
      if (old->is_object() && kv.second.is_object())
        patch.set(kv.first, diff_merge_patch(*old, kv.second));
      else
        patch.set(kv.first, kv.second);
    }
  }
  return patch;
}

namespace {
// Word-at-a-time mixing (a multiply-xorshift per 8 bytes, the length mixed in
// first so "ab"+"c" and "a"+"bc" differ). The byte-at-a-time FNV it replaces
// was 6% of the informer thread at 1,024 nodes (template and spec hashes of
// every parsed pod).
inline uint64_t mix(uint64_t h, uint64_t v) {
  h ^= v;
  h *= 0xff51afd7ed558ccdULL;
  return h ^ (h >> 33);
}
inline uint64_t fnv(uint64_t h, const void* data, size_t n) {
  const unsigned char* p = static_cast<const unsigned char*>(data);
  h = mix(h, n);
  for (; n >= 8; n -= 8, p += 8) {
    uint64_t w;
    std::memcpy(&w, p, 8);
    h = mix(h, w);
  }
  if (n) {
    uint64_t w = 0;
    std::memcpy(&w, p, n);
    h = mix(h, w);
  }
  return h;
}
}  // namespace

uint64_t json_hash(const Json& j, uint64_t h, std::string_view skip_key) {
  // Equal values hash equal: a Double that `==` an Int (1.0, which dump()
  // writes as "1" and parse() reads back as an Int) hashes as that Int.
  int64_t as_i;
  if (j.type() == Json::Type::Double && double_is_int64(j.as_double(), &as_i)) return json_hash(Json(as_i), h);
  uint8_t tag = static_cast<uint8_t>(j.type());
  h = fnv(h, &tag, 1);
  switch (j.type()) {
    case Json::Type::Null:
      break;
    case Json::Type::Bool: {
      uint8_t b = j.as_bool() ? 1 : 0;
      h = fnv(h, &b, 1);
      break;
    }
    case Json::Type::Int: {
      int64_t v = j.as_int();
      h = fnv(h, &v, sizeof v);
      break;
    }
    case Json::Type::Double: {
      double v = j.as_double();
      h = fnv(h, &v, sizeof v);
      break;
    }
    case Json::Type::String:
      h = fnv(h, j.as_string().data(), j.as_string().size());
      break;
    case Json::Type::Array:
      for (const auto& x : j.items()) h = json_hash(x, h);
      break;
    case Json::Type::Object:
      for (const auto& [k, v] : j.members()) {
        if (!skip_key.empty() && k == skip_key) continue;
        h = fnv(h, k.data(), k.size());  // length-prefixed: "ab"+"c" != "a"+"bc"
        h = json_hash(v, h);
      }
      break;
  }
  return h;
}

}  // namespace xsched
