// Small string helpers shared across the native core.
#pragma once

#include <cctype>
#include <charconv>
#include <string>
#include <string_view>
#include <utility>
#include <vector>

namespace xsched {

// `s` without the white space (isspace) at either end.
inline std::string_view trim(std::string_view s) {
  while (!s.empty() && std::isspace(static_cast<unsigned char>(s.front()))) s.remove_prefix(1);
  while (!s.empty() && std::isspace(static_cast<unsigned char>(s.back()))) s.remove_suffix(1);
  return s;
}

// Appends `v` in decimal (what "%d" prints), without the printf machinery.
inline void append_int(std::string& s, int v) {
  char buf[12];  // "-2147483648"
  auto r = std::to_chars(buf, buf + sizeof buf, v);
  s.append(buf, static_cast<size_t>(r.ptr - buf));
}

// "0,3" and "2:4,2:5": both write into `s`, cleared first, its buffer kept.
inline void join_ints(const std::vector<int>& v, std::string& s) {
  s.clear();
  for (size_t i = 0; i < v.size(); ++i) {
    if (i) s += ',';
    append_int(s, v[i]);
  }
}

inline void join_parts(const std::vector<std::pair<int, int>>& v, std::string& s) {
  s.clear();
  for (size_t i = 0; i < v.size(); ++i) {
    if (i) s += ',';
    append_int(s, v[i].first);
    s += ':';
    append_int(s, v[i].second);
  }
}

}  // namespace xsched
