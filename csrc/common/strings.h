// Small string helpers shared across the native core.
#pragma once

#include <cctype>
#include <string_view>

namespace xsched {

// `s` without the white space (isspace) at either end.
inline std::string_view trim(std::string_view s) {
  while (!s.empty() && std::isspace(static_cast<unsigned char>(s.front()))) s.remove_prefix(1);
  while (!s.empty() && std::isspace(static_cast<unsigned char>(s.back()))) s.remove_suffix(1);
  return s;
}

}  // namespace xsched
