// Sanitizer driver for what sits between the wire and the store: built with
// -fsanitize=address,undefined (nothing recoverable) by
// build_ext.build_patch_fuzz and run by tests/test_json_patch_conformance.py
// on the tables and generated cases of both conformance tests.
//
//   patch_selector <corpus>   records of <kind byte><u32 little-endian length><payload>
//     P  {"doc": ..., "patch": ...}   apply_json_patch(doc, patch)
//     O  an object                    kept, for the selectors that follow
//     L  a label selector             parsed, then matched against every object
//     F  a field selector             the same
//
// A refusal (the 422 ApiError, std::invalid_argument) is an answer; anything
// a sanitizer finds ends the process.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <exception>
#include <fstream>
#include <iterator>
#include <memory>
#include <stdexcept>
#include <string>
#include <string_view>
#include <vector>

#include "apiserver/api_error.h"
#include "apiserver/apiserver.h"
#include "common/json.h"

using namespace xsched;

namespace {
uint64_t g_sink = 0;  // keeps every result alive
std::vector<Json> g_objects;

bool run_patch(std::string_view text) {
  Json both = Json::parse(text);
  const Json before = both["doc"];
  try {
    Json after = apiserver::apply_json_patch(both["doc"], both["patch"]);
    g_sink += after.dump().size();
  } catch (const apiserver::ApiError& e) {
    g_sink += static_cast<uint64_t>(e.code);
    if (both["doc"] != before) throw std::runtime_error("a refused patch changed its document");
    return false;
  }
  if (both["doc"] != before) throw std::runtime_error("apply_json_patch changed its argument");
  return true;
}

bool run_selector(std::string_view text, bool labels) {
  try {
    auto reqs = labels ? apiserver::parse_selector(text) : apiserver::parse_field_selector(text);
    for (const auto& r : reqs) g_sink += r.key.size() + r.values.size();
    for (const Json& o : g_objects)
      g_sink += labels ? apiserver::labels_match(reqs, o) : apiserver::fields_match(reqs, o);
  } catch (const std::invalid_argument&) {
    return false;
  }
  return true;
}
}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: %s <corpus>\n", argv[0]);
    return 2;
  }
  std::ifstream in(argv[1], std::ios::binary);
  if (!in) {
    std::fprintf(stderr, "cannot read %s\n", argv[1]);
    return 2;
  }
  std::string data((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
  size_t at = 0, records = 0, accepted = 0;
  while (at + 5 <= data.size()) {
    char kind = data[at];
    uint32_t n = 0;
    for (int k = 0; k < 4; ++k) n |= static_cast<uint32_t>(static_cast<unsigned char>(data[at + 1 + k])) << (8 * k);
    at += 5;
    if (n > data.size() - at) {
      std::fprintf(stderr, "truncated record at byte %zu\n", at);
      return 2;
    }
    // An exact-size heap copy, so that one byte read past a record is seen.
    std::unique_ptr<char[]> copy(new char[n]);
    std::memcpy(copy.get(), data.data() + at, n);
    std::string_view text(copy.get(), n);
    at += n;
    ++records;
    try {
      switch (kind) {
        case 'P': accepted += run_patch(text); break;
        case 'O': g_objects.push_back(Json::parse(text)); break;
        case 'L': accepted += run_selector(text, true); break;
        case 'F': accepted += run_selector(text, false); break;
        default: throw std::runtime_error("unknown record kind");
      }
    } catch (const std::exception& e) {
      std::fprintf(stderr, "record %zu: %s\n", records, e.what());
      return 1;
    }
  }
  std::printf("%zu records, %zu accepted (%llx)\n", records, accepted, static_cast<unsigned long long>(g_sink));
  return at == data.size() ? 0 : 2;
}
