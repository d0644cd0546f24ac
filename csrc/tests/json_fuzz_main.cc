// Sanitizer driver for the text-facing half of the core: built with
// -fsanitize=address,undefined (float-cast-overflow included, nothing
// recoverable) by build_ext.build_json_fuzz and run by
// tests/test_json_conformance.py on its whole corpus.
//
//   json_fuzz <corpus>     records of <u32 little-endian length><document>
//
// Each document goes through parse -> dump -> parse -> json_hash ->
// Pod::from_json -> request()/limit_sum(), and arrays through
// parse_array_stream as well. A std::exception is an answer (a refused
// document, a bad quantity); anything a sanitizer finds ends the process.
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

#include "api/types.h"
#include "common/json.h"

using namespace xsched;

namespace {
uint64_t g_sink = 0;  // keeps every result alive

void decode_pod(const Json& doc) {
  try {
    auto pod = Pod::from_json(doc);
    g_sink += static_cast<uint64_t>(pod->request().get(kCPU)) + static_cast<uint64_t>(pod->limit_sum().get(kMemory)) +
              static_cast<uint64_t>(pod->nonzero_request().get(kCPU)) + pod->spec_hash + pod->template_hash +
              static_cast<uint64_t>(pod->priority) + pod->host_ports.size() + pod->gpu.gpus.size() +
              pod->gpu.partitions.size() + static_cast<uint64_t>(pod->meta.resource_version);
    for (const auto& t : pod->tolerations) g_sink += static_cast<uint64_t>(t.toleration_seconds);
    for (const auto& c : pod->spread_constraints) g_sink += static_cast<uint64_t>(c.max_skew);
    for (const auto& t : pod->preferred_node_terms) g_sink += static_cast<uint64_t>(t.weight);
    for (const auto& t : pod->pod_affinity_preferred) g_sink += static_cast<uint64_t>(t.weight);
  } catch (const std::exception&) {
  }
}

bool run(std::string_view text) {
  Json doc;
  try {
    doc = Json::parse(text);
  } catch (const JsonError&) {
    try {  // the stream must refuse it too, not crash on it
      Json::parse_array_stream(text, [](Json&& j) { g_sink += j.size(); });
    } catch (const JsonError&) {
    }
    return false;
  }
  const std::string out = doc.dump();
  g_sink += out.size();
  Json again = Json::parse(out);  // a throw here is a finding: main reports it
  if (!(again == doc)) throw std::runtime_error("dump() did not read back equal: " + out.substr(0, 200));
  if (json_hash(again) != json_hash(doc)) throw std::runtime_error("hash changed across dump(): " + out.substr(0, 200));
  if (doc.is_array()) {
    size_t n = 0;
    Json::parse_array_stream(text, [&](Json&& j) {
      if (!(j == doc.items()[n++])) throw std::runtime_error("stream element differs");
    });
    if (n != doc.size()) throw std::runtime_error("stream element count differs");
  }
  g_sink += static_cast<uint64_t>(doc.as_int());
  decode_pod(doc);
  Json patched = doc;
  patched.merge_patch(Json::diff_merge_patch(again, doc));
  return true;
}
}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: %s <corpus>\n", argv[0]);
    return 2;
  }
  std::ifstream in(argv[1], std::ios::binary);
  std::string data((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
  size_t at = 0, docs = 0, accepted = 0;
  while (at + 4 <= data.size()) {
    uint32_t n = 0;
    for (int k = 0; k < 4; ++k) n |= static_cast<uint32_t>(static_cast<unsigned char>(data[at + k])) << (8 * k);
    at += 4;
    if (n > data.size() - at) {
      std::fprintf(stderr, "truncated record at byte %zu\n", at);
      return 2;
    }
    // An exact-size heap copy, so that one byte read past a document is seen.
    std::unique_ptr<char[]> copy(new char[n]);
    std::memcpy(copy.get(), data.data() + at, n);
    std::string_view text(copy.get(), n);
    at += n;
    ++docs;
    try {
      accepted += run(text);
    } catch (const std::exception& e) {
      std::fprintf(stderr, "document %zu: %s\n", docs, e.what());
      return 1;
    }
  }
  std::printf("%zu documents, %zu accepted (%llx)\n", docs, accepted, static_cast<unsigned long long>(g_sink));
  return at == data.size() ? 0 : 2;
}
