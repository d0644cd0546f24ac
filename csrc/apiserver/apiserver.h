// Native HTTP API server over the ObjectStore (the envtest / kube-apiserver
// analog for service mode).
//
// The reference runs against a real kube-apiserver (Go) and its integration
// tier boots one through envtest (test/integration/main_test.go:31-49). Our
// first server (control/apiserver.py) is Python's http.server: every request
// pays the interpreter, so a scheduler in another process could bind only
// ~6k pods/s through it (profiles/r2s_remote_bench.jsonl). This one serves
// the same REST surface natively:
//
//   GET    <collection>[?labelSelector=&fieldSelector=&watch=1&resourceVersion=N
//                        &timeoutSeconds=&allowWatchBookmarks=1]
//   POST   <collection>                       create
//   POST   /api/v1/namespaces/<ns>/pods/<name>/binding (annotations copied)
//   GET    <collection>/<name>
//   PUT    <collection>/<name>[/status]       update (resourceVersion precondition)
//   PATCH  <collection>/<name>[/status]       merge / strategic-merge / json-patch
//   DELETE <collection>[/<name>]              DeleteOptions / collection delete
//   GET    /healthz /readyz /livez /version /api /apis
//
// One thread per connection (a scheduler keeps a pool of keep-alive
// connections plus one watch per kind; connections are few and long-lived),
// TCP_NODELAY, responses written in one send. Watches stream chunked JSON
// lines exactly like kube-apiserver (ERROR + 410 Status when the version is
// compacted, BOOKMARKs on request). Bearer-token auth; HTTPS and mutual TLS
// through OpenSSL (the handshake runs on the connection's own thread).
#pragma once

#include <atomic>
#include <condition_variable>
#include <cstdint>
#include <memory>
#include <mutex>
#include <set>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "common/json.h"
#include "store/store.h"

typedef struct ssl_ctx_st SSL_CTX;

namespace xsched::rest {
class Wire;  // one HTTP/1.1 connection (rest/wire.h)
}

namespace xsched::apiserver {

struct Options {
  std::string host = "127.0.0.1";
  int port = 0;               // 0: pick a free port
  std::string token;          // bearer token ("" = no auth)
  int bookmark_interval_ms = 10'000;
  int max_connections = 4096;
  // HTTPS (kube-apiserver --tls-cert-file / --tls-private-key-file) and,
  // with a client CA, mutual TLS (--client-ca-file). PEM files.
  std::string tls_cert_file, tls_key_file, client_ca_file;
};

// Label / field selector requirement (the string syntax of k8s.io/apimachinery
// labels and fields; tests/selector_ref.py writes the grammar out).
struct Requirement {
  enum Op { Eq, Ne, In, NotIn, Exists, NotExists, Gt, Lt } op = Eq;
  std::string key;
  std::vector<std::string> values;  // sorted, each once
};
// Both throw std::invalid_argument on a malformed selector.
// a=b, a==b, a!=b, a>1, a<1, a in (x,y), a notin (x), a, !a; keys and values validated.
std::vector<Requirement> parse_selector(std::string_view s);
// path=value, path==value, path!=value; nothing trimmed; \\ \, \= in a value.
std::vector<Requirement> parse_field_selector(std::string_view s);
bool labels_match(const std::vector<Requirement>& reqs, const Json& obj);
bool fields_match(const std::vector<Requirement>& reqs, const Json& obj);  // = / != on dotted paths
// RFC 6902 JSON patch, all or nothing (tests/json_patch_ref.py); a bad op
// throws the 422 "Invalid" ApiError (apiserver/api_error.h).
Json apply_json_patch(const Json& doc, const Json& ops);

class Server {
 public:
  Server(std::shared_ptr<ObjectStore> store, Options o);
  ~Server();
  Server(const Server&) = delete;
  Server& operator=(const Server&) = delete;

  void start();  // binds and starts accepting (throws on bind failure)
  void stop();   // closes the listener, ends every watch and connection, joins
  int port() const { return port_; }
  const std::string& host() const { return opts_.host; }
  uint64_t requests() const { return requests_.load(std::memory_order_relaxed); }
  size_t connections() const;

  struct Request;
  struct Reply;

 private:
  void accept_loop();
  void serve(int fd);
  // Handles one request; false when the connection must close.
  bool handle(rest::Wire& c, Request& r);
  // Fills in the reply to `r`; false when a watch has streamed its own.
  bool answer(rest::Wire& c, Request& r, Reply& out);
  void watch(rest::Wire& c, const std::string& kind, const std::string& ns, Request& r);

  std::shared_ptr<ObjectStore> store_;
  Options opts_;
  SSL_CTX* tls_ctx_ = nullptr;  // when serving HTTPS
  int listen_fd_ = -1;
  int port_ = 0;
  std::thread acceptor_;
  std::atomic<bool> stopping_{false};
  std::atomic<uint64_t> requests_{0};
  mutable std::mutex mu_;
  std::condition_variable idle_cv_;
  std::set<int> conns_;                 // open connection fds
  std::set<WatcherPtr> watchers_;       // active watches (stopped on shutdown)
  size_t live_threads_ = 0;
};

}  // namespace xsched::apiserver
