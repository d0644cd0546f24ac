#include "apiserver/apiserver.h"

#include <arpa/inet.h>
#include <netdb.h>
#include <netinet/in.h>
#include <netinet/tcp.h>
#include <poll.h>
#include <sys/socket.h>
#include <openssl/err.h>
#include <openssl/ssl.h>
#include <unistd.h>

#include <cerrno>
#include <chrono>
#include <cstring>
#include <map>
#include <set>
#include <stdexcept>

#include "apiserver/api_error.h"
#include "common/strings.h"
#include "rest/kube.h"
#include "rest/wire.h"

namespace xsched::apiserver {

using rest::Framing;
using rest::Wire;

struct Server::Request {
  std::string method, path;
  std::unordered_map<std::string, std::string> query;
  std::string content_type, authorization, body;
  bool keep_alive = true;
  std::string q(const char* k) const {
    auto it = query.find(k);
    return it == query.end() ? std::string() : it->second;
  }
  bool flag(const char* k) const {
    std::string v = q(k);
    return v == "true" || v == "1";
  }
};

struct Server::Reply {
  int code = 200;
  std::string body;
  std::string_view ctype = "application/json";
};

namespace {

using Request = Server::Request;
using Reply = Server::Reply;

constexpr size_t kMaxBody = 256u << 20;
constexpr size_t kMaxHeaders = 200;

const char* phrase(int code) {
  switch (code) {
    case 200: return "OK";
    case 201: return "Created";
    case 400: return "Bad Request";
    case 401: return "Unauthorized";
    case 403: return "Forbidden";
    case 404: return "Not Found";
    case 405: return "Method Not Allowed";
    case 409: return "Conflict";
    case 410: return "Gone";
    case 413: return "Payload Too Large";
    case 415: return "Unsupported Media Type";
    case 422: return "Unprocessable Entity";
    case 429: return "Too Many Requests";
    case 431: return "Request Header Fields Too Large";
    case 500: return "Internal Server Error";
    case 503: return "Service Unavailable";
    default: return code < 400 ? "OK" : "Error";
  }
}

// ------------------------------------------------------ reading a request --
std::string pct_decode(std::string_view s, bool plus_space) {
  std::string out;
  out.reserve(s.size());
  for (size_t i = 0; i < s.size(); ++i) {
    char c = s[i];
    if (c == '%' && i + 2 < s.size()) {
      int hi = rest::hexval(s[i + 1]), lo = rest::hexval(s[i + 2]);
      if (hi >= 0 && lo >= 0) {
        out.push_back(static_cast<char>(hi * 16 + lo));
        i += 2;
        continue;
      }
    }
    out.push_back(plus_space && c == '+' ? ' ' : c);
  }
  return out;
}

// "/path?k=v&..." -> r.path and r.query, percent-decoded.
void parse_target(std::string_view target, Request& r) {
  size_t qm = target.find('?');
  r.path = pct_decode(target.substr(0, qm), false);
  if (qm == std::string_view::npos) return;
  std::string_view qs = target.substr(qm + 1);
  size_t i = 0;
  while (i <= qs.size()) {
    size_t j = qs.find('&', i);
    if (j == std::string_view::npos) j = qs.size();
    std::string_view kv = qs.substr(i, j - i);
    if (!kv.empty()) {
      size_t eq = kv.find('=');
      r.query[pct_decode(kv.substr(0, eq), true)] = eq == std::string_view::npos ? "" : pct_decode(kv.substr(eq + 1), true);
    }
    i = j + 1;
  }
}

bool open_path(const std::string& path) {
  return path == "/healthz" || path == "/readyz" || path == "/livez" || path == "/version";
}

// The body the framing announces; the result reads as read_request's.
int read_body(Wire& c, const Framing& f, std::string& body) {
  if (f.chunked) {
    switch (c.chunked_body(body, kMaxBody)) {
      case Wire::Body::kOk: return 0;
      case Wire::Body::kMalformed: return 400;
      case Wire::Body::kTooLarge: return 413;
      case Wire::Body::kClosed: break;
    }
    return -1;
  }
  if (f.content_length > 0) {
    if (static_cast<size_t>(f.content_length) > kMaxBody) return 413;
    if (!c.exact(static_cast<size_t>(f.content_length), body)) return -1;
  }
  return 0;
}

// 0: ok, -1: connection closed, >0: HTTP error to send before closing. With
// a bearer `token`, a request without it is refused (401) before its body is
// read: an unauthenticated client cannot make the server buffer 256 MiB.
int read_request(Wire& c, Request& r, const std::string& token) {
  r.query.clear();
  r.content_type.clear();
  r.authorization.clear();
  std::string line;
  do {
    if (!c.line(line)) return -1;
  } while (line.empty());  // tolerate stray CRLFs between requests
  size_t a = line.find(' '), b = line.rfind(' ');
  if (a == std::string::npos || b == a) return 400;
  r.method = line.substr(0, a);
  r.keep_alive = line.compare(b + 1, std::string::npos, "HTTP/1.0") != 0;
  Framing f;
  Wire::Head h = c.headers(f, /*trim_name=*/true, kMaxHeaders, [&r](std::string_view name, std::string_view value) {
    if (name == "content-type") r.content_type = value;
    else if (name == "authorization") r.authorization = value;
  });
  if (h != Wire::Head::kOk) return h == Wire::Head::kTooMany ? 431 : -1;
  if (f.keep_alive) r.keep_alive = true;
  else if (f.close) r.keep_alive = false;
  parse_target(std::string_view(line).substr(a + 1, b - a - 1), r);
  r.body.clear();
  if (!token.empty() && !open_path(r.path) && r.authorization != "Bearer " + token) return 401;
  return read_body(c, f, r.body);
}

// ------------------------------------------------------------- answering --
Reply json_reply(int code, const Json& j) {
  Reply r{code};
  j.dump_to(r.body);
  return r;
}

Reply status_reply(int code, const std::string& reason, const std::string& message) {
  return json_reply(code, status_obj(code, reason, message));
}

// A 2xx Status ("status": "Success").
Reply success_reply(int code, const std::string& message) {
  Json ok = status_obj(code, "", message);
  ok.set("status", Json("Success"));
  return json_reply(code, ok);
}

bool respond(Wire& c, const Reply& r, bool keep_alive) {
  std::string out;
  out.reserve(r.body.size() + 160);
  out += "HTTP/1.1 ";
  out += std::to_string(r.code);
  out += ' ';
  out += phrase(r.code);
  out += "\r\nContent-Type: ";
  out += r.ctype;
  out += "\r\nContent-Length: ";
  out += std::to_string(r.body.size());
  if (!keep_alive) out += "\r\nConnection: close";
  out += "\r\n\r\n";
  out += r.body;
  return c.send_all(out);
}

bool write_chunk(Wire& c, std::string_view data) {
  char head[24];
  int n = std::snprintf(head, sizeof head, "%zx\r\n", data.size());
  std::string out;
  out.reserve(data.size() + 32);
  out.append(head, static_cast<size_t>(n));
  out += data;
  out += "\r\n";
  return c.send_all(out);
}

Json parse_body(const std::string& body) {
  if (body.empty()) return Json();
  try {
    return Json::parse(body);
  } catch (const JsonError& e) {
    throw ApiError(400, "BadRequest", std::string("invalid JSON body: ") + e.what());
  }
}

Json parse_object_body(const std::string& body) {
  Json j = parse_body(body);
  if (!j.is_object()) throw ApiError(400, "BadRequest", "request body must be a JSON object");
  return j;
}

void type_meta(Json& obj, const rest::ResourcePath& rp) {
  if (!obj.get("apiVersion")) obj.set("apiVersion", Json(rp.api_version));
  if (!obj.get("kind")) obj.set("kind", Json(rp.kind));
}

// The two selectors of a list or watch request.
struct Selectors {
  std::vector<Requirement> labels, fields;
  bool match(const Json& o) const {
    return (labels.empty() || labels_match(labels, o)) && (fields.empty() || fields_match(fields, o));
  }
};

// Throws std::invalid_argument for a malformed selector.
Selectors parse_selectors(const Request& r) {
  return {parse_selector(r.q("labelSelector")), parse_field_selector(r.q("fieldSelector"))};
}

// ---------------------------------------------------------------- routes --
// "<prefix>/<plural>" -> store kind, from the REST client's table (rest/kube.cc).
const std::unordered_map<std::string, std::string>& routes() {
  static const auto* m = [] {
    auto* r = new std::unordered_map<std::string, std::string>();
    for (const auto& [kind, rp] : rest::resource_table()) (*r)[rp.prefix + "/" + kind] = kind;
    return r;
  }();
  return *m;
}

struct Route {
  const std::string* kind = nullptr;  // store kind (the plural)
  const rest::ResourcePath* rp = nullptr;
  std::string ns, name, sub;  // "" where the path has none
};

// /api/<v>/[namespaces/<ns>/]<plural>[/<name>[/<sub>]], or the same under
// /apis/<g>/<v>/; anything else is the 404.
Route parse_route(const std::string& path) {
  std::vector<std::string> parts;
  for (size_t i = 0; i < path.size();) {
    size_t j = path.find('/', i);
    if (j == std::string::npos) j = path.size();
    if (j > i) parts.push_back(path.substr(i, j - i));
    i = j + 1;
  }
  std::string prefix;
  size_t rest = 0;
  if (parts.size() >= 2 && parts[0] == "api") {
    prefix = "/api/" + parts[1];
    rest = 2;
  } else if (parts.size() >= 3 && parts[0] == "apis") {
    prefix = "/apis/" + parts[1] + "/" + parts[2];
    rest = 3;
  } else {
    throw ApiError(404, "NotFound", "the server could not find the requested resource (" + path + ")");
  }
  Route rt;
  if (parts.size() - rest > 2 && parts[rest] == "namespaces") {
    rt.ns = std::move(parts[rest + 1]);
    rest += 2;
  }
  auto rit = rest < parts.size() ? routes().find(prefix + "/" + parts[rest]) : routes().end();
  if (rit == routes().end())
    throw ApiError(404, "NotFound", "the server could not find the requested resource (" + path + ")");
  rt.kind = &rit->second;
  rt.rp = &rest::resource_path(rit->second);
  if (parts.size() > rest + 1) rt.name = std::move(parts[rest + 1]);
  if (parts.size() > rest + 2) rt.sub = std::move(parts[rest + 2]);
  return rt;
}

// ----------------------------------------------------------------- verbs --
Reply api_groups() {
  std::map<std::string, std::set<std::string>> groups;
  for (const auto& [kind, rp] : rest::resource_table()) {
    size_t s = rp.api_version.find('/');
    if (s != std::string::npos) groups[rp.api_version.substr(0, s)].insert(rp.api_version.substr(s + 1));
  }
  Json list = Json::array();
  for (const auto& [g, vs] : groups) {
    Json gj = Json::object();
    gj.set("name", Json(g));
    Json versions = Json::array();
    for (const auto& v : vs) {
      Json vj = Json::object();
      vj.set("groupVersion", Json(g + "/" + v));
      vj.set("version", Json(v));
      versions.push_back(std::move(vj));
    }
    gj.set("versions", std::move(versions));
    list.push_back(std::move(gj));
  }
  Json out = Json::object();
  out.set("kind", Json("APIGroupList"));
  out.set("apiVersion", Json("v1"));
  out.set("groups", std::move(list));
  return json_reply(200, out);
}

Reply get_one(ObjectStore& store, const Route& rt) {
  JsonPtr obj = store.get(*rt.kind, rt.ns, rt.name);
  if (!obj) throw ApiError(404, "NotFound", *rt.kind + " \"" + rt.name + "\" not found");
  return json_reply(200, *obj);
}

Reply list_many(ObjectStore& store, const Route& rt, const Request& r) {
  Selectors sel;
  try {
    sel = parse_selectors(r);
  } catch (const std::invalid_argument& e) {
    throw ApiError(400, "BadRequest", e.what());
  }
  int64_t rv = 0;
  auto items = store.list(*rt.kind, rt.ns, &rv);
  Reply out;
  out.body.reserve(items.size() * 512 + 128);
  out.body += R"({"kind":")" + rt.rp->kind + R"(List","apiVersion":")" + rt.rp->api_version +
              R"(","metadata":{"resourceVersion":")" + std::to_string(rv) + R"("},"items":[)";
  bool first = true;
  for (const auto& it : items) {
    if (!sel.match(*it)) continue;
    if (!first) out.body += ',';
    first = false;
    it->dump_to(out.body);
  }
  out.body += "]}";
  return out;
}

Reply bind_pod(ObjectStore& store, const Route& rt, const Json& body) {
  std::string target = body["target"]["name"].as_string();
  if (target.empty()) throw ApiError(422, "Invalid", "Binding.target.name: Required value");
  const Json& md = body["metadata"];
  const Json& ann = md["annotations"];
  store.bind(rt.ns.empty() ? "default" : rt.ns, rt.name, md["uid"].as_string(), target,
             ann.is_object() ? ann : Json::object());
  return success_reply(201, "");
}

Reply create(ObjectStore& store, const Route& rt, const Request& r) {
  Json body = parse_object_body(r.body);
  if (*rt.kind == "pods" && !rt.name.empty() && rt.sub == "binding") return bind_pod(store, rt, body);
  if (!rt.name.empty()) throw ApiError(405, "MethodNotAllowed", "POST to a named resource");
  if (rt.rp->namespaced) {
    Json& md = body.at_or_create("metadata");
    if (!rt.ns.empty()) {
      const Json* cur = md.get("namespace");
      if (cur && cur->is_string() && cur->as_string() != rt.ns)
        throw ApiError(400, "BadRequest", "the namespace of the object does not match the request");
      md.set("namespace", Json(rt.ns));
    }
  }
  type_meta(body, *rt.rp);
  return json_reply(201, *store.create(*rt.kind, std::move(body)));
}

Reply update(ObjectStore& store, const Route& rt, const Request& r) {
  Json body = parse_object_body(r.body);
  Json& md = body.at_or_create("metadata");
  const Json* n = md.get("name");
  if (n && n->is_string() && n->as_string() != rt.name)
    throw ApiError(400, "BadRequest", "the name of the object does not match the request");
  md.set("name", Json(rt.name));
  if (rt.rp->namespaced) {
    std::string mns = rt.ns.empty() ? md["namespace"].str_or("") : rt.ns;
    md.set("namespace", Json(mns.empty() ? "default" : mns));
  }
  type_meta(body, *rt.rp);
  return json_reply(200, *store.update(*rt.kind, std::move(body), true));
}

Reply patch(ObjectStore& store, const Route& rt, const Request& r) {
  std::string ct(trim(std::string_view(r.content_type).substr(0, r.content_type.find(';'))));
  if (ct.empty()) ct = "application/merge-patch+json";
  Json body = parse_body(r.body);
  if (ct == "application/json-patch+json") {
    JsonPtr cur = store.get(*rt.kind, rt.ns, rt.name);
    if (!cur) throw ApiError(404, "NotFound", *rt.kind + " \"" + rt.name + "\" not found");
    Json next = apply_json_patch(*cur, body);
    // What is stored under this name stays an object of this name: the store would look the new one up.
    if (!next.is_object()) throw ApiError(422, "Invalid", "the patched " + rt.rp->kind + " is not a JSON object");
    const Json& md = next["metadata"];
    if (md["name"] != (*cur)["metadata"]["name"] || md["namespace"] != (*cur)["metadata"]["namespace"])
      throw ApiError(422, "Invalid", "metadata.name and metadata.namespace: field is immutable");
    return json_reply(200, *store.update(*rt.kind, std::move(next), true));
  }
  if (ct != "application/merge-patch+json" && ct != "application/strategic-merge-patch+json" &&
      ct != "application/apply-patch+yaml" && ct != "application/json")
    throw ApiError(415, "UnsupportedMediaType", "unsupported patch type " + ct);
  if (!body.is_object()) throw ApiError(400, "BadRequest", "merge patch body must be an object");
  return json_reply(200, *store.patch(*rt.kind, rt.ns, rt.name, body));
}

Reply erase(ObjectStore& store, const Route& rt, const Request& r) {
  if (rt.name.empty()) return success_reply(200, "deleted " + std::to_string(store.delete_all(*rt.kind, rt.ns)));
  Json opts = parse_body(r.body);
  int64_t grace = 0;
  if (opts["gracePeriodSeconds"].is_number()) grace = opts["gracePeriodSeconds"].as_int();
  else if (!r.q("gracePeriodSeconds").empty()) grace = std::strtoll(r.q("gracePeriodSeconds").c_str(), nullptr, 10);
  std::string uid = opts["preconditions"]["uid"].as_string();
  JsonPtr old = store.remove(*rt.kind, rt.ns, rt.name, grace, uid);
  return old ? json_reply(200, *old) : Reply{200, "{}"};
}

SSL_CTX* server_tls_context(const Options& o) {
  if (o.tls_cert_file.empty()) return nullptr;
  SSL_CTX* ctx = SSL_CTX_new(TLS_server_method());
  if (!ctx) throw std::runtime_error("apiserver: SSL_CTX_new: " + rest::ssl_error());
  auto fail = [ctx](const char* what) {
    std::string err = rest::ssl_error();
    SSL_CTX_free(ctx);
    throw std::runtime_error(std::string("apiserver: ") + what + ": " + err);
  };
  SSL_CTX_set_min_proto_version(ctx, TLS1_2_VERSION);
  const std::string& key = o.tls_key_file.empty() ? o.tls_cert_file : o.tls_key_file;
  if (SSL_CTX_use_certificate_chain_file(ctx, o.tls_cert_file.c_str()) != 1 ||
      SSL_CTX_use_PrivateKey_file(ctx, key.c_str(), SSL_FILETYPE_PEM) != 1 || SSL_CTX_check_private_key(ctx) != 1)
    fail("TLS certificate/key");
  if (!o.client_ca_file.empty()) {
    if (SSL_CTX_load_verify_locations(ctx, o.client_ca_file.c_str(), nullptr) != 1) fail("client CA");
    SSL_CTX_set_verify(ctx, SSL_VERIFY_PEER | SSL_VERIFY_FAIL_IF_NO_PEER_CERT, nullptr);
  }
  return ctx;
}

}  // namespace

// ---------------------------------------------------------------- server --
Server::Server(std::shared_ptr<ObjectStore> store, Options o) : store_(std::move(store)), opts_(std::move(o)) {
  tls_ctx_ = server_tls_context(opts_);
  addrinfo hints{}, *res = nullptr;
  hints.ai_family = AF_UNSPEC;
  hints.ai_socktype = SOCK_STREAM;
  hints.ai_flags = AI_PASSIVE | AI_NUMERICSERV;
  std::string port = std::to_string(opts_.port);
  const char* host = opts_.host.empty() || opts_.host == "0.0.0.0" ? nullptr : opts_.host.c_str();
  if (int e = ::getaddrinfo(host, port.c_str(), &hints, &res); e != 0)
    throw std::runtime_error(std::string("apiserver: resolve ") + opts_.host + ": " + gai_strerror(e));
  std::string err;
  for (addrinfo* ai = res; ai; ai = ai->ai_next) {
    int fd = ::socket(ai->ai_family, ai->ai_socktype | SOCK_CLOEXEC, ai->ai_protocol);
    if (fd < 0) continue;
    int one = 1;
    ::setsockopt(fd, SOL_SOCKET, SO_REUSEADDR, &one, sizeof one);
    if (::bind(fd, ai->ai_addr, ai->ai_addrlen) == 0 && ::listen(fd, 1024) == 0) {
      listen_fd_ = fd;
      sockaddr_storage ss{};
      socklen_t len = sizeof ss;
      ::getsockname(fd, reinterpret_cast<sockaddr*>(&ss), &len);
      port_ = ss.ss_family == AF_INET6 ? ntohs(reinterpret_cast<sockaddr_in6*>(&ss)->sin6_port)
                                       : ntohs(reinterpret_cast<sockaddr_in*>(&ss)->sin_port);
      break;
    }
    err = std::strerror(errno);
    ::close(fd);
  }
  ::freeaddrinfo(res);
  if (listen_fd_ < 0) {
    if (tls_ctx_) SSL_CTX_free(tls_ctx_);
    tls_ctx_ = nullptr;
    throw std::runtime_error("apiserver: cannot listen on " + opts_.host + ":" + port + ": " + err);
  }
}

Server::~Server() {
  stop();
  if (tls_ctx_) SSL_CTX_free(tls_ctx_);
}

void Server::start() {
  if (acceptor_.joinable() || stopping_) return;
  acceptor_ = std::thread([this] { accept_loop(); });
}

size_t Server::connections() const {
  std::lock_guard<std::mutex> g(mu_);
  return conns_.size();
}

void Server::accept_loop() {
  while (!stopping_.load()) {
    pollfd p{listen_fd_, POLLIN, 0};
    int r = ::poll(&p, 1, 100);
    if (r <= 0) continue;
    int fd = ::accept4(listen_fd_, nullptr, nullptr, SOCK_CLOEXEC);
    if (fd < 0) continue;
    int one = 1;
    ::setsockopt(fd, IPPROTO_TCP, TCP_NODELAY, &one, sizeof one);
    {
      std::lock_guard<std::mutex> g(mu_);
      if (stopping_ || conns_.size() >= static_cast<size_t>(opts_.max_connections)) {
        ::close(fd);
        continue;
      }
      conns_.insert(fd);
      ++live_threads_;
    }
    std::thread([this, fd] { serve(fd); }).detach();
  }
}

void Server::stop() {
  if (stopping_.exchange(true)) {
    // Second call (destructor after an explicit stop): nothing left to do.
    return;
  }
  if (acceptor_.joinable()) acceptor_.join();
  if (listen_fd_ >= 0) {
    ::close(listen_fd_);
    listen_fd_ = -1;
  }
  std::unique_lock<std::mutex> g(mu_);
  for (int fd : conns_) ::shutdown(fd, SHUT_RDWR);
  for (const auto& w : watchers_) w->stop();
  idle_cv_.wait_for(g, std::chrono::seconds(10), [this] { return live_threads_ == 0; });
}

void Server::serve(int fd) {
  // Runs last, after `c` has ended the TLS session and closed the socket.
  struct Done {
    Server* s;
    int fd;
    ~Done() {
      std::lock_guard<std::mutex> g(s->mu_);
      s->conns_.erase(fd);
      if (--s->live_threads_ == 0) s->idle_cv_.notify_all();
    }
  } done{this, fd};
  Wire c(Wire::Scratch::k64K, fd);
  if (tls_ctx_) {
    SSL* ssl = SSL_new(tls_ctx_);
    if (!ssl || SSL_set_fd(ssl, fd) != 1 || SSL_accept(ssl) != 1) {
      if (ssl) SSL_free(ssl);
      ERR_clear_error();
      return;
    }
    c.set_ssl(ssl);
  }
  Request r;
  for (;;) {
    int rc = read_request(c, r, opts_.token);
    if (rc < 0) break;
    if (rc > 0) {
      const char* reason = rc == 401 ? "Unauthorized" : rc == 413 ? "RequestEntityTooLarge" : "BadRequest";
      const char* msg = rc == 401 ? "Unauthorized" : rc == 413 ? "request body too large" : "malformed request";
      respond(c, status_reply(rc, reason, msg), false);
      break;
    }
    if (!handle(c, r) || stopping_) break;
  }
}

// The one place a request's reply is written: true when it went out and the
// connection stays open for the next request.
bool Server::handle(Wire& c, Request& r) {
  requests_.fetch_add(1, std::memory_order_relaxed);
  Reply reply;
  try {
    if (!answer(c, r, reply)) return false;  // a watch streamed its own response
  } catch (const ApiError& e) {
    reply = status_reply(e.code, e.reason, e.what());
  } catch (const StoreError& e) {
    reply = status_reply(e.code(), e.reason(), e.what());
  } catch (const JsonError& e) {
    reply = status_reply(400, "BadRequest", e.what());
  } catch (const std::exception& e) {
    reply = status_reply(500, "InternalError", e.what());
  }
  return respond(c, reply, r.keep_alive) && r.keep_alive;
}

bool Server::answer(Wire& c, Request& r, Reply& out) {
  const std::string& path = r.path;
  if (path == "/healthz" || path == "/readyz" || path == "/livez") {
    out = Reply{200, "ok", "text/plain"};
  } else if (path == "/version") {
    out.body = R"({"major":"1","minor":"23","gitVersion":"v1.23.3-xsched","platform":"linux/amd64"})";
  } else if (!opts_.token.empty() && r.authorization != "Bearer " + opts_.token) {
    throw ApiError(401, "Unauthorized", "Unauthorized");
  } else if (path == "/api") {
    out.body = R"({"kind":"APIVersions","versions":["v1"]})";
  } else if (path == "/apis") {
    out = api_groups();
  } else {
    Route rt = parse_route(path);
    if (r.method == "GET") {
      if (rt.name.empty() && r.flag("watch")) {
        watch(c, *rt.kind, rt.ns, r);
        return false;  // the stream ended; clients reconnect for the next watch
      }
      out = rt.name.empty() ? list_many(*store_, rt, r) : get_one(*store_, rt);
    } else if (r.method == "POST") {
      out = create(*store_, rt, r);
    } else if (r.method == "PUT") {
      out = update(*store_, rt, r);
    } else if (r.method == "PATCH") {
      out = patch(*store_, rt, r);
    } else if (r.method == "DELETE") {
      out = erase(*store_, rt, r);
    } else {
      throw ApiError(405, "MethodNotAllowed", "method " + r.method + " not allowed");
    }
  }
  return true;
}

void Server::watch(Wire& c, const std::string& kind, const std::string& ns, Request& r) {
  const rest::ResourcePath& rp = rest::resource_path(kind);
  Selectors sel;
  try {
    sel = parse_selectors(r);
  } catch (const std::invalid_argument& e) {
    respond(c, status_reply(400, "BadRequest", e.what()), false);
    return;
  }
  std::string rvp = r.q("resourceVersion");
  int64_t since = rvp.empty() || rvp == "0" ? 0 : std::strtoll(rvp.c_str(), nullptr, 10);
  double timeout_s = std::strtod(r.q("timeoutSeconds").c_str(), nullptr);
  bool bookmarks = r.flag("allowWatchBookmarks");

  WatcherPtr w;
  std::string expired;
  try {
    w = store_->watch({kind}, ns, since);
  } catch (const StoreError& e) {
    if (e.code() != 410) throw;
    expired = e.what();
  }
  if (w) {
    std::lock_guard<std::mutex> g(mu_);
    watchers_.insert(w);
    if (stopping_) w->stop();
  }
  struct Unregister {
    Server* s;
    WatcherPtr w;
    ~Unregister() {
      if (!w) return;
      s->store_->unwatch(w);
      std::lock_guard<std::mutex> g(s->mu_);
      s->watchers_.erase(w);
    }
  } unregister{this, w};

  if (!c.send_all("HTTP/1.1 200 OK\r\nContent-Type: application/json\r\nTransfer-Encoding: chunked\r\n\r\n")) return;
  if (!expired.empty()) {
    Json ev = Json::object();
    ev.set("type", Json("ERROR"));
    ev.set("object", status_obj(410, "Expired", expired));
    write_chunk(c, ev.dump() + "\n") && write_chunk(c, "");
    return;
  }
  int64_t floor = 0;
  if (since == 0) {
    auto items = store_->list(kind, ns, &floor);
    std::string out;
    for (const auto& it : items) {
      if (!sel.match(*it)) continue;
      out += R"({"type":"ADDED","object":)";
      it->dump_to(out);
      out += "}\n";
      if (out.size() > (1u << 20)) {
        if (!write_chunk(c, out)) return;
        out.clear();
      }
    }
    if (!out.empty() && !write_chunk(c, out)) return;
  }
  using clock = std::chrono::steady_clock;
  auto deadline = timeout_s > 0 ? clock::now() + std::chrono::microseconds(static_cast<int64_t>(timeout_s * 1e6))
                                : clock::time_point::max();
  int64_t last_rv = floor;
  auto last_beat = clock::now();
  while (!stopping_ && !w->stopped()) {
    if (clock::now() >= deadline) break;
    auto evs = w->next(500, 1024);
    if (evs.empty()) {
      if (c.peer_closed()) return;
      if (bookmarks && clock::now() - last_beat >= std::chrono::milliseconds(opts_.bookmark_interval_ms)) {
        std::string b = R"({"type":"BOOKMARK","object":{"kind":")" + rp.kind + R"(","apiVersion":")" + rp.api_version +
                        R"(","metadata":{"resourceVersion":")" + std::to_string(last_rv) + "\"}}}\n";
        if (!write_chunk(c, b)) return;
        last_beat = clock::now();
      }
      continue;
    }
    std::string out;
    for (const auto& ev : evs) {
      if (ev.rv <= floor || !ev.obj) continue;
      last_rv = ev.rv;
      if (!sel.match(*ev.obj)) continue;
      out += R"({"type":")";
      out += event_type_name(ev.type);
      out += R"(","object":)";
      if (ev.type == EventType::Deleted) {
        Json o = *ev.obj;
        o.at_or_create("metadata").set("resourceVersion", Json(std::to_string(ev.rv)));
        o.dump_to(out);
      } else {
        ev.obj->dump_to(out);
      }
      out += "}\n";
    }
    if (!out.empty() && !write_chunk(c, out)) return;
    last_beat = clock::now();
  }
  write_chunk(c, "");
}

}  // namespace xsched::apiserver
