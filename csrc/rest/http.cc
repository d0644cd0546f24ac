#include "rest/http.h"

#include "common/log.h"

#include <arpa/inet.h>
#include <netdb.h>
#include <netinet/in.h>
#include <netinet/tcp.h>
#include <openssl/err.h>
#include <openssl/pem.h>
#include <openssl/ssl.h>
#include <openssl/x509v3.h>
#include <sys/socket.h>
#include <sys/time.h>
#include <unistd.h>

#include <algorithm>
#include <cctype>
#include <cerrno>
#include <cstring>
#include <stdexcept>

namespace xsched::rest {

namespace {

constexpr int kWatchRecvTimeoutS = 330;  // > the watches' timeoutSeconds=300

std::string tls_error(const std::string& what) { return what + ": " + ssl_error(); }

bool is_ip_literal(const std::string& h) {
  in6_addr a6;
  in_addr a4;
  return inet_pton(AF_INET, h.c_str(), &a4) == 1 || inet_pton(AF_INET6, h.c_str(), &a6) == 1;
}

}  // namespace

class TlsContext {
 public:
  explicit TlsContext(const TlsOptions& o) : insecure(o.insecure) {
    ctx = SSL_CTX_new(TLS_client_method());
    if (!ctx) throw std::runtime_error(tls_error("SSL_CTX_new"));
    SSL_CTX_set_min_proto_version(ctx, TLS1_2_VERSION);
    if (!o.ca_file.empty()) {
      if (SSL_CTX_load_verify_locations(ctx, o.ca_file.c_str(), nullptr) != 1)
        throw std::runtime_error(tls_error("loading CA file"));
    } else if (!o.ca_pem.empty()) {
      BIO* bio = BIO_new_mem_buf(o.ca_pem.data(), static_cast<int>(o.ca_pem.size()));
      X509_STORE* store = SSL_CTX_get_cert_store(ctx);
      int n = 0;
      while (X509* x = PEM_read_bio_X509(bio, nullptr, nullptr, nullptr)) {
        X509_STORE_add_cert(store, x);
        X509_free(x);
        ++n;
      }
      BIO_free(bio);
      ERR_clear_error();  // the loop ends on a PEM "no start line"
      if (n == 0) throw std::runtime_error("CA data holds no certificate");
    } else {
      SSL_CTX_set_default_verify_paths(ctx);
    }
    if (!o.cert_file.empty()) {
      if (SSL_CTX_use_certificate_chain_file(ctx, o.cert_file.c_str()) != 1 ||
          SSL_CTX_use_PrivateKey_file(ctx, (o.key_file.empty() ? o.cert_file : o.key_file).c_str(), SSL_FILETYPE_PEM) != 1)
        throw std::runtime_error(tls_error("loading client certificate"));
    } else if (!o.cert_pem.empty()) {
      BIO* cb = BIO_new_mem_buf(o.cert_pem.data(), static_cast<int>(o.cert_pem.size()));
      X509* cert = PEM_read_bio_X509(cb, nullptr, nullptr, nullptr);
      BIO_free(cb);
      const std::string& kp = o.key_pem.empty() ? o.cert_pem : o.key_pem;
      BIO* kb = BIO_new_mem_buf(kp.data(), static_cast<int>(kp.size()));
      EVP_PKEY* key = PEM_read_bio_PrivateKey(kb, nullptr, nullptr, nullptr);
      BIO_free(kb);
      bool ok = cert && key && SSL_CTX_use_certificate(ctx, cert) == 1 && SSL_CTX_use_PrivateKey(ctx, key) == 1;
      if (cert) X509_free(cert);
      if (key) EVP_PKEY_free(key);
      if (!ok) throw std::runtime_error(tls_error("loading client certificate data"));
    }
    SSL_CTX_set_verify(ctx, insecure ? SSL_VERIFY_NONE : SSL_VERIFY_PEER, nullptr);
  }
  ~TlsContext() {
    if (ctx) SSL_CTX_free(ctx);
  }
  SSL_CTX* ctx = nullptr;
  bool insecure = false;
};

std::shared_ptr<TlsContext> make_tls_context(const TlsOptions& o) {
  return o.enabled ? std::make_shared<TlsContext>(o) : nullptr;
}

std::string url_segment(std::string_view s) {
  static const char* hex = "0123456789ABCDEF";
  std::string out;
  out.reserve(s.size());
  for (unsigned char c : s) {
    if (std::isalnum(c) || c == '-' || c == '_' || c == '.' || c == '~') {
      out.push_back(static_cast<char>(c));
    } else {
      out.push_back('%');
      out.push_back(hex[c >> 4]);
      out.push_back(hex[c & 15]);
    }
  }
  return out;
}

HttpConn::HttpConn(const Endpoint& ep, std::shared_ptr<TlsContext> tls, bool streaming) : ep_(ep), tls_(std::move(tls)) {
  addrinfo hints{};
  hints.ai_family = AF_UNSPEC;
  hints.ai_socktype = SOCK_STREAM;
  addrinfo* res = nullptr;
  std::string port = std::to_string(ep.port);
  if (int rc = getaddrinfo(ep.host.c_str(), port.c_str(), &hints, &res); rc != 0)
    throw std::runtime_error("resolve " + ep.host + ": " + gai_strerror(rc));
  std::string err = "connect " + ep.host + ":" + port + " failed";
  for (addrinfo* a = res; a; a = a->ai_next) {
    int fd = ::socket(a->ai_family, a->ai_socktype | SOCK_CLOEXEC, a->ai_protocol);
    if (fd < 0) continue;
    timeval tv{ep.timeout_ms / 1000, (ep.timeout_ms % 1000) * 1000};
    setsockopt(fd, SOL_SOCKET, SO_SNDTIMEO, &tv, sizeof(tv));
    if (!streaming) {
      setsockopt(fd, SOL_SOCKET, SO_RCVTIMEO, &tv, sizeof(tv));
    } else {
      // A watch idles between events until the server's timeoutSeconds
      // (300 s) ends it. A half-open connection (API server host lost, an
      // idle-dropping load balancer) would block recv forever: TCP keepalive
      // probes find a dead peer within ~1 min, and a receive timeout above
      // the watch timeout ends the stream regardless, so the mirror re-watches.
      timeval rtv{kWatchRecvTimeoutS, 0};
      setsockopt(fd, SOL_SOCKET, SO_RCVTIMEO, &rtv, sizeof(rtv));
      int on = 1, idle = 30, intvl = 10, cnt = 3;
      setsockopt(fd, SOL_SOCKET, SO_KEEPALIVE, &on, sizeof(on));
      setsockopt(fd, IPPROTO_TCP, TCP_KEEPIDLE, &idle, sizeof(idle));
      setsockopt(fd, IPPROTO_TCP, TCP_KEEPINTVL, &intvl, sizeof(intvl));
      setsockopt(fd, IPPROTO_TCP, TCP_KEEPCNT, &cnt, sizeof(cnt));
    }
    if (::connect(fd, a->ai_addr, a->ai_addrlen) == 0) {
      int one = 1;
      setsockopt(fd, IPPROTO_TCP, TCP_NODELAY, &one, sizeof(one));  // small keep-alive requests
      wire_.set_fd(fd);
      break;
    }
    err += std::string(": ") + std::strerror(errno);
    ::close(fd);
  }
  freeaddrinfo(res);
  if (wire_.fd() < 0) throw std::runtime_error(err);
  if (tls_) {
    SSL* ssl = SSL_new(tls_->ctx);
    SSL_set_fd(ssl, wire_.fd());
    if (!is_ip_literal(ep.host)) SSL_set_tlsext_host_name(ssl, ep.host.c_str());
    if (!tls_->insecure) {
      X509_VERIFY_PARAM* param = SSL_get0_param(ssl);
      if (is_ip_literal(ep.host))
        X509_VERIFY_PARAM_set1_ip_asc(param, ep.host.c_str());
      else
        X509_VERIFY_PARAM_set1_host(param, ep.host.c_str(), 0);
    }
    if (SSL_connect(ssl) != 1) {
      std::string e = tls_error("TLS handshake with " + ep.host);
      SSL_free(ssl);
      throw std::runtime_error(e);  // wire_ closes the socket
    }
    wire_.set_ssl(ssl);
  }
}

void HttpConn::fail(const std::string& what) {
  reusable_ = false;
  throw std::runtime_error(what);
}

void HttpConn::send_request(std::string_view method, std::string_view path, std::string_view body,
                            std::string_view content_type) {
  std::string req;
  req.reserve(256 + body.size());
  req.append(method).append(" ").append(path).append(" HTTP/1.1\r\nHost: ");
  req.append(ep_.host).append(":").append(std::to_string(ep_.port));
  req.append("\r\nAccept: application/json\r\nUser-Agent: xsched-native/1\r\n");
  if (!ep_.token.empty()) req.append("Authorization: Bearer ").append(ep_.token).append("\r\n");
  if (!body.empty()) {
    req.append("Content-Type: ").append(content_type).append("\r\nContent-Length: ");
    req.append(std::to_string(body.size())).append("\r\n");
  }
  req.append("\r\n").append(body);  // one write: headers and body in one segment
  if (!wire_.send_all(req)) fail(std::string("send: ") + (wire_.tls() ? "TLS write failed" : std::strerror(errno)));
}

int HttpConn::read_head(Framing* f) {
  std::string line;
  if (!wire_.line(line)) fail(wire_.overlong() ? "status line too long" : "connection closed before the response");
  // "HTTP/1.1 200 OK"
  size_t sp = line.find(' ');
  if (sp == std::string::npos || line.compare(0, 5, "HTTP/") != 0) fail("malformed status line: " + line.substr(0, 80));
  int status = std::atoi(line.c_str() + sp + 1);
  *f = Framing{};
  auto ignore = [](std::string_view, std::string_view) {};
  if (wire_.headers(*f, /*trim_name=*/false, kNoCap, ignore) != Wire::Head::kOk)
    fail(wire_.overlong() ? "response header line too long" : "connection closed in the response headers");
  if (f->close || line.compare(0, 8, "HTTP/1.0") == 0) reusable_ = false;
  return status;
}

Response HttpConn::roundtrip(std::string_view method, std::string_view path, std::string_view body,
                             std::string_view content_type) {
  wire_.begin_request();
  send_request(method, path, body, content_type);
  Framing f;
  Response r;
  r.status = read_head(&f);
  if (f.chunked) {
    Wire::Body b = wire_.chunked_body(r.body);
    if (b == Wire::Body::kMalformed) fail("malformed chunk size in the response body");
    if (b != Wire::Body::kOk) fail("connection closed in the response body");
  } else if (f.content_length >= 0) {
    if (!wire_.exact(static_cast<size_t>(f.content_length), r.body)) fail("connection closed in the response body");
  } else if (method == "HEAD" || r.status == 204 || r.status == 304) {
    // no body
  } else {  // body until the server closes
    reusable_ = false;
    while (wire_.fill()) {
    }
    r.body.assign(wire_.buffered());
    wire_.consume(r.body.size());
  }
  return r;
}

int HttpConn::open_stream(std::string_view path) {
  send_request("GET", path, {}, {});
  Framing f;
  int status = read_head(&f);
  stream_chunked_ = f.chunked;
  stream_left_ = f.chunked ? -1 : f.content_length;
  pending_.clear();
  reusable_ = false;  // a watch connection ends with its stream
  return status;
}

bool HttpConn::next_chunk() {
  if (stream_chunked_) {
    std::string line;
    size_t len = 0;
    if (!wire_.line(line)) return false;
    if (!parse_chunk_size(line, &len)) {  // not an end of stream: say so before the caller re-watches
      XS_WARN("watch stream ended by a malformed chunk size").kv("host", ep_.host).kv("line", line.substr(0, 40));
      return false;
    }
    if (len == 0) return false;  // end of stream
    if (!wire_.exact(len, pending_)) return false;
    return wire_.line(line);
  }
  if (stream_left_ == 0) return false;
  if (wire_.buffered().empty() && !wire_.fill()) return false;
  std::string_view avail = wire_.buffered();
  size_t take = stream_left_ < 0 ? avail.size() : std::min<size_t>(avail.size(), static_cast<size_t>(stream_left_));
  pending_.append(avail.substr(0, take));
  wire_.consume(take);
  if (stream_left_ > 0) stream_left_ -= static_cast<int64_t>(take);
  return true;
}

bool HttpConn::next_line(std::string& line) {
  for (;;) {
    size_t nl = pending_.find('\n');
    if (nl != std::string::npos) {
      line.assign(pending_, 0, nl);
      pending_.erase(0, nl + 1);
      if (!line.empty() && line.back() == '\r') line.pop_back();
      if (line.empty()) continue;
      return true;
    }
    if (!next_chunk()) {
      if (pending_.empty()) return false;
      line.swap(pending_);  // a final line without a newline
      pending_.clear();
      return true;
    }
  }
}

}  // namespace xsched::rest
