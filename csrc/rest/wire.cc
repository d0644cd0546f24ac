#include "rest/wire.h"

#include "common/strings.h"

#include <openssl/err.h>
#include <openssl/ssl.h>
#include <poll.h>
#include <sys/socket.h>
#include <unistd.h>

#include <algorithm>
#include <cctype>
#include <cerrno>
#include <cstdlib>

namespace xsched::rest {

std::string ssl_error() {
  unsigned long e = ERR_get_error();
  char buf[256];
  ERR_error_string_n(e, buf, sizeof buf);
  return buf;
}

int hexval(char c) {
  if (c >= '0' && c <= '9') return c - '0';
  if (c >= 'a' && c <= 'f') return c - 'a' + 10;
  if (c >= 'A' && c <= 'F') return c - 'A' + 10;
  return -1;
}

bool parse_chunk_size(std::string_view line, size_t* out) {
  size_t v = 0, i = 0;
  for (; i < line.size() && i < 16; ++i) {
    int d = hexval(line[i]);
    if (d < 0) break;
    v = v * 16 + static_cast<size_t>(d);
  }
  if (i == 0 || i > 15) return false;
  if (i < line.size() && line[i] != ';' && line[i] != ' ' && line[i] != '\t') return false;
  *out = v;
  return true;
}

namespace {

// Case-insensitive substring search; `needle` is lower case.
bool contains_lower(std::string_view hay, std::string_view needle) {
  auto it = std::search(hay.begin(), hay.end(), needle.begin(), needle.end(),
                        [](char h, char n) { return std::tolower(static_cast<unsigned char>(h)) == n; });
  return it != hay.end();
}

}  // namespace

bool scan_header(std::string_view line, bool trim_name, std::string& name, std::string_view& value) {
  size_t colon = line.find(':');
  if (colon == std::string_view::npos) return false;
  std::string_view n = line.substr(0, colon);
  name.assign(trim_name ? trim(n) : n);
  for (auto& c : name) c = static_cast<char>(std::tolower(static_cast<unsigned char>(c)));
  value = trim(line.substr(colon + 1));
  return true;
}

bool Framing::note(std::string_view name, std::string_view value) {
  if (name == "content-length") {
    content_length = std::strtoll(std::string(value).c_str(), nullptr, 10);
  } else if (name == "transfer-encoding") {
    chunked = contains_lower(value, "chunked");
  } else if (name == "connection") {
    if (contains_lower(value, "close")) {
      close = true;
      keep_alive = false;
    } else if (contains_lower(value, "keep-alive")) {
      keep_alive = true;
    }
  } else {
    return false;
  }
  return true;
}

Wire::~Wire() {
  if (ssl_) {
    SSL_shutdown(ssl_);
    SSL_free(ssl_);
    ERR_clear_error();
  }
  if (fd_ >= 0) ::close(fd_);
}

void Wire::shutdown() {
  if (fd_ >= 0) ::shutdown(fd_, SHUT_RDWR);
}

bool Wire::peer_closed() const {
  pollfd p{fd_, POLLIN | POLLRDHUP, 0};
  if (::poll(&p, 1, 0) <= 0) return false;
  if (p.revents & (POLLRDHUP | POLLHUP | POLLERR)) return true;
  char b;
  ssize_t n = ::recv(fd_, &b, 1, MSG_PEEK | MSG_DONTWAIT);
  return n == 0;
}

void Wire::begin_request() {
  fail_ = Fail::kNone;
  rx_bytes_ = 0;
  errno = 0;
}

void Wire::note_io_failure(ssize_t n) {
  const int e = errno;
  if (e == EAGAIN || e == EWOULDBLOCK || e == ETIMEDOUT)
    fail_ = Fail::kTimeout;  // SO_RCVTIMEO/SO_SNDTIMEO expired: the peer may be working on it
  else if (e == ECONNRESET || e == EPIPE || e == ECONNABORTED)
    fail_ = Fail::kReset;
  else if (n == 0)
    fail_ = Fail::kEof;
  else
    fail_ = Fail::kOther;
}

bool Wire::fill() {
  if (pos_ > 0 && pos_ == buf_.size()) {
    buf_.clear();
    pos_ = 0;
  } else if (pos_ > (1u << 16)) {
    buf_.erase(0, pos_);
    pos_ = 0;
  }
  return scratch_ == Scratch::k16K ? read_some<16384>() : read_some<65536>();
}

template <size_t N>
bool Wire::read_some() {
  char tmp[N];
  for (;;) {
    ssize_t n = ssl_ ? SSL_read(ssl_, tmp, sizeof tmp) : ::recv(fd_, tmp, sizeof tmp, 0);
    if (n > 0) {
      buf_.append(tmp, static_cast<size_t>(n));
      rx_bytes_ += static_cast<size_t>(n);
      return true;
    }
    if (!ssl_ && n < 0 && errno == EINTR) continue;
    note_io_failure(n);
    return false;
  }
}

bool Wire::send_all(std::string_view d) {
  while (!d.empty()) {
    ssize_t n = ssl_ ? SSL_write(ssl_, d.data(), static_cast<int>(std::min<size_t>(d.size(), 1u << 30)))
                     : ::send(fd_, d.data(), d.size(), MSG_NOSIGNAL);
    if (n <= 0) {
      if (!ssl_ && n < 0 && errno == EINTR) continue;
      note_io_failure(n);
      return false;
    }
    d.remove_prefix(static_cast<size_t>(n));
  }
  return true;
}

bool Wire::line(std::string& out, size_t max_len) {
  overlong_ = false;
  for (;;) {
    size_t e = buf_.find('\n', pos_);
    if (e != std::string::npos) {
      size_t end = e > pos_ && buf_[e - 1] == '\r' ? e - 1 : e;
      if (end - pos_ > max_len) return !(overlong_ = true);
      out.assign(buf_, pos_, end - pos_);
      pos_ = e + 1;
      return true;
    }
    // One byte of grace: a CR whose LF has not arrived yet.
    if (max_len != kNoCap && buf_.size() - pos_ > max_len + 1) return !(overlong_ = true);
    if (!fill()) return false;
  }
}

bool Wire::exact(size_t n, std::string& out) {
  while (buf_.size() - pos_ < n)
    if (!fill()) return false;
  out.append(buf_, pos_, n);
  pos_ += n;
  return true;
}

Wire::Body Wire::chunked_body(std::string& out, size_t cap) {
  std::string ln;
  for (size_t total = 0;;) {
    if (!line(ln)) return Body::kClosed;
    size_t sz = 0;
    if (!parse_chunk_size(ln, &sz)) return Body::kMalformed;
    if (sz == 0) {
      do {  // trailers until an empty line
        if (!line(ln)) return Body::kClosed;
      } while (!ln.empty());
      return Body::kOk;
    }
    if (sz > cap - total) return Body::kTooLarge;  // total <= cap: no wrap-around
    if (!exact(sz, out) || !line(ln)) return Body::kClosed;
    total += sz;
  }
}

}  // namespace xsched::rest
