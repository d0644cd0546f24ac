// The HTTP/1.1 wire below the request/response level, shared by the REST
// client (rest/http.cc) and the API server (apiserver/apiserver.cc): one
// connected socket, plain or TLS, with a read buffer in front; lines, exact
// reads, chunked bodies, header lines and the framing facts they carry.
// Socket setup (connect / accept, timeouts, handshakes) stays with each end.
#pragma once

#include <sys/types.h>

#include <cstddef>
#include <cstdint>
#include <string>
#include <string_view>

typedef struct ssl_st SSL;

namespace xsched::rest {

constexpr size_t kMaxLine = 1u << 20;           // status, header and chunk-size lines
constexpr size_t kNoCap = static_cast<size_t>(-1);

// Text of the calling thread's oldest queued OpenSSL error (and pops it).
std::string ssl_error();

int hexval(char c);  // -1 when c is no hex digit

// Chunk-size line of a chunked body: 1-15 hex digits, optionally followed by
// ";extensions" or blanks. False for anything else (an overlong or non-hex
// size is a malformed message, not a huge allocation).
bool parse_chunk_size(std::string_view line, size_t* out);

// "Name: value" -> lower-cased name and the value without surrounding white
// space (a view into `line`). False for a line without a colon. White space
// around the name is dropped only with `trim_name`: the server has always
// accepted "Name : value", the client has always ignored such a line.
bool scan_header(std::string_view line, bool trim_name, std::string& name, std::string_view& value);

// What the headers say about the message's framing.
struct Framing {
  int64_t content_length = -1;  // -1: none given
  bool chunked = false;
  bool close = false;       // some Connection header said close
  bool keep_alive = false;  // the last Connection header to say either said keep-alive
  // Takes Content-Length, Transfer-Encoding and Connection; false for any
  // other header. `name` is lower-cased (scan_header).
  bool note(std::string_view name, std::string_view value);
};

class Wire {
 public:
  // How much one read asks for. Each end keeps what it has always used: the
  // client reads small responses, the server pipelined requests and bodies.
  enum class Scratch { k16K, k64K };
  explicit Wire(Scratch scratch, int fd = -1) : fd_(fd), scratch_(scratch) {}
  ~Wire();  // SSL_shutdown and SSL_free (when TLS), then close
  Wire(const Wire&) = delete;
  Wire& operator=(const Wire&) = delete;

  // Take ownership: of a connected socket, and of its TLS session once the
  // handshake has succeeded (every read and write then goes through it).
  void set_fd(int fd) { fd_ = fd; }
  void set_ssl(SSL* ssl) { ssl_ = ssl; }
  int fd() const { return fd_; }
  bool tls() const { return ssl_ != nullptr; }
  void shutdown();  // shutdown(SHUT_RDWR): unblocks a reader on another thread
  // The peer has closed or reset, seen without reading (a watch stream only
  // writes when events arrive, so nothing else would notice).
  bool peer_closed() const;

  // Reads more bytes into the buffer; false on EOF or an error.
  bool fill();
  // Writes all of `d`; false on an error (never raises SIGPIPE).
  bool send_all(std::string_view d);
  // One line through the next CRLF or LF, without it. False on EOF, an
  // error, or a line longer than `max_len` bytes (kNoCap: any length); only
  // then is overlong() true afterwards.
  bool line(std::string& out, size_t max_len = kMaxLine);
  bool overlong() const { return overlong_; }
  // Appends exactly n bytes to `out`; false when the stream ends first.
  bool exact(size_t n, std::string& out);
  // Received and not yet consumed.
  std::string_view buffered() const { return std::string_view(buf_).substr(pos_); }
  void consume(size_t n) { pos_ += n; }

  enum class Body { kOk, kClosed, kMalformed, kTooLarge };
  // Appends a whole chunked body (through its trailers) to `out`, at most
  // `cap` bytes of it. The line after a chunk's data is read, not checked.
  Body chunked_body(std::string& out, size_t cap = kNoCap);

  enum class Head { kOk, kClosed, kTooMany };
  // Header lines through the empty one. Framing headers go into `f`, every
  // other one to other(name, value); more than `max_lines` lines: kTooMany.
  template <class F>
  Head headers(Framing& f, bool trim_name, size_t max_lines, F&& other) {
    std::string name;
    std::string_view value;
    for (size_t n = 0;; ++n) {
      if (n > max_lines) return Head::kTooMany;
      if (!line(line_)) return Head::kClosed;
      if (line_.empty()) return Head::kOk;
      if (scan_header(line_, trim_name, name, value) && !f.note(name, value)) other(name, value);
    }
  }

  // How the last failed read or write failed, and how many bytes have come
  // in since begin_request(): the client tells a keep-alive connection that
  // the server closed while idle (safe to send again) from one that may have
  // delivered the request. The server ignores both.
  enum class Fail { kNone, kEof, kReset, kTimeout, kOther };
  void begin_request();
  // EOF or a reset before any response byte, never a timeout.
  bool failed_stale() const { return (fail_ == Fail::kEof || fail_ == Fail::kReset) && rx_bytes_ == 0; }

 private:
  void note_io_failure(ssize_t n);  // classifies errno, right after the failing call
  template <size_t N>
  bool read_some();

  int fd_ = -1;
  Scratch scratch_;
  bool overlong_ = false;
  SSL* ssl_ = nullptr;
  std::string buf_;  // received; consumed up to pos_
  size_t pos_ = 0;
  std::string line_;  // headers(): the current line
  Fail fail_ = Fail::kNone;
  size_t rx_bytes_ = 0;
};

}  // namespace xsched::rest
