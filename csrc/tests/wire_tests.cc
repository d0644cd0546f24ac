// Native tests for the HTTP/1.1 wire layer (rest/wire.h), without Python and
// without a server: a Wire on one end of a socketpair, the test on the other
// end writing scripted bytes, half-closing, or reading back.
//
// Built by `python -m flex_gpu_scheduler_amd.build_ext --wire-tests` into
// build/xsched_wire_tests (`--wire-asan`: build/xsched_wire_tests_asan, with
// AddressSanitizer and UndefinedBehaviorSanitizer) and run by
// tests/test_http_wire.py. Needs only rest/wire.cc and OpenSSL.
#include <sched.h>
#include <sys/ioctl.h>
#include <sys/socket.h>
#include <unistd.h>

#include <cstdio>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "rest/wire.h"

using namespace xsched::rest;

namespace {

int g_failed = 0, g_checks = 0;
#define CHECK(cond)                                                          \
  do {                                                                       \
    ++g_checks;                                                              \
    if (!(cond)) {                                                           \
      ++g_failed;                                                            \
      std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
    }                                                                        \
  } while (0)
#define CHECK_EQ(a, b) CHECK((a) == (b))

void write_all(int fd, std::string_view d) {
  while (!d.empty()) {
    ssize_t n = ::send(fd, d.data(), d.size(), MSG_NOSIGNAL);
    if (n <= 0) return;
    d.remove_prefix(static_cast<size_t>(n));
  }
}

// A Wire and the peer end of its socket.
struct Pair {
  Wire w;
  int peer = -1;
  std::thread writer;
  explicit Pair(Wire::Scratch scratch = Wire::Scratch::k64K) : w(scratch) {
    int sv[2];
    if (::socketpair(AF_UNIX, SOCK_STREAM, 0, sv) != 0) std::abort();
    w.set_fd(sv[0]);
    peer = sv[1];
  }
  ~Pair() {
    if (writer.joinable()) writer.join();
    if (peer >= 0) ::close(peer);
  }
  void put(std::string_view d) { write_all(peer, d); }
  void eof() { ::shutdown(peer, SHUT_WR); }
  // Writes the parts from a second thread, each only once the Wire has taken
  // everything before it off the socket, then half-closes if asked: the Wire
  // sees every part in a read of its own.
  void put_parts(std::vector<std::string> parts, bool then_eof = false) {
    writer = std::thread([this, parts = std::move(parts), then_eof] {
      for (const auto& p : parts) {
        for (int unread = 1; unread > 0; sched_yield()) ::ioctl(w.fd(), FIONREAD, &unread);
        write_all(peer, p);
      }
      if (then_eof) eof();
    });
  }
};

void test_line() {
  Pair p;
  p.put("first\r\nsecond\n\r\n\nlast");
  p.eof();
  std::string s;
  CHECK(p.w.line(s));
  CHECK_EQ(s, "first");  // CRLF
  CHECK(p.w.line(s));
  CHECK_EQ(s, "second");  // bare LF
  CHECK(p.w.line(s));
  CHECK_EQ(s, "");  // empty line, CRLF
  CHECK(p.w.line(s));
  CHECK_EQ(s, "");  // empty line, LF
  CHECK(!p.w.line(s));  // EOF mid-line
}

void test_line_split_across_writes() {
  Pair p;
  p.put_parts({"GET / HT", "TP/1.1\r", "\nnext\n"});
  std::string s;
  CHECK(p.w.line(s));
  CHECK_EQ(s, "GET / HTTP/1.1");
  CHECK(p.w.line(s));
  CHECK_EQ(s, "next");
}

void test_line_limit() {
  std::string s;
  {
    Pair p;
    p.put("12345678\r\n12345678\n123456789\n");
    CHECK(p.w.line(s, 8));  // exactly at the limit, CRLF
    CHECK_EQ(s, "12345678");
    CHECK(p.w.line(s, 8));  // exactly at the limit, LF
    CHECK(!p.w.line(s, 8));  // one byte over
    CHECK(p.w.overlong());
  }
  {  // the same at the default limit, where the line spans many reads
    Pair p;
    p.put_parts({std::string(kMaxLine, 'a') + "\r\n", std::string(kMaxLine + 1, 'b') + "\r\n"});
    CHECK(p.w.line(s));
    CHECK_EQ(s.size(), kMaxLine);
    CHECK(!p.w.line(s));
    p.w.shutdown();  // the writer may still be blocked on the rest
  }
  {  // over the limit with no newline in sight: fails without waiting for one
    Pair p;
    p.put("0123456789");
    CHECK(!p.w.line(s, 8));
    CHECK(p.w.overlong());
  }
  {  // kNoCap is no limit; an EOF is not an overlong line
    Pair p;
    p.put("0123456789");
    p.eof();
    CHECK(!p.w.line(s, kNoCap));
    CHECK(!p.w.overlong());
  }
}

void test_exact() {
  std::string s;
  {
    Pair p;
    p.put("abcdef\n");
    CHECK(p.w.line(s, 0) == false);  // buffers all seven bytes; "abcdef" is over a limit of 0
    CHECK(p.w.exact(4, s = ""));     // already buffered: the peer writes nothing more
    CHECK_EQ(s, "abcd");
    CHECK(p.w.exact(2, s));          // appends
    CHECK_EQ(s, "abcdef");
  }
  {
    Pair p;
    p.put_parts({"ab", "cd", "efg"});
    CHECK(p.w.exact(6, s = ""));  // spans three writes
    CHECK_EQ(s, "abcdef");
    CHECK_EQ(p.w.buffered(), "g");
  }
  {
    Pair p;
    p.put_parts({"abc"}, /*then_eof=*/true);
    CHECK(!p.w.exact(4, s = ""));  // EOF one byte short
  }
}

void test_small_scratch() {
  // The client's 16 KiB reads: a body of several reads arrives whole.
  Pair p(Wire::Scratch::k16K);
  std::string body(50000, 'y'), s;
  p.put(body + "end\n");
  CHECK(p.w.exact(body.size(), s));
  CHECK(s == body);
  CHECK(p.w.line(s));
  CHECK_EQ(s, "end");
}

void test_buffer_compaction() {
  // 70,000 body bytes and the start of a line are on the socket before the
  // first read, so the body is consumed with "par" still buffered behind it:
  // the next read finds more than 64 KiB consumed and compacts the buffer.
  Pair p;
  p.put(std::string(70000, 'x') + "par");
  std::string s;
  CHECK(p.w.exact(70000, s));
  CHECK_EQ(s, std::string(70000, 'x'));
  CHECK_EQ(p.w.buffered(), "par");
  p.put_parts({"tial\r\nafter\n"});
  CHECK(p.w.line(s));
  CHECK_EQ(s, "partial");
  CHECK(p.w.line(s));
  CHECK_EQ(s, "after");
}

void test_chunk_sizes() {
  size_t v = 99;
  CHECK(parse_chunk_size("0", &v) && v == 0);
  CHECK(parse_chunk_size("a", &v) && v == 10);
  CHECK(parse_chunk_size("A;ext=1", &v) && v == 10);
  CHECK(parse_chunk_size("10 ", &v) && v == 16);
  CHECK(parse_chunk_size("fffffffffffffff", &v) && v == 0xfffffffffffffffULL);
  v = 99;
  CHECK(!parse_chunk_size("ffffffffffffffff", &v));
  CHECK(!parse_chunk_size("zz", &v));
  CHECK(!parse_chunk_size("", &v));
  CHECK(!parse_chunk_size("-1", &v));
  CHECK(!parse_chunk_size("0x10", &v));
  CHECK_EQ(v, 99u);  // untouched by a refusal
  CHECK_EQ(hexval('0'), 0);
  CHECK_EQ(hexval('f'), 15);
  CHECK_EQ(hexval('F'), 15);
  CHECK_EQ(hexval('g'), -1);
}

void test_chunked_body() {
  std::string s;
  {
    Pair p;
    p.put("3\r\nabc\r\n4;x=1\r\ndefg\r\n0\r\nTrailer: v\r\n\r\nNEXT\n");
    CHECK(p.w.chunked_body(s = "") == Wire::Body::kOk);  // two chunks and a trailer
    CHECK_EQ(s, "abcdefg");
    CHECK(p.w.line(s));
    CHECK_EQ(s, "NEXT");  // nothing past the body was eaten
  }
  {
    Pair p;
    p.put_parts({"5\r\nhe", "llo\r", "\n0\r\n\r\n"});
    CHECK(p.w.chunked_body(s = "") == Wire::Body::kOk);  // data straddles writes
    CHECK_EQ(s, "hello");
  }
  {
    // No CRLF after the data: the line that is read in its place takes the
    // "0", and the empty line after it is no chunk size.
    Pair p;
    p.put("3\r\nabc0\r\n\r\n");
    CHECK(p.w.chunked_body(s = "") == Wire::Body::kMalformed);
  }
  {
    Pair p;
    p.put("zz\r\n");
    CHECK(p.w.chunked_body(s = "") == Wire::Body::kMalformed);
  }
  {
    Pair p;
    p.put("3\r\nabc\r\n3\r\ndef\r\n0\r\n\r\n");
    CHECK(p.w.chunked_body(s = "", 6) == Wire::Body::kOk);  // exactly the cap
    CHECK_EQ(s, "abcdef");
  }
  {
    Pair p;
    p.put("3\r\nabc\r\n3\r\ndef\r\n0\r\n\r\n");
    CHECK(p.w.chunked_body(s = "", 5) == Wire::Body::kTooLarge);  // the second chunk passes the cap
    CHECK_EQ(s, "abc");
  }
  {
    // The largest size a chunk line can carry, after three bytes: it is held
    // against the allowance left (cap - received, which cannot wrap), never
    // added to what was received. The server once read such a body forever.
    Pair p;
    p.put("3\r\nabc\r\nfffffffffffffff\r\n");
    CHECK(p.w.chunked_body(s = "", size_t{256} << 20) == Wire::Body::kTooLarge);
    CHECK_EQ(s, "abc");
  }
  {
    Pair p;
    p.put_parts({"5\r\nab"}, /*then_eof=*/true);
    CHECK(p.w.chunked_body(s = "") == Wire::Body::kClosed);  // EOF inside a chunk
  }
}

void test_header_scanner() {
  std::string name;
  std::string_view value;
  Framing f;
  CHECK(scan_header("CoNtEnT-LeNgTh: 42   ", false, name, value));  // mixed case, trailing spaces
  CHECK_EQ(name, "content-length");
  CHECK_EQ(value, "42");
  CHECK(f.note(name, value));
  CHECK_EQ(f.content_length, 42);
  CHECK(scan_header("X-Padded: \t  a b \t ", false, name, value));  // spaces and tabs
  CHECK_EQ(name, "x-padded");
  CHECK_EQ(value, "a b");
  CHECK(!f.note(name, value));  // not a framing header: the caller's
  CHECK(scan_header("Transfer-Encoding: Chunked", false, name, value));
  CHECK(f.note(name, value));
  CHECK(f.chunked);
  CHECK(scan_header("Connection: Keep-Alive, Upgrade", false, name, value));
  CHECK(f.note(name, value));
  CHECK(f.keep_alive && !f.close);
  CHECK(scan_header("Connection: Upgrade, Close", false, name, value));
  CHECK(f.note(name, value));
  CHECK(f.close && !f.keep_alive);
  CHECK(scan_header("connection: keep-alive", false, name, value));
  CHECK(f.note(name, value));
  CHECK(f.close && f.keep_alive);  // close once said stays; the last word is keep-alive
  CHECK(!scan_header("no colon here", false, name, value));
  // White space before the colon: the server's reading drops it, the client's keeps it.
  CHECK(scan_header("Content-Length : 7", true, name, value));
  CHECK_EQ(name, "content-length");
  CHECK(scan_header("Content-Length : 7", false, name, value));
  CHECK_EQ(name, "content-length ");
  CHECK_EQ(value, "7");
}

void test_headers_over_the_wire() {
  Pair p;
  p.put(
      "Content-Type: application/json\r\ngarbage without a colon\r\nCONTENT-LENGTH:\t5 \r\n"
      "Authorization:Bearer t\r\n\r\nhello");
  Framing f;
  std::vector<std::pair<std::string, std::string>> others;
  auto keep = [&](std::string_view n, std::string_view v) { others.emplace_back(n, v); };
  CHECK(p.w.headers(f, true, 200, keep) == Wire::Head::kOk);
  CHECK_EQ(f.content_length, 5);
  CHECK(!f.chunked && !f.close && !f.keep_alive);
  CHECK_EQ(others.size(), 2u);
  CHECK(others.size() == 2 && others[0].first == "content-type" && others[0].second == "application/json");
  CHECK(others.size() == 2 && others[1].first == "authorization" && others[1].second == "Bearer t");
  std::string s;
  CHECK(p.w.exact(5, s));
  CHECK_EQ(s, "hello");

  Pair q;  // three lines where two are allowed; then EOF before the empty line
  q.put("a: 1\r\nb: 2\r\nc: 3\r\nd: 4\r\n");
  q.eof();
  Framing g;
  others.clear();
  CHECK(q.w.headers(g, true, 2, keep) == Wire::Head::kTooMany);
  CHECK_EQ(others.size(), 3u);  // lines 0..max_lines are read, the next one is refused
  CHECK(q.w.headers(g, true, 200, keep) == Wire::Head::kClosed);
}

void test_send_all() {
  std::string payload(8u << 20, '\0');  // far above any socket buffer
  for (size_t i = 0; i < payload.size(); ++i) payload[i] = static_cast<char>((i * 2654435761u) >> 24);
  Pair p;
  std::string got;
  std::thread reader([&] {  // a slow reader: small reads
    char buf[4096];
    for (ssize_t n; got.size() < payload.size() && (n = ::recv(p.peer, buf, sizeof buf, 0)) > 0;)
      got.append(buf, static_cast<size_t>(n));
  });
  CHECK(p.w.send_all(payload));
  reader.join();
  CHECK(got == payload);
  CHECK(p.w.send_all(""));  // nothing to write is no error

  ::close(p.peer);
  p.peer = -1;
  p.w.begin_request();
  CHECK(!p.w.send_all(payload));  // EPIPE, as a result and not as SIGPIPE
  CHECK(p.w.failed_stale());  // a reset with nothing received
}

void test_failure_record() {
  std::string s;
  {  // the peer closed while the connection was idle: nothing came back
    Pair p;
    p.eof();
    p.w.begin_request();
    CHECK(!p.w.failed_stale());
    CHECK(!p.w.line(s));
    CHECK(p.w.failed_stale());
  }
  {  // part of a response arrived before the EOF: the request was delivered
    Pair p;
    p.put("HTTP/1.1 2");
    p.eof();
    p.w.begin_request();
    CHECK(!p.w.line(s));
    CHECK(!p.w.failed_stale());
  }
  {  // begin_request() starts the count again
    Pair p;
    p.put("one\n");
    CHECK(p.w.line(s));
    p.eof();
    p.w.begin_request();
    CHECK(!p.w.line(s));
    CHECK(p.w.failed_stale());
  }
  {  // peer_closed() sees the close without consuming anything
    Pair p;
    CHECK(!p.w.peer_closed());
    p.put("x");
    CHECK(!p.w.peer_closed());
    ::close(p.peer);
    p.peer = -1;
    CHECK(p.w.peer_closed());
  }
}

}  // namespace

int main() {
  test_line();
  test_line_split_across_writes();
  test_line_limit();
  test_exact();
  test_small_scratch();
  test_buffer_compaction();
  test_chunk_sizes();
  test_chunked_body();
  test_header_scanner();
  test_headers_over_the_wire();
  test_send_all();
  test_failure_record();
  std::printf("%d checks, %d failed\n", g_checks, g_failed);
  return g_failed == 0 ? 0 : 1;
}
