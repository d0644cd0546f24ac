// Counting replacement of the global operator new / delete: calls and bytes per
// thread, reported under the thread's name. Linked only into the
// `build_ext --stress-count` flavour of the stress driver, never into the
// extension. The counts are deterministic for a given input (they are not
// times): they measure what a scheduling cycle allocates and where what it
// allocates is freed.
//
//   XSCHED_ALLOC_STACKS=1     also collect call stacks on one thread
//   XSCHED_ALLOC_THREAD=NAME  that thread (default xs-sched)
//
// Stacks are printed as `exe+0xOFFSET` frames for addr2line -f -C -i -e EXE.
#include "tools/alloc_count.h"

#include <dlfcn.h>
#include <execinfo.h>
#include <sys/prctl.h>

#include <algorithm>
#include <atomic>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <new>

namespace {

struct Slot {
  std::atomic<uint64_t> news{0}, bytes{0}, dels{0};
  char name[16] = {0};
  uint32_t since_name = 0;
};

constexpr int kSlots = 1024;
Slot g_slots[kSlots];
std::atomic<int> g_next{0};
std::atomic<bool> g_on{false};
thread_local Slot* tl_slot = nullptr;

// Stacks: open addressing, written by the one named thread only.
constexpr int kDepth = 14, kSkip = 2, kTable = 1 << 14;
struct StackRow {
  uint64_t hash = 0, count = 0, bytes = 0;
  int depth = 0;
  void* pcs[kDepth];
};
StackRow* g_stacks = nullptr;
char g_stack_thread[16] = "xs-sched";
thread_local bool tl_in_hook = false;

inline Slot* slot() {
  Slot* s = tl_slot;
  if (!s) {
    int i = g_next.fetch_add(1, std::memory_order_relaxed);
    s = &g_slots[i < kSlots ? i : kSlots - 1];
    tl_slot = s;
    s->since_name = 0;
  }
  // Threads name themselves after they start: refresh now and then.
  if ((s->since_name++ & 63) == 0) prctl(PR_GET_NAME, s->name, 0, 0, 0);
  return s;
}

void note_stack(Slot* s, size_t n) {
  if (tl_in_hook || std::strncmp(s->name, g_stack_thread, sizeof s->name) != 0) return;
  tl_in_hook = true;
  void* pcs[kDepth + kSkip];
  int d = backtrace(pcs, kDepth + kSkip);
  uint64_t h = 1469598103934665603ull;
  for (int i = kSkip; i < d; ++i) h = (h ^ reinterpret_cast<uintptr_t>(pcs[i])) * 1099511628211ull;
  if (h == 0) h = 1;
  for (int probe = 0; probe < kTable; ++probe) {
    StackRow& r = g_stacks[(h + probe) & (kTable - 1)];
    if (r.hash == 0) {
      r.hash = h;
      r.depth = std::max(0, d - kSkip);
      std::memcpy(r.pcs, pcs + kSkip, sizeof(void*) * r.depth);
    }
    if (r.hash == h) {
      ++r.count;
      r.bytes += n;
      break;
    }
  }
  tl_in_hook = false;
}

inline void* counted_alloc(size_t n, size_t align) {
  void* p = align > alignof(std::max_align_t) ? std::aligned_alloc(align, (n + align - 1) / align * align)
                                              : std::malloc(n ? n : 1);
  if (g_on.load(std::memory_order_relaxed)) {
    Slot* s = slot();
    s->news.fetch_add(1, std::memory_order_relaxed);
    s->bytes.fetch_add(n, std::memory_order_relaxed);
    if (g_stacks) note_stack(s, n);
  }
  return p;
}

inline void counted_free(void* p) {
  if (!p) return;
  if (g_on.load(std::memory_order_relaxed)) slot()->dels.fetch_add(1, std::memory_order_relaxed);
  std::free(p);
}

}  // namespace

// Exported although the build hides symbols by default: calls from inside
// libstdc++ (std::string's out-of-line members) must land here too.
#define XS_EXPORT __attribute__((visibility("default")))

XS_EXPORT void* operator new(size_t n) {
  void* p = counted_alloc(n, 0);
  if (!p) throw std::bad_alloc();
  return p;
}
XS_EXPORT void* operator new[](size_t n) {
  void* p = counted_alloc(n, 0);
  if (!p) throw std::bad_alloc();
  return p;
}
XS_EXPORT void* operator new(size_t n, const std::nothrow_t&) noexcept { return counted_alloc(n, 0); }
XS_EXPORT void* operator new[](size_t n, const std::nothrow_t&) noexcept { return counted_alloc(n, 0); }
XS_EXPORT void* operator new(size_t n, std::align_val_t a) {
  void* p = counted_alloc(n, static_cast<size_t>(a));
  if (!p) throw std::bad_alloc();
  return p;
}
XS_EXPORT void* operator new[](size_t n, std::align_val_t a) {
  void* p = counted_alloc(n, static_cast<size_t>(a));
  if (!p) throw std::bad_alloc();
  return p;
}
XS_EXPORT void operator delete(void* p) noexcept { counted_free(p); }
XS_EXPORT void operator delete[](void* p) noexcept { counted_free(p); }
XS_EXPORT void operator delete(void* p, size_t) noexcept { counted_free(p); }
XS_EXPORT void operator delete[](void* p, size_t) noexcept { counted_free(p); }
XS_EXPORT void operator delete(void* p, std::align_val_t) noexcept { counted_free(p); }
XS_EXPORT void operator delete[](void* p, std::align_val_t) noexcept { counted_free(p); }
XS_EXPORT void operator delete(void* p, size_t, std::align_val_t) noexcept { counted_free(p); }
XS_EXPORT void operator delete[](void* p, size_t, std::align_val_t) noexcept { counted_free(p); }
XS_EXPORT void operator delete(void* p, const std::nothrow_t&) noexcept { counted_free(p); }
XS_EXPORT void operator delete[](void* p, const std::nothrow_t&) noexcept { counted_free(p); }

namespace xsched::alloc_count {

void enable(bool on) {
  if (on && !g_stacks && std::getenv("XSCHED_ALLOC_STACKS") && std::atoi(std::getenv("XSCHED_ALLOC_STACKS")) > 0) {
    if (const char* t = std::getenv("XSCHED_ALLOC_THREAD")) std::snprintf(g_stack_thread, sizeof g_stack_thread, "%s", t);
    // backtrace()'s first call loads libgcc and allocates: do it before counting.
    void* warm[4];
    backtrace(warm, 4);
    g_stacks = static_cast<StackRow*>(std::calloc(kTable, sizeof(StackRow)));
  }
  g_on.store(on, std::memory_order_relaxed);
}

void report(std::FILE* out, uint64_t bound_pods) {
  const bool was_on = g_on.exchange(false);
  struct Sum {
    char name[16];
    uint64_t news = 0, bytes = 0, dels = 0;
    int threads = 0;
  };
  static Sum sums[kSlots];
  int nsum = 0;
  int n = std::min(g_next.load(), kSlots);
  for (int i = 0; i < n; ++i) {
    Slot& s = g_slots[i];
    uint64_t a = s.news.load(), d = s.dels.load();
    if (a == 0 && d == 0) continue;
    int k = 0;
    while (k < nsum && std::strncmp(sums[k].name, s.name, sizeof s.name) != 0) ++k;
    if (k == nsum) {
      std::memcpy(sums[k].name, s.name, sizeof s.name);
      sums[k].news = sums[k].bytes = sums[k].dels = 0;
      sums[k].threads = 0;
      ++nsum;
    }
    sums[k].news += a;
    sums[k].bytes += s.bytes.load();
    sums[k].dels += d;
    ++sums[k].threads;
  }
  std::sort(sums, sums + nsum, [](const Sum& a, const Sum& b) { return a.news + a.dels > b.news + b.dels; });
  const double pods = bound_pods ? static_cast<double>(bound_pods) : 1.0;
  std::fprintf(out, "alloc_count: %llu bound pods counted\n", static_cast<unsigned long long>(bound_pods));
  uint64_t sched_news = 0;
  for (int k = 0; k < nsum; ++k) {
    const Sum& s = sums[k];
    if (std::strcmp(s.name, "xs-sched") == 0) sched_news += s.news;
    std::fprintf(out,
                 "alloc_count thread=%s threads=%d new=%llu bytes=%llu delete=%llu new_per_pod=%.2f bytes_per_pod=%.0f "
                 "delete_per_pod=%.2f\n",
                 s.name, s.threads, static_cast<unsigned long long>(s.news), static_cast<unsigned long long>(s.bytes),
                 static_cast<unsigned long long>(s.dels), s.news / pods, s.bytes / pods, s.dels / pods);
  }
  std::fprintf(out, "new_per_bound_pod=%.2f\n", sched_news / pods);
  if (g_stacks) {
    static StackRow* rows[kTable];
    int nr = 0;
    for (int i = 0; i < kTable; ++i)
      if (g_stacks[i].hash) rows[nr++] = &g_stacks[i];
    std::sort(rows, rows + nr, [](const StackRow* a, const StackRow* b) { return a->count > b->count; });
    std::fprintf(out, "alloc_stacks thread=%s distinct=%d\n", g_stack_thread, nr);
    for (int i = 0; i < nr && i < 80; ++i) {
      const StackRow& r = *rows[i];
      std::fprintf(out, "stack count=%llu per_pod=%.3f avg_bytes=%.0f :", static_cast<unsigned long long>(r.count),
                   r.count / pods, r.count ? double(r.bytes) / r.count : 0.0);
      for (int f = 0; f < r.depth; ++f) {
        Dl_info info;
        uintptr_t pc = reinterpret_cast<uintptr_t>(r.pcs[f]);
        if (dladdr(r.pcs[f], &info) && info.dli_fbase) {
          const char* base = info.dli_fname ? std::strrchr(info.dli_fname, '/') : nullptr;
          std::fprintf(out, " %s+0x%llx", base ? base + 1 : (info.dli_fname ? info.dli_fname : "?"),
                       static_cast<unsigned long long>(pc - reinterpret_cast<uintptr_t>(info.dli_fbase)));
        } else {
          std::fprintf(out, " ?+0x%llx", static_cast<unsigned long long>(pc));
        }
      }
      std::fprintf(out, "\n");
    }
  }
  g_on.store(was_on);
}

}  // namespace xsched::alloc_count
