#include "scheduler/executor.h"

#include "common/clock.h"
#include "common/parallel.h"

#include <algorithm>
#include <cstdlib>

namespace xsched {

bool Executor::try_pop(std::function<void()>& fn) {
  if (q_.empty()) return false;
  fn = std::move(q_.front());
  q_.pop_front();
  queued_.fetch_sub(1, std::memory_order_relaxed);
  busy_.fetch_add(1);
  return true;
}

Executor::Executor(int threads) {
  if (const char* e = std::getenv("XSCHED_BIND_SPIN_NS")) spin_ns_ = std::max<int64_t>(0, std::atoll(e));
  base_ = std::max(1, threads);
  std::lock_guard<AdaptiveMutex> g(mu_);
  for (int i = 0; i < base_; ++i) spawn_locked();
}

void Executor::spawn_locked() {
  threads_.emplace_back([this] {
    name_this_thread("xs-bind");
    bool spin = false;  // just finished a task: poll before sleeping
    for (;;) {
      std::function<void()> fn;
      if (spin && spin_ns_ > 0) {
        if (spinners_.fetch_add(1) < kMaxSpinners) {
          const int64_t until = Parallelizer::now_ns() + spin_ns_;
          while (queued_.load(std::memory_order_relaxed) == 0 && Parallelizer::now_ns() < until)
            __builtin_ia32_pause();
        }
        // Leave the spinner set before the locked check below: a submit
        // that still saw this spinner finds its task taken here.
        spinners_.fetch_sub(1);
      }
      bool chain = false;
      {
        std::unique_lock<AdaptiveMutex> lk(mu_);
        if (!try_pop(fn)) {
          ++waiters_;
          while (!stop_ && q_.empty()) {
            cv_.wait(lk);
            if (wakes_ > 0) --wakes_;  // every wake-up consumes one, taken task or not
          }
          --waiters_;
          if (!try_pop(fn)) return;  // stop_ and drained
        }
        // Chain wake-up: a burst submitted at once (a gang's Allows) costs
        // the submitter one futex wake; each woken worker wakes the next.
        if (!q_.empty() && waiters_ > 0 && wakes_ == 0 && queued_.load(std::memory_order_relaxed) > spinners_.load()) {
          ++wakes_;
          chain = true;
        }
      }
      if (chain) cv_.notify_one();
      fn();
      busy_.fetch_sub(1);
      spin = true;
    }
  });
}

void Executor::enter_blocking() {
  std::lock_guard<AdaptiveMutex> g(mu_);
  ++blocked_;
  // Keep `base_` workers able to run tasks (Go's runtime hands a P to a new
  // M when a goroutine blocks in a syscall): the pool grows to the
  // high-water mark of concurrently blocked tasks, capped.
  if (!stop_ && static_cast<int>(threads_.size()) - blocked_ < base_ && threads_.size() < kMaxThreads) spawn_locked();
}

void Executor::exit_blocking() {
  std::lock_guard<AdaptiveMutex> g(mu_);
  --blocked_;
}

size_t Executor::threads() const {
  std::lock_guard<AdaptiveMutex> g(mu_);
  return threads_.size();
}

Executor::~Executor() { stop(); }

namespace {
thread_local Executor::Batch* tl_batch = nullptr;
}  // namespace

// A batch per scheduling cycle: its (emptied) task buffer is kept per thread
// for the next one instead of growing a new vector every cycle.
thread_local std::vector<std::function<void()>> tl_batch_spare;

Executor::Batch::Batch(Executor& e) : e_(e), prev_(tl_batch) {
  tl_batch = this;
  fns_.swap(tl_batch_spare);
}

Executor::Batch::~Batch() {
  tl_batch = prev_;
  struct KeepBuffer {
    std::vector<std::function<void()>>& v;
    ~KeepBuffer() {
      v.clear();
      if (v.capacity() > tl_batch_spare.capacity()) v.swap(tl_batch_spare);
    }
  } keep{fns_};
  if (fns_.empty()) return;
  bool wake = false;
  {
    std::lock_guard<AdaptiveMutex> g(e_.mu_);
    for (auto& fn : fns_) e_.q_.push_back(std::move(fn));
    e_.queued_.fetch_add(static_cast<int>(fns_.size()), std::memory_order_relaxed);
    if (e_.waiters_ > 0 && e_.wakes_ == 0 && e_.queued_.load(std::memory_order_relaxed) > e_.spinners_.load()) {
      ++e_.wakes_;
      wake = true;
    }
  }
  if (wake) e_.cv_.notify_one();
}

void Executor::submit(std::function<void()> fn) {
  for (Batch* b = tl_batch; b; b = b->prev_)
    if (&b->e_ == this) {
      b->fns_.push_back(std::move(fn));
      return;
    }
  bool wake = false;
  {
    std::lock_guard<AdaptiveMutex> g(mu_);
    q_.push_back(std::move(fn));
    queued_.fetch_add(1, std::memory_order_relaxed);
    // Wake a sleeper unless a spinning worker is free for this task or a
    // wake-up is already on its way (that worker wakes the next one).
    if (waiters_ > 0 && wakes_ == 0 && queued_.load(std::memory_order_relaxed) > spinners_.load()) {
      ++wakes_;
      wake = true;
    }
  }
  if (wake) cv_.notify_one();
}

void Executor::stop() {
  {
    std::lock_guard<AdaptiveMutex> g(mu_);
    if (stop_) return;
    stop_ = true;
  }
  cv_.notify_all();
  std::vector<std::thread> ts;
  {
    std::lock_guard<AdaptiveMutex> g(mu_);
    ts.swap(threads_);  // no spawn after stop_
  }
  for (auto& t : ts) t.join();
}

size_t Executor::pending() const {
  std::lock_guard<AdaptiveMutex> g(mu_);
  return q_.size() + static_cast<size_t>(busy_.load());
}

}  // namespace xsched
