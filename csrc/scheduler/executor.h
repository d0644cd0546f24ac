// Bounded worker pool for binding cycles.
#pragma once

#include "common/adaptive_mutex.h"

#include <atomic>
#include <condition_variable>
#include <deque>
#include <functional>
#include <thread>
#include <vector>

namespace xsched {

class Executor {
 public:
  explicit Executor(int threads);
  ~Executor();
  void submit(std::function<void()> fn);
  // While a Batch is alive, submit() calls from its thread to this executor
  // are collected and handed over under one lock with one wake-up when it
  // ends (a gang's Allows fire k binding cycles from one Permit call).
  class Batch {
   public:
    explicit Batch(Executor& e);
    ~Batch();
    Batch(const Batch&) = delete;
    Batch& operator=(const Batch&) = delete;

   private:
    friend class Executor;
    Executor& e_;
    Batch* prev_;
    std::vector<std::function<void()>> fns_;
  };
  void stop();
  size_t pending() const;
  // A task about to block for a long time (VolumeBinding's PreBind waiting
  // for the PV controller) brackets the wait with these, so blocked tasks
  // never take the pool's last runnable workers (BlockingScope below).
  void enter_blocking();
  void exit_blocking();
  size_t threads() const;

 private:
  // A worker that finishes a task spins briefly on `queued_` before it
  // sleeps, and submit() skips the futex wake while a spinning worker can
  // take the task: under load the scheduling thread hands bindings over
  // without a syscall.
  static constexpr int64_t kSpinNs = 30'000;  // XSCHED_BIND_SPIN_NS overrides (A/B runs)
  static constexpr int kMaxSpinners = 2;
  int64_t spin_ns_ = kSpinNs;
  bool try_pop(std::function<void()>& fn);  // under mu_
  void spawn_locked();
  static constexpr size_t kMaxThreads = 1024;
  int base_ = 1;
  int blocked_ = 0;  // under mu_
  mutable AdaptiveMutex mu_;
  std::condition_variable_any cv_;
  std::deque<std::function<void()>> q_;
  std::vector<std::thread> threads_;
  bool stop_ = false;
  std::atomic<int> busy_{0};
  std::atomic<int> queued_{0};
  std::atomic<int> spinners_{0};
  int waiters_ = 0;  // workers in cv_.wait (under mu_)
  int wakes_ = 0;    // notifications sent and not yet consumed by a waking worker (under mu_)
};

}  // namespace xsched
