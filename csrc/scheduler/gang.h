// One lister entry per (namespace, PodGroup name): what the scheduling cycle
// and the binders ask about a gang, behind the entry's own lock.
//
// Informers owns the entries (a map by "ns/name" under its lister lock) and
// points every lister pod of the group at its entry (Pod::gang). Copies of a
// pod carry the pointer, so PreFilter, Permit, PostBind and the gang records
// reach the PodGroup, the member count, the member list and the open record
// without the lister lock, a key string or a hash lookup.
//
// An entry lives while its group has a PodGroup object or at least one lister
// pod. When both are gone the informer takes it out of the map and marks it
// retired; a later group of the same name gets a new entry. A reader that
// finds its pod's entry retired (or a pod with no entry: one parsed outside
// the lister) asks the lister by name instead (Informers::gang_*), so a
// retired entry is never believed.
#pragma once

#include <atomic>
#include <cstdint>
#include <memory>
#include <mutex>
#include <string>
#include <string_view>
#include <vector>

#include "api/types.h"
#include "common/adaptive_mutex.h"

namespace xsched {

struct GangRecord {
  std::string pg;  // ns/name
  int size = 0;
  int bound = 0;
  int64_t first_enqueue_us = 0;
  int64_t admit_us = 0;   // last member allowed at Permit
  int64_t bound_us = 0;   // last member bound
  // Placement: distinct nodes the bound members landed on (hashes of their
  // names), and whether one node could take the whole gang when its first
  // rank was planned (-1: not planned, e.g. no GPU ranks or co-location off).
  std::vector<uint64_t> nodes;
  int hostable = -1;
};

class Gang {
 public:
  Gang(std::string_view ns_, std::string_view name_)
      : key(make_key(ns_, name_)), ns(key.data(), ns_.size()), name(key.data() + ns_.size() + 1, name_.size()) {
    live_count().fetch_add(1, std::memory_order_relaxed);
  }
  ~Gang() { live_count().fetch_sub(1, std::memory_order_relaxed); }
  Gang(const Gang&) = delete;
  Gang& operator=(const Gang&) = delete;

  const std::string key;            // "ns/name"
  const std::string_view ns, name;  // its two parts

  // Entries alive in the process (tests: none is left once every pod and
  // PodGroup is gone and the pods that pointed at them are released).
  static int64_t live() { return live_count().load(std::memory_order_relaxed); }

  bool retired() const { return retired_.load(std::memory_order_acquire); }

  // Each reader returns false when the entry is retired (`out` untouched):
  // the caller then asks the lister by name.
  bool pod_group(PodGroupPtr& out) const {
    std::lock_guard<AdaptiveMutex> g(mu_);
    if (retired_.load(std::memory_order_relaxed)) return false;
    out = pg_;
    return true;
  }
  // Lister pods of the group, bound and terminating ones included.
  bool count(size_t& out) const {
    const size_t n = n_.load(std::memory_order_acquire);
    if (retired()) return false;
    out = n;
    return true;
  }
  bool members(std::vector<PodPtr>& out) const {
    std::lock_guard<AdaptiveMutex> g(mu_);
    if (retired_.load(std::memory_order_relaxed)) return false;
    out = members_;
    return true;
  }

  // The gang's open record (Scheduler::note_gang_*). `fn(pg, rec, fresh)`
  // runs under the entry's lock with the current PodGroup and the open record
  // (nullptr: none). `open`: a record is opened first when there is none
  // (`fresh` tells fn so). fn returns true when the record is finished: it
  // is then closed and moved to `*done`. False when the entry is retired (fn
  // not run).
  template <typename F>
  bool with_record(bool open, GangRecord* done, F&& fn) {
    std::lock_guard<AdaptiveMutex> g(mu_);
    if (retired_.load(std::memory_order_relaxed)) return false;
    const bool fresh = !has_rec_ && open;
    if (fresh) {
      rec_ = GangRecord{};
      rec_.pg = key;
      has_rec_ = true;
    }
    if (fn(pg_, has_rec_ ? &rec_ : nullptr, fresh) && has_rec_) {
      has_rec_ = false;
      if (done) *done = std::move(rec_);
    }
    return true;
  }

 private:
  friend class Informers;
  static std::string make_key(std::string_view ns, std::string_view name) {
    std::string k;
    k.reserve(ns.size() + 1 + name.size());
    k.append(ns).push_back('/');
    k.append(name);
    return k;
  }
  static std::atomic<int64_t>& live_count() {
    static std::atomic<int64_t> n{0};
    return n;
  }
  mutable AdaptiveMutex mu_;  // pg_, members_, the record; retired_ is set under it
  std::atomic<size_t> n_{0};  // members_.size()
  std::atomic<bool> retired_{false};
  PodGroupPtr pg_;
  std::vector<PodPtr> members_;
  bool has_rec_ = false;
  GangRecord rec_;
};
using GangPtr = std::shared_ptr<Gang>;

}  // namespace xsched
