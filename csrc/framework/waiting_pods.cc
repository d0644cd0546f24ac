#include "framework/waiting_pods.h"

#include <algorithm>
#include <vector>

namespace xsched {

std::vector<std::string> WaitingPod::pending_plugins() const {
  std::lock_guard<AdaptiveMutex> g(mu_);
  std::vector<std::string> out;
  for (const Pending& e : pending_)
    if (e.plugin) out.push_back(*e.plugin);
  for (const Pending& e : more_)
    if (e.plugin) out.push_back(*e.plugin);
  std::sort(out.begin(), out.end());  // by plugin name, as the map this replaced
  return out;
}

// Entries keep their position (a timeout names its entry by index): taking
// one clears it in place.
void WaitingPod::add_pending(const std::string* plugin, uint64_t timer) {
  for (Pending& e : pending_)
    if (!e.plugin) {
      e = Pending{plugin, timer};
      ++npending_;
      return;
    }
  more_.push_back(Pending{plugin, timer});
  ++npending_;
}

uint64_t WaitingPod::take_pending(const std::string& plugin) {
  auto take = [&](Pending& e) {
    uint64_t id = e.timer;
    e = Pending{};
    --npending_;
    return id;
  };
  for (Pending& e : pending_)
    if (e.plugin && *e.plugin == plugin) return take(e);
  for (Pending& e : more_)
    if (e.plugin && *e.plugin == plugin) return take(e);
  return 0;
}

void WaitingPod::on_timeout(const std::shared_ptr<void>& self, int index) {
  WaitingPod* wp = static_cast<WaitingPod*>(self.get());
  const std::string* plugin = nullptr;
  {
    std::lock_guard<AdaptiveMutex> g(wp->mu_);
    if (index < kInlinePending) plugin = wp->pending_[index].plugin;
    else if (static_cast<size_t>(index - kInlinePending) < wp->more_.size()) plugin = wp->more_[index - kInlinePending].plugin;
  }
  if (plugin) wp->reject(*plugin, "rejected due to timeout after waiting at permit");
}

bool WaitingPod::allow(const std::string& plugin) {
  uint64_t cancel = 0;
  {
    std::lock_guard<AdaptiveMutex> g(mu_);
    if (done_) return false;
    cancel = take_pending(plugin);
    if (npending_ > 0) {
      if (cancel) owner_->timers_->cancel(cancel);
      return false;
    }
    done_ = true;
  }
  if (cancel) owner_->timers_->cancel(cancel);
  resolve(Status());
  return true;
}

bool WaitingPod::reject(const std::string& plugin, const std::string& msg) {
  uint64_t cancel[kInlinePending];
  int n = 0;
  std::vector<uint64_t> more;
  {
    std::lock_guard<AdaptiveMutex> g(mu_);
    if (done_) return false;
    done_ = true;
    for (Pending& e : pending_) {
      if (e.plugin) cancel[n++] = e.timer;
      e = Pending{};
    }
    for (Pending& e : more_)
      if (e.plugin) more.push_back(e.timer);
    more_.clear();
    npending_ = 0;
  }
  for (int i = 0; i < n; ++i) owner_->timers_->cancel(cancel[i]);
  for (uint64_t id : more) owner_->timers_->cancel(id);
  resolve(Status(Code::Unschedulable, msg).with_plugin(plugin));
  return true;
}

void WaitingPod::resolve(const Status& st) {
  owner_->remove(pod_->uid());
  Done cb;
  {
    std::lock_guard<AdaptiveMutex> g(mu_);
    cb = std::move(on_done_);
  }
  if (cb) cb(st);
}

WaitingPodPtr WaitingPods::add(const PodPtr& pod, const std::string& node, const Timeout* timeouts, size_t n,
                               WaitingPod::Done on_done) {
  auto wp = std::make_shared<WaitingPod>(pod, node, this);
  wp->on_done_ = std::move(on_done);
  wp->created_us_ = timers_->clock().now_us();
  {
    std::lock_guard<AdaptiveMutex> g(mu_);
    pods_.acquire(pod->uid()).first->second = wp;
    if (pod->pg_key) by_group_.acquire(pod->pg_key).first->second.push_back(wp);
  }
  // Arm timers after registration so a zero timeout cannot fire before the
  // pod is visible to IterateOverWaitingPods.
  std::lock_guard<AdaptiveMutex> g(wp->mu_);
  for (size_t i = 0; i < n; ++i) {
    // The entry this timer will name: the first free inline slot, else the
    // next position of more_ (add_pending fills the same one).
    int index = 0;
    while (index < WaitingPod::kInlinePending && wp->pending_[index].plugin) ++index;
    if (index == WaitingPod::kInlinePending) index += static_cast<int>(wp->more_.size());
    uint64_t id = timers_->schedule_after(timeouts[i].timeout_us, &WaitingPod::on_timeout, std::weak_ptr<WaitingPod>(wp), index);
    wp->add_pending(timeouts[i].plugin, id);
  }
  return wp;
}

WaitingPodPtr WaitingPods::get(const std::string& uid) const {
  std::lock_guard<AdaptiveMutex> g(mu_);
  auto it = pods_.find(uid);
  return it == pods_.end() ? nullptr : it->second;
}

void WaitingPods::iterate(const std::function<void(const WaitingPodPtr&)>& fn) const {
  std::vector<WaitingPodPtr> snap;
  {
    std::lock_guard<AdaptiveMutex> g(mu_);
    snap.reserve(pods_.size());
    for (const auto& kv : pods_) snap.push_back(kv.second);
  }
  for (const auto& wp : snap) fn(wp);
}

void WaitingPods::iterate_group(uint64_t pg_key, const std::function<void(const WaitingPodPtr&)>& fn) const {
  thread_local std::vector<WaitingPodPtr> scratch;
  thread_local bool scratch_busy = false;
  std::vector<WaitingPodPtr> nested;
  const bool mine = !scratch_busy;
  std::vector<WaitingPodPtr>& snap = mine ? scratch : nested;
  {
    std::lock_guard<AdaptiveMutex> g(mu_);
    auto it = by_group_.find(pg_key);
    if (it == by_group_.end()) return;
    snap.assign(it->second.begin(), it->second.end());
  }
  struct Release {
    std::vector<WaitingPodPtr>& v;
    bool mine;
    ~Release() {
      v.clear();  // the references go, the buffer stays
      if (mine) scratch_busy = false;
    }
  } release{snap, mine};
  if (mine) scratch_busy = true;
  for (const auto& wp : snap) fn(wp);
}

size_t WaitingPods::size() const {
  std::lock_guard<AdaptiveMutex> g(mu_);
  return pods_.size();
}

void WaitingPods::remove(const std::string& uid) {
  std::lock_guard<AdaptiveMutex> g(mu_);
  auto it = pods_.find(uid);
  if (it == pods_.end()) return;
  if (uint64_t key = it->second->pod()->pg_key) {
    auto git = by_group_.find(key);
    if (git != by_group_.end()) {
      auto& v = git->second;
      for (size_t i = 0; i < v.size(); ++i)
        if (v[i] == it->second) {
          v[i] = std::move(v.back());
          v.pop_back();
          break;
        }
      if (v.empty()) by_group_.release(git);
    }
  }
  pods_.release(it);
}

void WaitingPods::reject_all(const std::string& msg) {
  iterate([&](const WaitingPodPtr& wp) { wp->reject("", msg); });
}

}  // namespace xsched
