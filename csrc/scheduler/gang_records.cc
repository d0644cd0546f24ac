// Gang records (enqueue, admit, bound, placement) and group-denial census.
#include "scheduler/scheduler.h"

#include <algorithm>

namespace xsched {

namespace {
// "ns/group" in a per-thread buffer (the name a denial is recorded under).
const std::string& gang_key(const Pod& p) {
  thread_local std::string k;
  k.assign(p.ns());
  k.push_back('/');
  k.append(p.pod_group);
  return k;
}
}  // namespace

// A gang's open record lives in its lister entry (scheduler/gang.h), reached
// through the pod: these run once per pod on the informer, the scheduling
// thread and every binder, under that gang's lock only. A pod whose entry is
// retired, or that has none, finds the group's current entry by name.
template <typename F>
void Scheduler::with_gang_record(const Pod& p, bool open, GangRecord* done, F&& fn) {
  if (p.pod_group.empty()) return;
  if (p.gang && p.gang->with_record(open, done, fn)) return;
  if (GangPtr e = informers_->gang_by_name(p)) e->with_record(open, done, fn);
}

void Scheduler::note_gang_enqueue(const Pod& p, int64_t t) {
  with_gang_record(p, true, nullptr, [&](const PodGroupPtr&, GangRecord* r, bool fresh) {
    if (fresh) r->first_enqueue_us = t;
    return false;
  });
}

void Scheduler::note_gang_event(const Pod& p, bool bound) {
  if (p.pod_group.empty()) return;
  GangRecord done;
  bool finished = false;
  int need = 0;
  with_gang_record(p, false, &done, [&](const PodGroupPtr& pg, GangRecord* rp, bool) {
    if (!pg || !rp) return false;
    GangRecord& r = *rp;
    need = std::max(1, pg->min_member);
    r.size = need;
    int64_t now = clock_->now_us();
    if (!bound) {
      if (r.admit_us == 0) r.admit_us = now;
      return false;
    }
    const uint64_t nh = std::hash<std::string_view>{}(std::string_view(p.node_name));
    if (std::find(r.nodes.begin(), r.nodes.end(), nh) == r.nodes.end()) r.nodes.push_back(nh);
    if (++r.bound < need) return false;
    r.bound_us = now;
    if (r.admit_us == 0) r.admit_us = now;
    finished = true;
    return true;
  });
  if (!finished) return;
  // Once per gang: the finished record moves to the collected ones.
  std::lock_guard<std::mutex> g(stats_mu_);
  // The per-size histogram, looked up once per size and metrics epoch.
  const uint64_t epoch = metrics_->epoch();
  if (gang_hist_epoch_ != epoch) {
    gang_hist_.clear();
    gang_hist_epoch_ = epoch;
  }
  Histogram*& hist = gang_hist_[need];
  if (!hist) hist = &metrics_->histogram("xsched_gang_admit_seconds", "size=\"" + std::to_string(need) + "\"");
  hist->observe(static_cast<double>(done.bound_us - done.first_enqueue_us) / 1e6);
  gang_done_.push_back(std::move(done));
}

void Scheduler::note_gang_planned(const Pod& p, bool hostable) {
  with_gang_record(p, false, nullptr, [&](const PodGroupPtr&, GangRecord* r, bool) {
    if (r) r->hostable = hostable ? 1 : 0;
    return false;
  });
}

// Why was a gang denied? The cache's view (free SPX GPUs, those held by
// assumed pods of gangs still waiting at Permit) against the store's at the
// same moment (bound pods only): separates a stale cache (deletions not yet
// observed) from GPUs held by other waiting gangs and from a real shortage.
void Scheduler::note_gang_denied(const Pod& p, const char* why) {
  {
    std::lock_guard<std::mutex> g(stats_mu_);
    ++gang_denials_total_;
    if (gang_denials_.size() >= kMaxGangDenials) return;
  }
  GangDenial d;
  d.pg = gang_key(p);
  d.why = why;
  d.t_us = clock_->now_us();
  auto pg = informers_->gang_pod_group(p);
  d.min_member = pg ? pg->min_member : 0;
  d.assigned = cache_->assigned_in_group(p.pg_key);
  d.waiting_at_permit = static_cast<int>(permit_waiting());
  d.in_binding = std::max(0, inflight_.load() - d.waiting_at_permit);
  d.need_gpus = p.gpu_demand.kind == GpuDemand::Gpu ? p.gpu_demand.amount : 0;
  std::unordered_map<std::string, int> spx;
  for (const auto& r : cache_->gpu_census()) {
    spx[r.node] = r.spx;
    d.cache_free += r.free_whole;
    d.cache_max_node_free = std::max(d.cache_max_node_free, r.free_whole);
    d.assumed_held += r.assumed_whole;
  }
  if (store_ && opts_.gang_denial_census) {
    std::unordered_map<std::string, int> used;
    const std::string& gpu = gpu_names_->gpu;
    for (const auto& po : store_->list("pods", "")) {
      const Json& spec = (*po)["spec"];
      const std::string& node = spec["nodeName"].as_string();
      if (node.empty() || (*po)["metadata"].get("deletionTimestamp")) continue;
      int64_t n = 0;
      for (const auto& c : spec["containers"].items()) {
        const Json& lim = c["resources"]["limits"][gpu];
        if (lim.is_string()) n += Quantity::parse(lim.as_string()).value();
        else if (lim.is_number()) n += lim.as_int();
      }
      if (n) used[node] += static_cast<int>(n);
    }
    d.store_free = 0;
    for (const auto& [node, cap] : spx) {
      auto u = used.find(node);
      int f = std::max(0, cap - (u == used.end() ? 0 : u->second));
      d.store_free += f;
      d.store_max_node_free = std::max(d.store_max_node_free, f);
    }
  }
  // The gang still needed (min_member - assigned) more whole GPUs. GPUs free
  // in the store are either truly taken by pods in flight (waiting at Permit
  // or being bound: not yet bound in the store) or seen as used only by a
  // cache that has not observed the deletions yet.
  // Without the store census the cache alone separates GPUs held by pods in
  // flight (assumed, not yet bound) from a shortage of bound pods.
  const int64_t missing = d.need_gpus * std::max(0, d.min_member - d.assigned);
  const int64_t in_flight = d.need_gpus * (d.waiting_at_permit + d.in_binding);  // GPUs, not pods
  if (d.need_gpus == 0) d.cause = "not_whole_gpu";
  else if (d.store_free < 0)
    d.cause = d.cache_free >= missing ? "placement"
              : d.cache_free + d.assumed_held >= missing ? "held_by_gangs_in_flight"
                                                         : "capacity";
  else if (d.store_free < missing) d.cause = "capacity";
  else if (d.store_free - in_flight < missing) d.cause = "held_by_gangs_in_flight";
  else if (d.cache_free < missing) d.cause = "stale_cache";
  else d.cause = "placement";
  std::lock_guard<std::mutex> g(stats_mu_);
  if (gang_denials_.size() < kMaxGangDenials) gang_denials_.push_back(std::move(d));
}

std::vector<GangRecord> Scheduler::gang_records(bool clear) {
  std::lock_guard<std::mutex> g(stats_mu_);
  std::vector<GangRecord> out(gang_done_.begin(), gang_done_.end());
  if (clear) gang_done_.clear();
  return out;
}

uint64_t Scheduler::gang_parks(bool clear) {
  return clear ? gang_parks_total_.exchange(0) : gang_parks_total_.load();
}

std::vector<GangDenial> Scheduler::gang_denials(bool clear, uint64_t* total) {
  std::lock_guard<std::mutex> g(stats_mu_);
  std::vector<GangDenial> out = gang_denials_;
  if (total) *total = gang_denials_total_;
  if (clear) {
    gang_denials_.clear();
    gang_denials_total_ = 0;
  }
  return out;
}

}  // namespace xsched
