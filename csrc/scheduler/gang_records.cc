// Gang records (enqueue, admit, bound, placement) and group-denial census.
#include "scheduler/scheduler.h"

#include <algorithm>

namespace xsched {

namespace {
// "ns/group" in a per-thread buffer: gang bookkeeping runs per pod and a
// lookup must not allocate a key string.
const std::string& gang_key(const Pod& p) {
  thread_local std::string k;
  k.assign(p.ns());
  k.push_back('/');
  k.append(p.pod_group);
  return k;
}
}  // namespace

void Scheduler::note_gang_enqueue(const Pod& p, int64_t t) {
  if (p.pod_group.empty()) return;
  const std::string& key = gang_key(p);
  std::lock_guard<std::mutex> g(stats_mu_);
  auto it = gangs_.find(key);
  if (it != gangs_.end()) return;
  GangRecord& r = gangs_[key];
  r.pg = key;
  r.first_enqueue_us = t;
}

void Scheduler::note_gang_event(const Pod& p, bool bound) {
  if (p.pod_group.empty()) return;
  auto pg = informers_->pod_group_of(p);
  if (!pg) return;
  int need = std::max(1, pg->min_member);
  const std::string& key = gang_key(p);
  std::lock_guard<std::mutex> g(stats_mu_);
  auto it = gangs_.find(key);
  if (it == gangs_.end()) return;
  GangRecord& r = it->second;
  r.size = need;
  int64_t now = clock_->now_us();
  if (!bound) {
    if (r.admit_us == 0) r.admit_us = now;
    return;
  }
  const uint64_t nh = std::hash<std::string_view>{}(std::string_view(p.node_name));
  if (std::find(r.nodes.begin(), r.nodes.end(), nh) == r.nodes.end()) r.nodes.push_back(nh);
  if (++r.bound < need) return;
  r.bound_us = now;
  if (r.admit_us == 0) r.admit_us = now;
  // The per-size histogram, looked up once per size and metrics epoch.
  const uint64_t epoch = metrics_->epoch();
  if (gang_hist_epoch_ != epoch) {
    gang_hist_.clear();
    gang_hist_epoch_ = epoch;
  }
  Histogram*& hist = gang_hist_[need];
  if (!hist) hist = &metrics_->histogram("xsched_gang_admit_seconds", "size=\"" + std::to_string(need) + "\"");
  hist->observe(static_cast<double>(r.bound_us - r.first_enqueue_us) / 1e6);
  gang_done_.push_back(r);
  gangs_.erase(it);
}

void Scheduler::note_gang_planned(const Pod& p, bool hostable) {
  if (p.pod_group.empty()) return;
  const std::string& key = gang_key(p);
  std::lock_guard<std::mutex> g(stats_mu_);
  auto it = gangs_.find(key);
  if (it != gangs_.end()) it->second.hostable = hostable ? 1 : 0;
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
  auto pg = informers_->pod_group_of(p);
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
