#include "scheduler/scheduler.h"

#include "common/log.h"

#include <algorithm>
#include <chrono>
#include <stdexcept>
#include <thread>

namespace xsched {

// ------------------------------------------------------- SchedulerOptions ----
SchedulerOptions SchedulerOptions::from_json(const Json& j) {
  SchedulerOptions o;
  o.parallelism = static_cast<int>(j["parallelism"].as_int(o.parallelism));
  o.bind_workers = static_cast<int>(j["bindWorkers"].as_int(o.bind_workers));
  o.parallel_inline_below = static_cast<int>(j["parallelInlineBelow"].as_int(o.parallel_inline_below));
  o.percentage_of_nodes_to_score = static_cast<int>(j["percentageOfNodesToScore"].as_int(0));
  if (j["podInitialBackoffSeconds"].is_number())
    o.pod_initial_backoff_us = static_cast<int64_t>(j["podInitialBackoffSeconds"].as_double() * 1e6);
  if (j["podMaxBackoffSeconds"].is_number())
    o.pod_max_backoff_us = static_cast<int64_t>(j["podMaxBackoffSeconds"].as_double() * 1e6);
  if (j["assumedPodTTLSeconds"].is_number())
    o.assumed_pod_ttl_us = static_cast<int64_t>(j["assumedPodTTLSeconds"].as_double() * 1e6);
  o.metrics_sample_rate = j["metricsSampleRate"].as_double(o.metrics_sample_rate);
  o.status_updates = j["statusUpdates"].as_bool(o.status_updates);
  o.events = j["events"].as_bool(o.events);
  o.equivalence_cache = j["equivalenceCache"].as_bool(o.equivalence_cache);
  auto env_on = [](const char* var) {
    const char* v = std::getenv(var);
    return !v || std::string(v) != "0";
  };
  o.gang_window = j["gangWindow"].as_bool(env_on("XSCHED_GANG_WINDOW"));
  o.scan_memo = j["scanMemo"].as_bool(env_on("XSCHED_SCAN_MEMO"));
  o.scan_memo_verify = j["scanMemoVerify"].as_bool(false);
  o.trace = j["trace"].as_bool(false);
  o.seed = static_cast<uint64_t>(j["seed"].as_int(0));
  o.dump_on_fit_error = j["dumpOnFitError"].str_or("");
  o.gang_denial_census = j["gangDenialCensus"].as_bool(false);
  return o;
}

// ------------------------------------------------------------- Scheduler ----
namespace {
const std::vector<std::string> kBaseKinds = {"pods", "nodes", "podgroups", "elasticquotas", "noderesourcetopologies",
                                             "poddisruptionbudgets", "priorityclasses"};
}  // namespace

Scheduler::Scheduler(std::shared_ptr<ObjectStore> store, const Json& config, std::shared_ptr<Clock> clock,
                     std::shared_ptr<ApiClient> client)
    : store_(std::move(store)), clock_(clock ? std::move(clock) : std::make_shared<RealClock>()) {
  register_builtin_plugins();
  opts_ = SchedulerOptions::from_json(config["options"]);
  rng_.seed(opts_.seed ? opts_.seed : static_cast<uint64_t>(clock_->now_us()));
  tracer_.enable(opts_.trace);
  timers_ = std::make_unique<TimerService>(clock_);
  parallelizer_ = std::make_unique<Parallelizer>(opts_.parallelism, opts_.parallel_inline_below);
  if (const char* v = std::getenv("XSCHED_INFORMER_WINDOW")) informer_window_ = std::max<size_t>(1, std::atoll(v));
  // XSCHED_PARSE_POOL=1: parse informer windows on 4 helper threads. Off by
  // default: on the 16-CPU L3 domain a shard runs in, the helpers' spinning
  // made some box runs markedly slower (profiles/r4q_treeab_*).
  if (const char* v = std::getenv("XSCHED_PARSE_POOL"); v && std::string(v) == "1")
    parse_pool_ = std::make_unique<Parallelizer>(4, 32, "xs-parse");
  metrics_ = std::make_unique<Metrics>();
  cache_ = std::make_unique<SchedulerCache>(clock_, opts_.assumed_pod_ttl_us);
  informers_ = std::make_unique<Informers>();
  nominator_ = std::make_unique<Nominator>();
  if (client) {
    client_ = std::move(client);
  } else {
    auto sc = std::make_shared<StoreClient>(store_);
    sc->events_enabled = opts_.events;
    client_ = std::move(sc);
  }

  for (const auto& ej : config["extenders"].items())
    extenders_.push_back(std::make_shared<Extender>(ExtenderConfig::from_json(ej)));
  const auto& profiles = config["profiles"].items();
  if (profiles.empty()) throw std::runtime_error("scheduler config has no profiles");
  // GPU names: every profile's FlexGPU args must agree (one cache, one GPU
  // ledger per node); other schedulers in the process are unaffected.
  for (const auto& pj : profiles) {
    const Json* args = pj["pluginConfig"].get("FlexGPU");
    if (!args) continue;
    auto gn = GpuNames::from_args(*args);
    if (!gpu_names_) gpu_names_ = gn;
    else if (!(*gn == *gpu_names_))
      throw std::runtime_error("FlexGPU resource names differ between profiles of one scheduler (" +
                               gpu_names_->describe() + " vs " + gn->describe() + ")");
  }
  if (!gpu_names_) gpu_names_ = std::make_shared<GpuNames>();
  cache_->set_gpu_names(gpu_names_.get());
  for (const auto& pj : profiles) {
    ProfileConfig pc = ProfileConfig::from_json(pj);
    if (pc.percentage_of_nodes_to_score == 0) pc.percentage_of_nodes_to_score = opts_.percentage_of_nodes_to_score;
    if (by_name_.count(pc.scheduler_name)) throw std::runtime_error("duplicate profile " + pc.scheduler_name);
    waiting_.push_back(std::make_unique<WaitingPods>(timers_.get()));
    Handle h;
    h.cache = cache_.get();
    h.informers = informers_.get();
    h.client = client_.get();
    h.waiting_pods = waiting_.back().get();
    h.parallelizer = parallelizer_.get();
    h.nominator = nominator_.get();
    h.clock = clock_;
    h.timers = timers_.get();
    h.activate = [this](const std::vector<PodPtr>& pods) { queue_->activate(pods); };
    h.deactivate = [this](const std::vector<PodPtr>& pods) { queue_->deactivate(pods); };
    h.gang_denied = [this](const Pod& p, const char* why) { note_gang_denied(p, why); };
    h.gang_parked = [this](const Pod&) { gang_parks_total_.fetch_add(1, std::memory_order_relaxed); };
    gang_placements_.push_back(std::make_unique<GangPlacement>(cache_.get(), clock_));
    h.gangs = gang_placements_.back().get();
    h.gang_planned = [this](const Pod& p, bool hostable) { note_gang_planned(p, hostable); };
    h.blocking_begin = [this] {
      if (binder_) binder_->enter_blocking();
    };
    h.blocking_end = [this] {
      if (binder_) binder_->exit_blocking();
    };
    h.metrics = metrics_.get();
    h.snapshot = &snapshot_;
    h.extenders = &extenders_;
    h.gpu_names = gpu_names_.get();
    h.lookup = store_lookup_;
    frameworks_.push_back(std::make_unique<Framework>(pc, h));
    by_name_[pc.scheduler_name] = frameworks_.back().get();
  }
  // All profiles must share the queue sort (k8s validation); use the first.
  Framework* first = frameworks_.front().get();
  QueueOptions qo;
  qo.initial_backoff_us = opts_.pod_initial_backoff_us;
  qo.max_backoff_us = opts_.pod_max_backoff_us;
  queue_ = std::make_unique<SchedulingQueue>(
      [first](const QueuedPodInfo& a, const QueuedPodInfo& b) { return first->less(a, b); }, clock_, qo,
      nominator_.get());
  std::vector<std::pair<ClusterEvent, std::set<std::string>>> emap;
  for (const auto& fw : frameworks_) {
    for (const auto& pl : fw->all_plugins()) {
      for (const auto& ev : pl->events_to_register()) {
        bool merged = false;
        for (auto& [e, names] : emap)
          if (e.resource == ev.resource && e.action == ev.action) {
            names.insert(pl->name());
            merged = true;
          }
        if (!merged) emap.push_back({ev, {pl->name()}});
      }
    }
    for (const auto& k : fw->watched_kinds())
      if (std::find(plugin_kinds_.begin(), plugin_kinds_.end(), k) == plugin_kinds_.end()) plugin_kinds_.push_back(k);
  }
  queue_->set_cluster_event_map(std::move(emap));
  binder_ = std::make_unique<Executor>(opts_.bind_workers);
  status_writer_ = std::make_unique<Executor>(1);

  std::set<std::string> kinds(kBaseKinds.begin(), kBaseKinds.end());
  for (const auto& k : plugin_kinds_) kinds.insert(k);
  // Initial LIST (as informers do) then WATCH from that version.
  int64_t rv = 0;
  std::vector<WatchEvent> initial;
  for (const auto& k : kinds) {
    for (const auto& obj : store_->list(k, "", &rv)) initial.push_back(WatchEvent{EventType::Added, k, obj, nullptr, 0});
  }
  // Nodes before pods so assigned pods land on real NodeInfos.
  std::stable_sort(initial.begin(), initial.end(), [](const WatchEvent& a, const WatchEvent& b) {
    auto rank = [](const std::string& k) { return k == "nodes" ? 0 : k == "pods" ? 2 : 1; };
    return rank(a.kind) < rank(b.kind);
  });
  watcher_ = store_->watch(kinds, "", 0);
  // Events committed between list() and watch() would be lost: re-list is
  // avoided by watching from the listed version when history allows.
  store_->unwatch(watcher_);
  watcher_ = store_->watch(kinds, "", rv);
  for (const auto& ev : initial) handle_event(ev);
}

Scheduler::~Scheduler() {
  stop();
  free_frames();
}

void Scheduler::start() {
  if (running_.exchange(true)) return;
  for (auto& fw : frameworks_) fw->start();
  // Backoff expiry is checked every 100 ms (upstream: 1 s), so a retried
  // pod waits its backoff, not its backoff plus up to a second of tick phase.
  timer_ids_.push_back(timers_->every(100'000, [this] { queue_->flush_backoff_completed(); }));
  timer_ids_.push_back(timers_->every(30'000'000, [this] { queue_->flush_unschedulable_leftover(); }));
  timer_ids_.push_back(timers_->every(1'000'000, [this] { cache_->cleanup_expired_assumed_pods(); }));
  timer_ids_.push_back(timers_->every(1'000'000, [this] {
    auto c = queue_->counts();
    metrics_->set_gauge("scheduler_pending_pods", "queue=\"active\"", static_cast<double>(c.active));
    metrics_->set_gauge("scheduler_pending_pods", "queue=\"backoff\"", static_cast<double>(c.backoff));
    metrics_->set_gauge("scheduler_pending_pods", "queue=\"unschedulable\"", static_cast<double>(c.unschedulable));
    metrics_->set_gauge("scheduler_pending_pods", "queue=\"parked\"", static_cast<double>(c.parked));
    // Upstream metrics.go:102 (Goroutines, by work) and :171 (CacheSize).
    const int waiting = static_cast<int>(permit_waiting());
    const int inflight = inflight_.load();
    metrics_->set_gauge("scheduler_scheduler_goroutines", "work=\"binding\"",
                        static_cast<double>(std::max(0, inflight - waiting)));
    metrics_->set_gauge("scheduler_scheduler_goroutines", "work=\"permit\"", static_cast<double>(waiting));
    metrics_->set_gauge("scheduler_scheduler_cache_size", "type=\"assumed_pods\"", static_cast<double>(cache_->assumed_count()));
    metrics_->set_gauge("scheduler_scheduler_cache_size", "type=\"pods\"", static_cast<double>(cache_->pod_count()));
    metrics_->set_gauge("scheduler_scheduler_cache_size", "type=\"nodes\"", static_cast<double>(cache_->node_count()));
  }));
  informer_thread_ = std::thread([this] {
    name_this_thread("xs-informer");
    informer_loop();
  });
  sched_thread_ = std::thread([this] {
    name_this_thread("xs-sched");
    scheduling_loop();
  });
}

void Scheduler::stop() {
  bool was_running = running_.exchange(false);
  if (watcher_) {
    store_->unwatch(watcher_);
  }
  queue_->close();
  if (informer_thread_.joinable()) informer_thread_.join();
  if (sched_thread_.joinable()) sched_thread_.join();
  for (uint64_t id : timer_ids_) timers_->cancel(id);
  timer_ids_.clear();
  for (auto& w : waiting_) w->reject_all("scheduler stopped");
  if (binder_) binder_->stop();
  if (status_writer_) status_writer_->stop();
  if (was_running)
    for (auto& fw : frameworks_) fw->stop();
  timers_->stop();
}

Framework* Scheduler::framework_for(const std::string& scheduler_name) {
  auto it = by_name_.find(scheduler_name);
  return it == by_name_.end() ? nullptr : it->second;
}

bool Scheduler::responsible_for(const Pod& p) const { return by_name_.count(p.scheduler_name) > 0; }

Scheduler::Stats Scheduler::stats() const {
  Stats st;
  auto rd = [](const std::atomic<uint64_t>& a) { return a.load(std::memory_order_relaxed); };
  st.attempts = rd(cnt_.attempts);
  st.scheduled = rd(cnt_.scheduled);
  st.unschedulable = rd(cnt_.unschedulable);
  st.errors = rd(cnt_.errors);
  st.bound = rd(cnt_.bound);
  st.bind_failures = rd(cnt_.bind_failures);
  st.preemption_attempts = rd(cnt_.preemption_attempts);
  st.eq_filter_hits = rd(cnt_.eq_filter_hits);
  st.eq_filter_misses = rd(cnt_.eq_filter_misses);
  st.scan_memo_served = rd(cnt_.scan_memo_served);
  st.scan_memo_mismatches = rd(cnt_.scan_memo_mismatches);
  return st;
}

double Scheduler::loop_age_seconds() const {
  int64_t t = loop_tick_us_.load(std::memory_order_relaxed);
  if (!t || !running_.load()) return 0.0;
  return static_cast<double>(RealClock().now_us() - t) / 1e6;
}

void Scheduler::scheduling_loop() {
  RealClock rc;
  while (running_.load()) {
    loop_tick_us_.store(rc.now_us(), std::memory_order_relaxed);
    int64_t cycle = 0;
    auto qpi = queue_->pop(100, &cycle);
    if (!qpi) continue;
    std::lock_guard<std::mutex> g(sched_mu_);
    in_cycle_.fetch_add(1);
    schedule_cycle(qpi, cycle);
    in_cycle_.fetch_sub(1);
  }
}

bool Scheduler::schedule_one(int timeout_ms) {
  int64_t cycle = 0;
  auto qpi = queue_->pop(timeout_ms, &cycle);
  if (!qpi) return false;
  std::lock_guard<std::mutex> g(sched_mu_);
  in_cycle_.fetch_add(1);
  schedule_cycle(qpi, cycle);
  in_cycle_.fetch_sub(1);
  return true;
}

bool Scheduler::wait_idle(int timeout_ms) {
  int64_t deadline = clock_->now_us() + static_cast<int64_t>(timeout_ms) * 1000;
  RealClock rc;
  int64_t real_deadline = rc.now_us() + static_cast<int64_t>(timeout_ms) * 1000;
  for (;;) {
    auto c = queue_->counts();
    // Idle includes the FailedScheduling event writer: after an overload its
    // backlog would otherwise keep writing into the next measurement.
    if (c.active == 0 && c.backoff == 0 && permit_waiting() == 0 && inflight_.load() == 0 && in_cycle_.load() == 0 &&
        watcher_->pending() == 0 && (!status_writer_ || status_writer_->pending() == 0))
      return true;
    if (rc.now_us() > real_deadline && clock_->now_us() > deadline) return false;
    std::this_thread::sleep_for(std::chrono::microseconds(200));
  }
}

namespace {
// Polls `done` every 20 us until it holds or `timeout_us` passes (wall time,
// not clock_: a fake clock in tests does not advance). No spinning: the
// waiter shares its CPU domain with the scheduler's threads.
template <class F>
bool poll_until(F done, int64_t timeout_us) {
  const auto end = std::chrono::steady_clock::now() + std::chrono::microseconds(timeout_us);
  while (!done()) {
    if (std::chrono::steady_clock::now() > end) return false;
    std::this_thread::sleep_for(std::chrono::microseconds(20));
  }
  return true;
}
}  // namespace

bool Scheduler::wait_bound(uint64_t target, int64_t timeout_us) const {
  // Polls a counter instead of a condition variable: the binder threads
  // then pay nothing per bind.
  return poll_until([&] { return bound_total_.load(std::memory_order_acquire) >= target; }, timeout_us);
}

bool Scheduler::wait_cache_empty(int64_t timeout_us) const {
  return poll_until([&] { return cache_->pod_count() == 0; }, timeout_us);
}

}  // namespace xsched
