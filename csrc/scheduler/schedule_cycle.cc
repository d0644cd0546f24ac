// The scheduling cycle (Filter, Score, assume, Reserve, Permit), the binding
// cycle on the binder pool, and failure handling.
#include "scheduler/scheduler.h"

#include <algorithm>
#include <optional>

namespace xsched {

namespace {
void write_file(const std::string& path, const std::string& text) {
  if (FILE* f = std::fopen(path.c_str(), "w")) {
    std::fwrite(text.data(), 1, text.size(), f);
    std::fclose(f);
  }
}
}  // namespace

size_t Scheduler::select_host(const std::vector<NodeScore>& scores) {
  // Uniform among the top-scored nodes, as upstream's reservoir sampling
  // (generic_scheduler.go selectHost), with one draw per cycle instead of one
  // per tie: idle nodes of a large cluster tie by the hundred.
  int64_t best = scores[0].score;
  size_t first = 0;
  uint64_t cnt = 1;
  for (size_t i = 1; i < scores.size(); ++i) {
    if (scores[i].score > best) {
      best = scores[i].score;
      first = i;
      cnt = 1;
    } else if (scores[i].score == best) {
      ++cnt;
    }
  }
  if (cnt == 1) return first;
  uint64_t k = rng_() % cnt;
  for (size_t i = first;; ++i)
    if (scores[i].score == best && k-- == 0) return i;
}

Scheduler::CycleMetrics& Scheduler::cycle_metrics(const Framework& fw) {
  CycleMetrics& m = cycle_metrics_[&fw];
  uint64_t e = metrics_->epoch();
  if (m.epoch != e) {
    static const char* kResults[3] = {"scheduled", "unschedulable", "error"};
    m.algo = &metrics_->histogram("scheduler_scheduling_algorithm_duration_seconds", "");
    m.e2e = &metrics_->histogram("scheduler_e2e_scheduling_duration_seconds", "profile=\"" + fw.profile_name() + "\"");
    for (int i = 0; i < 3; ++i) {
      std::string labels = "profile=\"" + fw.profile_name() + "\",result=\"" + kResults[i] + "\"";
      m.attempt[i] = &metrics_->histogram("scheduler_scheduling_attempt_duration_seconds", labels);
      m.attempts[i] = &metrics_->counter_ref("scheduler_schedule_attempts_total", labels);
    }
    m.epoch = e;
  }
  return m;
}

// Activates the siblings plugins stashed in the cycle state (scheduler.go:543-548).
void Scheduler::activate_stashed(PodsToActivate& stash) {
  // The stash's buffer goes back to it afterwards (a recycled frame's stash
  // keeps its capacity); `act` is per thread: scheduling and binder threads
  // both come here.
  thread_local std::vector<PodPtr> act;
  act.clear();
  {
    std::lock_guard<std::mutex> g(stash.mu);
    act.swap(stash.pods);
  }
  if (!act.empty()) queue_->activate(act);
  act.clear();
  std::lock_guard<std::mutex> g(stash.mu);
  if (stash.pods.capacity() < act.capacity() && stash.pods.empty()) act.swap(stash.pods);
}

Scheduler::CycleFrame* Scheduler::take_frame() {
  if (!idle_frames_) {
    idle_frames_ = returned_frames_.exchange(nullptr, std::memory_order_acquire);
    idle_frame_count_ = 0;
    // Keep at most kMaxIdleFrames of them: a burst of parked gangs must not
    // pin its peak number of frames for good.
    for (CycleFrame* f = idle_frames_; f; f = f->next) {
      if (++idle_frame_count_ < kMaxIdleFrames) continue;
      CycleFrame* rest = f->next;
      f->next = nullptr;
      while (rest) {
        CycleFrame* n = rest->next;
        delete rest;
        rest = n;
      }
    }
  }
  CycleFrame* f = idle_frames_;
  if (!f) return new CycleFrame();
  idle_frames_ = f->next;
  --idle_frame_count_;
  f->next = nullptr;
  f->state.reset();
  {
    std::lock_guard<std::mutex> g(f->to_activate->mu);
    f->to_activate->pods.clear();
  }
  return f;
}

void Scheduler::keep_idle(CycleFrame* f) {
  f->task.qpi.reset();
  f->task.assumed.reset();
  if (idle_frame_count_ >= kMaxIdleFrames) {
    delete f;
    return;
  }
  f->next = idle_frames_;
  idle_frames_ = f;
  ++idle_frame_count_;
}

void Scheduler::hand_back_frame(CycleFrame* f) {
  f->task.qpi.reset();
  f->task.assumed.reset();
  CycleFrame* head = returned_frames_.load(std::memory_order_relaxed);
  do {
    f->next = head;
  } while (!returned_frames_.compare_exchange_weak(head, f, std::memory_order_release, std::memory_order_relaxed));
}

void Scheduler::free_frames() {
  for (CycleFrame* f : {idle_frames_, returned_frames_.exchange(nullptr, std::memory_order_acquire)})
    while (f) {
      CycleFrame* n = f->next;
      delete f;
      f = n;
    }
  idle_frames_ = nullptr;
  idle_frame_count_ = 0;
}

Status Scheduler::score_feasible(Framework& fw, CycleState& s, const Pod& p, const NodeList& feasible,
                                 const int* positions, EqEntry* eq, std::vector<NodeScore>& scores) {
  EqScoreCache& esc = esc_buf_;
  esc.local.clear();
  if (eq) fw.local_scorers(p, snapshot_, esc.local);
  if (esc.local.empty()) return fw.run_score(s, p, feasible, scores);
  esc.table = &eq->table;
  esc.pos = positions;
  esc.npos = feasible.size();
  esc.gen = snapshot_.gen.data();
  return fw.run_score(s, p, feasible, scores, nullptr, &esc);
}

void Scheduler::schedule_cycle(const QueuedPodInfoPtr& qpi, int64_t cycle) {
  PodPtr pod = qpi->pod;
  Framework* fw = framework_for(pod->scheduler_name);
  if (!fw) return;
  // skipPodSchedule: deleted or already assumed. The queued object is
  // usually still the lister's current one (no lookup then).
  if (informers_->lists(*pod)) {
    if (pod->terminating() || !pod->node_name.empty()) return;
  } else {
    PodPtr latest = informers_->pod(pod->ns(), pod->name());
    if (!latest || latest->uid() != pod->uid() || latest->terminating() || !latest->node_name.empty()) return;
  }

  int64_t cycle_start = clock_->now_us();
  // The cycle's frame goes back to the idle list on every return below,
  // unless the binding cycle took it over.
  struct FrameLease {
    Scheduler* self;
    CycleFrame* frame;
    ~FrameLease() {
      if (frame) self->keep_idle(frame);
    }
  } lease{this, take_frame()};
  CycleFrame* frame = lease.frame;
  CycleState* state = &frame->state;
  state->record_metrics = std::uniform_real_distribution<double>(0, 1)(rng_) < opts_.metrics_sample_rate;
  nom_changed_.clear();
  if (!nominator_->empty()) state->nominated = nominator_->view(&nom_changed_);
  // A reference of the cycle's own: the tail below still stashes and
  // activates after the binding cycle may have handed the frame back.
  std::shared_ptr<PodsToActivate> to_activate = frame->to_activate;
  state->write(kPodsToActivateKey, to_activate);
  if (tracer_.enabled())
    tracer_.record(TraceEvent{"queue_wait", pod->key(), "", qpi->timestamp_us, cycle_start - qpi->timestamp_us, 0});

  int64_t lock_wait = 0;
  int64_t snap_start = tracer_.enabled() ? clock_->now_us() : 0;
  bool already_assumed = false;
  int clones = cache_->update_snapshot(snapshot_, tracer_.enabled() ? &lock_wait : nullptr, &pod->uid(), &already_assumed);
  if (already_assumed) return;  // skipPodSchedule: assumed by an earlier cycle
  release_retired();
  refresh_nom_mark(state->nominated.get());
  cnt_.attempts.fetch_add(1, std::memory_order_relaxed);
  int64_t snap_end = tracer_.enabled() ? clock_->now_us() : 0;
  if (tracer_.enabled()) {
    tracer_.record(TraceEvent{"cycle_setup", pod->key(), "", cycle_start, snap_start - cycle_start, 0});
    tracer_.record(TraceEvent{"snapshot", pod->key(),
                              "clones=" + std::to_string(clones) + " lock_wait_us=" + std::to_string(lock_wait),
                              snap_start, snap_end - snap_start, 0});
    tracer_.record(TraceEvent{"snapshot_lock_wait", pod->key(), "", snap_start, lock_wait, 0});
  }

  Diagnosis diag;
  NodeList& feasible = feasible_buf_;
  EqEntry* eq = eq_entry(*fw, *pod);
  Status st = find_nodes_that_fit(*fw, *state, *pod, diag, feasible, eq, false, &feasible_pos_buf_);
  if (tracer_.enabled())
    tracer_.record(TraceEvent{"filter", pod->key(), std::to_string(feasible.size()), snap_end,
                              clock_->now_us() - snap_end, 0});
  std::string host;
  const NodeInfo* host_ni = nullptr;  // the snapshot's version of `host`
  if (st.is_success()) {
    if (feasible.size() == 1) {
      host_ni = feasible[0];
    } else {
      std::vector<NodeScore>& scores = scores_buf_;
      if (!fw->has(kScore)) {
        // No score plugins: every node 1, unless extenders score (then 0 +
        // their priorities, generic_scheduler.go:408-416).
        const bool ext_scores = extenders_interested(*pod);
        scores.assign(feasible.size(), NodeScore{});
        for (auto& sc : scores) sc.score = ext_scores ? 0 : 1;
        st = Status();
      } else {
        st = fw->run_pre_score(*state, *pod, feasible);
        if (st.is_success()) st = score_feasible(*fw, *state, *pod, feasible, feasible_pos_buf_.data(), eq, scores);
      }
      if (st.is_success() && !extenders_.empty()) add_extender_scores(*pod, feasible, scores);
      if (st.is_success()) host_ni = feasible[select_host(scores)];
    }
    if (host_ni) host = host_ni->name();
  }
  int64_t algo_end = clock_->now_us();
  CycleMetrics& cm = cycle_metrics(*fw);
  cm.algo->observe(static_cast<double>(algo_end - cycle_start) / 1e6);
  if (tracer_.enabled())
    tracer_.record(TraceEvent{"schedule", pod->key(), st.is_success() ? host : st.message(), cycle_start,
                              algo_end - cycle_start, 0});

  if (!st.is_success()) {
    std::string nominated;
    bool fit_error = st.is_unschedulable();
    if (fit_error && fw->has(kPostFilter)) {
      auto [res, pst] = fw->run_post_filter(*state, *pod, diag.node_to_status);
      if (pst.is_success()) nominated = res.nominated_node_name;
      cnt_.preemption_attempts.fetch_add(1, std::memory_order_relaxed);
    }
    if (fit_error && !opts_.dump_on_fit_error.empty() && !fit_error_dumped_.exchange(true)) {
      Json d = dump_cache();
      d.set("pod", Json(pod->key()));
      d.set("message", Json(st.message()));
      d.set("at_us", Json(clock_->now_us()));
      write_file(opts_.dump_on_fit_error, d.dump());
      if (tracer_.enabled())  // the trace ring up to this failure
        write_file(opts_.dump_on_fit_error + ".trace.json", tracer_.chrome_json());
    }
    const int result = fit_error ? 1 : 2;
    cm.attempts[result]->inc();
    cm.attempt[result]->observe(static_cast<double>(clock_->now_us() - cycle_start) / 1e6);
    (fit_error ? cnt_.unschedulable : cnt_.errors).fetch_add(1, std::memory_order_relaxed);
    handle_failure(*fw, qpi, st, fit_error ? "Unschedulable" : "SchedulerError", nominated, cycle,
                   diag.unschedulable_plugins);
    return;
  }

  // Assume.
  auto assumed = std::make_shared<Pod>(*pod);
  assumed->node_name = host;
  // Still the cycle's private copy: Reserve plugins that place from the
  // snapshot alone (FlexGPU) put their placement on it now, so the cache takes
  // the pod in once, with its final accounting.
  fw->run_prepare_assumed(*state, *assumed, *host_ni);
  Status ast = cache_->assume_pod(assumed);
  if (!ast.is_success()) {
    handle_failure(*fw, qpi, ast, "SchedulerError", "", cycle, {});
    return;
  }
  // An assumed pod is accounted on its node; drop its nomination so it is not
  // counted twice by nominated-pod-aware checks (scheduler.go assume():
  // DeleteNominatedPodIfExists).
  if (!nominator_->empty()) nominator_->remove(*assumed);
  int64_t t_assumed = tracer_.enabled() ? clock_->now_us() : 0;
  // Reserve.
  Status rst = fw->run_reserve(*state, assumed, host);
  int64_t t_reserved = tracer_.enabled() ? clock_->now_us() : 0;
  if (!rst.is_success()) {
    fail_assumed(*fw, *state, qpi, assumed, rst, rst.is_unschedulable() ? "Unschedulable" : "SchedulerError", cycle,
                 cnt_.errors, false);
    return;
  }
  // Permit.
  int64_t permit_start = clock_->now_us();
  inflight_.fetch_add(1);
  BindTask* task = &frame->task;
  task->self = this;
  task->fw = fw;
  task->frame = frame;
  task->qpi = qpi;
  task->assumed = assumed;
  task->host.assign(host);
  task->cycle = cycle;
  task->permit_start_us = permit_start;
  task->e2e = cycle_metrics(*fw).e2e;
  task->permit_status = Status();
  BindTask* tp = task;
  // From here the frame belongs to the binding cycle (run_bind_task hands it
  // back), unless Permit rejects the pod before any waiting.
  lease.frame = nullptr;
  // The binding cycles this Permit releases (the gang's waiting members and
  // this pod) reach the binder pool in one hand-over.
  std::optional<Executor::Batch> batch(std::in_place, *binder_);
  Status pst = fw->run_permit(*state, assumed, host, [tp](const Status& wst) {
    tp->permit_status = wst;
    tp->self->binder_->submit([tp] { run_bind_task(tp); });
  });
  if (!pst.is_success() && !pst.is_wait()) {
    lease.frame = frame;  // rejected before waiting: the callback never runs
    inflight_.fetch_sub(1);
    fail_assumed(*fw, *state, qpi, assumed, pst, pst.is_unschedulable() ? "Unschedulable" : "SchedulerError", cycle,
                 cnt_.unschedulable, false);
    return;
  }
  int64_t t_permitted = tracer_.enabled() ? clock_->now_us() : 0;
  if (pst.is_success()) note_gang_event(*assumed, false);
  activate_stashed(*to_activate);
  cm.attempts[0]->inc();
  cm.attempt[0]->observe(static_cast<double>(clock_->now_us() - cycle_start) / 1e6);
  cnt_.scheduled.fetch_add(1, std::memory_order_relaxed);
  if (pst.is_success()) binder_->submit([tp] { run_bind_task(tp); });
  batch.reset();
  if (tracer_.enabled()) {
    int64_t t_end = clock_->now_us();
    tracer_.record(TraceEvent{"assume_reserve_permit", assumed->key(), "", algo_end, t_end - algo_end, 0});
    tracer_.record(TraceEvent{"assume", assumed->key(), "", algo_end, t_assumed - algo_end, 0});
    tracer_.record(TraceEvent{"reserve", assumed->key(), "", t_assumed, t_reserved - t_assumed, 0});
    tracer_.record(TraceEvent{"permit", assumed->key(), "", t_reserved, t_permitted - t_reserved, 0});
    tracer_.record(TraceEvent{"activate_metrics", assumed->key(), "", t_permitted, t_end - t_permitted, 0});
  }
}

void Scheduler::run_bind_task(BindTask* t) {
  Scheduler* self = t->self;
  self->binding_cycle(*t, t->permit_status);
  self->hand_back_frame(t->frame);  // the frame's last user
}

// Replaced snapshot versions may hold the last reference to deleted pods;
// free them in batches on a binder thread instead of in the scheduling cycle.
void Scheduler::release_retired() {
  if (snapshot_.retired.size() >= 32) {
    // The batch is released on a binder thread; its emptied vector comes back
    // through retired_spare_ with its capacity (no allocation per batch).
    auto batch = std::make_shared<std::vector<NodeInfoPtr>>(std::move(snapshot_.retired));
    snapshot_.retired.clear();
    {
      std::lock_guard<std::mutex> g(retired_spare_mu_);
      if (!retired_spare_.empty()) {
        snapshot_.retired.swap(retired_spare_.back());
        retired_spare_.pop_back();
      }
    }
    if (snapshot_.retired.capacity() < 64) snapshot_.retired.reserve(64);
    binder_->submit([this, batch] {
      batch->clear();
      std::lock_guard<std::mutex> g(retired_spare_mu_);
      if (retired_spare_.size() < 8) retired_spare_.push_back(std::move(*batch));
    });
  }
  if (snapshot_.retired_deltas.size() >= 256) {
    auto batch = std::make_shared<std::vector<PodDelta>>(std::move(snapshot_.retired_deltas));
    snapshot_.retired_deltas.clear();
    snapshot_.retired_deltas.reserve(512);
    binder_->submit([batch] { batch->clear(); });
  }
}

Scheduler::BindMetrics& Scheduler::bind_metrics() {
  BindMetrics& m = bind_metrics_;
  uint64_t e = metrics_->epoch();
  if (m.epoch.load(std::memory_order_acquire) == e) return m;
  std::lock_guard<std::mutex> g(bind_metrics_mu_);
  if (m.epoch.load(std::memory_order_acquire) == e) return m;
  m.binding.store(&metrics_->histogram("xsched_binding_duration_seconds", ""));
  m.attempts.store(&metrics_->histogram("scheduler_pod_scheduling_attempts", ""));
  m.permit_wait[0].store(&metrics_->histogram("scheduler_permit_wait_duration_seconds", "result=\"Success\""));
  m.permit_wait[1].store(&metrics_->histogram("scheduler_permit_wait_duration_seconds", "result=\"Unschedulable\""));
  for (int a = 1; a <= 8; ++a)
    m.pod_duration[a - 1].store(
        &metrics_->histogram("scheduler_pod_scheduling_duration_seconds", "attempts=\"" + std::to_string(a) + "\""));
  m.epoch.store(e, std::memory_order_release);
  return m;
}

void Scheduler::binding_cycle(const BindTask& t, const Status& permit_status) {
  Framework* fw = t.fw;
  CycleState* s = &t.frame->state;
  const QueuedPodInfoPtr& qpi = t.qpi;
  const PodPtr& assumed = t.assumed;
  const std::string& host = t.host;
  const int64_t cycle = t.cycle, wait_start_us = t.permit_start_us;
  const std::shared_ptr<PodsToActivate>& to_activate = t.frame->to_activate;
  int64_t t0 = clock_->now_us();
  auto fail = [&](const Status& st, const std::string& reason) {
    fail_assumed(*fw, *s, qpi, assumed, st, reason, cycle, cnt_.bind_failures, true);
    inflight_.fetch_sub(1);
  };
  BindMetrics& bm = bind_metrics();
  if (wait_start_us > 0 && t0 - wait_start_us > 0) {
    bm.permit_wait[permit_status.is_success() ? 0 : 1].load(std::memory_order_relaxed)
        ->observe(static_cast<double>(t0 - wait_start_us) / 1e6);
    if (tracer_.enabled())
      tracer_.record(TraceEvent{"permit_wait", assumed->key(), code_name(permit_status.code()), wait_start_us,
                                t0 - wait_start_us, 1});
  }
  if (!permit_status.is_success()) {
    fail(permit_status, permit_status.is_unschedulable() ? "Unschedulable" : "SchedulerError");
    return;
  }
  Status st = fw->run_pre_bind(*s, assumed, host);
  if (!st.is_success()) {
    fail(st, "SchedulerError");
    return;
  }
  // extendersBinding (scheduler.go bind()): the first interested binder
  // extender binds instead of the Bind plugins.
  Extender* binder = nullptr;
  for (const auto& e : extenders_)
    if (e->is_binder() && e->interested(*assumed)) {
      binder = e.get();
      break;
    }
  if (binder) {
    try {
      binder->bind(assumed->ns(), assumed->name(), assumed->uid(), host);
      st = Status();
    } catch (const std::exception& ex) {
      st = Status::error(std::string("extender ") + binder->name() + " bind: " + ex.what());
    }
  } else {
    st = fw->run_bind(*s, assumed, host);
  }
  if (st.is_skip()) st = Status(Code::Error, "no bind plugin bound the pod");
  if (!st.is_success()) {
    fail(st, "SchedulerError");
    return;
  }
  cache_->finish_binding(*assumed);
  int64_t t1 = clock_->now_us();
  bm.binding.load(std::memory_order_relaxed)->observe(static_cast<double>(t1 - t0) / 1e6);
  t.e2e->observe(static_cast<double>(t1 - qpi->timestamp_us) / 1e6);
  Histogram* pd = qpi->attempts >= 1 && qpi->attempts <= 8
                      ? bm.pod_duration[qpi->attempts - 1].load(std::memory_order_relaxed)
                      : &metrics_->histogram("scheduler_pod_scheduling_duration_seconds",
                                             "attempts=\"" + std::to_string(qpi->attempts) + "\"");
  pd->observe(static_cast<double>(t1 - qpi->initial_attempt_us) / 1e6);
  bm.attempts.load(std::memory_order_relaxed)->observe(qpi->attempts);
  if (tracer_.enabled()) tracer_.record(TraceEvent{"bind", assumed->key(), host, t0, t1 - t0, 1});
  fw->run_post_bind(*s, assumed, host);
  if (tracer_.enabled()) {
    const int64_t t2 = clock_->now_us();
    tracer_.record(TraceEvent{"post_bind", assumed->key(), "", t1, t2 - t1, 1});
  }
  cnt_.bound.fetch_add(1, std::memory_order_relaxed);
  bound_total_.fetch_add(1, std::memory_order_release);
  note_gang_event(*assumed, true);
  activate_stashed(*to_activate);
  inflight_.fetch_sub(1);
}

void Scheduler::fail_assumed(Framework& fw, CycleState& s, const QueuedPodInfoPtr& qpi, const PodPtr& assumed,
                             const Status& st, const std::string& reason, int64_t cycle,
                             std::atomic<uint64_t>& counter, bool freed) {
  fw.run_unreserve(s, assumed, assumed->node_name);
  cache_->forget_pod(*assumed);
  if (freed) {
    // A forgotten pod frees resources: let waiting pods retry (AssignedPodDelete).
    queue_->move_all_to_active_or_backoff(ClusterEvent{"Pod", kDelete, "AssignedPodDelete"});
    capacity_freed();
  }
  counter.fetch_add(1, std::memory_order_relaxed);
  handle_failure(fw, qpi, st, reason, "", cycle,
                 st.failed_plugin().empty() ? std::set<std::string>{} : std::set<std::string>{st.failed_plugin()});
}

void Scheduler::handle_failure(Framework& fw, const QueuedPodInfoPtr& qpi, const Status& st, const std::string& reason,
                               const std::string& nominated, int64_t cycle, const std::set<std::string>& plugins) {
  PodPtr pod = qpi->pod;
  // updatePod is skipped when the condition and nomination are unchanged
  // since this pod's last failure (remembered on its queue entry, so the
  // memo lives and dies with the pod: no scheduler-wide map to sweep).
  std::string condition = st.message() + "|" + nominated;
  const bool same_condition = qpi->last_condition == condition && nominated == pod->nominated_node_name;
  // Requeue the latest version unless it was deleted or got assigned.
  PodPtr latest = informers_->pod(pod->ns(), pod->name());
  if (latest && latest->uid() == pod->uid() && latest->node_name.empty() && !latest->terminating()) {
    auto nq = std::make_shared<QueuedPodInfo>(*qpi);
    nq->pod = latest;
    nq->unschedulable_plugins = plugins;
    nq->last_condition = condition;
    queue_->add_unschedulable_if_not_present(nq, cycle);
  }
  // After the requeue (which re-registers the pod's *observed* nomination):
  // the next cycle must already see this one, before the status patch comes
  // back through the informer (scheduler.go handleSchedulingFailure).
  if (!nominated.empty()) nominator_->add(latest && latest->uid() == pod->uid() ? latest : pod, nominated);
  // The event goes out on the status writer (kube-scheduler's recorder is
  // asynchronous too); the status update stays on the scheduling loop, as
  // upstream's updatePod: written asynchronously it could land after a later
  // cycle bound the pod and overwrite its PodScheduled=True condition. (Moved
  // to the status writer with a resourceVersion precondition, it cost open-loop
  // capacity on the box: parked gangs at 112k pods/s went from 44-86 to 1,917,
  // profiles/r6/README.md, r6x. The inline patch is backpressure.)
  ApiClient* client = fw.handle().client;
  status_writer_->submit([client, pod, msg = st.message()] {
    try {
      client->record_event("Pod", pod->ns(), pod->name(), "Warning", "FailedScheduling", msg);
    } catch (const std::exception&) {
    }
  });
  if (!opts_.status_updates || same_condition) return;
  // updatePod: PodScheduled=False condition + nominatedNodeName, only when changed.
  std::string msg = st.message();
  Json patch = Json::object();
  Json status = Json::object();
  Json cond = Json::object();
  cond.set("type", Json("PodScheduled"));
  cond.set("status", Json("False"));
  cond.set("reason", Json(reason));
  cond.set("message", Json(msg));
  Json conds = Json::array();
  conds.push_back(std::move(cond));
  status.set("conditions", std::move(conds));
  if (!nominated.empty()) status.set("nominatedNodeName", Json(nominated));
  patch.set("status", std::move(status));
  try {
    client->patch("pods", pod->ns(), pod->name(), patch);
  } catch (const std::exception&) {
  }
}

}  // namespace xsched
