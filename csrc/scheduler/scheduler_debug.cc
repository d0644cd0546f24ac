// The debugging surface: cache debugger, plugin harness, explain and the
// Score micro-benchmark.
#include "scheduler/scheduler.h"

#include <algorithm>
#include <chrono>
#include <stdexcept>
#include <thread>

namespace xsched {

Json Scheduler::check_cache() const {
  // The listers and the cache are read one after the other, not atomically:
  // an informer event landing between the two reads shows as a difference
  // that the next read no longer has. Such a difference is read again (up to
  // ~50 ms); one that persists is reported. `reads` says how many it took.
  Json out;
  int reads = 0;
  for (; reads < 25; ++reads) {
    if (reads) std::this_thread::sleep_for(std::chrono::milliseconds(2));
    std::vector<PodPtr> assigned;
    for (auto& p : informers_->all_pods())
      if (!p->node_name.empty()) assigned.push_back(std::move(p));
    std::vector<std::string> nodes;
    for (const auto& n : store_->list("nodes", "")) nodes.push_back((*n)["metadata"]["name"].as_string());
    out = cache_->check(assigned, nodes);
    if (out["clean"].as_bool()) break;
  }
  out.set("reads", Json(static_cast<int64_t>(std::min(reads + 1, 25))));
  return out;
}

Json Scheduler::dump_cache() const {
  Json out = cache_->dump();
  auto c = queue_->counts();
  Json q = Json::object();
  q.set("active", Json(static_cast<int64_t>(c.active)));
  q.set("backoff", Json(static_cast<int64_t>(c.backoff)));
  q.set("unschedulable", Json(static_cast<int64_t>(c.unschedulable)));
  Json pending = Json::array();
  for (const auto& qpi : queue_->pending_pods()) pending.push_back(Json(qpi->pod->key()));
  q.set("pods", std::move(pending));
  out.set("queue", std::move(q));
  out.set("waiting_pods", Json(static_cast<int64_t>(permit_waiting())));
  out.set("nominated_pods", Json(static_cast<int64_t>(nominator_->size())));
  return out;
}

namespace {
Code code_from_name(const std::string& n) {
  for (Code c : {Code::Success, Code::Error, Code::Unschedulable, Code::UnschedulableAndUnresolvable, Code::Wait,
                 Code::Skip})
    if (n == code_name(c)) return c;
  throw std::runtime_error("unknown status code " + n);
}
Json status_json(const Status& st) {
  Json out = Json::object();
  out.set("code", Json(code_name(st.code())));
  out.set("message", Json(st.message()));
  return out;
}
}  // namespace

Json Scheduler::plugin_call(const std::string& plugin, const std::string& point, const Json& args) {
  std::lock_guard<std::mutex> g(sched_mu_);
  Framework* fw = frameworks_.front().get();
  if (args["schedulerName"].is_string()) fw = framework_for(args["schedulerName"].as_string());
  if (!fw) throw std::runtime_error("no such profile");
  Plugin* pl = nullptr;
  for (const auto& x : fw->all_plugins())
    if (x->name() == plugin) pl = x.get();
  if (!pl) throw std::runtime_error("plugin " + plugin + " is not enabled in the profile");
  cache_->update_snapshot(snapshot_);
  auto state = std::make_shared<CycleState>();
  state->write(kPodsToActivateKey, std::make_shared<PodsToActivate>());
  auto parse = [&](const Json& j) {
    auto p = Pod::from_json(j, *gpu_names_);
    if (p->uid().empty()) p->meta.uid = "harness-" + p->key();
    return p;
  };
  PodPtr pod = args.get("pod") ? parse(args["pod"]) : nullptr;
  const std::string node = args["node"].str_or("");
  if (point == "less") {
    QueuedPodInfo a, b;
    a.pod = parse(args["a"]);
    b.pod = parse(args["b"]);
    a.initial_attempt_wall = args["a_initial_attempt_us"].as_int(0);
    b.initial_attempt_wall = args["b_initial_attempt_us"].as_int(0);
    Json out = Json::object();
    out.set("less", Json(pl->less(a, b)));
    return out;
  }
  if (!pod) throw std::runtime_error("args.pod is required");
  if (point == "preFilter") return status_json(pl->pre_filter(*state, *pod));
  if (point == "postFilter") {
    NodeStatusMap m;
    for (const auto& [n, c] : args["statuses"].members()) {
      Status st(code_from_name(c.as_string()), c.as_string() == "Success" ? "" : "harness");
      m.emplace(n, st);
    }
    auto [res, st] = pl->post_filter(*state, *pod, m);
    Json out = status_json(st);
    out.set("nominatedNodeName", Json(res.nominated_node_name));
    return out;
  }
  if (point == "permit" || point == "reserve" || point == "unreserve" || point == "postBind") {
    // As in the real cycle these run on the assumed pod: the cache holds it
    // (Coscheduling's assigned count includes it) while the point runs.
    auto assumed = std::make_shared<Pod>(*pod);
    assumed->node_name = node;
    const bool assume = !node.empty() && args["assume"].as_bool(true) && point != "postBind";
    if (assume) {
      Status ast = cache_->assume_pod(assumed);
      if (!ast.is_success()) return status_json(ast);
    }
    Json out;
    if (point == "permit") {
      auto [st, timeout] = pl->permit(*state, assumed, node);
      out = status_json(st);
      out.set("timeout_us", Json(timeout));
    } else if (point == "reserve") {
      out = status_json(pl->reserve(*state, assumed, node));
    } else if (point == "unreserve") {
      pl->unreserve(*state, assumed, node);
      out = status_json(Status());
    } else {
      pl->post_bind(*state, assumed, node);
      out = status_json(Status());
    }
    if (assume) cache_->forget_pod(*assumed);
    return out;
  }
  if (point == "filter" || point == "score") {
    // One plugin's Filter verdicts / Score+NormalizeScore over the snapshot's
    // nodes (or args.nodes, in that order), as the reference's plugin unit
    // tests call them (after the plugin's own PreFilter / PreScore).
    NodeList nodes;
    if (args["nodes"].is_array()) {
      for (const auto& n : args["nodes"].items()) {
        auto it = snapshot_.index.find(n.as_string());
        if (it == snapshot_.index.end()) throw std::runtime_error("no node " + n.as_string());
        nodes.push_back(snapshot_.nodes[it->second].get());
      }
    } else {
      for (const auto& ni : snapshot_.nodes) nodes.push_back(ni.get());
    }
    Json out = Json::object();
    if (point == "filter") {
      if (pl->points() & kPreFilter) {
        Status pst = pl->pre_filter(*state, *pod);
        if (!pst.is_success()) {
          out.set("preFilter", status_json(pst));
          return out;
        }
      }
      Json per = Json::object();
      for (const NodeInfo* ni : nodes) per.set(ni->name(), status_json(pl->filter(*state, *pod, *ni)));
      out.set("nodes", std::move(per));
      return out;
    }
    if (pl->points() & kPreScore) {
      Status pst = pl->pre_score(*state, *pod, nodes);
      if (!pst.is_success()) {
        out.set("preScore", status_json(pst));
        return out;
      }
    }
    std::vector<NodeScore> scores(nodes.size());
    Json raw = Json::object();
    for (size_t i = 0; i < nodes.size(); ++i) {
      auto [sc, st] = pl->score(*state, *pod, *nodes[i]);
      if (!st.is_success()) throw std::runtime_error("score " + nodes[i]->name() + ": " + st.message());
      scores[i].name = &nodes[i]->name();
      scores[i].score = sc;
      raw.set(nodes[i]->name(), Json(sc));
    }
    if (pl->has_normalize_score()) {
      Status nst = pl->normalize_score(*state, *pod, scores);
      if (!nst.is_success()) throw std::runtime_error("normalize: " + nst.message());
    }
    Json norm = Json::object();
    for (size_t i = 0; i < nodes.size(); ++i) norm.set(nodes[i]->name(), Json(scores[i].score));
    out.set("raw", std::move(raw));
    out.set("scores", std::move(norm));
    return out;
  }
  if (args["runPreFilter"].as_bool(false)) {
    Status st = fw->run_pre_filter(*state, *pod);
    if (!st.is_success()) return status_json(st);
  }
  return pl->debug_call(point, *state, pod, args);
}

Json Scheduler::explain(const Json& pod_obj) {
  std::lock_guard<std::mutex> g(sched_mu_);
  Json out = Json::object();
  auto pod = Pod::from_json(pod_obj, *gpu_names_);
  Framework* fw = framework_for(pod->scheduler_name);
  if (!fw) {
    out.set("error", Json("no profile for schedulerName " + pod->scheduler_name.str()));
    return out;
  }
  if (pod->uid().empty()) pod->meta.uid = "explain-" + pod->key();
  cache_->update_snapshot(snapshot_);
  auto state = std::make_shared<CycleState>();
  state->write(kPodsToActivateKey, std::make_shared<PodsToActivate>());
  Diagnosis d;
  NodeList feasible;
  std::vector<int> feasible_pos;
  int saved_start = next_start_node_;
  Status st = find_nodes_that_fit(*fw, *state, *pod, d, feasible, nullptr, true, &feasible_pos);
  next_start_node_ = saved_start;
  out.set("code", Json(code_name(st.code())));
  out.set("message", Json(st.message()));
  Json filt = Json::object();
  for (const auto& [node, s] : d.node_to_status) {
    Json e = Json::object();
    e.set("plugin", Json(s.failed_plugin()));
    e.set("reason", Json(s.message()));
    e.set("code", Json(code_name(s.code())));
    filt.set(node, std::move(e));
  }
  out.set("filtered", std::move(filt));
  Json feas = Json::array();
  for (const auto& ni : feasible) feas.push_back(Json(ni->name()));
  out.set("feasible", std::move(feas));
  if (st.is_success() && !feasible.empty() && fw->has(kScore)) {
    std::vector<NodeScore> scores;
    Framework::ScoreBreakdown bd;
    Status ps = fw->run_pre_score(*state, *pod, feasible);
    if (ps.is_success()) ps = fw->run_score(*state, *pod, feasible, scores, &bd);
    if (ps.is_success()) {
      Json ext = Json::object();
      if (!extenders_.empty()) add_extender_scores(*pod, feasible, scores, &ext);
      Json sc = Json::object();
      for (size_t i = 0; i < feasible.size(); ++i) {
        Json node = Json::object();
        for (const auto& [plugin, vals] : bd) node.set(plugin, Json(vals[i]));
        if (const Json* e = ext.get(feasible[i]->name())) node.set("extenders", *e);
        node.set("total", Json(scores[i].score));
        sc.set(feasible[i]->name(), std::move(node));
      }
      out.set("scores", std::move(sc));
      out.set("selected", Json(feasible[select_host(scores)]->name()));
      // The scheduling path's totals (all-zero plugins skipped, their
      // normalized constant still added, the plugins' snapshot-array paths
      // given the nodes' positions) for parity checks against "total".
      // The template's equivalence slots are used as the scheduling cycle
      // uses them (hits included), so the parity check covers cached sums.
      std::vector<NodeScore> hot;
      if (score_feasible(*fw, *state, *pod, feasible, feasible_pos.data(), eq_entry(*fw, *pod), hot).is_success()) {
        Json h = Json::object();
        for (size_t i = 0; i < feasible.size(); ++i) h.set(feasible[i]->name(), Json(hot[i].score));
        out.set("hot_path_totals", std::move(h));
      }
    } else {
      out.set("score_error", Json(ps.message()));
    }
  } else if (feasible.size() == 1) {
    out.set("selected", Json(feasible[0]->name()));
  }
  return out;
}

double Scheduler::score_benchmark(const Json& pod_obj, int iterations, Json* out) {
  std::lock_guard<std::mutex> g(sched_mu_);
  auto pod = Pod::from_json(pod_obj, *gpu_names_);
  Framework* fw = framework_for(pod->scheduler_name);
  if (!fw) throw std::runtime_error("no profile for schedulerName " + pod->scheduler_name.str());
  cache_->update_snapshot(snapshot_);
  NodeList nodes;
  nodes.reserve(snapshot_.nodes.size());
  for (const auto& ni : snapshot_.nodes) nodes.push_back(ni.get());
  int64_t checksum = 0;
  int64_t t0 = clock_->now_us();
  for (int it = 0; it < std::max(1, iterations); ++it) {
    CycleState st;
    std::vector<NodeScore> scores;
    Status s = fw->run_pre_score(st, *pod, nodes);
    if (s.is_success()) s = fw->run_score(st, *pod, nodes, scores);
    if (!s.is_success()) throw std::runtime_error(s.message());
    for (const auto& x : scores) checksum += x.score;
  }
  double us = static_cast<double>(clock_->now_us() - t0) / std::max(1, iterations);
  if (out) {
    *out = Json::object();
    out->set("nodes", Json(static_cast<int64_t>(nodes.size())));
    out->set("us_per_pass", Json(us));
    out->set("checksum", Json(checksum));
  }
  return us;
}

}  // namespace xsched
