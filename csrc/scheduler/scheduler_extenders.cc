// The scheduler's side of the HTTP extenders (extender.h): Filter and
// Prioritize calls of a scheduling cycle.
#include "scheduler/scheduler.h"

#include <algorithm>

namespace xsched {

bool Scheduler::extenders_interested(const Pod& p) const {
  for (const auto& e : extenders_)
    if (e->interested(p)) return true;
  return false;
}

Json Scheduler::pod_object(const Pod& p) const {
  if (JsonPtr obj = store_->get("pods", p.ns(), p.name())) return *obj;
  Json md = Json::object();
  md.set("name", Json(p.name()));
  md.set("namespace", Json(p.ns()));
  md.set("uid", Json(p.uid()));
  Json o = Json::object();
  o.set("apiVersion", Json("v1"));
  o.set("kind", Json("Pod"));
  o.set("metadata", std::move(md));
  return o;
}

Status Scheduler::run_extender_filters(const Pod& p, NodeList& feasible, std::vector<int>* pos, Diagnosis& d) {
  Json pod;
  bool have_pod = false;
  for (const auto& e : extenders_) {
    if (feasible.empty()) break;
    if (!e->interested(p) || !e->is_filter()) continue;
    if (!have_pod) {
      pod = pod_object(p);
      have_pod = true;
    }
    std::vector<std::string> names;
    names.reserve(feasible.size());
    for (const auto* ni : feasible) names.push_back(ni->name());
    Extender::FilterResult r;
    try {
      r = e->filter(pod, names, store_lookup_);
    } catch (const std::exception& ex) {
      if (e->ignorable()) continue;  // "Skipping extender as it returned error and has ignorable flag set"
      return Status::error(ex.what());
    }
    for (const auto& [node, msg] : r.unresolvable) {
      std::vector<std::string> reasons;
      auto it = d.node_to_status.find(node);
      if (it != d.node_to_status.end()) reasons = it->second.reasons();
      reasons.push_back(msg);
      d.node_to_status[node] = Status(Code::UnschedulableAndUnresolvable, std::move(reasons));
    }
    for (const auto& [node, msg] : r.failed) {
      if (r.unresolvable.count(node)) continue;  // unresolvable takes precedence
      auto it = d.node_to_status.find(node);
      if (it == d.node_to_status.end()) {
        d.node_to_status[node] = Status(Code::Unschedulable, msg);
      } else {
        std::vector<std::string> reasons = it->second.reasons();
        reasons.push_back(msg);
        Status ns(it->second.code(), std::move(reasons));
        if (!it->second.failed_plugin().empty()) ns.with_plugin(it->second.failed_plugin());
        it->second = std::move(ns);
      }
    }
    std::set<std::string> keep(r.nodes.begin(), r.nodes.end());
    size_t w = 0;
    for (size_t i = 0; i < feasible.size(); ++i) {
      if (!keep.count(feasible[i]->name())) continue;
      feasible[w] = feasible[i];
      if (pos) (*pos)[w] = (*pos)[i];
      ++w;
    }
    feasible.resize(w);
    if (pos) pos->resize(w);
  }
  return {};
}

void Scheduler::add_extender_scores(const Pod& p, const NodeList& feasible, std::vector<NodeScore>& scores,
                                    Json* breakdown) {
  std::vector<std::string> names;
  std::unordered_map<std::string, int64_t> combined;
  Json pod;
  bool any = false;
  for (const auto& e : extenders_) {
    if (!e->interested(p) || !e->is_prioritizer()) continue;
    if (!any) {
      pod = pod_object(p);
      names.reserve(feasible.size());
      for (const auto* ni : feasible) names.push_back(ni->name());
      any = true;
    }
    try {
      for (const auto& [host, score] : e->prioritize(pod, names, store_lookup_)) {
        combined[host] += score * e->config().weight;
        if (breakdown) {
          Json& node = breakdown->at_or_create(host);
          node.set(e->name(), Json(score));
        }
      }
    } catch (const std::exception&) {
      // "Prioritization errors from extender can be ignored, let k8s/other
      // extenders determine the priorities" (generic_scheduler.go:460-463)
    }
  }
  if (!any) return;
  for (size_t i = 0; i < feasible.size(); ++i) {
    auto it = combined.find(feasible[i]->name());
    if (it != combined.end()) scores[i].score += it->second * (kMaxNodeScore / kMaxExtenderPriority);
  }
}

}  // namespace xsched
