// Informer ingestion: watch events into the listers, the cache and the queue.
#include "scheduler/scheduler.h"

#include "common/log.h"
#include "common/reaper.h"

#include <algorithm>

namespace xsched {

namespace {
std::string resource_for_kind(const std::string& kind) {
  if (kind == "pods") return "Pod";
  if (kind == "nodes") return "Node";
  if (kind == "podgroups") return "PodGroup";
  if (kind == "elasticquotas") return "ElasticQuota";
  if (kind == "noderesourcetopologies") return "NodeResourceTopology";
  if (kind == "poddisruptionbudgets") return "PodDisruptionBudget";
  if (kind == "priorityclasses") return "PriorityClass";
  if (kind == "persistentvolumes") return "PersistentVolume";
  if (kind == "persistentvolumeclaims") return "PersistentVolumeClaim";
  if (kind == "storageclasses") return "StorageClass";
  if (kind == "csinodes") return "CSINode";
  return kind;
}
uint32_t action_for(EventType t) {
  switch (t) {
    case EventType::Added: return kAdd;
    case EventType::Deleted: return kDelete;
    default: return kUpdate;
  }
}
int64_t resource_version_of(const Json& obj) {
  const Json& rv = obj["metadata"]["resourceVersion"];
  return rv.is_string() ? std::atoll(rv.as_string().c_str()) : rv.as_int();
}
// A copy of an earlier version of the pod takes the new object's
// resourceVersion and the fields Pod::from_json reads from status.
void refresh_version_and_status(Pod& np, const Json& obj) {
  np.meta.resource_version = resource_version_of(obj);
  const Json& status = obj["status"];
  np.phase = status["phase"].is_string() ? status["phase"].as_string() : std::string("Pending");
  np.nominated_node_name = status["nominatedNodeName"].as_string();
  np.start_time = status["startTime"].is_string() ? parse_rfc3339(status["startTime"].as_string()) : 0;
  np.scheduled_at = 0;
  for (const auto& c : status["conditions"].items())
    if (c["type"].as_string() == "PodScheduled" && c["status"].as_string() == "True")
      np.scheduled_at = parse_rfc3339(c["lastTransitionTime"].as_string());
}
}  // namespace

void Scheduler::informer_loop() {
  while (running_.load()) {
    auto evs = watcher_->next(50, 8192);
    if (evs.empty()) continue;
    int64_t batch_start = tracer_.enabled() ? clock_->now_us() : 0;
    // The batch is handled in windows of >= informer_window_ events that end
    // on a PodGroup boundary, so the scheduling thread starts on the first
    // gangs of a bulk create instead of waiting for the whole batch.
    // Per window, pass 1 parses every pod once and publishes it to the
    // listers, so a PreFilter racing the window sees every sibling of a
    // PodGroup created together (Coscheduling counts them); pass 2 then
    // drives cache and queue.
    std::vector<PodPtr> parsed(evs.size());
    std::vector<PodPtr> prev(evs.size());
    std::vector<size_t> to_parse;
    auto group_of = [](const WatchEvent& ev) -> const std::string& {
      return (*ev.obj)["metadata"]["labels"][kPodGroupLabel].as_string();
    };
    size_t lo = 0;
    while (lo < evs.size()) {
      size_t hi = lo;
      while (hi < evs.size()) {
        const auto& ev = evs[hi];
        if (hi - lo >= informer_window_) {
          const auto& pe = evs[hi - 1];
          bool same_group = ev.kind == "pods" && pe.kind == "pods" && ev.type == EventType::Added &&
                            pe.type == EventType::Added && !group_of(ev).empty() && group_of(ev) == group_of(pe);
          if (!same_group) break;
        }
        ++hi;
        if (ev.kind != "pods" || ev.type == EventType::Deleted) continue;
        try {
          if (ev.type == EventType::Modified) parsed[hi - 1] = copy_for_modified(ev);
        } catch (const std::exception&) {
          continue;
        }
        if (!parsed[hi - 1]) to_parse.push_back(hi - 1);
      }
      // Pod::from_json is pure: a window's parses run on the parse helpers.
      if (!to_parse.empty()) {
        auto parse_one = [&](int k) {
          const size_t i = to_parse[static_cast<size_t>(k)];
          try {
            parsed[i] = Pod::from_json(*evs[i].obj, *gpu_names_);
          } catch (const std::exception&) {
            // left unparsed: handle_event below parses it again and reports
          }
        };
        if (parse_pool_) {
          parse_pool_->until(static_cast<int>(to_parse.size()), parse_one, nullptr, &parse_site_);
        } else {
          for (size_t k = 0; k < to_parse.size(); ++k) parse_one(static_cast<int>(k));
        }
        to_parse.clear();
      }
      // The window's pods enter the listers under one lock (previous objects back).
      informers_->upsert_pods(&parsed[lo], &prev[lo], hi - lo);
      for (size_t i = lo; i < hi;) {
        if (!parsed[i] && evs[i].type == EventType::Deleted && evs[i].kind == "pods") {
          size_t j = i + 1;
          while (j < hi && evs[j].type == EventType::Deleted && evs[j].kind == "pods") ++j;
          if (j - i > 1) {
            handle_pod_deletes(&evs[i], j - i);
            i = j;
            continue;
          }
        }
        if (parsed[i])
          handle_parsed_pod_event(evs[i], parsed[i], prev[i]);
        else
          handle_event(evs[i]);
        parsed[i].reset();
        prev[i].reset();
        ++i;
      }
      lo = hi;
    }
    if (tracer_.enabled() && batch_start)
      tracer_.record(TraceEvent{"informer_batch", std::to_string(evs.size()) + " events", "", batch_start,
                                clock_->now_us() - batch_start, 2});
  }
}

size_t Scheduler::sync_informers(int timeout_ms) {
  size_t n = 0;
  for (;;) {
    auto evs = watcher_->next(n == 0 ? timeout_ms : 0, 8192);
    if (evs.empty()) break;
    for (const auto& ev : evs) handle_event(ev);
    n += evs.size();
  }
  return n;
}

void Scheduler::handle_event(const WatchEvent& ev) {
  try {
    if (ev.kind == "pods") {
      handle_pod_event(ev);
    } else if (ev.kind == "nodes") {
      handle_node_event(ev);
    } else {
      const Json& o = *ev.obj;
      bool del = ev.type == EventType::Deleted;
      if (ev.kind == "podgroups") {
        if (del) {
          // A deletion needs the key only (no parse: a wave tears down
          // hundreds of groups at once).
          const Json& md = o["metadata"];
          const std::string key = md["namespace"].as_string() + "/" + md["name"].as_string();
          // A gang deleted before it was admitted leaves no open record (it
          // goes with the entry's PodGroup): a later PodGroup of the same
          // name starts its own timeline.
          informers_->delete_pod_group(key);
        } else {
          informers_->upsert_pod_group(PodGroup::from_json(o));
        }
      } else if (ev.kind == "elasticquotas") {
        auto eq = ElasticQuota::from_json(o);
        if (del) informers_->delete_elastic_quota(eq->meta.key()); else informers_->upsert_elastic_quota(eq);
      } else if (ev.kind == "noderesourcetopologies") {
        auto n = NodeResourceTopology::from_json(o);
        if (del) informers_->delete_nrt(n->meta.name); else informers_->upsert_nrt(n);
        cache_->set_nrt(n->meta.name, del ? nullptr : n);
      } else if (ev.kind == "poddisruptionbudgets") {
        auto p = PodDisruptionBudget::from_json(o);
        if (del) informers_->delete_pdb(p->meta.key()); else informers_->upsert_pdb(p);
      } else if (ev.kind == "priorityclasses") {
        auto pc = PriorityClass::from_json(o);
        if (del) informers_->delete_priority_class(pc->meta.name); else informers_->upsert_priority_class(pc);
      } else if (ev.kind == "persistentvolumes") {
        auto pv = PersistentVolume::from_json(o);
        if (del) informers_->delete_pv(pv->meta.name); else informers_->upsert_pv(pv);
      } else if (ev.kind == "persistentvolumeclaims") {
        auto pvc = PersistentVolumeClaim::from_json(o);
        if (del) informers_->delete_pvc(pvc->meta.key()); else informers_->upsert_pvc(pvc);
      } else if (ev.kind == "storageclasses") {
        auto sc = StorageClass::from_json(o);
        if (del) informers_->delete_storage_class(sc->meta.name); else informers_->upsert_storage_class(sc);
      } else if (ev.kind == "csinodes") {
        auto n = CSINode::from_json(o);
        if (del) informers_->delete_csinode(n->meta.name); else informers_->upsert_csinode(n);
      }
      for (auto& fw : frameworks_) fw->dispatch_object_event(ev.kind, static_cast<int>(ev.type), ev.obj, ev.old);
      queue_->move_all_to_active_or_backoff(ClusterEvent{resource_for_kind(ev.kind), action_for(ev.type), ""});
    }
  } catch (const std::exception& e) {
    // A malformed object must not kill the informer thread.
    report_informer_error(ev, e.what());
  }
}

// The object is dropped from the scheduler's view: say so (log line and, for
// pods and nodes, a Warning event on the object) so that, e.g., a pod naming
// a 65th distinct resource does not just silently stay Pending.
void Scheduler::report_informer_error(const WatchEvent& ev, const char* what) {
  metrics_->inc("xsched_informer_errors_total", "kind=\"" + ev.kind + "\"");
  std::string ns, name;
  if (ev.obj) {
    const Json& md = (*ev.obj)["metadata"];
    ns = md["namespace"].str_or("");
    name = md["name"].str_or("");
  }
  XS_WARN("informer dropped object").kv("kind", ev.kind).kv("namespace", ns).kv("name", name).kv("err", what);
  if (name.empty() || ev.type == EventType::Deleted) return;
  if (ev.kind == "pods" || ev.kind == "nodes") {
    try {
      client_->record_event(ev.kind == "pods" ? "Pod" : "Node", ns, name, "Warning", "FailedToDecode",
                            std::string("scheduler cannot use this object: ") + what);
    } catch (const std::exception&) {
    }
  }
}

// The pod a Deleted event removes. The lister copy stands in for the final
// state when it is the same pod on the same node (all deletion needs), saving
// a parse per delete.
PodPtr Scheduler::deleted_pod(const WatchEvent& ev) {
  const Json& md = (*ev.obj)["metadata"];
  PodPtr p = informers_->pod(md["namespace"].as_string(), md["name"].as_string());
  if (!p || p->uid() != md["uid"].as_string() || p->node_name != (*ev.obj)["spec"]["nodeName"].as_string())
    p = Pod::from_json(*ev.obj, *gpu_names_);
  return p;
}

void Scheduler::forget_unassigned_pod(const Pod& p) {
  queue_->remove(p);
  for (auto& w : waiting_)
    if (auto wp = w->get(p.uid())) wp->reject("", "pod " + p.key() + " was deleted");
  // An assumed-but-unbound pod may still sit in the cache.
  if (cache_->is_assumed(p.uid())) {
    if (auto cached = cache_->get_pod(p.uid())) {
      cache_->forget_pod(*cached);
      queue_->move_all_to_active_or_backoff(ClusterEvent{"Pod", kDelete, "AssignedPodDelete"});
      capacity_freed();
    }
  }
}

void Scheduler::capacity_freed() {
  for (auto& fw : frameworks_) fw->notify_capacity_freed();
}

void Scheduler::handle_pod_deletes(const WatchEvent* evs, size_t n) {
  std::vector<PodPtr> gone, assigned;
  gone.reserve(n);
  assigned.reserve(n);
  // One lister lock for the run: keys out, lister objects back where they
  // still describe the deleted pod (no parse for those).
  std::vector<std::string> keys;
  std::vector<std::string_view> uids, nodes;
  std::vector<size_t> idx;
  keys.reserve(n);
  uids.reserve(n);
  nodes.reserve(n);
  idx.reserve(n);
  for (size_t i = 0; i < n; ++i) {
    try {
      for (auto& fw : frameworks_) fw->dispatch_object_event("pods", static_cast<int>(evs[i].type), evs[i].obj, evs[i].old);
      const Json& o = *evs[i].obj;
      const Json& md = o["metadata"];
      const std::string& ns = md["namespace"].as_string();
      const std::string& name = md["name"].as_string();
      std::string key;
      key.reserve(ns.size() + 1 + name.size());
      key.append(ns).push_back('/');
      key.append(name);
      keys.push_back(std::move(key));
      uids.push_back(md["uid"].as_string());
      nodes.push_back(o["spec"]["nodeName"].as_string());
      idx.push_back(i);
    } catch (const std::exception& e) {
      report_informer_error(evs[i], e.what());
    }
  }
  std::vector<PodPtr> listed = informers_->take_pods(keys, uids, nodes);
  for (size_t k = 0; k < idx.size(); ++k) {
    try {
      PodPtr p = listed[k] ? std::move(listed[k]) : Pod::from_json(*evs[idx[k]].obj, *gpu_names_);
      if (!p->node_name.empty()) assigned.push_back(p);
      gone.push_back(std::move(p));
    } catch (const std::exception& e) {
      report_informer_error(evs[idx[k]], e.what());
    }
  }
  if (!assigned.empty()) {
    cache_->remove_pods(assigned);
    queue_->move_all_to_active_or_backoff(ClusterEvent{"Pod", kDelete, "AssignedPodDelete"});
    capacity_freed();
  }
  for (const auto& p : gone)
    if (p->node_name.empty()) forget_unassigned_pod(*p);
  // The lister's and the cache's references are gone: the last ones to the
  // wave's Pod objects are here, freed off the informer thread.
  assigned.clear();
  defer_destroy(std::make_shared<std::vector<PodPtr>>(std::move(gone)));
}

void Scheduler::handle_pod_event(const WatchEvent& ev) {
  for (auto& fw : frameworks_) fw->dispatch_object_event("pods", static_cast<int>(ev.type), ev.obj, ev.old);
  if (ev.type == EventType::Deleted) {
    PodPtr p = deleted_pod(ev);
    informers_->delete_pod(*p);
    if (!p->node_name.empty()) {
      cache_->remove_pod(*p);
      queue_->move_all_to_active_or_backoff(ClusterEvent{"Pod", kDelete, "AssignedPodDelete"});
      capacity_freed();
    } else {
      forget_unassigned_pod(*p);
    }
    return;
  }
  PodPtr np = ev.type == EventType::Modified ? copy_for_modified(ev) : nullptr;
  if (!np) np = Pod::from_json(*ev.obj, *gpu_names_);
  PodPtr old = informers_->pod(np->ns(), np->name());
  informers_->upsert_pod(np);
  apply_pod_update(ev, np, old);
}

// The Modified event of our own Binding: the new object is the version the
// pod was assumed from plus nodeName, the Reserve annotations, the
// PodScheduled condition and a resourceVersion. When the previous version is
// exactly the one the assumed copy came from (same resourceVersion), the
// informer's object is built by copying the assumed pod and refreshing those
// fields, instead of parsing the whole Pod again (one parse per pod, not two).
PodPtr Scheduler::bound_copy_of_assumed(const WatchEvent& ev) {
  if (!ev.old) return nullptr;
  const Json& obj = *ev.obj;
  const Json& spec = obj["spec"];
  const std::string& node = spec["nodeName"].as_string();
  if (node.empty() || !(*ev.old)["spec"]["nodeName"].as_string().empty()) return nullptr;
  const Json& md = obj["metadata"];
  PodPtr assumed = cache_->get_pod(md["uid"].as_string());
  if (!assumed || !cache_->is_assumed(assumed->uid()) || assumed->node_name != node) return nullptr;
  const int64_t from_rv = resource_version_of(*ev.old);
  if (from_rv != assumed->meta.resource_version) return nullptr;  // updated since the cycle: parse
  if (md["annotations"].size() != assumed->meta.annotations.size()) return nullptr;
  auto np = std::make_shared<Pod>(*assumed);
  np->template_hash = 0;  // as Pod::from_json for an assigned pod
  refresh_version_and_status(*np, obj);
  return np;
}

// A failed cycle's PodScheduled=False patch (handle_failure) changes status
// only; at saturation thousands of them reach the informer while creations and
// deletions queue behind them. The lister's object for the previous version
// is copied and its status fields refreshed (the fields Pod::from_json reads
// from status) instead of parsing the pod again.
PodPtr Scheduler::status_copy_of_listed(const WatchEvent& ev) {
  if (!ev.status_only || !ev.old) return nullptr;
  const Json& obj = *ev.obj;
  const Json& md = obj["metadata"];
  PodPtr listed = informers_->pod(md["namespace"].as_string(), md["name"].as_string());
  if (!listed || listed->uid() != md["uid"].as_string()) return nullptr;
  const int64_t from_rv = resource_version_of(*ev.old);
  if (from_rv != listed->meta.resource_version) return nullptr;  // the lister holds another version: parse
  auto np = std::make_shared<Pod>(*listed);
  refresh_version_and_status(*np, obj);
  return np;
}

void Scheduler::handle_parsed_pod_event(const WatchEvent& ev, const PodPtr& np, PodPtr old) {
  try {
    for (auto& fw : frameworks_) fw->dispatch_object_event("pods", static_cast<int>(ev.type), ev.obj, ev.old);
    apply_pod_update(ev, np, std::move(old));
  } catch (const std::exception& e) {
    report_informer_error(ev, e.what());
  }
}

void Scheduler::apply_pod_update(const WatchEvent& ev, const PodPtr& np, PodPtr old) {
  if (old && old->uid() != np->uid()) old = nullptr;  // recreated with same name
  bool assigned = !np->node_name.empty();
  if (ev.type == EventType::Added || !old) {
    if (assigned) {
      cache_->add_pod(np);
      queue_->assigned_pod_added(*np);
    } else if (responsible_for(*np) && !np->terminating()) {
      // The gang record first: once queued, the pod can be scheduled, admitted
      // and bound by other threads before this one runs again, and a record
      // opened after its own completion would never close (the gang would
      // read as never bound).
      note_gang_enqueue(*np, clock_->now_us());
      queue_->add(np);
      // A new member may complete its PodGroup: re-activate siblings parked
      // in unschedulableQ/backoffQ (targeted form of the Pod/Add cluster
      // event Coscheduling registers; O(group size), not O(queue)).
      if (!np->pod_group.empty()) {
        std::vector<PodPtr> sib = informers_->gang_members(*np);
        sib.erase(std::remove_if(sib.begin(), sib.end(),
                                 [&](const PodPtr& q) { return q->uid() == np->uid() || !q->node_name.empty(); }),
                  sib.end());
        if (!sib.empty()) queue_->activate(sib);
      }
    }
    return;
  }
  bool was_assigned = !old->node_name.empty();
  if (was_assigned && assigned) {
    cache_->update_pod(old, np);
    queue_->assigned_pod_updated(*np);
  } else if (!was_assigned && assigned) {
    queue_->remove(*old);
    cache_->add_pod(np);
    queue_->assigned_pod_added(*np);
  } else if (!assigned && responsible_for(*np)) {
    if (np->terminating()) {
      queue_->remove(*np);
    } else if (!cache_->is_assumed(np->uid())) {
      queue_->update(old, np);
    }
  }
}

void Scheduler::handle_node_event(const WatchEvent& ev) {
  for (auto& fw : frameworks_) fw->dispatch_object_event("nodes", static_cast<int>(ev.type), ev.obj, ev.old);
  if (ev.type == EventType::Deleted) {
    auto n = Node::from_json(*ev.obj, *gpu_names_);
    cache_->remove_node(n->name());
    return;
  }
  auto n = Node::from_json(*ev.obj, *gpu_names_);
  if (ev.type == EventType::Added || !ev.old) {
    cache_->add_node(n);
    queue_->move_all_to_active_or_backoff(ClusterEvent{"Node", kAdd, "NodeAdd"});
    capacity_freed();
    return;
  }
  auto o = Node::from_json(*ev.old, *gpu_names_);
  cache_->update_node(n);
  uint32_t action = 0;
  if (!(o->allocatable == n->allocatable)) action |= kUpdateNodeAllocatable;
  if (o->meta.labels != n->meta.labels) action |= kUpdateNodeLabel;
  if (o->taints.size() != n->taints.size() || o->unschedulable != n->unschedulable) action |= kUpdateNodeTaint;
  else
    for (size_t i = 0; i < o->taints.size(); ++i)
      if (o->taints[i].key != n->taints[i].key || o->taints[i].value != n->taints[i].value ||
          o->taints[i].effect != n->taints[i].effect)
        action |= kUpdateNodeTaint;
  if (o->meta.annotations != n->meta.annotations) action |= kUpdateNodeLabel;  // GPU topology annotation
  if (action) queue_->move_all_to_active_or_backoff(ClusterEvent{"Node", action, "NodeUpdate"});
  if (action & kUpdateNodeAllocatable) capacity_freed();
}

}  // namespace xsched
