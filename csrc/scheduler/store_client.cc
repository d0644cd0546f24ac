// StoreClient: the ApiClient backed by the in-process ObjectStore, with
// client-go style Event aggregation.
#include "scheduler/scheduler.h"

namespace xsched {

void StoreClient::bind(const Pod& pod, const std::string& node, const Json& annotations) {
  store_->bind(pod.ns(), pod.name(), pod.uid(), node, annotations);
}

void StoreClient::delete_pod(const Pod& pod) { store_->remove("pods", pod.ns(), pod.name(), 0, pod.uid()); }

void StoreClient::patch(const std::string& kind, const std::string& ns, const std::string& name, const Json& patch) {
  store_->patch(kind, ns, name, patch);
}

void StoreClient::record_event(const std::string& kind, const std::string& ns, const std::string& name,
                               const std::string& type, const std::string& reason, const std::string& msg) {
  if (!events_enabled) return;
  const int64_t now = wall_now_us();
  std::string corr;
  corr.reserve(kind.size() + ns.size() + name.size() + reason.size() + msg.size() + 4);
  corr.append(kind).push_back('\0');
  corr.append(ns).push_back('\0');
  corr.append(name).push_back('\0');
  corr.append(reason).push_back('\0');
  corr.append(msg);
  Recent seen;
  {
    std::lock_guard<std::mutex> g(events_mu_);
    auto it = recent_.find(corr);
    if (it != recent_.end() && now - it->second.last_us < kAggregateUs) {
      it->second.count += 1;
      it->second.last_us = now;
      seen = it->second;
    }
  }
  if (seen.count > 0) {
    Json p = Json::object();
    p.set("count", Json(seen.count));
    p.set("lastTimestamp", Json(format_rfc3339(now)));
    try {
      store_->patch("events", seen.ns, seen.name, p);
      return;
    } catch (const StoreError&) {
      // expired or deleted: record a fresh Event below
    }
  }
  Json ev = Json::object();
  Json md = Json::object();
  md.set("generateName", Json(name + "."));
  md.set("namespace", Json(ns.empty() ? "default" : ns));
  ev.set("metadata", std::move(md));
  Json ref = Json::object();
  ref.set("kind", Json(kind));
  ref.set("namespace", Json(ns));
  ref.set("name", Json(name));
  ev.set("involvedObject", std::move(ref));
  ev.set("type", Json(type));
  ev.set("reason", Json(reason));
  ev.set("message", Json(msg));
  ev.set("reportingController", Json("xsched"));
  ev.set("count", Json(int64_t{1}));
  ev.set("firstTimestamp", Json(format_rfc3339(now)));
  ev.set("lastTimestamp", Json(format_rfc3339(now)));
  JsonPtr created;
  try {
    created = store_->create("events", std::move(ev));
  } catch (const StoreError&) {
    return;
  }
  const Json& md2 = (*created)["metadata"];
  std::lock_guard<std::mutex> g(events_mu_);
  recent_[std::move(corr)] = Recent{md2["namespace"].as_string(), md2["name"].as_string(), 1, now};
  if (recent_.size() > recent_sweep_at_) {  // amortized: sweep when doubled
    for (auto it = recent_.begin(); it != recent_.end();)
      it = now - it->second.last_us >= kAggregateUs ? recent_.erase(it) : std::next(it);
    recent_sweep_at_ = std::max<size_t>(4096, 2 * recent_.size());
  }
}

}  // namespace xsched
