#include "scheduler/informers.h"

#include <algorithm>
#include <mutex>

namespace xsched {

void Informers::group_remove(const PodPtr& p) {
  auto git = pods_by_group_.find(p->pg_key);
  if (git == pods_by_group_.end()) return;
  auto& v = git->second;
  for (size_t i = 0; i < v.size(); ++i)
    if (v[i] == p) {
      v[i] = std::move(v.back());
      v.pop_back();
      break;
    }
  if (v.empty()) pods_by_group_.erase(git);
}

namespace {
// "ns/name" in a per-thread buffer (no key string per lookup).
std::string_view gang_key_view(std::string_view ns, std::string_view name) {
  thread_local std::string k;
  k.assign(ns);
  k.push_back('/');
  k.append(name);
  return k;
}
}  // namespace

Informers::~Informers() {
  // Entries and their member pods point at each other: cut the entries' side.
  for (auto& kv : gangs_) {
    Gang& e = *kv.second;
    std::lock_guard<AdaptiveMutex> g(e.mu_);
    e.retired_.store(true, std::memory_order_release);
    e.members_.clear();
    e.n_.store(0, std::memory_order_release);
    e.pg_.reset();
    e.has_rec_ = false;
  }
}

GangPtr Informers::find_gang_locked(std::string_view ns, std::string_view name) const {
  auto it = gangs_.find(gang_key_view(ns, name));
  return it == gangs_.end() ? nullptr : it->second;
}

GangPtr Informers::live_gang_locked(GangPtr hint, std::string_view ns, std::string_view name) {
  if (hint && !hint->retired_.load(std::memory_order_relaxed) && hint->ns == ns && hint->name == name) {
    // A prepared entry enters the map here (or yields to the one that is in).
    auto [it, fresh] = gangs_.try_emplace(std::string_view(hint->key), hint);
    return it->second;
  }
  if (GangPtr e = find_gang_locked(ns, name)) return e;
  GangPtr e = std::make_shared<Gang>(ns, name);
  gangs_.emplace(std::string_view(e->key), e);
  return e;
}

// The calling thread's list of what left the lister; emptied (capacity kept)
// by Drain, which is declared before the lock and so runs after it.
Informers::Released& Informers::released() {
  thread_local Released r;
  return r;
}
struct Informers::Drain {
  Released& r;
  ~Drain() {
    r.pods.clear();
    r.gangs.clear();
    r.pgs.clear();
  }
};

void Informers::retire_if_empty_locked(const GangPtr& e, Released& rel) {
  {
    std::lock_guard<AdaptiveMutex> g(e->mu_);
    if (e->pg_ || !e->members_.empty() || e->retired_.load(std::memory_order_relaxed)) return;
    e->retired_.store(true, std::memory_order_release);
    e->has_rec_ = false;
  }
  auto it = gangs_.find(std::string_view(e->key));
  if (it != gangs_.end() && it->second == e) {
    rel.gangs.push_back(std::move(it->second));
    gangs_.erase(it);
  }
}

// Same order of members as group_remove leaves in pods_by_group_: the last
// one moves into the gap.
void Informers::gang_drop_member_locked(const PodPtr& p) {
  Gang* e = p->gang.get();
  if (!e) return;
  std::lock_guard<AdaptiveMutex> g(e->mu_);
  auto& v = e->members_;
  for (size_t i = 0; i < v.size(); ++i)
    if (v[i] == p) {
      v[i] = std::move(v.back());
      v.pop_back();
      e->n_.store(v.size(), std::memory_order_release);
      break;
    }
}

void Informers::gang_remove_locked(const PodPtr& p, Released& rel) {
  if (!p->gang) return;
  gang_drop_member_locked(p);
  retire_if_empty_locked(p->gang, rel);
}

// `p` (the lister's reference, moved out) leaves the group index and its entry.
void Informers::unlist_locked(PodPtr& p, Released& rel) {
  if (p->pg_key) group_remove(p);
  gang_remove_locked(p, rel);
  p->listed.by.store(0, std::memory_order_relaxed);
  rel.pods.push_back(std::move(p));
}

void Informers::upsert_pod(const PodPtr& p) {
  PodPtr prev;
  upsert_pods(&p, &prev, 1);
}

void Informers::upsert_pods(const PodPtr* ps, PodPtr* prev, size_t n) {
  // Before the lock: every pod's key, and the entry of every group named in
  // the run (looked up under the shared lock, allocated where missing).
  // Consecutive pods are mostly members of one gang: one lookup per run.
  thread_local std::vector<std::string> keys;
  thread_local std::vector<GangPtr> entry;  // per pod: its group's entry (null: no group)
  thread_local std::vector<size_t> missing;
  keys.resize(n);
  entry.assign(n, nullptr);
  missing.clear();
  auto same_group = [](const Pod& a, const Pod& b) { return a.pod_group == b.pod_group && a.ns() == b.ns(); };
  {
    std::shared_lock<std::shared_mutex> g(mu_);
    const Pod* last = nullptr;
    size_t last_i = 0;
    for (size_t i = 0; i < n; ++i) {
      if (!ps[i] || ps[i]->pod_group.empty()) continue;
      const Pod& p = *ps[i];
      if (last && same_group(*last, p)) {
        entry[i] = entry[last_i];
        if (!entry[i]) missing.push_back(i);
        continue;
      }
      // The pod's own entry (a copy of a lister pod carries it) needs no lookup.
      if (p.gang && !p.gang->retired() && p.gang->name == p.pod_group && p.gang->ns == p.ns()) entry[i] = p.gang;
      else entry[i] = find_gang_locked(p.ns(), p.pod_group);
      if (!entry[i]) missing.push_back(i);
      last = &p;
      last_i = i;
    }
  }
  for (size_t k = 0; k < missing.size(); ++k) {
    const size_t i = missing[k];
    if (k > 0 && same_group(*ps[missing[k - 1]], *ps[i])) entry[i] = entry[missing[k - 1]];
    else entry[i] = std::make_shared<Gang>(ps[i]->ns(), ps[i]->pod_group);
  }
  for (size_t i = 0; i < n; ++i)
    if (ps[i]) keys[i] = ps[i]->key();
  Released& rel = released();
  Drain drain{rel};
  {
    std::unique_lock<std::shared_mutex> g(mu_);
    for (size_t i = 0; i < n; ++i) {
      const PodPtr& p = ps[i];
      if (!p) continue;
      GangPtr e, was;  // the pod's entry; the entry of the version it replaces
      if (!p->pod_group.empty()) e = live_gang_locked(std::move(entry[i]), p->ns(), p->pod_group);
      auto [it, fresh] = pods_.try_emplace(std::move(keys[i]), p);
      if (!fresh) {
        prev[i] = it->second;
        PodPtr old = std::move(it->second);
        if (old->pg_key) group_remove(old);
        was = old->gang;
        gang_drop_member_locked(old);
        if (old != p) old->listed.by.store(0, std::memory_order_relaxed);
        rel.pods.push_back(std::move(old));
        it->second = p;
      }
      // The pod is in its entry, and points at it, before the lock is released
      // (nothing can find it sooner). The replaced version's entry is looked at
      // only now: a gang of one that is replaced must not retire in between.
      if (e) {
        std::lock_guard<AdaptiveMutex> eg(e->mu_);
        // One block for the whole gang where its PodGroup says how many come.
        if (e->members_.capacity() == 0 && e->pg_)
          e->members_.reserve(static_cast<size_t>(std::clamp(e->pg_->min_member, 1, 64)));
        e->members_.push_back(p);
        e->n_.store(e->members_.size(), std::memory_order_release);
      }
      if (was && was != e) retire_if_empty_locked(was, rel);
      if (p->gang != e) p->gang = std::move(e);
      p->listed.by.store(instance_, std::memory_order_relaxed);
      if (p->pg_key) pods_by_group_[p->pg_key].push_back(p);
    }
  }
  for (auto& e : entry) e.reset();
}

void Informers::delete_pod(const Pod& p) {
  const std::string key = p.key();
  Released& rel = released();
  Drain drain{rel};
  std::unique_lock<std::shared_mutex> g(mu_);
  auto it = pods_.find(key);
  if (it == pods_.end()) return;
  unlist_locked(it->second, rel);
  pods_.erase(it);
  g.unlock();
}

void Informers::delete_pods(const std::vector<PodPtr>& ps) {
  std::vector<std::string> keys;
  keys.reserve(ps.size());
  for (const auto& p : ps) keys.push_back(p->key());
  Released& rel = released();
  Drain drain{rel};
  std::unique_lock<std::shared_mutex> g(mu_);
  for (const auto& key : keys) {
    auto it = pods_.find(key);
    if (it == pods_.end()) continue;
    unlist_locked(it->second, rel);
    pods_.erase(it);
  }
  g.unlock();
}

std::vector<PodPtr> Informers::take_pods(const std::vector<std::string>& keys, const std::vector<std::string_view>& uids,
                                         const std::vector<std::string_view>& nodes) {
  std::vector<PodPtr> out(keys.size());
  Released& rel = released();
  Drain drain{rel};
  std::unique_lock<std::shared_mutex> g(mu_);
  for (size_t k = 0; k < keys.size(); ++k) {
    auto it = pods_.find(keys[k]);
    if (it == pods_.end()) continue;
    PodPtr p = it->second;
    unlist_locked(it->second, rel);
    pods_.erase(it);
    if (p->uid() == uids[k] && p->node_name == nodes[k]) out[k] = std::move(p);
  }
  g.unlock();
  return out;
}

void Informers::upsert_pod_group(const PodGroupPtr& pg) {
  const std::string& ns = pg->meta.ns;
  const std::string& name = pg->meta.name;
  PodGroupPtr old = pg;  // swapped with the entry's; the previous object is released after the locks
  {
    // An entry that exists takes the object under its own lock: the map is
    // only read. Every status event (WatchEvent::status_only, which our own
    // PostBind PATCH produces, twice per gang) ends here.
    std::shared_lock<std::shared_mutex> g(mu_);
    if (GangPtr e = find_gang_locked(ns, name)) {
      std::lock_guard<AdaptiveMutex> eg(e->mu_);
      e->pg_.swap(old);
      return;
    }
  }
  GangPtr fresh = std::make_shared<Gang>(ns, name);
  std::unique_lock<std::shared_mutex> g(mu_);
  GangPtr e = live_gang_locked(std::move(fresh), ns, name);
  std::lock_guard<AdaptiveMutex> eg(e->mu_);
  e->pg_.swap(old);
}

void Informers::delete_pod_group(const std::string& key) {
  Released& rel = released();
  Drain drain{rel};
  std::unique_lock<std::shared_mutex> g(mu_);
  auto it = gangs_.find(std::string_view(key));
  if (it == gangs_.end()) return;
  GangPtr e = it->second;
  {
    // The group's open record goes with its PodGroup: a later PodGroup of the
    // same name starts its own timeline.
    std::lock_guard<AdaptiveMutex> eg(e->mu_);
    if (e->pg_) rel.pgs.push_back(std::move(e->pg_));
    e->pg_.reset();
    e->has_rec_ = false;
  }
  retire_if_empty_locked(e, rel);
  g.unlock();
}
void Informers::upsert_elastic_quota(const ElasticQuotaPtr& eq) {
  std::unique_lock<std::shared_mutex> g(mu_);
  eqs_[eq->meta.key()] = eq;
}
void Informers::delete_elastic_quota(const std::string& key) {
  std::unique_lock<std::shared_mutex> g(mu_);
  eqs_.erase(key);
}
void Informers::upsert_nrt(const NRTPtr& n) {
  std::unique_lock<std::shared_mutex> g(mu_);
  nrts_[n->meta.name] = n;
}
void Informers::delete_nrt(const std::string& name) {
  std::unique_lock<std::shared_mutex> g(mu_);
  nrts_.erase(name);
}
void Informers::upsert_pdb(const PDBPtr& p) {
  std::unique_lock<std::shared_mutex> g(mu_);
  pdbs_[p->meta.key()] = p;
}
void Informers::delete_pdb(const std::string& key) {
  std::unique_lock<std::shared_mutex> g(mu_);
  pdbs_.erase(key);
}
void Informers::upsert_priority_class(const PriorityClassPtr& pc) {
  std::unique_lock<std::shared_mutex> g(mu_);
  pcs_[pc->meta.name] = pc;
}
void Informers::delete_priority_class(const std::string& name) {
  std::unique_lock<std::shared_mutex> g(mu_);
  pcs_.erase(name);
}

PodPtr Informers::pod(const std::string& ns, const std::string& name) const {
  thread_local std::string key;  // no key allocation per lookup
  key.assign(ns);
  key.push_back('/');
  key.append(name);
  std::shared_lock<std::shared_mutex> g(mu_);
  auto it = pods_.find(key);
  return it == pods_.end() ? nullptr : it->second;
}

namespace {
uint64_t group_hash(const std::string& ns, const std::string& pg) {
  std::string full;
  full.reserve(ns.size() + 1 + pg.size());
  full.append(ns).push_back('/');
  full.append(pg);
  return pg_key_of(full);
}
}  // namespace

std::vector<PodPtr> Informers::pods_in_group(const std::string& ns, const std::string& pg) const {
  std::vector<PodPtr> out;
  const uint64_t key = group_hash(ns, pg);
  std::shared_lock<std::shared_mutex> g(mu_);
  auto git = pods_by_group_.find(key);
  if (git == pods_by_group_.end()) return out;
  out.reserve(git->second.size());
  for (const auto& p : git->second)
    if (p->pod_group == pg && p->ns() == ns) out.push_back(p);
  return out;
}

size_t Informers::count_pods_in_group(const std::string& ns, const std::string& pg) const {
  const uint64_t key = group_hash(ns, pg);
  std::shared_lock<std::shared_mutex> g(mu_);
  auto git = pods_by_group_.find(key);
  if (git == pods_by_group_.end()) return 0;
  size_t n = 0;
  for (const auto& p : git->second) n += p->pod_group == pg && p->ns() == ns;
  return n;
}

std::vector<PodPtr> Informers::pods_in_group_of(const Pod& p) const {
  std::vector<PodPtr> out;
  if (!p.pg_key) return out;
  std::shared_lock<std::shared_mutex> g(mu_);
  auto git = pods_by_group_.find(p.pg_key);
  if (git == pods_by_group_.end()) return out;
  out.reserve(git->second.size());
  for (const auto& q : git->second)
    if (q->pod_group == p.pod_group && q->ns() == p.ns()) out.push_back(q);
  return out;
}

size_t Informers::count_pods_in_group_of(const Pod& p) const {
  if (!p.pg_key) return 0;
  std::shared_lock<std::shared_mutex> g(mu_);
  auto git = pods_by_group_.find(p.pg_key);
  if (git == pods_by_group_.end()) return 0;
  size_t n = 0;
  for (const auto& q : git->second) n += q->pod_group == p.pod_group && q->ns() == p.ns();
  return n;
}

std::vector<PodPtr> Informers::all_pods() const {
  std::shared_lock<std::shared_mutex> g(mu_);
  std::vector<PodPtr> out;
  out.reserve(pods_.size());
  for (const auto& kv : pods_) out.push_back(kv.second);
  return out;
}

size_t Informers::pod_count() const {
  std::shared_lock<std::shared_mutex> g(mu_);
  return pods_.size();
}

PodGroupPtr Informers::pod_group(const std::string& ns, const std::string& name) const {
  std::shared_lock<std::shared_mutex> g(mu_);
  GangPtr e = find_gang_locked(ns, name);
  if (!e) return nullptr;
  std::lock_guard<AdaptiveMutex> eg(e->mu_);
  return e->pg_;
}

PodGroupPtr Informers::pod_group_of(const Pod& p) const {
  if (!p.pg_key) return nullptr;
  return pod_group(p.ns(), p.pod_group);
}

std::vector<PodGroupPtr> Informers::pod_groups() const {
  std::shared_lock<std::shared_mutex> g(mu_);
  std::vector<PodGroupPtr> out;
  for (const auto& kv : gangs_) {
    std::lock_guard<AdaptiveMutex> eg(kv.second->mu_);
    if (kv.second->pg_) out.push_back(kv.second->pg_);
  }
  return out;
}

GangPtr Informers::gang_by_name(const Pod& p) const {
  if (p.pod_group.empty()) return nullptr;
  std::shared_lock<std::shared_mutex> g(mu_);
  return find_gang_locked(p.ns(), p.pod_group);
}

PodGroupPtr Informers::gang_pod_group(const Pod& p) const {
  PodGroupPtr pg;
  if (p.gang && p.gang->pod_group(pg)) return pg;
  return pod_group_of(p);
}

size_t Informers::gang_count(const Pod& p) const {
  size_t n = 0;
  if (p.gang && p.gang->count(n)) return n;
  return count_pods_in_group_of(p);
}

std::vector<PodPtr> Informers::gang_members(const Pod& p) const {
  std::vector<PodPtr> out;
  if (p.gang && p.gang->members(out)) return out;
  return pods_in_group_of(p);
}

ElasticQuotaPtr Informers::elastic_quota_for_namespace(const std::string& ns) const {
  std::shared_lock<std::shared_mutex> g(mu_);
  auto it = eqs_.lower_bound(ns + "/");
  if (it != eqs_.end() && it->second->meta.ns == ns) return it->second;
  return nullptr;
}

std::vector<ElasticQuotaPtr> Informers::elastic_quotas() const {
  std::shared_lock<std::shared_mutex> g(mu_);
  std::vector<ElasticQuotaPtr> out;
  for (const auto& kv : eqs_) out.push_back(kv.second);
  return out;
}

NRTPtr Informers::nrt(const std::string& node) const {
  std::shared_lock<std::shared_mutex> g(mu_);
  auto it = nrts_.find(node);
  return it == nrts_.end() ? nullptr : it->second;
}

std::vector<PDBPtr> Informers::pdbs() const {
  std::shared_lock<std::shared_mutex> g(mu_);
  std::vector<PDBPtr> out;
  for (const auto& kv : pdbs_) out.push_back(kv.second);
  return out;
}

PriorityClassPtr Informers::priority_class(const std::string& name) const {
  std::shared_lock<std::shared_mutex> g(mu_);
  auto it = pcs_.find(name);
  return it == pcs_.end() ? nullptr : it->second;
}

// ------------------------------------------------------------- storage ----
void Informers::upsert_pv(const PVPtr& pv) {
  std::unique_lock<std::shared_mutex> g(mu_);
  auto it = pvs_.find(pv->meta.name);
  if (it != pvs_.end()) {
    auto& old = pvs_by_class_[it->second->storage_class];
    std::erase(old, it->second);
    it->second = pv;
  } else {
    pvs_.emplace(pv->meta.name, pv);
  }
  pvs_by_class_[pv->storage_class].push_back(pv);
}

void Informers::delete_pv(const std::string& name) {
  std::unique_lock<std::shared_mutex> g(mu_);
  auto it = pvs_.find(name);
  if (it == pvs_.end()) return;
  std::erase(pvs_by_class_[it->second->storage_class], it->second);
  pvs_.erase(it);
}

void Informers::upsert_pvc(const PVCPtr& pvc) {
  std::unique_lock<std::shared_mutex> g(mu_);
  pvcs_[pvc->meta.key()] = pvc;
}

void Informers::delete_pvc(const std::string& key) {
  std::unique_lock<std::shared_mutex> g(mu_);
  pvcs_.erase(key);
}

void Informers::upsert_storage_class(const StorageClassPtr& sc) {
  std::unique_lock<std::shared_mutex> g(mu_);
  scs_[sc->meta.name] = sc;
}

void Informers::delete_storage_class(const std::string& name) {
  std::unique_lock<std::shared_mutex> g(mu_);
  scs_.erase(name);
}

void Informers::upsert_csinode(const CSINodePtr& n) {
  std::unique_lock<std::shared_mutex> g(mu_);
  csinodes_[n->meta.name] = n;
}

void Informers::delete_csinode(const std::string& name) {
  std::unique_lock<std::shared_mutex> g(mu_);
  csinodes_.erase(name);
}

PVPtr Informers::pv(const std::string& name) const {
  std::shared_lock<std::shared_mutex> g(mu_);
  auto it = pvs_.find(name);
  return it == pvs_.end() ? nullptr : it->second;
}

PVCPtr Informers::pvc(const std::string& ns, const std::string& name) const {
  std::shared_lock<std::shared_mutex> g(mu_);
  auto it = pvcs_.find(ns + "/" + name);
  return it == pvcs_.end() ? nullptr : it->second;
}

StorageClassPtr Informers::storage_class(const std::string& name) const {
  std::shared_lock<std::shared_mutex> g(mu_);
  auto it = scs_.find(name);
  return it == scs_.end() ? nullptr : it->second;
}

CSINodePtr Informers::csinode(const std::string& name) const {
  std::shared_lock<std::shared_mutex> g(mu_);
  auto it = csinodes_.find(name);
  return it == csinodes_.end() ? nullptr : it->second;
}

std::vector<PVPtr> Informers::pvs_of_class(const std::string& cls) const {
  std::shared_lock<std::shared_mutex> g(mu_);
  auto it = pvs_by_class_.find(cls);
  return it == pvs_by_class_.end() ? std::vector<PVPtr>{} : it->second;
}

}  // namespace xsched
