// Native tests for the lister's gang entries (scheduler/gang.h, Informers).
//
// Seeded random sequences of lister operations over 3 namespaces, 5 group
// names and gangs of 1-8 pods. After every step, what a pod's entry says
// (Informers::gang_count / gang_members / gang_pod_group, and the entry read
// directly) must equal the locked lookups by name (count_pods_in_group_of,
// pods_in_group_of, pod_group_of) and a plain model kept by the test. Pods
// that left the lister and still hold a retired entry must get the by-name
// answer. Once a sequence has deleted everything and released its pods, no
// Gang object is alive. A second test reads entries from several threads
// while the lister changes (the ThreadSanitizer build of this file is what
// gives it teeth).
//
// Built by `python -m flex_gpu_scheduler_amd.build_ext --gang-tests` into
// build/xsched_gang_tests (`--gang-tests-tsan`: build/xsched_gang_tests_tsan)
// and run by tests/test_native_gang.py.
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <functional>
#include <map>
#include <mutex>
#include <random>
#include <set>
#include <string>
#include <thread>
#include <vector>

#include "api/types.h"
#include "common/json.h"
#include "scheduler/gang.h"
#include "scheduler/informers.h"

using namespace xsched;

namespace {

int g_failed = 0, g_checks = 0;
#define CHECK(cond)                                                          \
  do {                                                                       \
    ++g_checks;                                                              \
    if (!(cond)) {                                                           \
      ++g_failed;                                                            \
      std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
    }                                                                        \
  } while (0)
#define CHECK_EQ(a, b) CHECK((a) == (b))

const char* kNs[] = {"alpha", "beta", "gamma"};
const char* kGroups[] = {"g0", "g1", "g2", "g3", "a-group-name-longer-than-the-small-string-buffer"};

int g_uid = 0;
int g_retired_seen = 0, g_live_unlisted_seen = 0;  // the sequences must reach both cases

PodPtr make_pod(const std::string& ns, const std::string& name, const std::string& group, const std::string& node = "") {
  std::string labels = group.empty() ? "{}" : std::string(R"({")") + kPodGroupLabel + R"(":")" + group + R"("})";
  std::string j = R"({"metadata":{"namespace":")" + ns + R"(","name":")" + name + R"(","uid":"u)" +
                  std::to_string(++g_uid) + R"(","labels":)" + labels + R"(},"spec":{"nodeName":")" + node +
                  R"(","containers":[{"name":"c","resources":{"requests":{"cpu":"1"}}}]}})";
  return Pod::from_json(Json::parse(j));
}

PodGroupPtr make_pg(const std::string& ns, const std::string& name, int min_member, int scheduled = 0) {
  std::string j = R"({"metadata":{"namespace":")" + ns + R"(","name":")" + name + R"(","uid":"pg)" +
                  std::to_string(++g_uid) + R"("},"spec":{"minMember":)" + std::to_string(min_member) +
                  R"(},"status":{"scheduled":)" + std::to_string(scheduled) + "}}";
  return PodGroup::from_json(Json::parse(j));
}

// The test's own picture of the lister.
struct Model {
  std::map<std::string, PodPtr> pods;      // "ns/name"
  std::map<std::string, PodGroupPtr> pgs;  // "ns/group"
  std::set<Pod*> members_of(const Pod& p) const {
    std::set<Pod*> out;
    for (const auto& kv : pods)
      if (!kv.second->pod_group.empty() && kv.second->pod_group == p.pod_group && kv.second->ns() == p.ns())
        out.insert(kv.second.get());
    return out;
  }
  PodGroupPtr pg_of(const Pod& p) const {
    if (p.pod_group.empty()) return nullptr;
    auto it = pgs.find(p.ns() + "/" + p.pod_group);
    return it == pgs.end() ? nullptr : it->second;
  }
};

std::set<Pod*> as_set(const std::vector<PodPtr>& v) {
  std::set<Pod*> s;
  for (const auto& p : v) s.insert(p.get());
  CHECK_EQ(s.size(), v.size());  // no pod listed twice
  return s;
}

// Every pod the sequence ever made (`held`), listed or not, against the
// locked lookups and the model.
void verify(const Informers& inf, const Model& m, const std::vector<PodPtr>& held) {
  for (const auto& hp : held) {
    const Pod& p = *hp;
    auto it = m.pods.find(p.key());
    const bool listed = it != m.pods.end() && it->second == hp;
    CHECK_EQ(inf.lists(p), listed);
    const std::set<Pod*> want = p.pod_group.empty() ? std::set<Pod*>{} : m.members_of(p);
    const PodGroupPtr want_pg = m.pg_of(p);
    // The locked lookups (the oracle) agree with the model ...
    CHECK_EQ(inf.count_pods_in_group_of(p), want.size());
    CHECK(as_set(inf.pods_in_group_of(p)) == want);
    CHECK(inf.pod_group_of(p) == want_pg);
    // ... and so does what the pod's entry (or its fallback) says.
    CHECK_EQ(inf.gang_count(p), want.size());
    CHECK(as_set(inf.gang_members(p)) == want);
    CHECK(inf.gang_pod_group(p) == want_pg);
    if (p.pod_group.empty()) {
      CHECK(!p.gang || !listed);
      continue;
    }
    if (listed) {
      // A lister pod's entry is live, is the one the lister finds by name, and
      // answers by itself (no fallback).
      CHECK(p.gang != nullptr);
      if (!p.gang) continue;
      CHECK(!p.gang->retired());
      CHECK(inf.gang_by_name(p) == p.gang);
      CHECK_EQ(p.gang->ns, p.ns());
      CHECK_EQ(p.gang->name, p.pod_group);
      size_t n = ~size_t{0};
      std::vector<PodPtr> mem;
      static const PodGroupPtr kSentinel = make_pg("x", "x", 1);
      PodGroupPtr pg = kSentinel;
      CHECK(p.gang->count(n) && n == want.size());
      CHECK(p.gang->members(mem) && as_set(mem) == want);
      CHECK(p.gang->pod_group(pg) && pg == want_pg);
      // Same order as the locked list (sibling activation follows it).
      std::vector<PodPtr> locked = inf.pods_in_group_of(p);
      CHECK(mem == locked);
    } else if (p.gang && p.gang->retired()) {
      // A retired entry answers nothing by itself.
      ++g_retired_seen;
      size_t n = 77;
      std::vector<PodPtr> mem;
      PodGroupPtr pg;
      CHECK(!p.gang->count(n) && n == 77);
      CHECK(!p.gang->members(mem));
      CHECK(!p.gang->pod_group(pg));
      CHECK(inf.gang_by_name(p) != p.gang);
    } else if (p.gang) {
      ++g_live_unlisted_seen;  // an earlier version of a pod whose group lives on
    }
  }
}

void run_sequence(uint64_t seed, int steps) {
  std::mt19937_64 r(seed);
  const int64_t live_before = Gang::live();
  {
    Informers inf;
    Model m;
    std::vector<PodPtr> held;
    int serial = 0;
    auto pick = [&](size_t n) { return static_cast<size_t>(r() % n); };
    auto rand_ns = [&] { return std::string(kNs[pick(3)]); };
    auto rand_group = [&] { return std::string(kGroups[pick(5)]); };
    auto group_size = [&](const std::string& ns, const std::string& g) {
      size_t n = 0;
      for (const auto& kv : m.pods) n += kv.second->ns() == ns && kv.second->pod_group == g;
      return n;
    };
    auto random_listed = [&]() -> PodPtr {
      if (m.pods.empty()) return nullptr;
      auto it = m.pods.begin();
      std::advance(it, static_cast<long>(pick(m.pods.size())));
      return it->second;
    };
    auto upsert = [&](std::vector<PodPtr> batch) {
      for (const auto& p : batch) held.push_back(p);
      std::vector<PodPtr> want_prev;
      for (const auto& p : batch) {
        auto it = m.pods.find(p->key());
        want_prev.push_back(it == m.pods.end() ? nullptr : it->second);
        m.pods[p->key()] = p;
      }
      if (batch.size() == 1 && (r() & 1)) {
        inf.upsert_pod(batch[0]);
      } else {
        std::vector<PodPtr> prev(batch.size());
        inf.upsert_pods(batch.data(), prev.data(), batch.size());
        CHECK(prev == want_prev);
      }
    };
    for (int step = 0; step < steps; ++step) {
      switch (pick(12)) {
        case 0:
        case 1: {  // new pods: a run of members of one group (gangs of 1-8), or a pod without a group
          std::string ns = rand_ns(), g = pick(6) == 0 ? std::string() : rand_group();
          size_t room = g.empty() ? 1 : 8 - std::min<size_t>(8, group_size(ns, g));
          size_t k = room == 0 ? 0 : 1 + pick(room);
          std::vector<PodPtr> batch;
          for (size_t i = 0; i < k; ++i) batch.push_back(make_pod(ns, "p" + std::to_string(++serial), g));
          if (pick(3) == 0) batch.insert(batch.begin() + static_cast<long>(pick(batch.size() + 1)), PodPtr());  // a hole
          std::vector<PodPtr> prev(batch.size());
          for (const auto& p : batch)
            if (p) {
              held.push_back(p);
              m.pods[p->key()] = p;
            }
          inf.upsert_pods(batch.data(), prev.data(), batch.size());
          for (const auto& p : prev) CHECK(!p);
          break;
        }
        case 2: {  // a replacement under the same key, same group (a new version; sometimes a copy, now bound)
          PodPtr old = random_listed();
          if (!old) break;
          PodPtr np = (r() & 1) ? std::make_shared<Pod>(*old) : make_pod(old->ns(), old->name(), old->pod_group, "node-1");
          np->node_name = "node-1";
          upsert({np});
          break;
        }
        case 3: {  // a replacement whose group label changed or vanished
          PodPtr old = random_listed();
          if (!old) break;
          std::string g = pick(3) == 0 ? std::string() : rand_group();
          if (!g.empty() && g != old->pod_group && group_size(old->ns(), g) >= 8) break;
          upsert({make_pod(old->ns(), old->name(), g)});
          break;
        }
        case 4: {  // the same object again
          PodPtr old = random_listed();
          if (old) upsert({old});
          break;
        }
        case 5: {  // delete_pod
          PodPtr old = random_listed();
          if (!old) break;
          m.pods.erase(old->key());
          inf.delete_pod(*old);
          break;
        }
        case 6: {  // a take_pods run (some keys unknown, some uids stale)
          std::vector<std::string> keys;
          std::vector<std::string> uid_store, node_store;
          std::vector<PodPtr> want;
          for (size_t i = 0, k = 1 + pick(6); i < k; ++i) {
            PodPtr old = random_listed();
            if (!old || pick(5) == 0) {
              keys.push_back("alpha/none" + std::to_string(i));
              uid_store.push_back("x");
              node_store.push_back("");
              want.push_back(nullptr);
              continue;
            }
            if (std::find(keys.begin(), keys.end(), old->key()) != keys.end()) continue;
            const bool stale = pick(4) == 0;
            keys.push_back(old->key());
            uid_store.push_back(stale ? "stale" : old->uid());
            node_store.push_back(old->node_name);
            want.push_back(stale ? nullptr : old);
            m.pods.erase(old->key());
          }
          std::vector<std::string_view> uids(uid_store.begin(), uid_store.end()), nodes(node_store.begin(), node_store.end());
          CHECK(inf.take_pods(keys, uids, nodes) == want);
          break;
        }
        case 7: {  // delete_pods: a whole group at once
          PodPtr old = random_listed();
          if (!old) break;
          std::vector<PodPtr> gone;
          for (const auto& kv : m.pods)
            if (kv.second->ns() == old->ns() && kv.second->pod_group == old->pod_group) gone.push_back(kv.second);
          for (const auto& p : gone) m.pods.erase(p->key());
          inf.delete_pods(gone);
          break;
        }
        case 8:
        case 9: {  // a PodGroup: new (before or after its pods), or a new version of the same object (status)
          std::string ns = rand_ns(), g = rand_group();
          auto it = m.pgs.find(ns + "/" + g);
          PodGroupPtr pg;
          if (it == m.pgs.end()) {
            pg = make_pg(ns, g, 1 + static_cast<int>(pick(8)));
          } else {
            pg = std::make_shared<PodGroup>(*it->second);
            pg->scheduled += 1;
            pg->phase = "Scheduling";
          }
          m.pgs[ns + "/" + g] = pg;
          inf.upsert_pod_group(pg);
          CHECK(inf.pod_group(ns, g) == pg);
          break;
        }
        case 10: {  // a PodGroup deleted, with members left or not
          if (m.pgs.empty()) break;
          auto it = m.pgs.begin();
          std::advance(it, static_cast<long>(pick(m.pgs.size())));
          inf.delete_pod_group(it->first);
          m.pgs.erase(it);
          break;
        }
        case 11: {  // re-created under the same name with a new uid
          if (m.pgs.empty()) break;
          auto it = m.pgs.begin();
          std::advance(it, static_cast<long>(pick(m.pgs.size())));
          PodGroupPtr was = it->second;
          inf.delete_pod_group(it->first);
          PodGroupPtr pg = make_pg(was->meta.ns, was->meta.name, 1 + static_cast<int>(pick(8)));
          CHECK(pg->meta.uid != was->meta.uid);
          inf.upsert_pod_group(pg);
          it->second = pg;
          break;
        }
      }
      verify(inf, m, held);
      CHECK_EQ(inf.pod_count(), m.pods.size());
      CHECK_EQ(inf.pod_groups().size(), m.pgs.size());
      // Now and then the test lets go of pods that left the lister.
      if (pick(40) == 0)
        held.erase(std::remove_if(held.begin(), held.end(),
                                  [&](const PodPtr& p) {
                                    auto it = m.pods.find(p->key());
                                    return it == m.pods.end() || it->second != p;
                                  }),
                   held.end());
    }
    // Everything goes: the pods one way or another, then the PodGroups.
    std::vector<PodPtr> rest;
    for (const auto& kv : m.pods) rest.push_back(kv.second);
    m.pods.clear();
    inf.delete_pods(rest);
    rest.clear();
    for (const auto& kv : m.pgs) inf.delete_pod_group(kv.first);
    m.pgs.clear();
    verify(inf, m, held);
    // Pods still held point at retired entries only.
    for (const auto& p : held) CHECK(!p->gang || p->gang->retired());
    held.clear();
    CHECK_EQ(Gang::live(), live_before);
  }
  CHECK_EQ(Gang::live(), live_before);
}

void random_sequences_match_locked_lookups_and_model() {
  for (uint64_t seed = 1; seed <= 12; ++seed) run_sequence(seed, 350);
  CHECK(g_retired_seen > 1000);
  CHECK(g_live_unlisted_seen > 1000);
}

// A lister destroyed with pods and PodGroups still in it lets go of every
// entry (entries and member pods point at each other).
void lister_destruction_frees_entries() {
  const int64_t live_before = Gang::live();
  std::vector<PodPtr> kept;
  {
    Informers inf;
    inf.upsert_pod_group(make_pg("alpha", "g0", 3));
    for (int i = 0; i < 3; ++i) {
      kept.push_back(make_pod("alpha", "d" + std::to_string(i), "g0"));
      inf.upsert_pod(kept.back());
    }
    inf.upsert_pod_group(make_pg("beta", "g1", 2));
    CHECK_EQ(Gang::live(), live_before + 2);
  }
  for (const auto& p : kept) CHECK(p->gang && p->gang->retired());
  kept.clear();
  CHECK_EQ(Gang::live(), live_before);
}

// Readers on several threads (as the scheduling thread and the binders) go
// through pods' entries while the lister replaces pods, swaps PodGroup
// versions and retires and re-creates the group.
void concurrent_readers_see_consistent_answers() {
  Informers inf;
  constexpr int kMembers = 8;
  std::vector<PodPtr> pods;
  std::mutex pods_mu;
  auto snapshot = [&] {
    std::lock_guard<std::mutex> g(pods_mu);
    return pods;
  };
  inf.upsert_pod_group(make_pg("alpha", "g0", kMembers));
  for (int i = 0; i < kMembers; ++i) {
    pods.push_back(make_pod("alpha", "m" + std::to_string(i), "g0"));
    inf.upsert_pod(pods.back());
  }
  std::atomic<bool> stop{false};
  std::atomic<int> bad{0};
  std::vector<std::thread> readers;
  for (int t = 0; t < 4; ++t)
    readers.emplace_back([&] {
      while (!stop.load(std::memory_order_acquire)) {
        for (const auto& p : snapshot()) {
          const size_t n = inf.gang_count(*p);
          auto mem = inf.gang_members(*p);
          auto pg = inf.gang_pod_group(*p);
          if (n > kMembers || mem.size() > kMembers) bad.fetch_add(1);
          for (const auto& q : mem)
            if (q->pod_group != "g0" || q->ns() != "alpha") bad.fetch_add(1);
          if (pg && (pg->meta.name != "g0" || pg->min_member != kMembers)) bad.fetch_add(1);
        }
      }
    });
  std::mt19937_64 r(5);
  for (int round = 0; round < 300; ++round) {
    const size_t i = r() % kMembers;
    PodPtr np = std::make_shared<Pod>(*snapshot()[i]);  // a bound copy
    np->node_name = "n";
    inf.upsert_pod(np);
    {
      std::lock_guard<std::mutex> g(pods_mu);
      pods[i] = np;
    }
    auto pg = std::make_shared<PodGroup>(*inf.pod_group("alpha", "g0"));
    pg->scheduled += 1;
    inf.upsert_pod_group(pg);  // a status event
    if (round % 50 == 49) {    // the whole gang goes and comes back under the same name
      inf.delete_pods(snapshot());
      inf.delete_pod_group("alpha/g0");
      inf.upsert_pod_group(make_pg("alpha", "g0", kMembers));
      std::vector<PodPtr> fresh;
      for (int k = 0; k < kMembers; ++k) fresh.push_back(make_pod("alpha", "m" + std::to_string(k), "g0"));
      std::vector<PodPtr> prev(fresh.size());
      inf.upsert_pods(fresh.data(), prev.data(), fresh.size());
      std::lock_guard<std::mutex> g(pods_mu);
      pods = fresh;
    }
  }
  stop.store(true, std::memory_order_release);
  for (auto& t : readers) t.join();
  CHECK_EQ(bad.load(), 0);
  for (const auto& p : snapshot()) {
    CHECK_EQ(inf.gang_count(*p), static_cast<size_t>(kMembers));
    CHECK_EQ(inf.count_pods_in_group_of(*p), static_cast<size_t>(kMembers));
  }
}

// The open record lives in the entry: opened once, closed when fn says so,
// gone with the PodGroup, and never reachable through a retired entry.
void record_follows_the_entry() {
  Informers inf;
  auto pg = make_pg("alpha", "g0", 2);
  inf.upsert_pod_group(pg);
  auto a = make_pod("alpha", "a", "g0"), b = make_pod("alpha", "b", "g0");
  inf.upsert_pod(a);
  inf.upsert_pod(b);
  int opened = 0;
  auto open = [&](const PodGroupPtr&, GangRecord* r, bool fresh) {
    CHECK(r != nullptr);
    opened += fresh;
    if (fresh) r->first_enqueue_us = 5;
    return false;
  };
  CHECK(a->gang->with_record(true, nullptr, open));
  CHECK(b->gang->with_record(true, nullptr, open));
  CHECK_EQ(opened, 1);
  GangRecord done;
  CHECK(a->gang->with_record(false, &done, [&](const PodGroupPtr& g, GangRecord* r, bool) {
    CHECK(g == pg);
    CHECK(r && r->pg == "alpha/g0" && r->first_enqueue_us == 5);
    return true;
  }));
  CHECK_EQ(done.pg, std::string("alpha/g0"));
  CHECK(b->gang->with_record(false, nullptr, [&](const PodGroupPtr&, GangRecord* r, bool) {
    CHECK(r == nullptr);  // closed
    return false;
  }));
  // Deleted before admission: the record goes with the PodGroup.
  CHECK(a->gang->with_record(true, nullptr, open));
  CHECK_EQ(opened, 2);
  inf.delete_pod_group("alpha/g0");
  CHECK(a->gang->with_record(false, nullptr, [&](const PodGroupPtr& g, GangRecord* r, bool) {
    CHECK(!g && !r);
    return false;
  }));
  // Retired: not even run.
  GangPtr e = a->gang;
  inf.delete_pod(*a);
  inf.delete_pod(*b);
  CHECK(e->retired());
  CHECK(!e->with_record(true, nullptr, [&](const PodGroupPtr&, GangRecord*, bool) {
    CHECK(false);
    return false;
  }));
}

}  // namespace

int main() {
  struct {
    const char* name;
    void (*fn)();
  } tests[] = {
      {"random_sequences_match_locked_lookups_and_model", random_sequences_match_locked_lookups_and_model},
      {"lister_destruction_frees_entries", lister_destruction_frees_entries},
      {"concurrent_readers_see_consistent_answers", concurrent_readers_see_consistent_answers},
      {"record_follows_the_entry", record_follows_the_entry},
  };
  for (const auto& t : tests) {
    int before = g_failed;
    t.fn();
    std::printf("[%s] %s\n", g_failed == before ? " OK " : "FAIL", t.name);
  }
  std::printf("%d checks, %d failed, %zu tests\n", g_checks, g_failed, sizeof(tests) / sizeof(tests[0]));
  return g_failed == 0 ? 0 : 1;
}
