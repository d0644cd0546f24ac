// Native unit tests for the C++ core (no Python in the loop): Quantity, JSON,
// RecycledMap against the std containers and a counting allocator, the GPU
// ledger's incremental aggregates (checked against a brute-force
// recomputation over random assignment sequences), the pod heap and
// scheduling-queue backoff under a fake clock, the timer service, CycleState
// memo invalidation, store watch replay/expiry, PodGroup-aligned chunked
// creates and the parallelizer's inline-vs-parallel cost model.
//
// Built by `python -m flex_gpu_scheduler_amd.build_ext --tests` into
// build/xsched_native_tests and run by tests/test_native_unit.py.
#include <algorithm>
#include <cstdio>
#include <chrono>
#include <functional>
#include <iterator>
#include <map>
#include <memory>
#include <mutex>
#include <set>
#include <thread>
#include <random>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "api/types.h"
#include "framework/plugin.h"
#include "common/clock.h"
#include "common/json.h"
#include "common/parallel.h"
#include "common/quantity.h"
#include "common/recycled_map.h"
#include "framework/types.h"
#include "scheduler/cache.h"
#include "scheduler/queue.h"
#include "scheduler/scheduler.h"
#include "store/store.h"

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

struct TestCase {
  const char* name;
  std::function<void()> fn;
};
std::vector<TestCase>& tests() {
  static std::vector<TestCase> t;
  return t;
}
struct Reg {
  Reg(const char* n, std::function<void()> f) { tests().push_back({n, std::move(f)}); }
};
#define TEST(name)            \
  void name();                \
  Reg reg_##name(#name, name); \
  void name()

// ------------------------------------------------------------------ Quantity
TEST(quantity_parse_format) {
  CHECK_EQ(Quantity::parse("1536Mi").str(), "1536Mi");
  CHECK_EQ(Quantity::parse("2048Mi").str(), "2Gi");
  CHECK_EQ(Quantity::parse("1.5").str(), "1500m");
  CHECK_EQ(Quantity::parse("500m").milli_value(), 500);
  CHECK_EQ(Quantity::parse("500m").value(), 1);  // rounds up
  CHECK_EQ(Quantity::parse("288Gi").value(), 288LL << 30);
  Quantity a = Quantity::parse("1"), b = Quantity::parse("250m");
  a.add(b);
  CHECK_EQ(a.milli_value(), 1250);
  a.sub(Quantity::parse("2"));
  CHECK_EQ(a.sign(), -1);
  Quantity bad;
  CHECK(!Quantity::try_parse("1.2.3", &bad));
}

// ------------------------------------------------------------- NodeStatusMap
TEST(node_status_map_matches_unordered_map) {
  NodeStatusMap m;
  std::unordered_map<std::string, Code> ref;
  m.reserve(3);  // grows past the reservation below
  for (int i = 0; i < 5000; ++i) {
    std::string n = "node-" + std::to_string(i * 7 % 5003);
    Code c = i % 3 ? Code::Unschedulable : Code::UnschedulableAndUnresolvable;
    bool fresh = m.emplace(n, Status(c, "r")).second;
    CHECK_EQ(fresh, ref.emplace(n, c).second);
  }
  CHECK_EQ(m.size(), ref.size());
  for (const auto& [n, c] : ref) {
    auto it = m.find(n);
    CHECK(it != m.end() && it->first == n && it->second.code() == c);
  }
  CHECK(m.find("node-missing") == m.end());
  CHECK_EQ(m.count("node-missing"), 0u);
  m["node-0"] = Status(Code::Error, "e");  // overwrite through operator[]
  CHECK(m.find("node-0")->second.code() == Code::Error);
  m["brand-new"] = Status(Code::Unschedulable, "u");
  CHECK_EQ(m.size(), ref.size() + 1);
  size_t seen = 0;
  for (const auto& [n, st] : m) seen += !n.empty();
  CHECK_EQ(seen, m.size());
  m.clear();
  CHECK(m.empty() && m.find("node-0") == m.end());
}

// --------------------------------------------------------------- RecycledMap
// Keys for the model checks: a small pool so that keys repeat; every third one
// is longer than the small-string buffer.
std::string pool_key(uint32_t i) { return (i % 3 ? "k" : std::string(40, 'x')) + std::to_string(i); }

template <class R, class Ref>
void check_same_unique(const R& m, const Ref& ref) {
  CHECK_EQ(m.size(), ref.size());
  CHECK_EQ(m.empty(), ref.empty());
  CHECK(m.container() == ref);
  size_t seen = 0;
  for (auto it = m.begin(); it != m.end(); ++it) ++seen;
  CHECK_EQ(seen, ref.size());
}

TEST(recycled_map_matches_std_containers) {
  std::mt19937 rng(7);
  {  // string -> int, keys short and long
    using C = std::unordered_map<std::string, int>;
    RecycledMap<C> m;
    C ref;
    for (int step = 0; step < 4000; ++step) {
      std::string k = pool_key(rng() % 48);
      uint32_t op = rng() % 100;
      if (op < 50) {  // acquire, also of a key that is present
        auto [it, fresh] = m.acquire(k);
        auto [rit, rfresh] = ref.try_emplace(k);
        CHECK_EQ(fresh, rfresh);
        CHECK(it->first == k);
        if (fresh) CHECK_EQ(it->second, 0);  // scrubbed or value-initialised
        else CHECK_EQ(it->second, rit->second);  // a present entry is left alone
        it->second = rit->second = static_cast<int>(rng() % 1000) + 1;
      } else if (op < 75) {
        CHECK_EQ(m.release(k), ref.erase(k) > 0);
      } else if (op < 98) {
        auto it = m.find(k);
        CHECK_EQ(it != m.end(), ref.count(k) > 0);
        CHECK_EQ(m.count(k), ref.count(k));
        CHECK_EQ(m.contains(k), ref.count(k) > 0);
        if (it != m.end()) {
          m.release(it);
          ref.erase(k);
        }
      } else {
        m.release_all();
        ref.clear();
      }
      check_same_unique(m, ref);
    }
  }
  {  // uint64_t -> vector
    using C = std::unordered_map<uint64_t, std::vector<int>>;
    RecycledMap<C> m;
    C ref;
    for (int step = 0; step < 4000; ++step) {
      uint64_t k = rng() % 48 * 0x9E3779B97F4A7C15ull;
      uint32_t op = rng() % 100;
      if (op < 60) {
        auto [it, fresh] = m.acquire(k);
        auto [rit, rfresh] = ref.try_emplace(k);
        CHECK_EQ(fresh, rfresh);
        if (fresh) CHECK(it->second.empty());
        int v = static_cast<int>(rng() % 1000);
        it->second.push_back(v);
        rit->second.push_back(v);
      } else if (op < 98) {
        CHECK_EQ(m.release(k), ref.erase(k) > 0);
      } else {
        m.release_all();
        ref.clear();
      }
      check_same_unique(m, ref);
    }
  }
  {  // set of strings
    using C = std::unordered_set<std::string>;
    RecycledMap<C> m;
    C ref;
    for (int step = 0; step < 4000; ++step) {
      std::string k = pool_key(rng() % 48);
      uint32_t op = rng() % 100;
      if (op < 55) {
        auto [it, fresh] = m.acquire(k);
        CHECK_EQ(fresh, ref.insert(k).second);
        CHECK(*it == k);
      } else if (op < 97) {
        CHECK_EQ(m.release(k), ref.erase(k) > 0);
      } else {
        m.release_all();
        ref.clear();
      }
      check_same_unique(m, ref);
    }
  }
  {  // multimap: equal keys keep insertion order, as std::multimap's emplace
    using C = std::multimap<int64_t, uint64_t>;
    RecycledMap<C> m;
    C ref;
    uint64_t next = 1;
    for (int step = 0; step < 4000; ++step) {
      uint32_t op = rng() % 100;
      if (op < 55 || ref.empty()) {
        int64_t k = rng() % 16;
        auto it = m.acquire(k, next);
        auto rit = ref.emplace(k, next);
        ++next;
        CHECK(*it == *rit);
        CHECK_EQ(std::distance(m.begin(), it), std::distance(ref.begin(), rit));
      } else if (op < 98) {
        size_t n = rng() % ref.size();
        m.release(std::next(m.begin(), n));
        ref.erase(std::next(ref.begin(), n));
      } else {
        m.release_all();
        ref.clear();
      }
      CHECK_EQ(m.size(), ref.size());
      CHECK_EQ(m.empty(), ref.empty());
      CHECK(std::equal(m.begin(), m.end(), ref.begin(), ref.end()));  // contents and order
    }
  }
}

TEST(recycled_map_release_drops_references) {
  auto target = std::make_shared<int>(1);
  const long before = target.use_count();
  struct Holder {
    std::shared_ptr<int> p;
    int extra = 0;
  };
  RecycledMap<std::unordered_map<std::string, std::shared_ptr<int>>> direct;
  RecycledMap<std::unordered_map<uint64_t, Holder>> held;
  RecycledMap<std::unordered_map<uint64_t, std::vector<std::shared_ptr<int>>>> listed;
  RecycledMap<std::multimap<int64_t, std::shared_ptr<int>>> ordered;
  for (int round = 0; round < 2; ++round) {
    for (uint64_t i = 0; i < 3; ++i) {
      direct.acquire(pool_key(i)).first->second = target;
      held.acquire(i).first->second = Holder{target, 1};
      listed.acquire(i).first->second.push_back(target);
      ordered.acquire(5, target);
    }
    CHECK_EQ(target.use_count(), before + 12);
    if (round == 0) {
      for (uint64_t i = 0; i < 3; ++i) {
        direct.release(pool_key(i));
        held.release(held.find(i));
        listed.release(i);
        ordered.release(ordered.begin());
      }
    } else {
      direct.release_all();
      held.release_all();
      listed.release_all();
      ordered.release_all();
    }
    CHECK_EQ(target.use_count(), before);  // parked nodes hold nothing
    CHECK_EQ(direct.parked(), 3u);
  }
  // A reused node comes back scrubbed.
  auto [it, fresh] = held.acquire(9);
  CHECK(fresh && !it->second.p && it->second.extra == 0);
}

size_t g_counted_allocs = 0;
template <class T>
struct CountingAlloc {
  using value_type = T;
  CountingAlloc() = default;
  template <class U>
  CountingAlloc(const CountingAlloc<U>&) {}
  T* allocate(size_t n) {
    ++g_counted_allocs;
    return std::allocator<T>().allocate(n);
  }
  void deallocate(T* p, size_t n) { std::allocator<T>().deallocate(p, n); }
  template <class U>
  bool operator==(const CountingAlloc<U>&) const { return true; }
  template <class U>
  bool operator!=(const CountingAlloc<U>&) const { return false; }
};
template <class K, class V>
using CountedMap = std::unordered_map<K, V, std::hash<K>, std::equal_to<K>, CountingAlloc<std::pair<const K, V>>>;

TEST(recycled_map_steady_state_allocates_nothing) {
  constexpr int N = 64;
  using IntVec = std::vector<int, CountingAlloc<int>>;
  RecycledMap<CountedMap<std::string, int>> by_name;  // keys fit the small-string buffer
  RecycledMap<CountedMap<uint64_t, IntVec>> lists;
  using Str = std::string;
  RecycledMap<std::unordered_set<Str, std::hash<Str>, std::equal_to<Str>, CountingAlloc<Str>>> names;
  using HeapAlloc = CountingAlloc<std::pair<const int64_t, uint64_t>>;
  RecycledMap<std::multimap<int64_t, uint64_t, std::less<int64_t>, HeapAlloc>> heap;
  auto name = [](int i) { return "p-" + std::to_string(i); };
  auto fill = [&](int shift) {
    for (int i = 0; i < N; ++i) {
      by_name.acquire(name(i + shift)).first->second = i;
      auto& v = lists.acquire(static_cast<uint64_t>(i + shift)).first->second;
      if (shift) {
        CHECK(v.empty());
        CHECK_EQ(v.capacity(), 8u);  // the capacity it was released with
      } else {
        v.reserve(8);
      }
      v.assign(8, i);
      names.acquire(name(i + shift));
      heap.acquire(i % 7, static_cast<uint64_t>(i));
    }
  };
  auto drain = [&](bool all) {
    if (all) {
      by_name.release_all();
      lists.release_all();
      names.release_all();
      heap.release_all();
      return;
    }
    while (!by_name.empty()) by_name.release(by_name.begin());
    while (!lists.empty()) lists.release(lists.begin()->first);
    while (!names.empty()) names.release(*names.begin());
    while (!heap.empty()) heap.release(heap.begin());
  };
  fill(0);  // warm-up: nodes, bucket arrays and vector buffers are made here
  drain(false);
  CHECK(g_counted_allocs > 0);
  const size_t warm = g_counted_allocs;
  for (int round = 1; round <= N; ++round) {
    fill(round);
    CHECK_EQ(by_name.size(), size_t(N));
    drain(round % 2 == 0);
  }
  CHECK_EQ(g_counted_allocs, warm);
}

TEST(recycled_map_cap_bounds_parked_nodes) {
  RecycledMap<CountedMap<uint64_t, int>> m(/*cap=*/4);
  for (uint64_t i = 0; i < 10; ++i) m.acquire(i);
  for (uint64_t i = 0; i < 10; ++i) m.release(i);
  CHECK_EQ(m.parked(), 4u);
  const size_t before = g_counted_allocs;
  for (uint64_t i = 0; i < 10; ++i) CHECK(m.acquire(i + 100).second);
  CHECK_EQ(g_counted_allocs - before, 6u);  // 4 came from the parked nodes
  CHECK_EQ(m.parked(), 0u);
  CHECK_EQ(m.size(), 10u);
}

// ---------------------------------------------------------------------- JSON
TEST(json_roundtrip_and_merge_patch) {
  Json j = Json::parse(R"({"a":[1,2,{"b":null}],"c":"x\"y","d":{"e":1.5,"f":true}})");
  CHECK_EQ(Json::parse(j.dump()).dump(), j.dump());
  Json p = Json::parse(R"({"c":null,"d":{"e":2,"g":"new"}})");
  j.merge_patch(p);
  CHECK(!j.get("c"));
  CHECK_EQ(j["d"]["e"].as_int(), 2);
  CHECK_EQ(j["d"]["g"].as_string(), "new");
  CHECK(j["d"]["f"].as_bool());
  Json from = Json::parse(R"({"a":1,"b":{"c":2,"d":3}})"), to = Json::parse(R"({"a":1,"b":{"c":5},"e":[1]})");
  Json diff = Json::diff_merge_patch(from, to);
  Json applied = from;
  applied.merge_patch(diff);
  CHECK_EQ(applied.dump(), to.dump());
}

// ----------------------------------------------------------------- GpuLedger
GpuLedger::GpuFree brute(const GpuLedger& L, int g) {
  GpuLedger::GpuFree f;
  if (L.monopoly[g] > 0) return f;
  bool untouched = true;
  for (int p = 0; p < L.parts[g]; ++p) {
    const auto& s = L.slots[L.offset[g] + p];
    if (s.exclusive || s.used_mem || s.mem_pods) untouched = false;
    if (!s.exclusive && !s.used_mem && !s.mem_pods) {
      ++f.free_slots;
      f.xcds += L.xcds_per_part(g);
    }
    if (!s.exclusive) {
      f.mem += L.part_mem(g) - s.used_mem;
      f.max_slot_mem = std::max(f.max_slot_mem, L.part_mem(g) - s.used_mem);
    }
  }
  f.whole = L.parts[g] == 1 && untouched;
  return f;
}

TEST(gpu_ledger_aggregates_match_bruteforce) {
  std::mt19937 rng(7);
  for (int trial = 0; trial < 50; ++trial) {
    Node n;
    n.gpu_count = 8;
    n.gpu_memory_per_gpu = 288;
    const int modes[] = {1, 2, 4, 8};
    for (int g = 0; g < 8; ++g) {
      n.gpu_partitions.push_back(modes[rng() % 4]);
      n.gpu_numa.push_back(g / 4);
    }
    GpuLedger L;
    L.init(n);
    std::vector<GpuAssignment> live;
    for (int step = 0; step < 200; ++step) {
      if (!live.empty() && rng() % 3 == 0) {
        size_t i = rng() % live.size();
        L.apply(live[i], -1);
        live.erase(live.begin() + static_cast<long>(i));
      } else {
        GpuAssignment a;
        int g = static_cast<int>(rng() % 8);
        switch (rng() % 3) {
          case 0:
            a.kind = GpuAssignment::Kind::WholeGpu;
            a.gpus = {g};
            break;
          case 1:
            a.kind = GpuAssignment::Kind::Partition;
            a.gpus = {g};
            a.partitions = {{g, static_cast<int>(rng() % static_cast<unsigned>(n.gpu_partitions[g]))}};
            break;
          default:
            a.kind = GpuAssignment::Kind::Memory;
            a.gpus = {g};
            a.partitions = {{g, static_cast<int>(rng() % static_cast<unsigned>(n.gpu_partitions[g]))}};
            a.memory = 1 + rng() % 20;
        }
        L.apply(a, +1);
        live.push_back(a);
      }
      int whole = 0, xcds = 0;
      int64_t mem = 0;
      int zw[2] = {0, 0}, zx[2] = {0, 0};
      for (int g = 0; g < 8; ++g) {
        auto b = brute(L, g);
        CHECK_EQ(L.free[g].whole, b.whole);
        CHECK_EQ(L.free[g].free_slots, b.free_slots);
        CHECK_EQ(L.free[g].xcds, b.xcds);
        CHECK_EQ(L.free[g].mem, b.mem);
        CHECK_EQ(L.free[g].max_slot_mem, b.max_slot_mem);
        whole += b.whole;
        xcds += b.xcds;
        mem += b.mem;
        zw[g / 4] += b.whole;
        zx[g / 4] += b.xcds;
      }
      CHECK_EQ(L.free_gpus(), whole);
      CHECK_EQ(L.free_xcds(), xcds);
      CHECK_EQ(L.free_memory(), mem);
      CHECK_EQ(L.zone_whole[0], zw[0]);
      CHECK_EQ(L.zone_xcds[1], zx[1]);
    }
  }
}

// --------------------------------------------------------------- PodHeap/queue
PodPtr mk_pod(const std::string& name, int prio) {
  Json j = Json::parse(R"({"metadata":{"namespace":"d","name":")" + name + R"(","uid":")" + name +
                       R"("},"spec":{"priority":)" + std::to_string(prio) + R"(,"containers":[{"name":"c"}]}})");
  return Pod::from_json(j);
}

TEST(pod_heap_orders_and_updates) {
  PodHeap h([](const QueuedPodInfo& a, const QueuedPodInfo& b) { return a.pod->priority > b.pod->priority; });
  for (int i = 0; i < 20; ++i) {
    auto q = std::make_shared<QueuedPodInfo>();
    q->pod = mk_pod("p" + std::to_string(i), (i * 7) % 11);
    h.push(q);
  }
  auto upd = std::make_shared<QueuedPodInfo>();
  upd->pod = mk_pod("p3", 100);
  h.push(upd);  // update in place
  CHECK_EQ(h.size(), 20u);
  CHECK_EQ(h.pop()->pod->name(), "p3");
  int last = 1 << 30;
  while (!h.empty()) {
    int p = h.pop()->pod->priority;
    CHECK(p <= last);
    last = p;
  }
}

TEST(queue_backoff_and_unschedulable_flush) {
  auto clock = std::make_shared<FakeClock>();
  Nominator nom;
  QueueOptions o;
  SchedulingQueue q([](const QueuedPodInfo& a, const QueuedPodInfo& b) { return a.pod->priority > b.pod->priority; },
                    clock, o, &nom);
  q.add(mk_pod("a", 1));
  auto qa = q.pop(0);
  CHECK(qa && qa->pod->name() == "a");
  qa->unschedulable_plugins = {"X"};
  q.add_unschedulable_if_not_present(qa, q.scheduling_cycle());
  CHECK_EQ(q.counts().unschedulable, 1u);
  // An event nobody registered leaves it where it is; a wildcard moves it to backoff.
  q.move_all_to_active_or_backoff(ClusterEvent{"*", kAll, ""});
  CHECK_EQ(q.counts().unschedulable + q.counts().backoff + q.counts().active, 1u);
  q.flush_backoff_completed();
  clock->advance_us(1'100'000);
  q.flush_backoff_completed();
  auto again = q.pop(0);
  CHECK(again && again->pod->name() == "a");
  // Leftover flush after 60 s.
  again->unschedulable_plugins = {"Y"};
  q.add_unschedulable_if_not_present(again, q.scheduling_cycle());
  clock->advance_us(61'000'000);
  q.flush_unschedulable_leftover();
  q.flush_backoff_completed();
  CHECK_EQ(q.counts().unschedulable, 0u);
  q.close();
}

// An activation that arrives while the pod is in flight (popped, cycle not yet
// failed) must survive until the failure is recorded: the pod goes straight to
// activeQ instead of parking in unschedulableQ until the 60 s flush.
TEST(queue_activation_while_in_flight_is_not_lost) {
  auto clock = std::make_shared<FakeClock>();
  Nominator nom;
  QueueOptions o;
  SchedulingQueue q([](const QueuedPodInfo& a, const QueuedPodInfo& b) { return a.pod->name() < b.pod->name(); },
                    clock, o, &nom);
  auto a = mk_pod("a", 0), b = mk_pod("b", 0);
  q.add(a);
  q.add(b);
  auto qa = q.pop(0);
  CHECK(qa && qa->pod->name() == "a");
  int64_t cycle = q.scheduling_cycle();
  CHECK_EQ(q.in_flight(), 1u);
  q.activate({a, b});  // b is already active; a is mid-cycle
  CHECK_EQ(q.pending_activations(), 1u);
  qa->unschedulable_plugins = {"Coscheduling"};
  CHECK(q.add_unschedulable_if_not_present(qa, cycle));
  CHECK_EQ(q.counts().unschedulable, 0u);
  CHECK_EQ(q.counts().active, 2u);
  CHECK_EQ(q.in_flight(), 0u);
  // Without an activation mark the failure parks the pod as before.
  auto q1 = q.pop(0);
  int64_t c1 = q.scheduling_cycle();
  q1->unschedulable_plugins = {"Coscheduling"};
  CHECK(q.add_unschedulable_if_not_present(q1, c1));
  CHECK_EQ(q.counts().unschedulable, 1u);
  // A pod that binds drops its in-flight entry (no mark leaks).
  auto q2 = q.pop(0);
  CHECK(q2);
  q.activate({q2->pod});
  Pod bound = *q2->pod;
  bound.node_name = "n0";
  q.assigned_pod_added(bound);
  CHECK_EQ(q.in_flight(), 0u);
  CHECK_EQ(q.pending_activations(), 0u);
  q.close();
}

// -------------------------------------------------------------- TimerService
TEST(timers_fire_in_deadline_order_with_fake_clock) {
  auto clock = std::make_shared<FakeClock>();
  TimerService ts(clock);
  std::vector<int> fired;
  std::mutex mu;
  ts.schedule_after(300, [&] { std::lock_guard<std::mutex> g(mu); fired.push_back(3); });
  ts.schedule_after(100, [&] { std::lock_guard<std::mutex> g(mu); fired.push_back(1); });
  uint64_t c = ts.schedule_after(200, [&] { std::lock_guard<std::mutex> g(mu); fired.push_back(2); });
  CHECK(ts.cancel(c));
  clock->advance_us(1000);
  ts.poke_and_drain();
  std::lock_guard<std::mutex> g(mu);
  CHECK_EQ(fired.size(), 2u);
  if (fired.size() == 2) {
    CHECK_EQ(fired[0], 1);
    CHECK_EQ(fired[1], 3);
  }
  ts.stop();
}

// ---------------------------------------------------------------- CycleState
struct IntState : StateData {
  int v = 0;
  explicit IntState(int x) : v(x) {}
  std::shared_ptr<StateData> clone() const override { return std::make_shared<IntState>(v); }
};

TEST(cycle_state_memo_invalidated_by_writes) {
  CycleState s;
  s.write("k", std::make_shared<IntState>(1));
  CHECK_EQ(s.read_as<IntState>("k")->v, 1);
  s.write("k", std::make_shared<IntState>(2));
  CHECK_EQ(s.read_as<IntState>("k")->v, 2);
  auto c = s.clone();
  CHECK_EQ(c->read_as<IntState>("k")->v, 2);
  c->write("k", std::make_shared<IntState>(3));
  CHECK_EQ(s.read_as<IntState>("k")->v, 2);
  CHECK_EQ(c->read_as<IntState>("k")->v, 3);
  s.erase("k");
  CHECK(s.read_as<IntState>("k") == nullptr);
  // Different keys, same type: the memo keys on the name too.
  s.write("a", std::make_shared<IntState>(10));
  s.write("b", std::make_shared<IntState>(20));
  CHECK_EQ(s.read_as<IntState>("a")->v, 10);
  CHECK_EQ(s.read_as<IntState>("b")->v, 20);
}

// --------------------------------------------------------------------- Store
TEST(store_watch_replay_and_expiry) {
  ObjectStore st;
  st.create("pods", Json::parse(R"({"metadata":{"name":"a","namespace":"d"}})"));
  int64_t rv = st.resource_version();
  st.create("pods", Json::parse(R"({"metadata":{"name":"b","namespace":"d"}})"));
  auto w = st.watch({"pods"}, "d", rv);
  auto evs = w->next(100, 10);
  CHECK_EQ(evs.size(), 1u);
  if (!evs.empty()) CHECK_EQ((*evs[0].obj)["metadata"]["name"].as_string(), "b");
  st.unwatch(w);
  Json patch = Json::parse(R"({"metadata":{"resourceVersion":"1"},"spec":{"x":1}})");
  bool conflict = false;
  try {
    st.patch("pods", "d", "b", patch);
  } catch (const StoreError& e) {
    conflict = e.code() == 409;
  }
  CHECK(conflict);
  bool dup = false;
  try {
    st.create("pods", Json::parse(R"({"metadata":{"name":"a","namespace":"d"}})"));
  } catch (const StoreError& e) {
    dup = e.code() == 409;
  }
  CHECK(dup);
}

TEST(store_remove_many_is_one_batch) {
  // A gang's members deleted in one call: one watch hand-off with every
  // Deleted event, names that do not exist skipped, other pods untouched.
  ObjectStore st;
  for (int i = 0; i < 5; ++i)
    st.create("pods", Json::parse(R"({"metadata":{"namespace":"d","name":"p)" + std::to_string(i) + R"("}})"));
  auto w = st.watch({"pods"}, "d", 0);
  size_t n = st.remove_many("pods", "d", {"p0", "p2", "nope", "p4"});
  CHECK_EQ(n, 3u);
  auto evs = w->next(100, 100000);
  CHECK_EQ(evs.size(), 3u);
  for (const auto& ev : evs) CHECK(ev.type == EventType::Deleted);
  CHECK_EQ(st.count("pods"), 2u);
}

TEST(store_events_expire_after_ttl) {
  // Events live event_ttl_us (kube-apiserver --event-ttl); expiry is lazy, on
  // a later event write, and watchers see DELETED. Other kinds never expire.
  ObjectStore st;
  st.set_event_ttl_us(20'000);
  st.create("events", Json::parse(R"({"metadata":{"namespace":"d","name":"e0"}})"));
  st.create("pods", Json::parse(R"({"metadata":{"namespace":"d","name":"p0"}})"));
  auto w = st.watch({"events"}, "d", 0);
  std::this_thread::sleep_for(std::chrono::milliseconds(40));
  st.create("events", Json::parse(R"({"metadata":{"namespace":"d","name":"e1"}})"));
  CHECK_EQ(st.count("events"), 1u);
  CHECK(st.get("events", "d", "e0") == nullptr && st.get("events", "d", "e1") != nullptr);
  CHECK_EQ(st.count("pods"), 1u);
  auto evs = w->next(100, 100);
  bool deleted = false;
  for (const auto& ev : evs) deleted |= ev.type == EventType::Deleted;
  CHECK(deleted);
}

TEST(store_create_chunked_keeps_gangs_whole) {
  // 200 pods in gangs of 3 (plus ungrouped pods every 10th), streamed from
  // JSON text: watchers see commits of >= kCreateChunk pods, each ending on a
  // gang boundary, and the first commit before the producer has finished.
  std::string text = "[";
  std::vector<std::string> group(200);
  for (int i = 0; i < 200; ++i) {
    group[i] = i % 10 == 9 ? "" : "g" + std::to_string(i / 3);
    std::string labels = group[i].empty() ? "{}" : R"({"pod-group.scheduling.sigs.k8s.io":")" + group[i] + "\"}";
    text += (i ? "," : "") + std::string(R"({"metadata":{"namespace":"d","name":"p)") + std::to_string(i) +
            R"(","labels":)" + labels + "}}";
  }
  text += "]";
  ObjectStore st;
  auto w = st.watch({"pods"}, "d", 0);
  std::vector<size_t> seen_at_emit;  // visible events when each object was emitted
  size_t visible = 0, emitted = 0;
  std::vector<size_t> commits;
  size_t n = st.create_chunked("pods", [&](const std::function<void(Json&&)>& emit) {
    Json::parse_array_stream(text, [&](Json&& o) {
      auto evs = w->next(0, 100000);
      if (!evs.empty()) {
        visible += evs.size();
        commits.push_back(visible);
      }
      ++emitted;
      emit(std::move(o));
    });
  });
  auto rest = w->next(100, 100000);
  visible += rest.size();
  CHECK_EQ(n, 200u);
  CHECK_EQ(visible, 200u);
  CHECK(!commits.empty());  // pipelined: something was visible mid-stream
  size_t prev = 0;
  for (size_t c : commits) {
    CHECK(c - prev >= ObjectStore::kCreateChunk);
    CHECK(c < 200);
    // Commit ends on a gang boundary.
    CHECK(group[c].empty() || group[c] != group[c - 1]);
    prev = c;
  }
  bool bad_array = false;
  try {
    Json::parse_array_stream("{}", [](Json&&) {});
  } catch (const JsonError&) {
    bad_array = true;
  }
  CHECK(bad_array);
}

TEST(parallelizer_cost_model_inline_vs_parallel) {
  // Cheap items above inline_below stay on the caller once measured; items
  // whose serial work is far above kMinParallelWorkNs fan out to helpers.
  Parallelizer par(8, 16);
  ParallelSite cheap_site, heavy_site;
  auto threads_used = [&](int n, ParallelSite* site, bool heavy) {
    std::mutex mu;
    std::set<std::thread::id> ids;
    par.until(n, [&](int) {
      if (heavy) {
        auto end = std::chrono::steady_clock::now() + std::chrono::microseconds(4);
        while (std::chrono::steady_clock::now() < end) {
        }
      }
      std::lock_guard<std::mutex> g(mu);
      ids.insert(std::this_thread::get_id());
    }, nullptr, site);
    return ids.size();
  };
  for (int i = 0; i < 3; ++i) threads_used(512, &cheap_site, false);
  CHECK_EQ(threads_used(512, &cheap_site, false), 1u);
  threads_used(512, &heavy_site, true);  // first call is an inline probe
  size_t most = 0;
  // Helpers must win a wake-up race against the caller; on a loaded host
  // (a parallel build) give them several rounds.
  for (int i = 0; i < 12 && most <= 1; ++i) most = std::max(most, threads_used(512, &heavy_site, true));
  CHECK(most > 1);  // 512 x 4 us = 2 ms of serial work
  CHECK(heavy_site.ns_per_item_x16.load() / 16 >= 1000);
}

TEST(parallelizer_ranges_cover_every_item_once_and_stop) {
  // until_forked_ranges hands out disjoint chunks that cover [0, n); a chunk
  // function that raises `stop` ends the claiming of further chunks.
  Parallelizer par(8, 16);
  for (int n : {1, 7, 100, 1024, 4099}) {
    std::vector<std::atomic<int>> seen(static_cast<size_t>(n));
    par.until_forked_ranges(n, [&](int b, int e) {
      CHECK(b < e);
      for (int i = b; i < e; ++i) seen[static_cast<size_t>(i)].fetch_add(1);
    }, nullptr, nullptr);
    int bad = 0;
    for (auto& s : seen) bad += s.load() != 1;
    CHECK_EQ(bad, 0);
  }
  std::atomic<bool> stop{false};
  std::atomic<int> chunks{0};
  par.until_forked_ranges(100000, [&](int, int) {
    chunks.fetch_add(1);
    stop.store(true);
  }, &stop, nullptr);
  CHECK(chunks.load() <= 9);  // at most one chunk per participant after the stop
}

}  // namespace

TEST(store_optimistic_updates_lose_nothing) {
  // 8 writers patch (and one binds) the same pod concurrently: each update
  // is built outside the store lock and committed only on the version it was
  // built from, so every patch lands and resourceVersions stay contiguous.
  ObjectStore st;
  st.create("pods", Json::parse(R"({"metadata":{"name":"p","namespace":"d","uid":"u1"},"spec":{}})"));
  int64_t rv0 = st.resource_version();
  constexpr int kThreads = 8, kEach = 150;
  std::vector<std::thread> ts;
  for (int t = 0; t < kThreads; ++t)
    ts.emplace_back([&st, t] {
      for (int i = 0; i < kEach; ++i) {
        Json patch = Json::object();
        Json labels = Json::object();
        labels.set("k" + std::to_string(t) + "-" + std::to_string(i), Json("v"));
        Json md = Json::object();
        md.set("labels", std::move(labels));
        patch.set("metadata", std::move(md));
        st.patch("pods", "d", "p", patch);
      }
    });
  bool bound = false;
  std::thread binder([&] {
    try {
      st.bind("d", "p", "u1", "node-1", Json::object());
      bound = true;
    } catch (const StoreError&) {
    }
  });
  for (auto& th : ts) th.join();
  binder.join();
  JsonPtr cur = st.get("pods", "d", "p");
  CHECK_EQ(static_cast<int>((*cur)["metadata"]["labels"].size()), kThreads * kEach);
  CHECK(bound);
  CHECK_EQ((*cur)["spec"]["nodeName"].as_string(), "node-1");
  CHECK_EQ(st.resource_version() - rv0, static_cast<int64_t>(kThreads * kEach + 1));
}

TEST(cache_debugger_reports_drift) {
  auto node = [](const std::string& name) {
    return Node::from_json(Json::parse(R"({"metadata":{"name":")" + name +
                                       R"("},"status":{"allocatable":{"cpu":"8","memory":"16Gi","pods":"10"}}})"));
  };
  auto pod = [](const std::string& name, const std::string& on) {
    return Pod::from_json(Json::parse(R"({"metadata":{"namespace":"d","name":")" + name + R"(","uid":"u-)" + name +
                                      R"("},"spec":{"nodeName":")" + on +
                                      R"(","containers":[{"name":"c","resources":{"requests":{"cpu":"1"}}}]}})"));
  };
  SchedulerCache cache(std::make_shared<FakeClock>(0), 1'000'000);
  cache.add_node(node("a"));
  cache.add_node(node("b"));
  auto p1 = pod("p1", "a"), p2 = pod("p2", "b");
  cache.add_pod(p1);
  cache.add_pod(p2);
  Json ok = cache.check({p1, p2}, {"a", "b"});
  CHECK(ok["clean"].as_bool());
  // Listers with a pod the cache lacks, without one it has, a moved pod and
  // an extra Node.
  auto p3 = pod("p3", "a"), p2b = pod("p2", "a");
  Json bad = cache.check({p2b, p3}, {"a", "b", "c"});
  CHECK(!bad["clean"].as_bool());
  CHECK_EQ(bad["missing_pods"].items().size(), 1u);
  CHECK_EQ(bad["missing_pods"].items()[0].as_string(), "d/p3");
  CHECK_EQ(bad["redundant_pods"].items()[0].as_string(), "d/p1");
  CHECK_EQ(bad["wrong_node"].items().size(), 1u);
  CHECK_EQ(bad["missing_nodes"].items()[0].as_string(), "c");
  // A NodeInfo whose incremental totals drifted from its pods.
  NodeInfo ni;
  ni.set_node(node("x"));
  ni.add_pod(pod("q", "x"));
  CHECK(ni.verify().empty());
  ni.requested.v[kCPU] += 500;
  auto fields = ni.verify();
  CHECK_EQ(fields.size(), 1u);
  CHECK_EQ(fields[0], "requested");
}

TEST(default_normalize_matches_integer_division) {
  // The table and reciprocal paths of default_normalize_score against the
  // plain max_priority * score / max over small, mid and 2^40-sized raws.
  std::mt19937_64 r(7);
  for (int t = 0; t < 3000; ++t) {
    const int n = 1 + static_cast<int>(r() % 600);
    const int64_t cap = t % 3 == 0 ? 200 : t % 3 == 1 ? (int64_t{1} << 40) : 100000;
    std::vector<NodeScore> a(static_cast<size_t>(n));
    for (auto& s : a) s.score = static_cast<int64_t>(r() % static_cast<uint64_t>(cap + 1));
    std::vector<NodeScore> b = a;
    const bool rev = (r() & 1) != 0;
    default_normalize_score(kMaxNodeScore, rev, a);
    int64_t mx = 0;
    for (const auto& s : b) mx = std::max(mx, s.score);
    for (auto& s : b) {
      if (mx == 0) {
        if (rev) s.score = kMaxNodeScore;
        continue;
      }
      const int64_t sc = kMaxNodeScore * s.score / mx;
      s.score = rev ? kMaxNodeScore - sc : sc;
    }
    for (int i = 0; i < n; ++i) CHECK_EQ(a[static_cast<size_t>(i)].score, b[static_cast<size_t>(i)].score);
  }
}

TEST(gpu_assignment_direct_matches_annotations) {
  // FlexGPU Reserve sets the assignment from its placement; the informer's
  // copy derives it from the annotations Reserve wrote. Both must agree.
  const GpuNames& gn = default_gpu_names();
  const char* limits[] = {R"({"amd.com/gpu":"2"})", R"({"amd.com/gpu-xcd":"2"})", R"({"amd.com/gpu-memory":"3"})"};
  for (const char* lim : limits) {
    Json j = Json::parse(std::string(R"({"metadata":{"namespace":"d","name":"p","uid":"u",)") +
                         R"("annotations":{"amd.com/gpu-index":"1,3,12","amd.com/gpu-partitions":"0:2,3:1,12:7"}},)" +
                         R"("spec":{"containers":[{"name":"c","resources":{"limits":)" + lim + "}}]}}");
    auto a = Pod::from_json(j, gn);
    Pod b = *a;
    b.set_gpu_assignment({1, 3, 12}, {{0, 2}, {3, 1}, {12, 7}}, gn);
    CHECK(a->gpu.valid());
    CHECK(a->gpu.kind == b.gpu.kind);
    CHECK(a->gpu.gpus == b.gpu.gpus);
    CHECK(a->gpu.partitions == b.gpu.partitions);
    CHECK_EQ(a->gpu.memory, b.gpu.memory);
  }
}

TEST(executor_runs_every_task_with_chain_wakeups_and_batches) {
  // Bursts from several submitters, some inside Batches, with idle gaps so
  // workers go to sleep between bursts: every task must run (a lost wake-up
  // would leave tasks queued past the deadline).
  Executor ex(8);
  std::atomic<int> ran{0};
  int want = 0;
  for (int round = 0; round < 40; ++round) {
    std::vector<std::thread> ts;
    for (int t = 0; t < 3; ++t)
      ts.emplace_back([&, t] {
        if (t == 0) {
          Executor::Batch b(ex);
          for (int k = 0; k < 9; ++k) ex.submit([&] { ran.fetch_add(1); });
        } else {
          for (int k = 0; k < 5; ++k) ex.submit([&] { ran.fetch_add(1); });
        }
      });
    for (auto& th : ts) th.join();
    want += 9 + 5 + 5;
    const auto deadline = std::chrono::steady_clock::now() + std::chrono::seconds(5);
    while (ran.load() < want && std::chrono::steady_clock::now() < deadline)
      std::this_thread::sleep_for(std::chrono::microseconds(50));
    CHECK_EQ(ran.load(), want);
    if (round % 4 == 0) std::this_thread::sleep_for(std::chrono::milliseconds(2));  // let workers sleep
  }
  ex.stop();
}

int main() {
  for (const auto& t : tests()) {
    int before = g_failed;
    t.fn();
    std::printf("[%s] %s\n", g_failed == before ? " OK " : "FAIL", t.name);
  }
  std::printf("%d checks, %d failed, %zu tests\n", g_checks, g_failed, tests().size());
  return g_failed == 0 ? 0 : 1;
}
