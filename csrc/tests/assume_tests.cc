// Native tests for the scheduling cycle's fixed per-pod work: assuming a pod
// with its GPU placement (Plugin::prepare_assumed, FlexGPU), the cycle number
// SchedulingQueue::pop hands out and integer formatting without printf
// (common/strings.h).
//
// The placement tests run FlexGPU twice over caches with the same two nodes
// (one SPX, one CPX, 8 GPUs each): once the way a cycle went before the hook
// (assume_pod, then reserve(), which annotates the assumed pod under the
// cache lock) and once the fused way (prepare_assumed on the private copy,
// then assume_pod, then reserve() answering from the cycle state). After
// every pod the two caches' nodes must agree field by field. Forget, the
// informer's confirmation, Unreserve and a placement that fails follow.
//
// Built by `python -m flex_gpu_scheduler_amd.build_ext --assume-tests` into
// build/xsched_assume_tests (`--assume-tests-tsan`: build/xsched_assume_tests_tsan)
// and run by tests/test_native_assume.py.
#include <climits>
#include <cstdio>
#include <functional>
#include <memory>
#include <string>
#include <vector>

#include "api/types.h"
#include "common/clock.h"
#include "common/json.h"
#include "common/strings.h"
#include "framework/plugin.h"
#include "framework/types.h"
#include "scheduler/cache.h"
#include "scheduler/queue.h"

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
#define TEST(name)             \
  void name();                 \
  Reg reg_##name(#name, name); \
  void name()

// ------------------------------------------------------------- fixtures ----
NodePtr gpu_node(const std::string& name, const std::string& mode) {
  return Node::from_json(Json::parse(
      R"({"metadata":{"name":")" + name + R"(","labels":{"amd.com/gpu.compute-partition":")" + mode +
      R"("}},"status":{"allocatable":{"cpu":"256","memory":"3Ti","pods":"256","amd.com/gpu":"8",)" +
      R"("amd.com/gpu-memory":"2304","amd.com/gpu-xcd":"64"}}})"));
}

// `limits`: the container's limits object, "" for a pod without GPU demand.
// `node` and `annotations` (a JSON object) only for the informer's bound copy.
PodPtr gpu_pod(const std::string& name, const std::string& limits, const std::string& node = "",
               const std::string& annotations = "") {
  std::string j = R"({"metadata":{"namespace":"d","name":")" + name + R"(","uid":"u-)" + name +
                  R"(","resourceVersion":"7")";
  if (!annotations.empty()) j += R"(,"annotations":)" + annotations;
  j += R"(},"spec":{)";
  if (!node.empty()) j += R"("nodeName":")" + node + R"(",)";
  j += R"("containers":[{"name":"c","resources":{"requests":{"cpu":"1"})";
  if (!limits.empty()) j += R"(,"limits":)" + limits;
  j += "}}]}}";
  return Pod::from_json(Json::parse(j));
}

// One scheduler's worth of what FlexGPU reaches: a cache, its snapshot and
// the plugin built from the registry against them.
struct Rig {
  SchedulerCache cache{std::make_shared<FakeClock>(0), 1'000'000};
  Snapshot snap;
  Handle h;
  PluginPtr flex;
  Rig() {
    cache.add_node(gpu_node("spx", "spx"));
    cache.add_node(gpu_node("cpx", "cpx"));
    h.cache = &cache;
    h.snapshot = &snap;
    flex = Registry::global().make("FlexGPU", Json::object(), h);
    cache.update_snapshot(snap);
  }
  // The cycle's private copy of `p` for `node`.
  static PodPtr copy_for(const PodPtr& p, const std::string& node) {
    auto c = std::make_shared<Pod>(*p);
    c->node_name = node;
    return c;
  }
  // A cycle's assume and Reserve as they were: the pod enters the cache
  // without a placement, reserve() places it and annotates it in the cache.
  Status place_two_steps(CycleState& s, const PodPtr& copy) {
    cache.update_snapshot(snap);
    Status st = cache.assume_pod(copy);
    if (!st.is_success()) return st;
    return flex->reserve(s, copy, copy->node_name);
  }
  // The fused cycle: placement on the private copy, one entry into the cache.
  Status place_fused(CycleState& s, const PodPtr& copy, bool* prepared = nullptr) {
    cache.update_snapshot(snap);
    NodeInfoPtr ni = snap.get(copy->node_name);
    bool ok = flex->prepare_assumed(s, *copy, *ni);
    if (prepared) *prepared = ok;
    Status st = cache.assume_pod(copy);
    if (!st.is_success()) return st;
    return flex->reserve(s, copy, copy->node_name);
  }
};

void check_same_ledger(const GpuLedger& a, const GpuLedger& b) {
  CHECK_EQ(a.gpu_count, b.gpu_count);
  CHECK_EQ(a.tot_whole, b.tot_whole);
  CHECK_EQ(a.tot_xcds, b.tot_xcds);
  CHECK_EQ(a.tot_mem, b.tot_mem);
  CHECK(a.monopoly == b.monopoly);
  CHECK_EQ(a.free.size(), b.free.size());
  for (size_t g = 0; g < a.free.size() && g < b.free.size(); ++g) {
    CHECK_EQ(a.free[g].whole, b.free[g].whole);
    CHECK_EQ(a.free[g].free_slots, b.free[g].free_slots);
    CHECK_EQ(a.free[g].xcds, b.free[g].xcds);
    CHECK_EQ(a.free[g].mem, b.free[g].mem);
    CHECK_EQ(a.free[g].max_slot_mem, b.free[g].max_slot_mem);
  }
  CHECK_EQ(a.slots.size(), b.slots.size());
  for (size_t i = 0; i < a.slots.size() && i < b.slots.size(); ++i) {
    CHECK_EQ(a.slots[i].exclusive, b.slots[i].exclusive);
    CHECK_EQ(a.slots[i].used_mem, b.slots[i].used_mem);
    CHECK_EQ(a.slots[i].mem_pods, b.slots[i].mem_pods);
  }
  CHECK(a.diff(b).empty());
}

void check_same_pod(const Pod& a, const Pod& b) {
  CHECK_EQ(a.uid(), b.uid());
  CHECK_EQ(a.node_name, b.node_name);
  CHECK(a.meta.annotations.get() == b.meta.annotations.get());
  CHECK(a.gpu.kind == b.gpu.kind);
  CHECK(a.gpu.gpus == b.gpu.gpus);
  CHECK(a.gpu.partitions == b.gpu.partitions);
  CHECK_EQ(a.gpu.memory, b.gpu.memory);
}

void check_same_node(const SchedulerCache& ca, const SchedulerCache& cb, const std::string& node) {
  NodeInfoPtr a = ca.node_info_copy(node), b = cb.node_info_copy(node);
  CHECK(a && b);
  if (!a || !b) return;
  check_same_ledger(a->gpu, b->gpu);
  CHECK(a->requested == b->requested);
  CHECK(a->nonzero_requested == b->nonzero_requested);
  CHECK_EQ(a->pods.size(), b->pods.size());
  for (size_t i = 0; i < a->pods.size() && i < b->pods.size(); ++i) check_same_pod(*a->pods[i], *b->pods[i]);
  CHECK(a->verify().empty());
  CHECK(b->verify().empty());
}

struct Case {
  const char* name;
  const char* limits;
  const char* node;
  bool gpu;         // has a GPU demand
  bool partitions;  // carries the partition annotation
};
const Case kCases[] = {
    {"one-gpu", R"({"amd.com/gpu":"1"})", "spx", true, false},
    {"two-gpus", R"({"amd.com/gpu":"2"})", "spx", true, false},
    {"two-xcds", R"({"amd.com/gpu-xcd":"2"})", "cpx", true, true},
    {"mem-slice", R"({"amd.com/gpu-memory":"16"})", "cpx", true, true},
    {"no-gpu", "", "spx", false, false},
};

const std::string kIndex = "amd.com/gpu-index", kParts = "amd.com/gpu-partitions";

// ------------------------------------------------ assume with placement ----
TEST(fused_assume_equals_assume_then_reserve) {
  Rig two, fused;  // `two`: the two-step path
  for (const Case& c : kCases) {
    PodPtr p = gpu_pod(c.name, c.limits);
    PodPtr ca = Rig::copy_for(p, c.node), cb = Rig::copy_for(p, c.node);
    const int64_t gen_before = fused.cache.node_info_copy(c.node)->generation;
    CycleState sa, sb;
    bool prepared = false;
    CHECK(two.place_two_steps(sa, ca).is_success());
    CHECK(fused.place_fused(sb, cb, &prepared).is_success());
    CHECK_EQ(prepared, c.gpu);
    check_same_node(two.cache, fused.cache, "spx");
    check_same_node(two.cache, fused.cache, "cpx");
    // The cached pod is the cycle's copy, as placed.
    PodPtr cached = fused.cache.get_pod(cb->uid());
    CHECK(cached.get() == cb.get());
    CHECK(fused.cache.is_assumed(cb->uid()));
    check_same_pod(*two.cache.get_pod(ca->uid()), *cached);
    CHECK_EQ(strmap_get(cached->meta.annotations, kIndex) != nullptr, c.gpu);
    CHECK_EQ(strmap_get(cached->meta.annotations, kParts) != nullptr, c.partitions);
    CHECK_EQ(cached->gpu.valid(), c.gpu);
    // The queued object was not touched.
    CHECK(p->meta.annotations.empty());
    CHECK(!p->gpu.valid());
    // The node's generation advanced and the node was dirty: the next
    // snapshot refresh picks the generation and the GPU summary up.
    NodeInfoPtr now = fused.cache.node_info_copy(c.node);
    CHECK(now->generation > gen_before);
    fused.cache.update_snapshot(fused.snap);
    const size_t i = fused.snap.index.at(c.node);
    CHECK_EQ(fused.snap.gen[i], now->generation);
    CHECK_EQ(fused.snap.free_whole[i], now->gpu.free_gpus());
    CHECK_EQ(fused.snap.free_xcd[i], now->gpu.free_xcds());
  }
}

TEST(forget_after_fused_assume_restores_the_node) {
  for (const Case& c : kCases) {
    Rig r;
    NodeInfoPtr before = r.cache.node_info_copy(c.node);
    PodPtr cp = Rig::copy_for(gpu_pod(c.name, c.limits), c.node);
    CycleState s;
    CHECK(r.place_fused(s, cp).is_success());
    if (c.gpu) CHECK(!r.cache.node_info_copy(c.node)->gpu.diff(before->gpu).empty());
    r.cache.forget_pod(*cp);
    NodeInfoPtr after = r.cache.node_info_copy(c.node);
    check_same_ledger(before->gpu, after->gpu);
    CHECK(before->requested == after->requested);
    CHECK_EQ(after->pods.size(), 0u);
    CHECK(r.cache.get_pod(cp->uid()) == nullptr);
    CHECK_EQ(r.cache.assumed_count(), 0u);
  }
}

TEST(informer_confirms_a_fused_assume_in_place) {
  for (const Case& c : kCases) {
    Rig r;
    PodPtr cp = Rig::copy_for(gpu_pod(c.name, c.limits), c.node);
    CycleState s;
    CHECK(r.place_fused(s, cp).is_success());
    const int64_t gen = r.cache.node_info_copy(c.node)->generation;
    // The bound object as Scheduler::bound_copy_of_assumed builds it: a copy
    // of the assumed pod with the version refreshed.
    auto bound = std::make_shared<Pod>(*cp);
    bound->template_hash = 0;
    bound->meta.resource_version = cp->meta.resource_version + 1;
    CHECK_EQ(bound->meta.annotations.size(), cp->meta.annotations.size());
    r.cache.update_pod(cp, bound);
    CHECK(!r.cache.is_assumed(cp->uid()));
    CHECK(r.cache.get_pod(cp->uid()).get() == bound.get());
    // Same accounting: the NodeInfo kept the assumed object and its generation.
    NodeInfoPtr ni = r.cache.node_info_copy(c.node);
    CHECK_EQ(ni->generation, gen);
    CHECK_EQ(ni->pods.size(), 1u);
    CHECK(ni->pods[0].get() == cp.get());
    CHECK(ni->verify().empty());
  }
  // The same when the informer parsed the bound object from the API server's
  // JSON: the annotations the fused path wrote parse to the assignment it set.
  for (const Case& c : kCases) {
    Rig r;
    PodPtr cp = Rig::copy_for(gpu_pod(c.name, c.limits), c.node);
    CycleState s;
    CHECK(r.place_fused(s, cp).is_success());
    const int64_t gen = r.cache.node_info_copy(c.node)->generation;
    Json ann = Json::object();
    for (const auto& kv : cp->meta.annotations) ann.set(kv.first, Json(kv.second));
    PodPtr parsed = gpu_pod(c.name, c.limits, c.node, cp->meta.annotations.empty() ? "" : ann.dump());
    CHECK(parsed->gpu.kind == cp->gpu.kind);
    CHECK(parsed->gpu.gpus == cp->gpu.gpus);
    CHECK(parsed->gpu.partitions == cp->gpu.partitions);
    CHECK_EQ(parsed->gpu.memory, cp->gpu.memory);
    r.cache.add_pod(parsed);
    CHECK(!r.cache.is_assumed(cp->uid()));
    CHECK_EQ(r.cache.node_info_copy(c.node)->generation, gen);
  }
}

TEST(unreserve_after_fused_assume_strips_the_placement) {
  for (const Case& c : kCases) {
    Rig two, fused;
    PodPtr p = gpu_pod(c.name, c.limits);
    PodPtr ca = Rig::copy_for(p, c.node), cb = Rig::copy_for(p, c.node);
    NodeInfoPtr before = fused.cache.node_info_copy(c.node);
    CycleState sa, sb;
    CHECK(two.place_two_steps(sa, ca).is_success());
    CHECK(fused.place_fused(sb, cb).is_success());
    two.flex->unreserve(sa, ca, c.node);
    fused.flex->unreserve(sb, cb, c.node);
    CHECK(sb.read("FlexGPU/assignment") == nullptr);
    PodPtr cached = fused.cache.get_pod(cb->uid());
    CHECK(cached != nullptr);
    if (!cached) continue;
    CHECK(strmap_get(cached->meta.annotations, kIndex) == nullptr);
    CHECK(strmap_get(cached->meta.annotations, kParts) == nullptr);
    CHECK(!cached->gpu.valid());
    CHECK(fused.cache.is_assumed(cb->uid()));
    check_same_node(two.cache, fused.cache, c.node);
    // Still accounted as a pod, no longer on any GPU.
    NodeInfoPtr after = fused.cache.node_info_copy(c.node);
    check_same_ledger(before->gpu, after->gpu);
    CHECK_EQ(after->pods.size(), 1u);
    CHECK(after->verify().empty());
  }
}

TEST(failed_placement_is_left_to_reserve) {
  Rig r;
  // Take all eight GPUs of the SPX node.
  for (int i = 0; i < 8; ++i) {
    PodPtr cp = Rig::copy_for(gpu_pod("fill" + std::to_string(i), R"({"amd.com/gpu":"1"})"), "spx");
    CycleState s;
    bool prepared = false;
    CHECK(r.place_fused(s, cp, &prepared).is_success());
    CHECK(prepared);
  }
  CHECK_EQ(r.cache.node_info_copy("spx")->gpu.free_gpus(), 0);
  PodPtr p = gpu_pod("ninth", R"({"amd.com/gpu":"1"})");
  PodPtr cp = Rig::copy_for(p, "spx");
  CycleState s;
  r.cache.update_snapshot(r.snap);
  CHECK(!r.flex->prepare_assumed(s, *cp, *r.snap.get("spx")));
  // Nothing changed: not the copy, not the cycle state.
  CHECK(cp->meta.annotations.empty());
  CHECK(!cp->gpu.valid());
  CHECK(s.read("FlexGPU/assignment") == nullptr);
  // The old path reports it, as before.
  CHECK(r.cache.assume_pod(cp).is_success());
  Status st = r.flex->reserve(s, cp, "spx");
  CHECK(st.is_unschedulable());
  CHECK_EQ(st.message(), "allocate index fail");
  r.cache.forget_pod(*cp);
  CHECK(r.cache.node_info_copy("spx")->verify().empty());

  // Neither kind of pod the hook declines is touched either.
  PodPtr none = Rig::copy_for(gpu_pod("none", ""), "spx");
  CHECK(!r.flex->prepare_assumed(s, *none, *r.snap.get("spx")));
  PodPtr both = Rig::copy_for(gpu_pod("both", R"({"amd.com/gpu":"1","amd.com/gpu-xcd":"2"})"), "cpx");
  CHECK(both->gpu_demand.kind == GpuDemand::Conflict);
  CHECK(!r.flex->prepare_assumed(s, *both, *r.snap.get("cpx")));
  CHECK(both->meta.annotations.empty());
  CHECK(r.cache.assume_pod(both).is_success());
  Status cst = r.flex->reserve(s, both, "cpx");
  CHECK(!cst.is_success());
  CHECK_EQ(cst.message(), "pod conflict resources");
}

// A state prepared for one copy must not answer Reserve for another object
// or another node: those take the old path.
TEST(reserve_answers_only_for_the_prepared_copy) {
  Rig r;
  PodPtr p = gpu_pod("one", R"({"amd.com/gpu":"1"})");
  PodPtr cp = Rig::copy_for(p, "spx");
  CycleState s;
  r.cache.update_snapshot(r.snap);
  CHECK(r.flex->prepare_assumed(s, *cp, *r.snap.get("spx")));
  // Another copy of the same pod, assumed without a placement.
  PodPtr other = Rig::copy_for(p, "spx");
  CHECK(r.cache.assume_pod(other).is_success());
  CHECK(r.flex->reserve(s, other, "spx").is_success());
  PodPtr cached = r.cache.get_pod(other->uid());
  CHECK(cached && strmap_get(cached->meta.annotations, kIndex) != nullptr);  // placed by the old path
  CHECK(r.cache.node_info_copy("spx")->verify().empty());
  CHECK_EQ(r.cache.node_info_copy("spx")->gpu.free_gpus(), 7);
}

// ---------------------------------------------------------- append_int ----
TEST(append_int_matches_printf) {
  const int values[] = {0, 9, 10, 99, 100, 12345, INT_MAX, -1, INT_MIN};
  for (int v : values) {
    char want[16];
    std::snprintf(want, sizeof want, "%d", v);
    std::string s = "x";
    append_int(s, v);
    CHECK_EQ(s, std::string("x") + want);
  }
  std::string s;
  s.reserve(200);
  const size_t cap = s.capacity();
  join_parts({{0, 0}, {7, 7}, {10, 3}}, s);
  CHECK_EQ(s, "0:0,7:7,10:3");
  CHECK_EQ(s.capacity(), cap);
  join_ints({0, 3, 12}, s);
  CHECK_EQ(s, "0,3,12");
  CHECK_EQ(s.capacity(), cap);
  join_ints({}, s);
  CHECK_EQ(s, "");
  CHECK_EQ(s.capacity(), cap);
  join_parts({}, s);
  CHECK_EQ(s, "");
  CHECK_EQ(s.capacity(), cap);
}

// --------------------------------------------------------------- queue ----
TEST(pop_delivers_the_scheduling_cycle) {
  auto clock = std::make_shared<FakeClock>();
  Nominator nom;
  QueueOptions o;
  SchedulingQueue q([](const QueuedPodInfo& a, const QueuedPodInfo& b) { return a.pod->priority > b.pod->priority; },
                    clock, o, &nom);
  for (int i = 0; i < 100; ++i) q.add(gpu_pod("q" + std::to_string(i), ""));
  int64_t last = q.scheduling_cycle();
  for (int i = 0; i < 100; ++i) {
    int64_t cycle = -1;
    auto qpi = q.pop(0, &cycle);
    CHECK(qpi != nullptr);
    CHECK_EQ(cycle, q.scheduling_cycle());
    CHECK_EQ(cycle, last + 1);
    last = cycle;
  }
  int64_t untouched = -5;
  CHECK(q.pop(0, &untouched) == nullptr);  // empty: no cycle started
  CHECK_EQ(untouched, -5);
  CHECK_EQ(q.scheduling_cycle(), last);
  q.close();
}

}  // namespace

int main() {
  for (const auto& t : tests()) {
    int before = g_failed;
    t.fn();
    std::printf("[%s] %s\n", g_failed == before ? " OK " : "FAIL", t.name);
  }
  std::printf("%d checks, %d failed, %zu tests\n", g_checks, g_failed, tests().size());
  return g_failed == 0 ? 0 : 1;
}
