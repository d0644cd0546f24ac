// PreFilter, the Filter walk over the node window (equivalence cache, scan
// memo, serial and forked strategies) and its FitError.
#include "scheduler/scheduler.h"

#include <algorithm>
#include <cstring>
#include <map>

namespace xsched {

int Scheduler::num_feasible_nodes_to_find(Framework& fw, int n) const {
  constexpr int kMinFeasible = 100;       // generic_scheduler.go:47
  constexpr int kMinPercentage = 5;
  int pct = fw.config().percentage_of_nodes_to_score;
  if (n < kMinFeasible || pct >= 100) return n;
  int adaptive = pct;
  if (adaptive <= 0) {
    adaptive = 50 - n / 125;
    if (adaptive < kMinPercentage) adaptive = kMinPercentage;
  }
  int num = n * adaptive / 100;
  if (num < kMinFeasible) return kMinFeasible;
  return num;
}

// Which snapshot positions carry nominated pods: rebuilt from the view when
// the view object or the node set changed, else updated for the nodes the
// view's change log touched (a preemption wave keeps hundreds of pods
// nominated; re-deriving every position per cycle was a hash lookup each).
// Stale marks only send a node down the exact (uncached) path; every node
// nominated in the view is always marked.
void Scheduler::refresh_nom_mark(const NominatedMap* view) {
  if (!view || view->empty()) {
    nom_mark_valid_ = false;
    return;
  }
  const size_t n = snapshot_.nodes.size();
  auto mark = [&](const std::string& node) {
    auto it = snapshot_.index.find(node);
    if (it == snapshot_.index.end()) return;
    auto vit = view->find(node);
    const bool on = vit != view->end() && !vit->second.empty();
    nom_mark_[it->second] = on;
    nom_list_[it->second] = on ? &vit->second : nullptr;  // map nodes do not move
  };
  if (!nom_mark_valid_ || view != nom_src_ || snapshot_.node_epoch != nom_epoch_ || nom_mark_.size() != n) {
    nom_mark_.assign(n, 0);
    nom_list_.assign(n, nullptr);
    for (const auto& [node, pods] : *view)
      if (!pods.empty()) mark(node);
  } else {
    for (const auto& node : nom_changed_) mark(node);
  }
  nom_changed_.clear();
  nom_src_ = view;
  nom_epoch_ = snapshot_.node_epoch;
  nom_mark_valid_ = true;
}

Scheduler::EqEntry* Scheduler::eq_entry(Framework& fw, const Pod& p) {
  if (!opts_.equivalence_cache || p.template_hash == 0) return nullptr;
  auto& per_fw = eq_[&fw];
  auto& e = per_fw[p.template_hash];
  if (!e) {
    if (per_fw.size() > 256) {  // bounded: drop every template (they refill on demand)
      per_fw.clear();
      return eq_entry(fw, p);
    }
    e = std::make_unique<EqEntry>();
  }
  if (e->epoch != snapshot_.node_epoch || e->table.n != snapshot_.nodes.size()) {
    e->epoch = snapshot_.node_epoch;
    e->table.reset(snapshot_.nodes.size());
    e->scan.valid = false;
  }
  return e.get();
}

namespace {

// "0/N nodes are available: k reason, ..." from a tally of failure reasons.
std::string fit_error_message(int n, const std::map<std::string, int>& reasons) {
  std::string msg = "0/" + std::to_string(n) + " nodes are available:";
  bool first = true;
  for (const auto& kv : reasons) {
    msg += (first ? " " : ", ") + std::to_string(kv.second) + " " + kv.first;
    first = false;
  }
  return msg + ".";
}

// The same over a complete diagnosis.
std::string fit_error_message(int n, const NodeStatusMap& m) {
  std::map<std::string, int> reasons;
  m.for_each([&](std::string_view, const Status& st) {
    for (const auto& r : st.reasons()) ++reasons[r];
  });
  return fit_error_message(n, reasons);
}

}  // namespace

// Every node of the snapshot gets `st` in the diagnosis, except the positions
// in `own` (optional), which get the verdict listed for them.
void Scheduler::diagnose_every_node(Diagnosis& d, const Status& st,
                                    const std::vector<std::pair<int, const Status*>>* own) {
  const auto& names = snapshot_.names;
  d.node_to_status.reserve(names.size());
  const bool fresh = d.node_to_status.empty();
  for (size_t pos = 0; pos < names.size(); ++pos) {
    const Status* x = &st;
    if (own)
      for (const auto& [q, fs] : *own)
        if (q == static_cast<int>(pos)) x = fs;
    if (fresh) d.node_to_status.append_unique(names[pos], *x);
    else d.node_to_status.emplace(names[pos], *x);
  }
  d.unschedulable_plugins.insert(st.failed_plugin());
  if (own)
    for (const auto& [q, fs] : *own) d.unschedulable_plugins.insert(fs->failed_plugin());
}

// The end of every Filter path that found nodes: interested extenders (`ext`)
// narrow the list; when they leave none, the FitError over the diagnosis
// (Unschedulable: an extender's own failure is an Error).
Status Scheduler::extender_tail(const Pod& p, int n, NodeList& feasible, std::vector<int>* feasible_pos, Diagnosis& d,
                                bool ext) {
  if (!ext) return {};
  Status es = run_extender_filters(p, feasible, feasible_pos, d);
  if (!es.is_success() || !feasible.empty()) return es;
  return Status(Code::Unschedulable, fit_error_message(n, d.node_to_status));
}

// One Filter pass of one pod over the snapshot: what the walk strategies below
// share. It lives for one call of find_nodes_that_fit and borrows the
// scheduler's scratch vectors (fail_buf_, fail_ptr_, found_buf_,
// found_pos_buf_), which are reused across cycles.
struct Scheduler::FilterPass {
  Scheduler& sc;
  Framework& fw;
  CycleState& s;
  const Pod& p;
  Diagnosis& d;
  NodeList& feasible;
  std::vector<int>* feasible_pos;
  EqEntry* eq;
  // The PreFilter node set this pass honours (null: every node). With a mask,
  // walk() gives the nodes outside it rs->excluded and no Filter call; with a
  // list, listed() evaluates only those positions.
  const NodeRestriction* rs;
  const bool full_diagnosis, ext;
  const int n, to_find;

  const char* rmask = nullptr;
  bool eq_filter = false;
  const char* nom_mark = nullptr;
  int start = 0;
  EqEntry::ScanMemo* memo = nullptr;
  // The pass so far: feasible nodes kept in found_buf_, nodes evaluated,
  // equivalence-cache hits among them, the first plugin error.
  int c = 0, processed = 0;
  uint64_t hits = 0;
  Status first_err;
  bool has_err = false;

  // Filter verdicts are reused only when every Filter plugin is node-local for
  // this pod. A node with nominated pods is evaluated with them added; that
  // verdict is cached too, keyed by the set of nominated pods that count for
  // this pod (Framework::nominated_signature), unless one of them reacts
  // with a PreFilter extension (the state would then not be node-local).
  void use_equivalence_cache() {
    eq_filter = eq && fw.filters_node_local(p, sc.snapshot_);
    if (eq_filter && s.nominated && !s.nominated->empty()) {
      if (!sc.nom_mark_valid_ || s.nominated.get() != sc.nom_src_) sc.refresh_nom_mark(s.nominated.get());
      nom_mark = sc.nom_mark_.data();
    } else if (eq_filter && sc.nominator_ && !sc.nominator_->empty()) {
      // Nominations without this cycle's view (explain, or a caller that did
      // not snapshot them): no per-node knowledge, so no reuse.
      eq_filter = false;
    }
  }

  // One node's verdict: from the equivalence cache when it is valid for the
  // node's version (and, on a node with nominated pods, for the same set of
  // nominated pods), else computed into `own` or the cache slot.
  const Status* verdict(int pos, const NodeInfo& ni, Status& own, bool* hit) {
    if (rmask && !rmask[pos]) {
      *hit = true;
      return &rs->excluded;
    }
    if (!eq_filter) {
      own = fw.run_filter_with_nominated_pods(s, p, ni);
      return &own;
    }
    EqTable& t = eq->table;
    uint64_t sig = 0;
    bool cacheable = true;
    if (nom_mark && nom_mark[pos]) sig = fw.nominated_signature(s, p, sc.nom_list_[pos], &cacheable);
    const int64_t gen = sc.snapshot_.gen[pos];
    if (sig == 0) {  // no nominated pod counts for this pod: the plain verdict
      if (t.filter_gen[pos] == gen) {
        *hit = true;
      } else {
        t.filter[pos] = fw.run_filter(s, p, ni);
        t.filter_gen[pos] = gen;
      }
      return &t.filter[pos];
    }
    if (cacheable && t.nom_gen[pos] == gen && t.nom_sig[pos] == sig) {
      *hit = true;
      return &t.nom_filter[pos];
    }
    Status st = fw.run_filter_with_nominated_pods(s, p, ni);
    if (!cacheable) {
      own = std::move(st);
      return &own;
    }
    t.nom_filter[pos] = std::move(st);
    t.nom_gen[pos] = gen;
    t.nom_sig[pos] = sig;
    return &t.nom_filter[pos];
  }

  // The members of one gang that share a pod template are evaluated over the
  // node window of the first of them (upstream rotates the window every
  // cycle, numFeasibleNodesToFind > 100 nodes): a rank then reuses its
  // sibling's Filter verdicts and node-local scores for every node but the
  // one the sibling took, and the gang's candidates are the same nodes
  // XGMIGangAffinity ranks.
  void choose_window() {
    start = sc.next_start_node_;
    if (!sc.opts_.gang_window || full_diagnosis || !p.pg_key) return;
    if (p.pg_key == sc.window_gang_ && p.template_hash == sc.window_tmpl_ && sc.window_n_ == n) {
      start = sc.window_start_;
    } else {
      sc.window_gang_ = p.pg_key;
      sc.window_tmpl_ = p.template_hash;
      sc.window_start_ = start;
      sc.window_n_ = n;
    }
  }

  int at(int off) const { return start + off >= n ? start + off - n : start + off; }

  // The node at scan offset `off` evaluated again, its verdict recorded in the memo.
  const Status* rescan(int off, int pos) {
    bool hit = false;
    const Status* fp = verdict(pos, *sc.snapshot_.nodes[pos], sc.fail_buf_[pos], &hit);
    if (off < static_cast<int>(memo->gens.size())) {
      memo->gens[off] = sc.snapshot_.gen[pos];
      memo->ok[off] = fp->is_success();
    } else {
      memo->gens.push_back(sc.snapshot_.gen[pos]);
      memo->ok.push_back(fp->is_success());
    }
    return fp;
  }

  // The template's last scan of this window (EqEntry::scan): a gang rank
  // after its sibling re-evaluates only the scanned nodes whose version
  // changed since (usually the node the sibling took) and re-cuts the list at
  // numFeasibleNodesToFind, instead of walking the whole window again.
  // False (and the memo dropped) when the full walk has to run after all.
  bool serve_from_memo() {
    const auto& all = sc.snapshot_.nodes;
    bool ok = true;
    int reevaluated = 0;
    const int m = memo->processed;
    // The window is at most two contiguous runs of positions; each is checked
    // in blocks with memcmp, and only a block that differs element-wise.
    const int64_t* mg = memo->gens.data();
    const int64_t* sg = sc.snapshot_.gen.data();
    constexpr int kBlock = 32;
    for (int off0 = 0; off0 < m && ok;) {
      const int pos0 = at(off0);
      const int run = std::min({m - off0, n - pos0, kBlock});
      if (std::memcmp(mg + off0, sg + pos0, static_cast<size_t>(run) * sizeof(int64_t)) != 0) {
        for (int j = 0; j < run && ok; ++j) {
          const int off = off0 + j, pos = pos0 + j;
          if (mg[off] == sg[pos]) continue;
          const Status* fp = rescan(off, pos);
          ++reevaluated;
          ok = fp->is_success() || fp->is_unschedulable();
        }
      }
      off0 += run;
    }
    // Re-cut the list: branch-free appends (the buffers hold to_find + 1),
    // over the window's two contiguous runs ([start, n), then [0, ...)), with
    // every bound and base pointer in a local: a store to the int buffer
    // could alias the pass's own fields (`start` among them), which are
    // reached through `this`, and forced a reload per node.
    int off = 0, cc = 0;
    if (ok) {
      const char* okv = memo->ok.data();
      const NodeInfoPtr* allp = all.data();
      const NodeInfo** fb = sc.found_buf_.data();
      int* fpb = sc.found_pos_buf_.data();
      const int s0 = start, nn = n, mm = m, want = to_find;
      for (int run = 0; run < 2 && off < mm && cc < want; ++run) {
        const int first_off = off;
        const int first_pos = run == 0 ? s0 : 0;
        const int end_off = run == 0 ? std::min(mm, nn - s0) : mm;
        for (; off < end_off && cc < want; ++off) {
          const int pos = first_pos + (off - first_off);
          fb[cc] = allp[pos].get();
          fpb[cc] = pos;
          cc += okv[off] != 0;
        }
      }
    }
    for (; ok && cc < to_find && off < n; ++off) {  // the scan has to reach further now
      const int pos = at(off);
      const Status* fp = rescan(off, pos);
      ++reevaluated;
      ok = fp->is_success() || fp->is_unschedulable();
      if (fp->is_success()) {
        sc.found_buf_[cc] = all[pos].get();
        sc.found_pos_buf_[cc] = pos;
        ++cc;
      }
    }
    if (!ok || cc == 0) {  // an error, or nothing feasible (the diagnosis needs every verdict): the full walk
      memo->valid = false;
      return false;
    }
    c = cc;
    processed = off;
    memo->processed = off;
    hits = static_cast<uint64_t>(std::max(0, processed - reevaluated));
    return true;
  }

  // scanMemoVerify: the full walk must find the same nodes as the memo's
  // answer and stop at the same one.
  void verify_memo() {
    const auto& all = sc.snapshot_.nodes;
    bool mismatch = false;
    if (sc.opts_.scan_memo_verify) {
      int vc = 0, vp = 0;
      for (int i = 0; i < n && vc < to_find && !mismatch; ++i) {
        const int pos = at(i);
        bool hit = false;
        const Status* fp = verdict(pos, *all[pos], sc.fail_buf_[pos], &hit);
        ++vp;
        if (fp->is_success()) mismatch = vc >= c || sc.found_pos_buf_[vc++] != pos;
      }
      mismatch = mismatch || vc != c || vp != processed;
    }
    sc.cnt_.scan_memo_served.fetch_add(1, std::memory_order_relaxed);
    sc.cnt_.scan_memo_mismatches.fetch_add(mismatch, std::memory_order_relaxed);
  }

  // Serial path (every cluster below the parallel threshold, and larger
  // ones whose verdicts mostly come from the equivalence cache): plain
  // counters, no std::function call or atomic per node.
  void walk_serial() {
    const auto& all = sc.snapshot_.nodes;
    const int64_t t0 = Parallelizer::now_ns();
    if (memo) {  // one allocation for a new template's memo, not a doubling series
      memo->gens.clear();
      memo->ok.clear();
      memo->gens.reserve(static_cast<size_t>(n));
      memo->ok.reserve(static_cast<size_t>(n));
    }
    int cc = 0, done = 0;
    uint64_t nhit = 0;
    for (int i = 0; i < n; ++i) {
      int pos = start + i;
      if (pos >= n) pos -= n;
      const NodeInfo& ni = *all[pos];
      bool hit = false;
      const Status* fp = verdict(pos, ni, sc.fail_buf_[pos], &hit);
      nhit += hit;
      ++done;
      if (memo) {
        memo->gens.push_back(sc.snapshot_.gen[pos]);
        memo->ok.push_back(fp->is_success());
      }
      if (fp->is_success()) {
        sc.found_buf_[cc] = &ni;
        sc.found_pos_buf_[cc] = pos;
        if (++cc == to_find) break;
        continue;
      }
      if (fp->is_unschedulable()) {
        sc.fail_ptr_[pos] = fp;
        continue;
      }
      first_err = *fp;
      has_err = true;
      break;
    }
    c = cc;
    processed = done;
    hits = nhit;
    if (memo) {
      memo->valid = !has_err && c > 0;
      memo->start = start;
      memo->n = n;
      memo->to_find = to_find;
      memo->epoch = sc.snapshot_.node_epoch;
      memo->processed = processed;
    }
    Parallelizer::record_inline(&sc.filter_site_, Parallelizer::now_ns() - t0, processed, n);
  }

  // Forked walk over claimed chunks: a thread keeps its chunk's feasible
  // positions and cache misses in locals and publishes them with one
  // atomic each per chunk (a shared counter bumped per node serialised 16
  // workers on one cache line: the forked walk ran slower than the serial
  // one at 1,024 nodes, profiles/r6/README.md). Feasible nodes are kept in
  // chunk order up to numFeasibleNodesToFind; a chunk in flight when the
  // quota fills finishes its node, the rest of it stops at `stop`.
  void walk_forked() {
    const auto& all = sc.snapshot_.nodes;
    if (memo) memo->valid = false;
    std::atomic<int> count{0};
    std::atomic<bool> stop{false};
    std::atomic<uint64_t> amiss{0};
    std::mutex mu;
    sc.parallelizer_->until_forked_ranges(n, [&](int b, int e) {
      constexpr int kLocal = 64;
      int lpos[kLocal];
      int lc = 0;
      uint64_t miss = 0;
      auto flush = [&] {
        if (lc == 0) return;
        const int base = count.fetch_add(lc, std::memory_order_relaxed);
        const int keep = std::min(lc, to_find - base);
        for (int j = 0; j < keep; ++j) {
          sc.found_buf_[base + j] = all[lpos[j]].get();
          sc.found_pos_buf_[base + j] = lpos[j];
        }
        if (base + lc >= to_find) stop.store(true, std::memory_order_relaxed);
        lc = 0;
      };
      for (int i = b; i < e; ++i) {
        if (stop.load(std::memory_order_relaxed)) break;
        const int pos = at(i);
        Status own;
        bool hit = false;
        const Status* fp = verdict(pos, *all[pos], own, &hit);
        miss += !hit;
        if (fp->is_success()) {
          lpos[lc++] = pos;
          if (lc == kLocal) flush();
          continue;
        }
        if (fp->is_unschedulable()) {
          if (fp == &own) {
            sc.fail_buf_[pos] = std::move(own);
            fp = &sc.fail_buf_[pos];
          }
          sc.fail_ptr_[pos] = fp;
          continue;
        }
        std::lock_guard<std::mutex> g(mu);
        if (!has_err) {
          first_err = *fp;
          has_err = true;
          stop.store(true);
        }
        break;
      }
      flush();
      if (miss) amiss.fetch_add(miss, std::memory_order_relaxed);
    }, &stop, &sc.filter_site_);
    c = std::min(count.load(), to_find);
    // Processed = feasible kept + failed (upstream's feasible +
    // len(NodeToStatusMap)); counted here instead of by a shared atomic
    // that every worker would bump per node.
    processed = c;
    for (int pos = 0; pos < n; ++pos) processed += sc.fail_ptr_[pos] != nullptr;
    hits = static_cast<uint64_t>(std::max<int64_t>(0, static_cast<int64_t>(processed) - static_cast<int64_t>(amiss.load())));
  }

  // The failed nodes into the diagnosis; returns the count of failed nodes
  // per reason. Failed nodes mostly share a few Status objects (plugins
  // memoize their failures), so plugins and reasons are tallied per distinct
  // Status first.
  std::map<std::string, int> diagnose() {
    std::vector<std::pair<const Status*, int>> distinct;
    std::unordered_map<const void*, std::unordered_map<const void*, size_t>> index;  // past 32 distinct
    // A fresh diagnosis is recorded in deferred form: (position, status)
    // pairs over the snapshot's names and this cycle's Filter buffers, which
    // outlive every consumer of the diagnosis (PostFilter, FitError).
    const bool fresh = d.node_to_status.empty();
    if (fresh) d.node_to_status.defer(&sc.snapshot_.names, &sc.snapshot_.index);
    else d.node_to_status.reserve(d.node_to_status.size() + static_cast<size_t>(n));
    for (int pos = 0; pos < n; ++pos) {
      const Status* fs = sc.fail_ptr_[pos];
      if (!fs) continue;
      if (fresh) d.node_to_status.append_deferred(pos, fs);
      else d.node_to_status.emplace(sc.snapshot_.names[pos], *fs);
      size_t k = distinct.size();
      if (distinct.size() <= 32) {
        for (size_t j = 0; j < distinct.size(); ++j)
          if (distinct[j].first->reasons_id() == fs->reasons_id() && distinct[j].first->plugin_id() == fs->plugin_id()) {
            k = j;
            break;
          }
      } else {
        auto& by_plugin = index[fs->reasons_id()];
        auto it = by_plugin.find(fs->plugin_id());
        if (it != by_plugin.end()) k = it->second;
      }
      if (k == distinct.size()) {
        distinct.emplace_back(fs, 0);
        if (distinct.size() == 33)  // switch to the index
          for (size_t j = 0; j < distinct.size(); ++j)
            index[distinct[j].first->reasons_id()][distinct[j].first->plugin_id()] = j;
        else if (distinct.size() > 33)
          index[fs->reasons_id()][fs->plugin_id()] = k;
      }
      ++distinct[k].second;
    }
    std::map<std::string, int> reasons;
    for (const auto& [s0, cnt] : distinct) {
      d.unschedulable_plugins.insert(s0->failed_plugin());
      for (const auto& r : s0->reasons()) reasons[r] += cnt;
    }
    return reasons;
  }

  // Counters, the next cycle's start node, the feasible list out of the
  // scratch buffers, and the cycle's verdict.
  Status finish() {
    if (eq_filter) {
      sc.cnt_.eq_filter_hits.fetch_add(hits, std::memory_order_relaxed);
      sc.cnt_.eq_filter_misses.fetch_add(static_cast<uint64_t>(processed) - hits, std::memory_order_relaxed);
    }
    if (has_err) return first_err;
    sc.next_start_node_ = (start + processed) % n;
    feasible.assign(sc.found_buf_.begin(), sc.found_buf_.begin() + c);
    if (feasible_pos) feasible_pos->assign(sc.found_pos_buf_.begin(), sc.found_pos_buf_.begin() + c);
    if (feasible.empty()) return Status(Code::Unschedulable, fit_error_message(n, diagnose()));
    if (full_diagnosis) diagnose();
    return sc.extender_tail(p, n, feasible, feasible_pos, d, ext);
  }

  // The walk over the node window, by the strategy that fits it.
  Status walk() {
    rmask = rs ? rs->mask.data() : nullptr;
    use_equivalence_cache();
    choose_window();
    // Per-node failures go to a position-indexed buffer (no lock, no map
    // insert per node); the NodeToStatusMap is only materialized when the
    // diagnosis is consumed: no feasible node (PostFilter / FitError) or explain.
    // Equivalence-cache verdicts are referenced in place, not copied: a Status
    // copy bumps the refcount of a failure status shared by every node, and 16
    // workers doing that per node serialize on its cache line.
    if (static_cast<int>(sc.fail_buf_.size()) < n) sc.fail_buf_.resize(n);
    sc.fail_ptr_.assign(n, nullptr);
    if (static_cast<int>(sc.found_buf_.size()) < to_find + 1) sc.found_buf_.resize(to_find + 1);
    if (static_cast<int>(sc.found_pos_buf_.size()) < to_find + 1) sc.found_pos_buf_.resize(to_find + 1);
    memo = (sc.opts_.scan_memo && eq && eq_filter && !nom_mark && !full_diagnosis && !ext && !rmask) ? &eq->scan
                                                                                                      : nullptr;
    if (memo && !(memo->valid && memo->start == start && memo->n == n && memo->to_find == to_find &&
                  memo->epoch == sc.snapshot_.node_epoch))
      memo->valid = false;
    const bool inline_ok = sc.parallelizer_->plan_inline(n, &sc.filter_site_);
    if (memo && memo->valid && inline_ok && serve_from_memo()) verify_memo();
    else if (inline_ok) walk_serial();
    else walk_forked();
    return finish();
  }

  // Filter over a node set given as a short position list (the nodes hosting
  // a gang): only those nodes are evaluated, through the same verdict() as
  // the walk; the others get the set's `excluded` verdict in the diagnosis.
  Status listed() {
    const auto& all = sc.snapshot_.nodes;
    use_equivalence_cache();
    if (static_cast<int>(sc.fail_buf_.size()) < n) sc.fail_buf_.resize(n);
    std::vector<std::pair<int, const Status*>> failed;
    for (int pos : rs->list) {
      if (pos < 0 || pos >= n) continue;
      const NodeInfo& ni = *all[pos];
      bool hit = false;
      const Status* fp = verdict(pos, ni, sc.fail_buf_[pos], &hit);
      hits += hit;
      if (fp->is_success()) {
        feasible.push_back(&ni);
        if (feasible_pos) feasible_pos->push_back(pos);
      } else if (fp->is_unschedulable()) {
        failed.emplace_back(pos, fp);
      } else {
        return *fp;
      }
    }
    if (eq_filter) {
      sc.cnt_.eq_filter_hits.fetch_add(hits, std::memory_order_relaxed);
      sc.cnt_.eq_filter_misses.fetch_add(rs->list.size() - hits, std::memory_order_relaxed);
    }
    if (!feasible.empty()) {
      Status es = sc.extender_tail(p, n, feasible, feasible_pos, d, ext);
      if (!feasible.empty() || !es.is_unschedulable()) return es;
    }
    if (rs->fallback) return Status(Code::Unschedulable);  // the caller evaluates every node
    sc.diagnose_every_node(d, rs->excluded, &failed);
    return Status(Code::Unschedulable, fit_error_message(n, d.node_to_status));
  }
};

Status Scheduler::find_nodes_that_fit(Framework& fw, CycleState& s, const Pod& p, Diagnosis& d, NodeList& feasible,
                                      EqEntry* eq, bool full_diagnosis, std::vector<int>* feasible_pos) {
  // Extenders filter after the plugins; the diagnosis must then be complete,
  // since the FitError may come from nodes only an extender rejected.
  const bool ext = extenders_interested(p);
  full_diagnosis = full_diagnosis || ext;
  int64_t pf0 = tracer_.enabled() ? clock_->now_us() : 0;
  Status st = fw.run_pre_filter(s, p);
  if (tracer_.enabled()) tracer_.record(TraceEvent{"prefilter", p.key(), "", pf0, clock_->now_us() - pf0, 0});
  const auto& all = snapshot_.nodes;
  const int n = static_cast<int>(all.size());
  feasible.clear();
  if (feasible_pos) feasible_pos->clear();
  if (!st.is_success()) {
    if (!st.is_unschedulable()) return st;
    diagnose_every_node(d, st);
    return Status(Code::Unschedulable, st.message()).with_plugin(st.failed_plugin());
  }
  // Prefer the nominated node (PreferNominatedNode, beta in 1.23).
  if (!p.nominated_node_name.empty()) {
    auto it = snapshot_.index.find(p.nominated_node_name);
    if (it != snapshot_.index.end()) {
      const NodeInfo* ni = all[it->second].get();
      Status nst = fw.run_filter_with_nominated_pods(s, p, *ni);
      if (nst.is_success()) {
        feasible.push_back(ni);
        if (feasible_pos) feasible_pos->push_back(static_cast<int>(it->second));
        // evaluateNominatedNode: the extenders see the nominated node too;
        // when they reject it the full search below runs.
        Status es = extender_tail(p, n, feasible, feasible_pos, d, ext);
        if (!es.is_unschedulable()) return es;
      } else if (!nst.is_unschedulable()) {
        return nst;
      }
    }
  }
  if (n == 0) return Status(Code::Unschedulable, "no nodes available to schedule pods");
  const int to_find = num_feasible_nodes_to_find(fw, n);
  if (!fw.has(kFilter)) {
    for (int i = 0; i < std::min(n, to_find); ++i) {
      int pos = (next_start_node_ + i) % n;
      feasible.push_back(all[pos].get());
      if (feasible_pos) feasible_pos->push_back(pos);
    }
    next_start_node_ = (next_start_node_ + static_cast<int>(feasible.size())) % n;
    return extender_tail(p, n, feasible, feasible_pos, d, ext);
  }
  // A PreFilter node set (NodeRestriction, upstream's PreFilterResult; the
  // xGMI gang co-location plan of NodeResourceTopologyMatch): a short list is
  // evaluated directly, a larger set through a mask over the usual walk.
  const NodeRestriction* rs = s.read_as<NodeRestriction>(kNodeRestrictionKey);
  if (rs && rs->nodes != all.size()) rs = nullptr;  // planned for another node set
  if (rs && rs->list.empty() && rs->mask.empty()) {
    if (!rs->fallback) {  // nothing qualifies and the plugin allows no fallback
      diagnose_every_node(d, rs->excluded);
      return Status(Code::Unschedulable, fit_error_message(n, d.node_to_status)).with_plugin(rs->excluded.failed_plugin());
    }
    rs = nullptr;
  }
  auto pass = [&](const NodeRestriction* set) {
    return FilterPass{*this, fw, s, p, d, feasible, feasible_pos, eq, set, full_diagnosis, ext, n, to_find};
  };
  if (rs) {
    Status r = rs->mask.empty() ? pass(rs).listed() : pass(rs).walk();
    // None of the set's nodes fits and the plugin allows the fallback: every
    // node, as without the set.
    if (!(r.is_unschedulable() && feasible.empty() && rs->fallback)) return r;
    d = Diagnosis{};
    feasible.clear();
    if (feasible_pos) feasible_pos->clear();
  }
  return pass(nullptr).walk();
}

}  // namespace xsched
