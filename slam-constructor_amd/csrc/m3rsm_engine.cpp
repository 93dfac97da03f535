// m3rsm_engine.cpp -- see m3rsm_engine.h.  No HIP in here: compiles with any C++17 compiler (-ffp-contract=off).
#include "m3rsm_engine.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <queue>
#include <vector>

namespace slamhip {
namespace m3rsm {
namespace {

// are_equal / less_or_equal of math_utils.h:15-39
bool are_equal(double a, double b) {
  const double eps_scale = std::max(1.0, std::max(std::abs(a), std::abs(b)));
  return std::abs(a - b) <= 1e-7 * eps_scale;
}
bool less_or_equal(double a, double b) { return are_equal(a, b) || less(a, b); }

struct Match {
  double prob, rotation;
  Rect rect;
  double abs_rotation, drift_amount;
  int request;  // (Match::spe / filtered_scan / pose / map: whose they are; no part of the order)
  bool finest() const { return drift_amount <= 0; }
  // true if this match is LESS preferable (Match::operator<)
  bool operator<(const Match &that) const {
    if (!are_equal(prob, that.prob)) return less(prob, that.prob);
    if (!are_equal(drift_amount, that.drift_amount)) return drift_amount > that.drift_amount;
    return abs_rotation > that.abs_rotation;
  }
};

Match make_match(int request, double rotation, const Rect &r, double prob) {
  return Match{prob, rotation, r, std::abs(rotation), (r.right - r.left) + (r.top - r.bot), request};
}

struct Key {
  uint64_t w[6];
  bool operator==(const Key &o) const { return std::memcmp(w, o.w, sizeof(w)) == 0; }
};
struct KeyHash {
  size_t operator()(const Key &k) const {
    uint64_t h = 0x9e3779b97f4a7c15ull;
    for (uint64_t v : k.w) {
      h ^= v + 0x9e3779b97f4a7c15ull + (h << 6) + (h >> 2);
      h *= 0xff51afd7ed558ccdull;
      h ^= h >> 32;
    }
    return (size_t)h;
  }
};
Key key_of(int request, double rotation, const Rect &r) {
  const double v[5] = {rotation, r.bot, r.top, r.left, r.right};
  Key k;
  std::memcpy(k.w, v, sizeof(v));
  k.w[5] = (uint64_t)request;
  return k;
}
struct Bound {
  double score;
  int level;
};

// The memo: key -> bound, open addressing with linear probing in ONE array of 64-byte entries; nothing is ever erased.
// (A node-based map costs an allocation per insert and two or three cache misses per lookup; a match memoises 22 636
// nodes on the benchmark scene and the host is the larger part of its time)  An entry is in use when it
// carries the table's stamp, so a table is emptied by a new stamp, and a thread keeps the tables of the searches it
// has finished for the ones it starts next: a match after the first neither allocates nor clears its memo.
class Memo {
 public:
  explicit Memo(size_t expected) {
    size_t cap = 1024;
    while (cap * 3 < expected * 4) cap *= 2;  // load <= 3/4
    std::vector<Table> &spare = spares();
    for (size_t i = 0; i < spare.size(); ++i)
      if (spare[i].entries.size() >= cap) {
        t_.entries.swap(spare[i].entries);
        t_.stamp = spare[i].stamp;
        spare.erase(spare.begin() + (long)i);
        if (t_.stamp == 0x7fffffff) {  // (stamps used up: clear for once)
          std::fill(t_.entries.begin(), t_.entries.end(), Entry{});
          t_.stamp = 0;
        }
        ++t_.stamp;
        return;
      }
    t_.entries.resize(cap);
    t_.stamp = 1;
  }
  ~Memo() {
    std::vector<Table> &spare = spares();
    if (spare.size() < kSpares && t_.entries.size() <= kSpareEntries) spare.push_back(std::move(t_));
  }
  Memo(const Memo &) = delete;
  Memo &operator=(const Memo &) = delete;
  const Bound *find(const Key &k) const {
    const Entry &e = *slot(t_, k);
    return e.stamp == t_.stamp ? &e.bound : nullptr;
  }
  void set(const Key &k, const Bound &b) {
    if ((size_ + 1) * 4 > t_.entries.size() * 3) grow();
    Entry *e = slot(t_, k);
    if (e->stamp != t_.stamp) {
      e->stamp = t_.stamp;
      e->key = k;
      ++size_;
    }
    e->bound = b;
  }

 private:
  struct Entry {
    Key key;
    Bound bound;
    int stamp;  // 0: never used
  };
  struct Table {
    std::vector<Entry> entries;  // a power of two of them
    int stamp = 1;
  };
  static constexpr size_t kSpares = 16, kSpareEntries = (size_t)1 << 16;  // what a thread keeps: 16 tables of <= 4 MiB
  static std::vector<Table> &spares() {
    thread_local std::vector<Table> kept;
    return kept;
  }
  // the entry that holds k, or the free one where it would go
  template <class T>
  static auto slot(T &t, const Key &k) -> decltype(&t.entries[0]) {
    const size_t mask = t.entries.size() - 1;
    for (size_t i = KeyHash()(k) & mask;; i = (i + 1) & mask)
      if (t.entries[i].stamp != t.stamp || t.entries[i].key == k) return &t.entries[i];
  }
  void grow() {
    Table bigger;
    bigger.entries.resize(t_.entries.size() * 2);
    for (const Entry &e : t_.entries)
      if (e.stamp == t_.stamp) {
        Entry *to = slot(bigger, e.key);
        *to = e;
        to->stamp = bigger.stamp;
      }
    t_ = std::move(bigger);
  }
  Table t_;
  size_t size_ = 0;
};

// std::priority_queue, plus a look at the heap it keeps (the speculation reads ahead in it without popping)
struct Queue : std::priority_queue<Match> {
  const std::vector<Match> &heap() const { return c; }
};

}  // namespace

struct Search::Impl {
  const Config &cfg;
  Result *res;
  std::vector<Call> *trace;
  Queue matches;
  double best_finest = 0.0;
  Memo memo;
  std::vector<double> p_rot, p_rect;
  std::vector<int> p_req;
  std::vector<size_t> front;
  Match waiting{};  // the popped match whose children the expand call at hand scores
  int waiting_child = 0;
  bool has_waiting = false;

  // (room per request for what a lone match memoises: the table is not rebuilt on the way up)
  Impl(const Config &c, int n_requests, Result *r, std::vector<Call> *t)
      : cfg(c), res(r), trace(t), memo((size_t)(3 << 13) * (size_t)std::min(std::max(n_requests, 1), 64)) {}

  // M3RSMEngine::add_match with max_finest_prob_diff = 0, after the call has been committed to the trace
  void commit(int request, double rotation, const Rect &r, const Bound &b) {
    ++res->scorer_calls;
    if (trace) trace->push_back(Call{rotation, r, b.score, b.level, request});
    Match m = make_match(request, rotation, r, b.score);
    if (m.prob < best_finest) return;
    if (m.finest()) best_finest = std::max(best_finest, m.prob - 0.0);
    matches.push(std::move(m));
  }

  bool expanded(const Match &m) const {
    Rect kids[kMaxChildren];
    const int n = children(m.rect, cfg.translation_step, kids);
    return n == 0 || memo.find(key_of(m.request, m.rotation, kids[0])) != nullptr;
  }

  // the parents of one expand call: `first` and the next width - 1 entries of the queue that have children nobody has
  // scored yet
  void gather(const Match &first) {
    p_req.clear();
    p_rot.clear();
    p_rect.clear();
    auto add = [&](const Match &m) {
      p_req.push_back(m.request);
      p_rot.push_back(m.rotation);
      p_rect.insert(p_rect.end(), {m.rect.bot, m.rect.top, m.rect.left, m.rect.right});
    };
    add(first);
    if (cfg.width > 1 && !matches.empty()) {
      // the queue's entries from the top down, without popping: a best-first walk over the binary heap (an entry is not
      // better than its parent), through a small heap of positions.  Which entries ride along changes no result.
      const std::vector<Match> &heap = matches.heap();
      const auto worse = [&heap](size_t a, size_t b) { return heap[a] < heap[b]; };
      front.assign(1, 0);
      long long looked = 0;
      const long long look_limit = 4ll * cfg.width + 64;  // (points and expanded entries are passed over, not for ever)
      while ((int)p_rot.size() < cfg.width && !front.empty() && looked < look_limit) {
        std::pop_heap(front.begin(), front.end(), worse);
        const size_t i = front.back();
        front.pop_back();
        const Match &m = heap[i];
        if (!m.finest() && !expanded(m)) add(m);
        for (size_t c = 2 * i + 1; c <= 2 * i + 2 && c < heap.size(); ++c) {
          front.push_back(c);
          std::push_heap(front.begin(), front.end(), worse);
        }
        ++looked;
      }
    }
  }

  // The children of the popped match, committed in the reference's order, from child `from` on.  A child the memo lacks
  // stops it: kPending with the parents of the expand call that will deliver it (the queue holds the children committed
  // so far, as it would mid-branch), the match and the child kept for the resumption.  Usually that is child 0 -- an
  // expand call scores all children of a parent --, but a point may have been scored as the corner of a neighbouring box.
  int branch(const Match &m, int from, bool may_ask) {
    Rect kids[kMaxChildren];
    const int n = children(m.rect, cfg.translation_step, kids);
    for (int c = from; c < n; ++c) {
      const Bound *it = memo.find(key_of(m.request, m.rotation, kids[c]));
      if (!it) {
        if (!may_ask) return kErrScorer;
        if (res->super_steps >= cfg.max_super_steps) return kErrSuperSteps;
        gather(m);
        waiting = m;
        waiting_child = c;
        has_waiting = true;
        return kPending;
      }
      commit(m.request, m.rotation, kids[c], *it);
      may_ask = true;
    }
    return kOk;
  }
};

int Search::check(const Config &cfg, int n_requests) {
  if (!(cfg.angle_step > 0) || !(cfg.translation_step > 0) || !(cfg.max_x_error >= 0) || !(cfg.max_y_error >= 0) ||
      !(cfg.max_th_error >= 0) || !std::isfinite(cfg.max_x_error) || !std::isfinite(cfg.max_y_error) ||
      !std::isfinite(cfg.max_th_error) || !std::isfinite(cfg.angle_step) || !std::isfinite(cfg.translation_step) ||
      cfg.width < 1 || cfg.depth < 1 || cfg.depth > kMaxDepth || cfg.max_super_steps < 1 || n_requests < 1)
    return kErrInvalid;
  return kOk;
}

Search::Search(const Config &cfg, int n_requests, Result *result, std::vector<Call> *trace)
    : impl_(new Impl(cfg, n_requests, result, trace)) {
  *result = Result{};
  if (trace) trace->clear();
}

Search::~Search() { delete impl_; }

void Search::commit_roots(size_t n, const int *request, const double *rotation, const double *rect, const double *score,
                          const int *level) {
  for (size_t g = 0; g < n; ++g)
    impl_->commit(request[g], rotation[g], Rect{rect[4 * g], rect[4 * g + 1], rect[4 * g + 2], rect[4 * g + 3]},
                  Bound{score[g], level[g]});
}

// BruteForceMultiResolutionScanMatcher::process_scan's loop around M3RSMEngine::next_best_match
int Search::advance() {
  Impl &e = *impl_;
  Result *result = e.res;
  if (e.has_waiting) {  // (the expand call it waited for has been absorbed: the child is there, or the scorer is wrong)
    e.has_waiting = false;
    const Match m = e.waiting;
    const int rc = e.branch(m, e.waiting_child, false);
    if (rc) return rc;
  }
  for (;;) {
    if (e.matches.empty()) return kErrNoMatch;
    const Match best = e.matches.top();
    e.matches.pop();
    if (best.finest()) {
      const double hside = best.rect.right - best.rect.left, vside = best.rect.top - best.rect.bot;
      result->delta[0] = best.rect.left + hside / 2;
      result->delta[1] = best.rect.bot + vside / 2;
      result->delta[2] = best.rotation;
      result->prob = best.prob;
      result->request = best.request;
      return kOk;
    }
    // (children() is next_best_match's branching decision and, for a box that no longer branches, the five points)
    ++result->branching_pops;
    const int rc = e.branch(best, 0, true);
    if (rc) return rc;
  }
}

int Search::n_parents() const { return (int)impl_->p_rot.size(); }
const int *Search::parent_request() const { return impl_->p_req.data(); }
const double *Search::parent_rotation() const { return impl_->p_rot.data(); }
const double *Search::parent_rect() const { return impl_->p_rect.data(); }

void Search::absorb(const double *s_rect, const double *s_score, const int *s_level) {
  Impl &e = *impl_;
  ++e.res->super_steps;
  ++e.res->launches;
  const int n = (int)e.p_rot.size(), slots = slots_of(e.cfg.depth);
  for (int i = 0; i < n; ++i)
    for (int s = 0; s < slots; ++s) {
      const size_t g = (size_t)i * slots + s;
      if (std::isnan(s_rect[4 * g])) continue;  // no node in this slot
      ++e.res->scored;
      const Rect r{s_rect[4 * g], s_rect[4 * g + 1], s_rect[4 * g + 2], s_rect[4 * g + 3]};
      e.memo.set(key_of(e.p_req[i], e.p_rot[i], r), Bound{s_score[g], s_level[g]});
    }
}

void root_candidates(const Config &cfg, std::vector<double> *rotation, std::vector<Rect> *rect) {
  rotation->clear();
  rect->clear();
  const Rect empty{0, 0, 0, 0}, entire{-cfg.max_y_error, cfg.max_y_error, -cfg.max_x_error, cfg.max_x_error};
  const double sector = 2 * cfg.max_th_error;
  double drift = 0;
  while (less_or_equal(2 * drift, sector)) {
    // std::set<double>{drift, -drift}: ascending, and -0 is 0 (the first of the two stays)
    const double rots[2] = {-drift, drift};
    for (int k = (drift == 0 ? 1 : 0); k < 2; ++k) {
      rotation->push_back(rots[k]);
      rect->push_back(empty);
      rotation->push_back(rots[k]);
      rect->push_back(entire);
    }
    drift += cfg.angle_step;
  }
}

int run(const Config &cfg, const ScoreFn &score_roots, const ExpandFn &expand, Result *result, std::vector<Call> *trace) {
  const ScoreManyFn roots = [&](int n, const int *, const double *rotation, const double *rect, double *score, int *level) {
    return score_roots(n, rotation, rect, score, level);
  };
  const ExpandManyFn expand_many = [&](int n, const int *, const double *rotation, const double *rect, int depth,
                                       double *slot_rect, double *slot_score, int *slot_level) {
    return expand(n, rotation, rect, depth, slot_rect, slot_score, slot_level);
  };
  return run_many(cfg, 1, roots, expand_many, result, trace);
}

int run_many(const Config &cfg, int n_requests, const ScoreManyFn &score_roots, const ExpandManyFn &expand, Result *result,
             std::vector<Call> *trace) {
  *result = Result{};
  if (trace) trace->clear();
  if (Search::check(cfg, n_requests) != kOk) return kErrInvalid;
  Search e(cfg, n_requests, result, trace);
  {
    // add_scan_matching_request once per request: every request's root layer is the same list, bounded in one call
    std::vector<double> rot;
    std::vector<Rect> rect;
    root_candidates(cfg, &rot, &rect);
    const size_t per = rot.size(), n = per * (size_t)n_requests;
    if (n > 0x7fffffffu) return kErrInvalid;
    std::vector<double> all_rot(n), flat(4 * n), score(n);
    std::vector<int> req(n), level(n);
    for (size_t g = 0; g < n; ++g) {
      const size_t i = g % per;
      req[g] = (int)(g / per);
      all_rot[g] = rot[i];
      flat[4 * g] = rect[i].bot;
      flat[4 * g + 1] = rect[i].top;
      flat[4 * g + 2] = rect[i].left;
      flat[4 * g + 3] = rect[i].right;
    }
    const int rc = score_roots((int)n, req.data(), all_rot.data(), flat.data(), score.data(), level.data());
    ++result->launches;
    result->scored += (long long)n;
    if (rc) {
      result->callback_rc = rc;
      return kErrCallback;
    }
    e.commit_roots(n, req.data(), all_rot.data(), flat.data(), score.data(), level.data());
  }
  std::vector<double> s_rect, s_score;
  std::vector<int> s_level;
  const int slots = slots_of(cfg.depth);
  for (;;) {
    const int rc = e.advance();
    if (rc != kPending) return rc;
    const int n = e.n_parents();
    const size_t n_out = (size_t)n * slots;
    s_rect.resize(4 * n_out);
    s_score.resize(n_out);
    s_level.resize(n_out);
    const int xrc = expand(n, e.parent_request(), e.parent_rotation(), e.parent_rect(), cfg.depth, s_rect.data(), s_score.data(),
                           s_level.data());
    if (xrc) {
      ++result->super_steps;
      ++result->launches;
      result->callback_rc = xrc;
      return kErrCallback;
    }
    e.absorb(s_rect.data(), s_score.data(), s_level.data());
  }
}

}  // namespace m3rsm
}  // namespace slamhip
