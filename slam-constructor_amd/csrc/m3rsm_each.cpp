// m3rsm_each.cpp -- see m3rsm_each.h.  No HIP in here: any C++17 compiler (-ffp-contract=off), linked with -pthread.
#include "m3rsm_each.h"

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <functional>
#include <memory>
#include <mutex>
#include <thread>

namespace slamhip {
namespace m3rsm {

// run(n, fn) has fn(0) .. fn(n - 1) called, each once, by the workers and the caller, and returns when all of them have
// returned; the items are independent, so who takes which changes nothing.
struct Pool::Workers {
  explicit Workers(int n_threads) {
    for (int t = 1; t < n_threads; ++t) threads_.emplace_back([this] { loop(); });
  }
  ~Workers() {
    {
      std::lock_guard<std::mutex> lock(mu_);
      stop_ = true;
    }
    go_.notify_all();
    for (std::thread &t : threads_) t.join();
  }
  void run(int n_items, const std::function<void(int)> &fn) {
    if (threads_.empty() || n_items <= 1) {
      for (int i = 0; i < n_items; ++i) fn(i);
      return;
    }
    {
      std::lock_guard<std::mutex> lock(mu_);
      fn_ = &fn;
      n_items_ = n_items;
      next_.store(0, std::memory_order_relaxed);
      busy_ = (int)threads_.size();
      ++generation_;
    }
    go_.notify_all();
    take(fn, n_items);
    std::unique_lock<std::mutex> lock(mu_);
    done_.wait(lock, [this] { return busy_ == 0; });
  }


  void take(const std::function<void(int)> &fn, int n_items) {
    for (int i; (i = next_.fetch_add(1, std::memory_order_relaxed)) < n_items;) fn(i);
  }
  void loop() {
    long long seen = 0;
    for (;;) {
      const std::function<void(int)> *fn;
      int n_items;
      {
        std::unique_lock<std::mutex> lock(mu_);
        go_.wait(lock, [&] { return stop_ || generation_ != seen; });
        if (stop_) return;
        seen = generation_;
        fn = fn_;
        n_items = n_items_;
      }
      take(*fn, n_items);
      {
        std::lock_guard<std::mutex> lock(mu_);
        if (--busy_ == 0) done_.notify_one();
      }
    }
  }
  std::vector<std::thread> threads_;
  std::mutex mu_;
  std::condition_variable go_, done_;
  const std::function<void(int)> *fn_ = nullptr;
  std::atomic<int> next_{0};
  int n_items_ = 0, busy_ = 0;
  long long generation_ = 0;
  bool stop_ = false;
};

Pool::Pool(int threads) : threads_(std::max(1, std::min(threads, kEachMaxThreads))), workers_(new Workers(threads_)) {}
Pool::~Pool() { delete workers_; }

void split_by_bytes(const size_t *bytes, int n, size_t limit, std::vector<int> *first) {
  first->assign(1, 0);
  size_t sum = 0;
  for (int i = 0; i < n; ++i) {
    if (i > first->back() && (bytes[i] > limit || sum > limit - bytes[i])) {
      first->push_back(i);
      sum = 0;
    }
    sum += bytes[i];
  }
  if (n > 0) first->push_back(n);
}

int each_default_threads(int n_jobs) { return std::max(1, std::min(n_jobs, 8)); }

int run_each(const Config *cfgs, int n_jobs, const ScoreManyFn &score_roots, const ExpandManyFn &expand, Result *results,
             int *codes, std::vector<Call> *traces, int threads) {
  if (n_jobs < 1 || threads < 0 || threads > kEachMaxThreads) return kErrInvalid;
  if (threads == 0) threads = each_default_threads(n_jobs);
  Pool pool(std::min(threads, n_jobs));
  return run_each(cfgs, n_jobs, score_roots, expand, results, codes, traces, &pool);
}

int run_each(const Config *cfgs, int n_jobs, const ScoreManyFn &score_roots, const ExpandManyFn &expand, Result *results,
             int *codes, std::vector<Call> *traces, Pool *pool) {
  if (n_jobs < 1 || !cfgs || !results || !codes || !pool) return kErrInvalid;
  for (int j = 0; j < n_jobs; ++j) {
    results[j] = Result{};
    codes[j] = kPending;
    if (traces) traces[j].clear();
  }
  for (int j = 0; j < n_jobs; ++j)
    if (Search::check(cfgs[j], 1) != kOk || cfgs[j].width != cfgs[0].width || cfgs[j].depth != cfgs[0].depth ||
        cfgs[j].max_super_steps != cfgs[0].max_super_steps)
      return kErrInvalid;
  const int depth = cfgs[0].depth, slots = slots_of(depth);
  Pool::Workers &workers = *pool->workers_;

  // what goes into a call and comes out of it: the candidates (or parents) of the jobs one after another, job `live[k]`
  // owning entries [first[k], first[k + 1])
  std::vector<int> live(n_jobs), req;
  std::vector<size_t> first(n_jobs + 1, 0);
  std::vector<double> rot, rect, out_rect, out_score;
  std::vector<int> out_level;
  std::vector<std::unique_ptr<Search>> search(n_jobs);
  // (a callback's failure: every job that has not ended carries its code)
  const auto callback_failed = [&](int rc) {
    for (int j = 0; j < n_jobs; ++j)
      if (codes[j] == kPending) results[j].callback_rc = rc;
    return kErrCallback;
  };

  {  // all root layers in ONE call, job by job
    std::vector<double> r_rot;
    std::vector<Rect> r_rect;
    for (int j = 0; j < n_jobs; ++j) {
      live[j] = j;
      root_candidates(cfgs[j], &r_rot, &r_rect);
      first[j + 1] = first[j] + r_rot.size();
      if (first[j + 1] > 0x7fffffffu) return kErrInvalid;
      for (size_t i = 0; i < r_rot.size(); ++i) {
        req.push_back(j);
        rot.push_back(r_rot[i]);
        rect.insert(rect.end(), {r_rect[i].bot, r_rect[i].top, r_rect[i].left, r_rect[i].right});
      }
    }
    const size_t n = first[n_jobs];
    out_score.resize(n);
    out_level.resize(n);
    const int rc = score_roots((int)n, req.data(), rot.data(), rect.data(), out_score.data(), out_level.data());
    if (rc) return callback_failed(rc);
  }
  const std::vector<int> zeros(first[n_jobs], 0);  // (a search numbers its one request 0, as the lone run does)
  bool roots = true;
  for (;;) {
    // the host half of a round, job by job on the workers: take the answer in, run on to the end or the next request
    const std::function<void(int)> step = [&](int k) {
      const int j = live[k];
      const size_t at = first[k], n = first[k + 1] - first[k];
      if (roots) {
        search[j].reset(new Search(cfgs[j], 1, &results[j], traces ? &traces[j] : nullptr));
        ++results[j].launches;
        results[j].scored += (long long)n;
        search[j]->commit_roots(n, zeros.data(), rot.data() + at, rect.data() + 4 * at, out_score.data() + at,
                                out_level.data() + at);
      } else {
        search[j]->absorb(out_rect.data() + 4 * at * slots, out_score.data() + at * slots, out_level.data() + at * slots);
      }
      codes[j] = search[j]->advance();
      if (codes[j] != kPending) search[j].reset();  // (its memo goes here, on the worker, not at the end of the call)
    };
    workers.run((int)live.size(), step);
    roots = false;
    // the waiting searches' parents in job order; a search that has ended takes no further part
    int failed = kOk;
    size_t n_live = 0, n = 0;
    req.clear();
    rot.clear();
    rect.clear();
    for (size_t k = 0; k < live.size(); ++k) {
      const int j = live[k];
      if (codes[j] == kErrSuperSteps || codes[j] == kErrScorer) {
        if (failed == kOk) failed = codes[j];
        continue;
      }
      if (codes[j] != kPending) continue;
      const Search &s = *search[j];
      const int np = s.n_parents();
      req.insert(req.end(), np, j);
      rot.insert(rot.end(), s.parent_rotation(), s.parent_rotation() + np);
      rect.insert(rect.end(), s.parent_rect(), s.parent_rect() + 4 * (size_t)np);
      live[n_live] = j;
      first[n_live] = n;
      n += (size_t)np;
      first[++n_live] = n;
    }
    live.resize(n_live);
    if (failed != kOk) return failed;
    if (n_live == 0) return kOk;
    if (n * (size_t)slots > 0x7fffffffu) return kErrInvalid;
    out_rect.resize(4 * n * slots);
    out_score.resize(n * slots);
    out_level.resize(n * slots);
    const int rc = expand((int)n, req.data(), rot.data(), rect.data(), depth, out_rect.data(), out_score.data(), out_level.data());
    if (rc) return callback_failed(rc);
  }
}

}  // namespace m3rsm
}  // namespace slamhip
