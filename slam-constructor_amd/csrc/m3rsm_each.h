// m3rsm_each.h -- K INDEPENDENT multi-resolution searches advancing in lock-step: one scoring call for all root layers,
// then one expand call per round for the parents of every search that waits for one.  Host C++ without HIP, like the
// engine (m3rsm_engine.h) whose resumable Search it drives; this file holds the threads, the engine has none.
//
// Every search has its own queue, best finest probability, memo and trace, so job j's Result, code and trace are those of
// m3rsm::run on cfgs[j] alone (same width and depth), bit for bit, whatever the other jobs are and however many threads
// work: the searches share nothing but the calls.
#pragma once

#include <vector>

#include "m3rsm_engine.h"

namespace slamhip {
namespace m3rsm {

constexpr int kEachMaxThreads = 16;
// the workers of a call when the caller names none (threads = 0): min(n_jobs, 8) -- never the machine's CPU count
int each_default_threads(int n_jobs);

// Worker threads kept between calls (a thread keeps the memo tables of the searches it has run for the next ones):
// `threads` - 1 of them, the caller being the first worker; 1 .. kEachMaxThreads.  One call at a time uses a pool.
class Pool {
 public:
  explicit Pool(int threads);
  ~Pool();
  Pool(const Pool &) = delete;
  Pool &operator=(const Pool &) = delete;
  int threads() const { return threads_; }

 private:
  struct Workers;
  friend int run_each(const Config *, int, const ScoreManyFn &, const ExpandManyFn &, Result *, int *, std::vector<Call> *, Pool *);
  int threads_;
  Workers *workers_;
};

// cfgs[j]: job j's limits and steps; width, depth and max_super_steps must be the same in all of them.
//   score_roots: ONE call, the root layers job by job, request[i] = job.
//   expand:      one call per round, the parents of the waiting jobs concatenated in job order, request[i] = job.
// Both callbacks run on the calling thread.  Between two calls the live searches absorb their slice of the answer and
// run on to their end or their next expand request on `threads` workers (1: inline on the caller; 0: the default; at most
// kEachMaxThreads); every output is the same for every thread count.
// results[j], codes[j], traces[j] (traces may be null): per job.  Result::launches of a job is what its lone run would
// have made (1 + its super-steps); the call itself makes 1 + the number of rounds callbacks.
// Returns kOk when every job ended with kOk or kErrNoMatch (a job that finds no match ends alone); kErrInvalid;
// kErrSuperSteps / kErrScorer of the lowest job that met one, which ends the call; kErrCallback (the callback's code is
// in the Result of every job that had not ended).  A job the call's end overtook has code kPending.
int run_each(const Config *cfgs, int n_jobs, const ScoreManyFn &score_roots, const ExpandManyFn &expand, Result *results,
             int *codes, std::vector<Call> *traces, int threads);
// the same on the workers of a pool the caller keeps
int run_each(const Config *cfgs, int n_jobs, const ScoreManyFn &score_roots, const ExpandManyFn &expand, Result *results,
             int *codes, std::vector<Call> *traces, Pool *pool);

// A call whose staging would outgrow `limit` bytes, cut into consecutive calls: entry i needs bytes[i]; *first receives
// the index each call starts at, then n.  A call takes entries while their sum stays within the limit, and one entry at
// least (an entry larger than the limit goes alone).  n < 1: *first = {0}.
void split_by_bytes(const size_t *bytes, int n, size_t limit, std::vector<int> *first);

}  // namespace m3rsm
}  // namespace slamhip
