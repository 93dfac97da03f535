// m3rsm_engine.h -- the best-first engine of the multi-resolution matcher (BF_M3RSM) as a replay over memoised scores.
// Host C++ without HIP: the two scoring calls are injected, so the engine runs on a CPU against any scorer.
//
// What it restates (paths relative to the reference root):
//   Match::operator<                               src/core/scan_matchers/m3rsm_engine.h:192-204
//   M3RSMEngine (add_match, the root layer, next_best_match, branch)
//                                                  src/core/scan_matchers/m3rsm_engine.h:252-365
//   BruteForceMultiResolutionScanMatcher::process_scan
//                                                  src/core/scan_matchers/bf_multi_res_scan_matcher.h:24-67
//
// The loop is the reference's, call for call: a std::priority_queue of matches (libstdc++'s heap, as there: the
// comparator is no strict weak order, so WHICH heap it is matters), the `< best finest probability` cut of add_match,
// the five crucial points of a box that no longer branches, the end at a top that is a point.  What differs is where a
// score comes from: a memo keyed by (request, rotation, rectangle) bit patterns.  When the loop needs a child the memo does not
// hold, the engine takes the popped match and the next `width` - 1 unexpanded non-point entries of a copy of the queue
// and has ONE expand call score all their descendants to `depth` generations (a "super-step").  A score is a pure
// function of its node, so the sequence of committed calls -- the trace -- is the reference's whatever width and depth.
#pragma once

#include <functional>
#include <vector>

#include "m3rsm_split.h"

namespace slamhip {
namespace m3rsm {

struct Config {
  double max_x_error = 1, max_y_error = 1, max_th_error = 0.08726646259971647;  // init_bf_m3rsm's defaults
  double angle_step = 0.0017453292519943296, translation_step = 0.05;
  int width = 32, depth = 3;  // speculation: parents per expand call, generations per parent (measured: DESIGN.md §6)
  long long max_super_steps = 1 << 20;  // per match: reaching it is an error, not a spin
};

// one committed scorer call: what the reference's Match constructor computed, in its order
struct Call {
  double rotation;
  Rect rect;
  double score;
  int level;
  int request = 0;  // run_many: the request the call belongs to
};

// Scores n candidates (rotation[i], rect[4 i ..]) -> score[i], level[i]; returns 0 or an error code passed through.
using ScoreFn = std::function<int(int n, const double *rotation, const double *rect, double *score, int *level)>;
// Expands n parents to `depth` generations: slots_of(depth) slots per parent, breadth first (m3rsm_split.h): per slot the
// rectangle (NaN where the slot has no node), the score and the level (-1 where it has none).
using ExpandFn = std::function<int(int n, const double *rotation, const double *rect, int depth, double *slot_rect,
                                   double *slot_score, int *slot_level)>;

// the same two calls for candidates of several requests (run_many): request[i] says whose scan, pose and map
using ScoreManyFn =
    std::function<int(int n, const int *request, const double *rotation, const double *rect, double *score, int *level)>;
using ExpandManyFn = std::function<int(int n, const int *request, const double *rotation, const double *rect, int depth,
                                       double *slot_rect, double *slot_score, int *slot_level)>;

struct Result {
  double delta[3] = {0, 0, 0};  // centre x, centre y, rotation of the winning point
  double prob = 0;
  int request = 0;              // run_many: the request the winning point belongs to
  long long scorer_calls = 0;   // committed calls: what the reference would have made
  long long scored = 0;         // candidates the two callbacks were asked to score (roots + non-empty slots)
  long long launches = 0;       // callback invocations: the root layer + the super-steps
  long long super_steps = 0;
  long long branching_pops = 0;
  int callback_rc = 0;
};

constexpr int kOk = 0;
constexpr int kErrInvalid = 1;     // bad configuration
constexpr int kErrSuperSteps = 2;  // max_super_steps reached
constexpr int kErrScorer = 3;      // an expand call did not deliver a child the rule says exists
constexpr int kErrNoMatch = 4;     // the queue ran empty (every bound under the cut)
constexpr int kErrCallback = 5;    // a callback failed: its code is in Result::callback_rc
constexpr int kPending = -1;       // Search::advance: parents wait for an expand call; run_each: the call ended first

// The root layer of M3RSMEngine::add_scan_matching_request: rotation_drift = 0, step, 2 step, ... (accumulated) while
// 2 drift <= 2 max_th_error under less_or_equal; per drift the rotations of std::set{drift, -drift}; per rotation the
// empty rectangle, then the entire one.
void root_candidates(const Config &cfg, std::vector<double> *rotation, std::vector<Rect> *rect);

// The search as a RESUMABLE object: the loop stops where it needs an expand call and goes on once the caller has made it.
// run_many drives one Search to its end; run_each (m3rsm_each.h) drives several, one expand call per round for all of
// them.  The loop stops at the first child of a popped match that the memo lacks -- usually child 0, but a point may be
// there already as the corner of a neighbouring box -- with the children before it committed, and resumes at that child:
// the queue the ride-alongs are read from is the one a mid-branch super-step has always seen.
//   Search s(cfg, n_requests, &result, &trace);   // cfg, result and trace outlive s; Search::check(cfg, n) said kOk
//   s.commit_roots(n, request, rotation, rect, score, level);       // add_scan_matching_request, request by request
//   while ((rc = s.advance()) == kPending) { <expand s.parent_*() to cfg.depth>; s.absorb(slot_rect, slot_score, slot_level); }
class Search {
 public:
  static int check(const Config &cfg, int n_requests);  // kOk or kErrInvalid
  Search(const Config &cfg, int n_requests, Result *result, std::vector<Call> *trace);
  ~Search();
  Search(const Search &) = delete;
  Search &operator=(const Search &) = delete;
  // the root layer: candidates in the order they are to be committed, with their bounds
  void commit_roots(size_t n, const int *request, const double *rotation, const double *rect, const double *score,
                    const int *level);
  // Runs the matcher's loop until it ends (kOk, kErrNoMatch, kErrSuperSteps, kErrScorer: the result is complete) or
  // needs a child the memo lacks: kPending, with the popped match and the next width - 1 unexpanded non-point entries of
  // the queue as parents.
  int advance();
  int n_parents() const;
  const int *parent_request() const;
  const double *parent_rotation() const;
  const double *parent_rect() const;  // 4 per parent
  // the expand call's answer for the parents at hand: slots_of(cfg.depth) slots per parent (counts the super-step)
  void absorb(const double *slot_rect, const double *slot_score, const int *slot_level);

 private:
  struct Impl;
  Impl *impl_;
};

// One match; returns one of the codes above.  `trace` (may be null) receives every committed call.
int run(const Config &cfg, const ScoreFn &score_roots, const ExpandFn &expand, Result *result, std::vector<Call> *trace);

// Several requests in one search, as M3RSMEngine takes them: add_scan_matching_request once per request, in order -- the
// root layers committed request by request, all of them bounded by ONE score_roots call --, then the matcher's loop over
// the one queue under the one best finest probability.  A super-step's parents are whatever the queue holds on top, of
// whichever request; the memo is keyed by (request, rotation, rectangle).  run() is run_many() with one request.
int run_many(const Config &cfg, int n_requests, const ScoreManyFn &score_roots, const ExpandManyFn &expand, Result *result,
             std::vector<Call> *trace);

}  // namespace m3rsm
}  // namespace slamhip
