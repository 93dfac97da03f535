// bf_batch_plan.h -- the bookkeeping of K brute-force enumerator streams on one matcher (slamhip_matcher_set_bf_streams):
// which stream a job of a batch call uses, which base pose its sweep enumerates around, and which streams latch theirs
// if the call goes through.  Plain C++ without HIP: tests/native/bf_batch_plan_test.cpp compiles it with a host compiler.
//
//   BruteForcePoseEnumerator   src/core/scan_matchers/brute_force_scan_matcher.h:10-81
// An enumerator latches the pose it is given at the FIRST next() of its life as its base and never clears it (:27-40):
// reset() rewinds the offsets' cursor only.  Stream k is what a matcher of its own would hold for robot k: the shared
// offsets (the matcher's range9) and a base of its own, unlatched until the stream's first match that scores anything.
// The cursor is not kept here: every match starts from a rewound enumerator (pose_enumeration_scan_matcher.h:47).
#pragma once

#include <vector>

namespace slamhip {

struct BfStream {
  bool base_set = false;
  double base[3] = {0, 0, 0};
  long long matches = 0;  // matches that ran on the stream (a raw job whose filter kept nothing is none)
};

// what a batch call will do to the streams, worked out on copies: nothing here changes a stream
struct BfBatchPlan {
  std::vector<int> stream;   // per job
  std::vector<double> base;  // per job three doubles: the base its sweep enumerates around (unused for an empty job)
  std::vector<int> latches;  // the jobs whose stream latches its base (= the job's initial pose) when the plan is committed
};

struct BfStreams {
  std::vector<BfStream> s;
  std::vector<int> job_streams;  // stream of job j of the next batch calls (empty: job j uses stream j)

  bool any() const { return !s.empty(); }
  // n fresh streams (0: none): every base forgotten, the job mapping dropped
  void set(int n) {
    s.assign(n > 0 ? (size_t)n : 0, BfStream{});
    job_streams.clear();
  }
  // slamhip_matcher_reset_state: the cursors are rewound (none is kept: see above); latched bases stay, as the
  // reference's reset() leaves them
  void reset() {}

  // a mapping's fault, or null: a stream out of range, two jobs on one stream, more jobs than streams
  const char *mapping_fault(int n, const int *stream_of_job) const {
    const int ns = (int)s.size();
    if (n > ns) return "more jobs than enumerator streams (slamhip_matcher_set_bf_streams)";
    std::vector<char> used((size_t)ns, 0);
    for (int c = 0; c < n; ++c) {
      const int k = stream_of_job ? stream_of_job[c] : c;
      if (k < 0 || k >= ns) return "a job's enumerator stream is out of range";
      if (used[(size_t)k]) return "two jobs of one batch on the same enumerator stream";
      used[(size_t)k] = 1;
    }
    return nullptr;
  }
  // slamhip_matcher_set_bf_job_streams: null or 0 = identity.  A refused mapping leaves the one in force.
  const char *set_job_streams(int n, const int *stream_of_job) {
    if (!stream_of_job || n <= 0) {
      job_streams.clear();
      return nullptr;
    }
    if (const char *why = mapping_fault(n, stream_of_job)) return why;
    job_streams.assign(stream_of_job, stream_of_job + n);
    return nullptr;
  }
  // the streams of the n_jobs jobs of a batch call, checked again (the streams may have been set anew since the
  // mapping was given): null and *out filled, or the fault and nothing touched
  const char *streams_of(int n_jobs, std::vector<int> *out) const {
    if (!job_streams.empty() && n_jobs > (int)job_streams.size())
      return "more jobs than slamhip_matcher_set_bf_job_streams named streams for";
    if (const char *why = mapping_fault(n_jobs, job_streams.empty() ? nullptr : job_streams.data())) return why;
    out->resize((size_t)n_jobs);
    for (int c = 0; c < n_jobs; ++c) (*out)[(size_t)c] = job_streams.empty() ? c : job_streams[(size_t)c];
    return nullptr;
  }

  // The plan of a call whose job c runs on stream_of[c] (streams_of's answer: no stream twice) from init3[3 c ..]:
  // live[c] == 0 (live may be null: all live) marks a raw job whose filter kept nothing -- it scores nothing, so it
  // neither uses nor latches a base.
  BfBatchPlan plan(int n_jobs, const int *stream_of, const double *init3, const unsigned char *live) const {
    BfBatchPlan p;
    p.stream.assign(stream_of, stream_of + n_jobs);
    p.base.assign(3 * (size_t)n_jobs, 0.0);
    for (int c = 0; c < n_jobs; ++c) {
      if (live && !live[c]) continue;
      const BfStream &k = s[(size_t)stream_of[c]];
      const double *from = k.base_set ? k.base : init3 + 3 * (size_t)c;
      for (int q = 0; q < 3; ++q) p.base[3 * (size_t)c + q] = from[q];
      if (!k.base_set) p.latches.push_back(c);
    }
    return p;
  }
  // ... and the call going through: the bases latch (validation lies behind)
  void commit(const BfBatchPlan &p) {
    for (int c : p.latches) {
      BfStream &k = s[(size_t)p.stream[(size_t)c]];
      k.base_set = true;
      for (int q = 0; q < 3; ++q) k.base[q] = p.base[3 * (size_t)c + q];
    }
  }
};

}  // namespace slamhip
