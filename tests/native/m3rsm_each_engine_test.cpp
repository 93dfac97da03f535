// tests/native/m3rsm_each_engine_test.cpp -- K INDEPENDENT multi-resolution searches in lock-step (m3rsm::run_each,
// slam-constructor_amd/csrc/m3rsm_each.cpp over the resumable Search of m3rsm_engine.cpp) on the host, replayed against
// the lone matches of the compiled reference (tests/golden/m3rsm.npz, handed over by tests/test_m3rsm_each_host.py as one
// flat file of doubles in m3rsm_engine_test.cpp's format).
//
// The scorer is m3rsm_many_engine_test.cpp's: a candidate the reference scored gets the reference's value and level,
// looked up by (job, rotation, rectangle) bits; speculative work gets a deterministic value not above its parent's and
// the level -77, which must never reach a trace.  ONE batch holds all lone scenes, each with its own limits and steps.
// For (width, depth) in (1, 1), (8, 2), (32, 3) and 1, 3 and 8 threads:
//   * every job's trace, delta and prob are the lone golden's bit for bit; its Result counters are those of m3rsm::run on
//     that job alone;
//   * all roots arrive in one call, job by job; a round's parents come in job order, at most `width` per job;
//   * callbacks = 1 + rounds, rounds = the largest lone super-step count; the lone counts are not all equal and the
//     number of jobs in a round goes down: searches that have ended take no further part;
//   * every output is the same for every thread count.
// Further: a job whose bounds all fall under the cut ends alone with kErrNoMatch, a job whose bounds are all NaN ends as
// its lone run does, the others unaffected; max_super_steps = 1 fails the call for the lowest job; bad configurations
// are refused; a callback's failure is handed through; split_by_bytes cuts a round where its staging would outgrow a limit.
// Its own main, nothing preloaded; built plainly, under -fsanitize=address,undefined and under -fsanitize=thread.
//   g++ -std=c++17 -O1 -g -ffp-contract=off -pthread [-fsanitize=...] -I<repo>/slam-constructor_amd/csrc
//       m3rsm_each_engine_test.cpp <repo>/slam-constructor_amd/csrc/m3rsm_engine.cpp <repo>/slam-constructor_amd/csrc/m3rsm_each.cpp
//   m3rsm_each_engine_test <lone.bin>
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <vector>

#include "m3rsm_each.h"

using namespace slamhip::m3rsm;

static int fails = 0;
#define CHECK(c)                                              \
  do {                                                        \
    if (!(c)) {                                               \
      std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
      if (++fails > 20) std::exit(1);                         \
    }                                                         \
  } while (0)

struct Key {
  uint64_t w[5];
  bool operator<(const Key &o) const { return std::memcmp(w, o.w, sizeof(w)) < 0; }
};
static Key key_of(double rot, const Rect &r) {
  const double v[5] = {rot, r.bot, r.top, r.left, r.right};
  Key k;
  std::memcpy(k.w, v, sizeof(v));
  return k;
}
struct Val {
  double score;
  int level;
};

struct Scene {
  Config cfg;
  double delta[3], prob;
  std::vector<Call> trace;
  std::map<Key, Val> golden;
};

enum Mode { kGolden, kAllNan, kAllLow };

// what the injected scorer answers for one job
struct Scorer {
  const Scene *sc;
  Mode mode = kGolden;
  std::map<Key, Val> made;  // speculative nodes, so that one node always gets one value
  long long speculative = 0;
  Val score(double rot, const Rect &r, double parent_score) {
    if (mode == kAllNan) return Val{std::nan(""), 0};
    if (mode == kAllLow) return Val{-1.0, 0};  // (under add_match's cut: best finest probability starts at 0)
    const Key k = key_of(rot, r);
    auto g = sc->golden.find(k);
    if (g != sc->golden.end()) return g->second;
    auto m = made.find(k);
    if (m != made.end()) return m->second;
    uint64_t h = 1469598103934665603ull;
    for (uint64_t v : k.w) h = (h ^ v) * 1099511628211ull;
    const Val v{parent_score - (double)(h >> 40) / (double)(1 << 24) * 0.25, -77};
    made[k] = v;
    ++speculative;
    return v;
  }
  // one parent's slots, breadth first
  void expand(const Config &cfg, double rot, const Rect &parent, int depth, double *slot_rect, double *slot_score, int *slot_level) {
    const int slots = slots_of(depth);
    const double parent_score = score(rot, parent, 1.0).score;
    std::vector<double> got(slots, 0.0);
    for (int s = 0; s < slots; ++s) {
      Rect node;
      if (!slot_node(parent, cfg.translation_step, s, &node)) {
        slot_rect[4 * s] = slot_rect[4 * s + 1] = slot_rect[4 * s + 2] = slot_rect[4 * s + 3] = std::nan("");
        slot_score[s] = std::nan("");
        slot_level[s] = -1;
        continue;
      }
      const double above = s < 5 ? parent_score : got[s < 30 ? (s - 5) / 5 : 5 + (s - 30) / 5];
      const Val v = score(rot, node, above);
      got[s] = v.score;
      slot_rect[4 * s] = node.bot;
      slot_rect[4 * s + 1] = node.top;
      slot_rect[4 * s + 2] = node.left;
      slot_rect[4 * s + 3] = node.right;
      slot_score[s] = v.score;
      slot_level[s] = v.level;
    }
  }
};

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, 8) == 0; }
static bool same_call(const Call &a, const Call &b) {
  return a.request == b.request && same_bits(a.rotation, b.rotation) && same_bits(a.rect.bot, b.rect.bot) &&
         same_bits(a.rect.top, b.rect.top) && same_bits(a.rect.left, b.rect.left) && same_bits(a.rect.right, b.rect.right) &&
         same_bits(a.score, b.score) && a.level == b.level;
}
static bool same_trace(const std::vector<Call> &a, const std::vector<Call> &b) {
  if (a.size() != b.size()) return false;
  for (size_t i = 0; i < a.size(); ++i)
    if (!same_call(a[i], b[i])) return false;
  return true;
}
static bool same_result(const Result &a, const Result &b) {
  return same_bits(a.delta[0], b.delta[0]) && same_bits(a.delta[1], b.delta[1]) && same_bits(a.delta[2], b.delta[2]) &&
         same_bits(a.prob, b.prob) && a.scorer_calls == b.scorer_calls && a.scored == b.scored && a.super_steps == b.super_steps &&
         a.branching_pops == b.branching_pops && a.request == b.request;
}

static std::vector<Scene> read_scenes(const char *path) {
  std::vector<double> in;
  FILE *f = std::fopen(path, "rb");
  if (!f) std::exit(2);
  std::fseek(f, 0, SEEK_END);
  const long bytes = std::ftell(f);
  std::fseek(f, 0, SEEK_SET);
  in.resize(bytes / sizeof(double));
  if (std::fread(in.data(), sizeof(double), in.size(), f) != in.size()) std::exit(2);
  std::fclose(f);
  size_t at = 0;
  const int n_scenes = (int)in[at++];
  std::vector<Scene> scenes(n_scenes);
  for (Scene &s : scenes) {
    s.cfg.max_x_error = in[at++];
    s.cfg.max_y_error = in[at++];
    s.cfg.max_th_error = in[at++];
    s.cfg.angle_step = in[at++];
    s.cfg.translation_step = in[at++];
    for (double &d : s.delta) d = in[at++];
    s.prob = in[at++];
    const int n = (int)in[at++];
    for (int i = 0; i < n; ++i) {
      const Call c{in[at], Rect{in[at + 1], in[at + 2], in[at + 3], in[at + 4]}, in[at + 5], (int)in[at + 6], 0};
      at += 7;
      s.trace.push_back(c);
      s.golden[key_of(c.rotation, c.rect)] = Val{c.score, c.level};
    }
  }
  CHECK(at == in.size());
  return scenes;
}

struct Job {
  const Scene *sc;
  Mode mode;
};

// m3rsm::run on one job alone
struct Lone {
  Result res;
  std::vector<Call> trace;
  int rc;
};
static Lone lone_run(const Job &job, int width, int depth, long long max_super_steps) {
  Lone out;
  Scorer scorer{job.sc, job.mode};
  Config cfg = job.sc->cfg;
  cfg.width = width;
  cfg.depth = depth;
  cfg.max_super_steps = max_super_steps;
  const ScoreFn roots = [&](int n, const double *rot, const double *rect, double *score, int *level) {
    for (int i = 0; i < n; ++i) {
      const Val v = scorer.score(rot[i], Rect{rect[4 * i], rect[4 * i + 1], rect[4 * i + 2], rect[4 * i + 3]}, 1.0);
      score[i] = v.score;
      level[i] = v.level;
    }
    return 0;
  };
  const ExpandFn expand = [&](int n, const double *rot, const double *rect, int d, double *slot_rect, double *slot_score,
                              int *slot_level) {
    const size_t slots = slots_of(d);
    for (int i = 0; i < n; ++i)
      scorer.expand(cfg, rot[i], Rect{rect[4 * i], rect[4 * i + 1], rect[4 * i + 2], rect[4 * i + 3]}, d, slot_rect + 4 * i * slots,
                    slot_score + i * slots, slot_level + i * slots);
    return 0;
  };
  out.rc = run(cfg, roots, expand, &out.res, &out.trace);
  return out;
}

struct Batch {
  int rc = 0;
  std::vector<Result> res;
  std::vector<int> codes;
  std::vector<std::vector<Call>> traces;
  int root_calls = 0, expand_calls = 0;
  std::vector<int> jobs_per_round;
  long long speculative = 0;
};
static Batch batch_run(const std::vector<Job> &jobs, int width, int depth, long long max_super_steps, int threads) {
  const int n_jobs = (int)jobs.size();
  Batch out;
  out.res.resize(n_jobs);
  out.codes.assign(n_jobs, 99);
  out.traces.resize(n_jobs);
  std::vector<Scorer> scorer;
  std::vector<Config> cfgs;
  for (const Job &j : jobs) {
    scorer.push_back(Scorer{j.sc, j.mode});
    Config cfg = j.sc->cfg;
    cfg.width = width;
    cfg.depth = depth;
    cfg.max_super_steps = max_super_steps;
    cfgs.push_back(cfg);
  }
  const ScoreManyFn roots = [&](int n, const int *req, const double *rot, const double *rect, double *score, int *level) {
    ++out.root_calls;
    CHECK(out.expand_calls == 0);
    int at = 0;
    for (int j = 0; j < n_jobs; ++j) {  // job by job, each its own lone list
      std::vector<double> lone_rot;
      std::vector<Rect> lone_rect;
      root_candidates(cfgs[j], &lone_rot, &lone_rect);
      for (size_t i = 0; i < lone_rot.size() && at < n; ++i, ++at) {
        CHECK(req[at] == j && same_bits(rot[at], lone_rot[i]) && same_bits(rect[4 * at + 1], lone_rect[i].top) &&
              same_bits(rect[4 * at + 3], lone_rect[i].right));
        const Val v = scorer[j].score(rot[at], Rect{rect[4 * at], rect[4 * at + 1], rect[4 * at + 2], rect[4 * at + 3]}, 1.0);
        score[at] = v.score;
        level[at] = v.level;
      }
    }
    CHECK(at == n);
    return 0;
  };
  const ExpandManyFn expand = [&](int n, const int *req, const double *rot, const double *rect, int d, double *slot_rect,
                                  double *slot_score, int *slot_level) {
    ++out.expand_calls;
    CHECK(n >= 1 && d == depth);
    const size_t slots = slots_of(d);
    int n_in_round = 0, run_length = 0;
    for (int i = 0; i < n; ++i) {
      CHECK(req[i] >= 0 && req[i] < n_jobs);
      if (i > 0) CHECK(req[i] >= req[i - 1]);  // concatenated in job order
      if (i == 0 || req[i] != req[i - 1]) {
        ++n_in_round;
        run_length = 0;
      }
      CHECK(++run_length <= width);
      scorer[req[i]].expand(cfgs[req[i]], rot[i], Rect{rect[4 * i], rect[4 * i + 1], rect[4 * i + 2], rect[4 * i + 3]}, d,
                            slot_rect + 4 * i * slots, slot_score + i * slots, slot_level + i * slots);
    }
    out.jobs_per_round.push_back(n_in_round);
    return 0;
  };
  out.rc = run_each(cfgs.data(), n_jobs, roots, expand, out.res.data(), out.codes.data(), out.traces.data(), threads);
  for (const Scorer &s : scorer) out.speculative += s.speculative;
  return out;
}

static bool same_batch(const Batch &a, const Batch &b) {
  bool same = a.rc == b.rc && a.codes == b.codes && a.root_calls == b.root_calls && a.expand_calls == b.expand_calls &&
              a.jobs_per_round == b.jobs_per_round && a.res.size() == b.res.size();
  for (size_t j = 0; same && j < a.res.size(); ++j)
    same = same_result(a.res[j], b.res[j]) && a.res[j].launches == b.res[j].launches && same_trace(a.traces[j], b.traces[j]);
  return same;
}

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  const std::vector<Scene> scenes = read_scenes(argv[1]);
  CHECK(scenes.size() >= 2);
  std::vector<Job> all;
  for (const Scene &s : scenes) all.push_back(Job{&s, kGolden});
  const int shapes[3][2] = {{1, 1}, {8, 2}, {32, 3}};
  const int thread_counts[3] = {1, 3, 8};
  const long long no_bound = 1 << 20;
  long long runs = 0, total_spec = 0;
  for (const auto &wd : shapes) {
    std::vector<Lone> lone;
    long long most = 0, least = no_bound;
    for (const Job &j : all) {
      lone.push_back(lone_run(j, wd[0], wd[1], no_bound));
      CHECK(lone.back().rc == kOk && same_trace(lone.back().trace, j.sc->trace));
      most = std::max(most, lone.back().res.super_steps);
      least = std::min(least, lone.back().res.super_steps);
    }
    CHECK(least < most);  // jobs end in different rounds: the drop-out path runs
    Batch first;
    for (int threads : thread_counts) {
      const Batch b = batch_run(all, wd[0], wd[1], no_bound, threads);
      CHECK(b.rc == kOk && b.root_calls == 1);
      for (size_t j = 0; j < all.size(); ++j) {
        const Scene &sc = *all[j].sc;
        CHECK(b.codes[j] == kOk);
        CHECK(same_trace(b.traces[j], sc.trace));
        CHECK(same_bits(b.res[j].delta[0], sc.delta[0]) && same_bits(b.res[j].delta[1], sc.delta[1]) &&
              same_bits(b.res[j].delta[2], sc.delta[2]) && same_bits(b.res[j].prob, sc.prob));
        CHECK(same_result(b.res[j], lone[j].res));
        CHECK(b.res[j].launches == lone[j].res.launches);
      }
      // launches = 1 + rounds; a round per super-step of the longest job
      CHECK(b.expand_calls == (int)b.jobs_per_round.size() && b.expand_calls <= most && b.expand_calls == most);
      CHECK(b.jobs_per_round.front() == (int)all.size() && b.jobs_per_round.back() < (int)all.size());
      CHECK(std::is_sorted(b.jobs_per_round.rbegin(), b.jobs_per_round.rend()));  // nobody comes back
      if (threads == thread_counts[0]) first = b;
      else CHECK(same_batch(first, b));
      total_spec += b.speculative;
      ++runs;
    }
  }
  // a job that finds nothing, and one whose bounds are all NaN, beside good jobs: each ends as it does alone
  for (Mode mode : {kAllLow, kAllNan}) {
    std::vector<Job> jobs{all[0], Job{all[1].sc, mode}, all[2]};
    const Lone alone = lone_run(jobs[1], 8, 2, no_bound);
    if (mode == kAllLow) CHECK(alone.rc == kErrNoMatch);
    std::printf("mode %d: the lone run ends with code %d, prob %g after %lld calls\n", (int)mode, alone.rc, alone.res.prob,
                alone.res.scorer_calls);
    Batch first;
    for (int threads : thread_counts) {
      const Batch b = batch_run(jobs, 8, 2, no_bound, threads);
      CHECK(b.rc == kOk && b.root_calls == 1);
      CHECK(b.codes[1] == alone.rc && same_result(b.res[1], alone.res) && same_trace(b.traces[1], alone.trace));
      for (int j : {0, 2}) {
        CHECK(b.codes[j] == kOk && same_trace(b.traces[j], jobs[j].sc->trace) && same_bits(b.res[j].prob, jobs[j].sc->prob));
        CHECK(same_result(b.res[j], lone_run(jobs[j], 8, 2, no_bound).res));
      }
      if (mode == kAllLow) CHECK(b.jobs_per_round.front() == 2);  // it ended before the first round
      if (threads == thread_counts[0]) first = b;
      else CHECK(same_batch(first, b));
      ++runs;
    }
  }
  {  // the bound on super-steps fails the call, for the lowest job that meets it
    for (int threads : thread_counts) {
      const Batch b = batch_run(all, 1, 1, 1, threads);
      CHECK(b.rc == kErrSuperSteps && b.expand_calls == 1);
      int lowest = -1;
      for (size_t j = 0; j < all.size(); ++j)
        if (lone_run(all[j], 1, 1, 1).rc == kErrSuperSteps && lowest < 0) lowest = (int)j;
      CHECK(lowest >= 0 && b.codes[lowest] == kErrSuperSteps);
      for (int j = 0; j < lowest; ++j) CHECK(b.codes[j] == kOk);
      ++runs;
    }
  }
  {  // bad configurations are refused; a callback's failure is handed through
    const ScoreManyFn none = [](int, const int *, const double *, const double *, double *, int *) { return 0; };
    const ExpandManyFn none_x = [](int, const int *, const double *, const double *, int, double *, double *, int *) { return 0; };
    Result res[2];
    int codes[2];
    Config cfgs[2];
    CHECK(run_each(cfgs, 0, none, none_x, res, codes, nullptr, 1) == kErrInvalid);
    CHECK(run_each(cfgs, -1, none, none_x, res, codes, nullptr, 1) == kErrInvalid);
    CHECK(run_each(nullptr, 2, none, none_x, res, codes, nullptr, 1) == kErrInvalid);
    CHECK(run_each(cfgs, 2, none, none_x, res, codes, nullptr, -1) == kErrInvalid);
    CHECK(run_each(cfgs, 2, none, none_x, res, codes, nullptr, kEachMaxThreads + 1) == kErrInvalid);
    cfgs[1].width = 7;  // width, depth and the bound are common to all jobs
    CHECK(run_each(cfgs, 2, none, none_x, res, codes, nullptr, 1) == kErrInvalid);
    cfgs[1] = Config{};
    cfgs[1].depth = 2;
    CHECK(run_each(cfgs, 2, none, none_x, res, codes, nullptr, 1) == kErrInvalid);
    cfgs[1] = Config{};
    cfgs[1].max_super_steps = 5;
    CHECK(run_each(cfgs, 2, none, none_x, res, codes, nullptr, 1) == kErrInvalid);
    cfgs[1] = Config{};
    cfgs[1].translation_step = 0;
    CHECK(run_each(cfgs, 2, none, none_x, res, codes, nullptr, 1) == kErrInvalid);
    cfgs[1] = Config{};
    cfgs[0].depth = cfgs[1].depth = 4;
    CHECK(run_each(cfgs, 2, none, none_x, res, codes, nullptr, 1) == kErrInvalid);
    cfgs[0] = cfgs[1] = Config{};
    CHECK(each_default_threads(1) == 1 && each_default_threads(5) == 5 && each_default_threads(100) == 8);
    const ScoreManyFn failing = [](int, const int *, const double *, const double *, double *, int *) { return -4; };
    CHECK(run_each(cfgs, 2, failing, none_x, res, codes, nullptr, 2) == kErrCallback && res[0].callback_rc == -4 &&
          res[1].callback_rc == -4 && codes[0] == kPending && codes[1] == kPending);
    const ScoreManyFn ones = [](int n, const int *, const double *, const double *rect, double *score, int *level) {
      for (int i = 0; i < n; ++i) score[i] = rect[4 * i + 1] > rect[4 * i] ? 0.9 : 0.5, level[i] = 0;  // (the box comes first)
      return 0;
    };
    const ExpandManyFn failing_x = [](int, const int *, const double *, const double *, int, double *, double *, int *) { return -9; };
    CHECK(run_each(cfgs, 2, ones, failing_x, res, codes, nullptr, 2) == kErrCallback && res[1].callback_rc == -9);
  }
  {  // a round cut into consecutive calls by the bytes its entries need
    std::vector<int> first;
    const size_t bytes[6] = {4, 4, 4, 9, 1, 8};
    split_by_bytes(bytes, 6, 1 << 20, &first);
    CHECK((first == std::vector<int>{0, 6}));
    split_by_bytes(bytes, 6, 8, &first);
    CHECK((first == std::vector<int>{0, 2, 3, 4, 5, 6}));  // (9 > 8 goes alone; 1 + 8 does not fit)
    split_by_bytes(bytes, 6, 12, &first);
    CHECK((first == std::vector<int>{0, 3, 5, 6}));
    split_by_bytes(bytes, 6, 0, &first);
    CHECK((first == std::vector<int>{0, 1, 2, 3, 4, 5, 6}));
    split_by_bytes(bytes, 1, 2, &first);
    CHECK((first == std::vector<int>{0, 1}));
    split_by_bytes(bytes, 0, 2, &first);
    CHECK((first == std::vector<int>{0}));
    const size_t huge[2] = {~(size_t)0, ~(size_t)0};
    split_by_bytes(huge, 2, ~(size_t)0 - 1, &first);
    CHECK((first == std::vector<int>{0, 1, 2}));
  }
  if (fails) return 1;
  std::printf("ok %zu jobs in a batch, %lld runs, %lld speculative candidates kept out of the traces\n", scenes.size(), runs,
              total_spec);
  return 0;
}
