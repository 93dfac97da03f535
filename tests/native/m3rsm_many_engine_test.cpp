// tests/native/m3rsm_many_engine_test.cpp -- the best-first engine of the multi-resolution matcher given SEVERAL requests
// (m3rsm::run_many, slam-constructor_amd/csrc/m3rsm_engine.cpp) on the host, replayed against traces of the compiled
// reference's M3RSMEngine with several scan matching requests (tests/golden/m3rsm_many.npz, handed over by
// tests/test_m3rsm_many_host.py as one flat file of doubles), and with ONE request against the lone matches of
// tests/golden/m3rsm.npz (a second file, in m3rsm_engine_test.cpp's format).
//
// The two scoring callbacks are injected: a candidate the reference scored gets the reference's value and level, looked
// up by (request, rotation, rectangle) bits; a candidate it never scored -- speculative work -- gets a deterministic value
// not above its parent's and the level -77, which must never reach the trace.  Checked for every scene and (width, depth)
// in (1, 1), (8, 2), (128, 3):
//   * the committed calls equal the golden trace row for row, bit for bit, request included; winner, delta and prob too;
//   * all roots of all requests arrive in ONE call, request by request; a super-step's parents come from more than one
//     request somewhere in every scene (at width > 1);
//   * with one request run_many and run give the lone golden's trace; bad request counts are refused.
// Run once plainly and once under -fsanitize=address,undefined (its own main, nothing preloaded).
//   g++ -std=c++17 -O1 -g -ffp-contract=off [-fsanitize=address,undefined] -I<repo>/slam-constructor_amd/csrc
//       m3rsm_many_engine_test.cpp <repo>/slam-constructor_amd/csrc/m3rsm_engine.cpp
//   m3rsm_many_engine_test <many.bin> <lone.bin>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <set>
#include <vector>

#include "m3rsm_engine.h"

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
  uint64_t w[6];
  bool operator<(const Key &o) const { return std::memcmp(w, o.w, sizeof(w)) < 0; }
};
static Key key_of(int request, double rot, const Rect &r) {
  const double v[5] = {rot, r.bot, r.top, r.left, r.right};
  Key k;
  std::memcpy(k.w, v, sizeof(v));
  k.w[5] = (uint64_t)request;
  return k;
}
struct Val {
  double score;
  int level;
};

struct Scene {
  Config cfg;
  int n_requests = 1, winner = 0;
  double delta[3], prob;
  std::vector<Call> trace;
  std::map<Key, Val> golden;
};

// what the injected scorer answers: the reference's value, or for a node it never scored a value not above the parent's
struct Scorer {
  const Scene &sc;
  std::map<Key, Val> made;  // speculative nodes, so that one node always gets one value
  long long speculative = 0;
  Val score(int request, double rot, const Rect &r, double parent_score) {
    const Key k = key_of(request, rot, r);
    auto g = sc.golden.find(k);
    if (g != sc.golden.end()) return g->second;
    auto m = made.find(k);
    if (m != made.end()) return m->second;
    uint64_t h = 1469598103934665603ull;
    for (uint64_t v : k.w) h = (h ^ v) * 1099511628211ull;
    const Val v{parent_score - (double)(h >> 40) / (double)(1 << 24) * 0.25, -77};
    made[k] = v;
    ++speculative;
    return v;
  }
};

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, 8) == 0; }

static bool read_file(const char *path, std::vector<double> *in) {
  FILE *f = std::fopen(path, "rb");
  if (!f) return false;
  std::fseek(f, 0, SEEK_END);
  const long bytes = std::ftell(f);
  std::fseek(f, 0, SEEK_SET);
  in->resize(bytes / sizeof(double));
  const bool ok = std::fread(in->data(), sizeof(double), in->size(), f) == in->size();
  std::fclose(f);
  return ok;
}

// many = true: limits, n_requests, winner, delta, prob, n, rows of 8 (request first); else m3rsm_engine_test.cpp's format
static std::vector<Scene> read_scenes(const std::vector<double> &in, bool many) {
  size_t at = 0;
  const int n_scenes = (int)in[at++];
  std::vector<Scene> scenes(n_scenes);
  for (Scene &s : scenes) {
    s.cfg.max_x_error = in[at++];
    s.cfg.max_y_error = in[at++];
    s.cfg.max_th_error = in[at++];
    s.cfg.angle_step = in[at++];
    s.cfg.translation_step = in[at++];
    if (many) {
      s.n_requests = (int)in[at++];
      s.winner = (int)in[at++];
    }
    for (double &d : s.delta) d = in[at++];
    s.prob = in[at++];
    const int n = (int)in[at++];
    for (int i = 0; i < n; ++i) {
      const int request = many ? (int)in[at++] : 0;
      const Call c{in[at], Rect{in[at + 1], in[at + 2], in[at + 3], in[at + 4]}, in[at + 5], (int)in[at + 6], request};
      at += 7;
      s.trace.push_back(c);
      CHECK(request >= 0 && request < s.n_requests);
      const Key k = key_of(request, c.rotation, c.rect);
      auto it = s.golden.find(k);
      if (it != s.golden.end()) CHECK(same_bits(it->second.score, c.score) && it->second.level == c.level);  // a pure function
      s.golden[k] = Val{c.score, c.level};
    }
  }
  CHECK(at == in.size());
  return scenes;
}

struct Replay {
  Result res;
  std::vector<Call> trace;
  int rc = 0;
  int root_calls = 0;
  long long mixed_steps = 0, speculative = 0;
};

static Replay replay(const Scene &sc, int width, int depth, bool through_run) {
  Replay out;
  Scorer scorer{sc};
  Config cfg = sc.cfg;
  cfg.width = width;
  cfg.depth = depth;
  const ScoreManyFn roots = [&](int n, const int *req, const double *rot, const double *rect, double *score, int *level) {
    ++out.root_calls;
    std::vector<double> lone_rot;
    std::vector<Rect> lone_rect;
    root_candidates(cfg, &lone_rot, &lone_rect);
    const int per = (int)lone_rot.size();
    CHECK(n == per * sc.n_requests);
    for (int i = 0; i < n; ++i) {
      CHECK(req[i] == i / per && same_bits(rot[i], lone_rot[i % per]));  // request by request, each the lone list
      const Val v = scorer.score(req[i], rot[i], Rect{rect[4 * i], rect[4 * i + 1], rect[4 * i + 2], rect[4 * i + 3]}, 1.0);
      score[i] = v.score;
      level[i] = v.level;
    }
    return 0;
  };
  const ExpandManyFn expand = [&](int n, const int *req, const double *rot, const double *rect, int d, double *slot_rect,
                                  double *slot_score, int *slot_level) {
    CHECK(n >= 1 && n <= width && d == depth);
    const int slots = slots_of(d);
    std::set<int> who;
    for (int i = 0; i < n; ++i) {
      CHECK(req[i] >= 0 && req[i] < sc.n_requests);
      who.insert(req[i]);
      const Rect parent{rect[4 * i], rect[4 * i + 1], rect[4 * i + 2], rect[4 * i + 3]};
      const double parent_score = scorer.score(req[i], rot[i], parent, 1.0).score;
      std::vector<double> got(slots, 0.0);
      for (int s = 0; s < slots; ++s) {
        const size_t g = (size_t)i * slots + s;
        Rect node;
        if (!slot_node(parent, cfg.translation_step, s, &node)) {
          slot_rect[4 * g] = slot_rect[4 * g + 1] = slot_rect[4 * g + 2] = slot_rect[4 * g + 3] = std::nan("");
          slot_score[g] = std::nan("");
          slot_level[g] = -1;
          continue;
        }
        // (breadth first: the slot of this node's parent comes before it)
        const double above = s < 5 ? parent_score : got[s < 30 ? (s - 5) / 5 : 5 + (s - 30) / 5];
        const Val v = scorer.score(req[i], rot[i], node, above);
        got[s] = v.score;
        slot_rect[4 * g] = node.bot;
        slot_rect[4 * g + 1] = node.top;
        slot_rect[4 * g + 2] = node.left;
        slot_rect[4 * g + 3] = node.right;
        slot_score[g] = v.score;
        slot_level[g] = v.level;
      }
    }
    out.mixed_steps += who.size() > 1;
    return 0;
  };
  if (through_run) {  // m3rsm::run: the one-request form, its callbacks without a request
    const ScoreFn roots1 = [&](int n, const double *rot, const double *rect, double *score, int *level) {
      const std::vector<int> zero(n, 0);
      return roots(n, zero.data(), rot, rect, score, level);
    };
    const ExpandFn expand1 = [&](int n, const double *rot, const double *rect, int d, double *slot_rect, double *slot_score,
                                 int *slot_level) {
      const std::vector<int> zero(n, 0);
      return expand(n, zero.data(), rot, rect, d, slot_rect, slot_score, slot_level);
    };
    out.rc = run(cfg, roots1, expand1, &out.res, &out.trace);
  } else {
    out.rc = run_many(cfg, sc.n_requests, roots, expand, &out.res, &out.trace);
  }
  out.speculative = scorer.speculative;
  return out;
}

static void check_against(const Scene &sc, const Replay &r, int width, int depth) {
  CHECK(r.rc == kOk && r.root_calls == 1);
  CHECK(r.trace.size() == sc.trace.size() && r.res.scorer_calls == (long long)sc.trace.size());
  bool same = r.trace.size() == sc.trace.size();
  for (size_t i = 0; same && i < r.trace.size(); ++i) {
    const Call &a = r.trace[i], &b = sc.trace[i];
    same = a.request == b.request && same_bits(a.rotation, b.rotation) && same_bits(a.rect.bot, b.rect.bot) &&
           same_bits(a.rect.top, b.rect.top) && same_bits(a.rect.left, b.rect.left) && same_bits(a.rect.right, b.rect.right) &&
           same_bits(a.score, b.score) && a.level == b.level;
    if (!same) std::printf("first differing call: %zu (width %d, depth %d)\n", i, width, depth);
  }
  CHECK(same);
  CHECK(r.res.request == sc.winner);
  CHECK(same_bits(r.res.delta[0], sc.delta[0]) && same_bits(r.res.delta[1], sc.delta[1]) && same_bits(r.res.delta[2], sc.delta[2]));
  CHECK(same_bits(r.res.prob, sc.prob));
  CHECK(r.res.launches == r.res.super_steps + 1 && r.res.super_steps >= 1);
}

int main(int argc, char **argv) {
  if (argc != 3) return 2;
  std::vector<double> in_many, in_lone;
  if (!read_file(argv[1], &in_many) || !read_file(argv[2], &in_lone)) return 2;
  const std::vector<Scene> many = read_scenes(in_many, true), lone = read_scenes(in_lone, false);
  const int shapes[3][2] = {{1, 1}, {8, 2}, {128, 3}};
  long long runs = 0, total_spec = 0;
  for (const Scene &sc : many) {
    CHECK(sc.n_requests >= 2);
    long long steps_w1 = -1, steps_w128 = -1;
    for (const auto &wd : shapes) {
      const Replay r = replay(sc, wd[0], wd[1], false);
      check_against(sc, r, wd[0], wd[1]);
      if (wd[0] == 1) {
        steps_w1 = r.res.super_steps;
        CHECK(r.mixed_steps == 0);
      } else {
        CHECK(r.mixed_steps > 0);  // the shared queue's top holds more than one request's matches
      }
      if (wd[0] == 128) steps_w128 = r.res.super_steps;
      total_spec += r.speculative;
      ++runs;
    }
    CHECK(steps_w128 < steps_w1);
  }
  // one request: run_many and run (a call of it) give the lone reference's match
  for (const Scene &sc : lone)
    for (const auto &wd : shapes)
      for (bool through_run : {false, true}) {
        const Replay r = replay(sc, wd[0], wd[1], through_run);
        check_against(sc, r, wd[0], wd[1]);
        for (const Call &c : r.trace) CHECK(c.request == 0);
        ++runs;
      }
  {
    Result res;
    const ScoreManyFn none = [](int, const int *, const double *, const double *, double *, int *) { return 0; };
    const ExpandManyFn none_x = [](int, const int *, const double *, const double *, int, double *, double *, int *) { return 0; };
    CHECK(run_many(Config{}, 0, none, none_x, &res, nullptr) == kErrInvalid);
    CHECK(run_many(Config{}, -3, none, none_x, &res, nullptr) == kErrInvalid);
    Config bad;
    bad.depth = 4;
    CHECK(run_many(bad, 2, none, none_x, &res, nullptr) == kErrInvalid);
    // a callback's failure is handed through
    const ScoreManyFn failing = [](int, const int *, const double *, const double *, double *, int *) { return -4; };
    CHECK(run_many(Config{}, 2, failing, none_x, &res, nullptr) == kErrCallback && res.callback_rc == -4);
  }
  if (fails) return 1;
  std::printf("ok %zu + %zu scenes, %lld runs, %lld speculative candidates kept out of the traces\n", many.size(), lone.size(), runs,
              total_spec);
  return 0;
}
