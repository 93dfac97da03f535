// CPU check of the batched Monte-Carlo chains (csrc/mc_chain.h as the batch form of csrc/mc_chain.hip drives it): K
// chains, each on its OWN engine stream, advance in lock-step -- one "kernel" = one super-step of every chain that has
// not ended, at most S candidates per chain, a chain that has ended leaves at once and counts itself once.  The K windows
// of the K pair tapes lie in ONE arena, as the host driver stages them.  Executed over synthetic score functions; every
// chain's trace (candidate poses, scores, accepted flags), final pose, pairs consumed and enumerator state must equal a
// plain PoseEnumerationScanMatcher::process_scan loop (pose_enumeration_scan_matcher.h:31-77) over a
// GaussianPoseEnumerator of the same seed, bit for bit, over three consecutive matches, whatever S is.
// Run by tests/test_mc_batch_host.py at -O2 and under ASan / UBSan.
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "matchers.h"
#include "mc_chain.h"

using namespace slamhip;

namespace {

struct Entry {
  double x, y, theta, score;
  long long accepted;
};

struct ScoreFn {
  double tx, ty, tt, quantum;
  double operator()(double x, double y, double th) const {
    const double d2 = (x - tx) * (x - tx) + (y - ty) * (y - ty) + 0.5 * (th - tt) * (th - tt);
    double v = 1.0 / (1.0 + d2) + 0.02 * std::sin(40 * x) * std::cos(31 * y) + 0.01 * std::sin(25 * th);
    if (quantum > 0) v = std::floor(v / quantum) * quantum;
    return v;
  }
};

std::vector<Entry> reference_loop(GaussianPoseEnumerator &pe, const Pose &init, const ScoreFn &f, Pose *best_out) {
  std::vector<Entry> tr;
  Pose best = init;
  double best_prob = f(init.x, init.y, init.theta);
  pe.reset();
  tr.push_back(Entry{init.x, init.y, init.theta, best_prob, 1});
  while (pe.has_next()) {
    const Pose c = pe.next(best);
    const double p = f(c.x, c.y, c.theta);
    const bool ok = best_prob < p;
    pe.feedback(ok);
    tr.push_back(Entry{c.x, c.y, c.theta, p, ok ? 1 : 0});
    if (ok) {
      best = c;
      best_prob = p;
    }
  }
  *best_out = best;
  return tr;
}

size_t tape_need(const GaussianPoseEnumerator &pe) {
  return 3 * (pe.max_poses() / 2 + 2 + pe.max_poses() / (pe.max_failed() / 3 + 1) + 2) + 8;
}

struct Chain {
  McState s{};
  const McPair *tape = nullptr;
  std::vector<Entry> trace;
  bool ended = false;
};

// one call of the batch driver: K chains in lock-step; returns the kernels it took
int batch(std::vector<std::unique_ptr<GaussianPoseEnumerator>> &pe, const std::vector<Pose> &init,
          const std::vector<ScoreFn> &f, int n_slots, std::vector<Chain> &ch) {
  const int K = (int)pe.size();
  const size_t need = tape_need(*pe[0]);
  std::vector<double> arena(2 * need * K);  // exactly the windows: a read past one is a read of the next (or of the end)
  for (int c = 0; c < K; ++c) {
    pe[c]->reset();
    pe[c]->copy_tape_abs(pe[c]->tape_pos(), need, arena.data() + 2 * need * c);
  }
  ch.assign(K, Chain{});
  for (int c = 0; c < K; ++c) {
    Chain &q = ch[c];
    q.tape = reinterpret_cast<const McPair *>(arena.data()) + need * c;
    q.s.x = init[c].x;
    q.s.y = init[c].y;
    q.s.theta = init[c].theta;
    q.s.td = pe[c]->base_td();
    q.s.rd = pe[c]->base_rd();
    q.s.first = 1;
  }
  const unsigned max_failed = pe[0]->max_failed(), max_poses = pe[0]->max_poses();
  unsigned n_done = 0;
  int kernels = 0;
  while (n_done < (unsigned)K) {
    ++kernels;
    for (int c = 0; c < K; ++c) {  // grid row c
      Chain &q = ch[c];
      if (q.ended) continue;  // (done_epoch == epoch: leaves at once)
      McState &s = q.s;
      const int avail = (int)mc_available(s, max_failed, max_poses);
      const int n = avail < n_slots ? avail : n_slots;
      if (s.first) {
        s.best_prob = f[c](s.x, s.y, s.theta);
        s.calls = 1;
        q.trace.push_back(Entry{s.x, s.y, s.theta, s.best_prob, 1});
      }
      std::vector<Entry> cand(n);
      for (int j = 0; j < n; ++j) {  // "workgroup j of row c"
        mc_candidate(s, q.tape, j, &cand[j].x, &cand[j].y, &cand[j].theta);
        cand[j].score = f[c](cand[j].x, cand[j].y, cand[j].theta);
        cand[j].accepted = 0;
      }
      int j_acc = -1;
      for (int j = 0; j < n && j_acc < 0; ++j)
        if (s.best_prob < cand[j].score) j_acc = j;
      const int used = j_acc >= 0 ? j_acc + 1 : n;
      if (j_acc >= 0) cand[j_acc].accepted = 1;
      for (int j = 0; j < used; ++j) q.trace.push_back(cand[j]);
      const Entry a = j_acc >= 0 ? cand[j_acc] : Entry{0, 0, 0, 0, 0};
      mc_advance(s, q.tape, n, j_acc, a.x, a.y, a.theta, a.score, 0u, max_failed, max_poses);
      s.first = 0;
      if ((size_t)s.pos + 3 > need) {
        std::printf("chain %d ran past its window: %lld of %zu\n", c, s.pos, need);
        std::exit(1);
      }
      if (s.done) {
        q.ended = true;
        ++n_done;  // (once per chain)
      }
    }
    if (kernels > (1 << 16)) {
      std::printf("the chains did not end\n");
      std::exit(1);
    }
  }
  for (int c = 0; c < K; ++c) {
    const McState &s = ch[c].s;
    pe[c]->set_chain_result((size_t)s.pos, s.failed, s.poses, s.td, s.rd, s.has_saved != 0, s.saved);
    pe[c]->trim();
  }
  return kernels;
}

}  // namespace

int main() {
  int matches = 0;
  const unsigned limits[][2] = {{20, 100}, {1, 5}, {3, 100}, {600, 1200}, {7, 7}, {100, 33}};
  for (const auto &lim : limits)
    for (int K : {1, 2, 5, 20})
      for (int n_slots : {1, 2, 7, 20, 511})
        for (double quantum : {0.0, 0.01}) {
          std::vector<std::unique_ptr<GaussianPoseEnumerator>> ref, dev;
          std::vector<Pose> init(K);
          for (int c = 0; c < K; ++c) {
            const unsigned seed = 99u + 7919u * (unsigned)c + lim[0];
            ref.push_back(std::make_unique<GaussianPoseEnumerator>(seed, 0.2, 0.1, lim[0], lim[1]));
            dev.push_back(std::make_unique<GaussianPoseEnumerator>(seed, 0.2, 0.1, lim[0], lim[1]));
            init[c] = Pose{0.3 + 0.05 * c, -0.2 + 0.01 * c, 0.1};
          }
          for (int rep = 0; rep < 3; ++rep) {  // consecutive calls: no stream is ever reseeded
            std::vector<ScoreFn> f(K);
            // (chain 0 of every call starts on its target: zero error; the last one far off)
            for (int c = 0; c < K; ++c) f[c] = ScoreFn{init[c].x + 0.04 * c * (rep + 1), init[c].y, init[c].theta + 0.01 * c, quantum};
            std::vector<Chain> ch;
            const int kernels = batch(dev, init, f, n_slots, ch);
            long long steps = 0;
            for (int c = 0; c < K; ++c) {
              Pose br;
              const size_t pos0 = ref[c]->tape_pos();
              const std::vector<Entry> tr = reference_loop(*ref[c], init[c], f[c], &br);
              const std::vector<Entry> &td = ch[c].trace;
              const Pose bd{ch[c].s.x, ch[c].s.y, ch[c].s.theta};
              std::string ka, kb;
              ref[c]->key(ka);
              dev[c]->key(kb);
              if (tr.size() != td.size() || std::memcmp(tr.data(), td.data(), tr.size() * sizeof(Entry)) != 0 ||
                  std::memcmp(&br, &bd, sizeof(Pose)) != 0 || ref[c]->tape_pos() != dev[c]->tape_pos() ||
                  ref[c]->tape_pos() - pos0 != (size_t)ch[c].s.pos || ka != kb) {
                std::printf("MISMATCH limits %u/%u K %d slots %d quantum %g call %d chain %d: %zu vs %zu calls, tape %zu vs %zu\n",
                            lim[0], lim[1], K, n_slots, quantum, rep, c, tr.size(), td.size(), ref[c]->tape_pos(),
                            dev[c]->tape_pos());
                return 1;
              }
              steps += ch[c].s.steps;
              ++matches;
            }
            (void)steps;
            if (kernels < 1) return 1;
            for (int c = 0; c < K; ++c) init[c] = Pose{init[c].x + 0.01, init[c].y - 0.02, init[c].theta + 0.005};
          }
        }
  std::printf("ok %d matches\n", matches);
  return 0;
}
