// resident_policy_test.cpp -- csrc/resident_policy.h walked through the sequences its three users produce (the lone
// hill-climbing / Monte-Carlo drivers and the K-matches driver share a matcher's policy, the filter's
// one-chain-per-particle driver has its own), against the rule as the drivers spelled it out before the type existed:
//
//     if (gave_up_row >= 3 && ++since_off >= 64) { gave_up_row = 0; since_off = 0; }     // once per driver call
//     asked = <the driver's own conditions> && gave_up_row < 3;
//     a launch that gave up: ++gave_up_row (and the total); one that came through: gave_up_row = 0,
//     us_max = max(0.98 * us_max, us);  slamhip_matcher_set_device_chain: gave_up_row = 0 (since_off stays)
//
// The copies agreed on all of it.  What differs between the drivers stays at their call sites and is modelled here as
// the parameter `counts_error5`: the lone drivers count a give-up for error 4 alone (a chain longer than a tag counts,
// error 5, fails over without counting), the many-chains driver counts every launch that left without a result.
// Every driver call made while the form is off counts towards the 64, whatever the driver's other conditions say.
#include <cstdio>
#include <cstdlib>
#include <random>

#include "resident_policy.h"

using slamhip::ResidentPolicy;

#define CHECK(cond)                                                  \
  do {                                                               \
    if (!(cond)) {                                                   \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);    \
      return 1;                                                      \
    }                                                                \
  } while (0)

namespace {

struct SpelledOut {  // the rule as the drivers had it, field by field
  int gave_up_row = 0, since_off = 0;
  double us_max = 0;
  long long gave_up = 0;
  bool call() {
    if (gave_up_row >= 3 && ++since_off >= 64) {
      gave_up_row = 0;
      since_off = 0;
    }
    return gave_up_row < 3;
  }
  unsigned spin_limit() const {
    constexpr unsigned kMax = 1u << 17, kMin = 1u << 12;
    if (!(us_max > 0)) return kMax;
    const double polls = 25.0 * us_max;
    return polls >= (double)kMax ? kMax : (polls <= (double)kMin ? kMin : (unsigned)polls);
  }
};

// one driver call: the launch's outcome is 0 = came through, 4 / 5 = left without a result
int drive(ResidentPolicy &p, SpelledOut &s, bool other_conditions, int outcome, double us, bool counts_error5) {
  const bool armed = p.armed(), armed_ref = s.call();
  CHECK(armed == armed_ref);
  CHECK(p.spin_limit() == s.spin_limit());
  if (!(armed && other_conditions)) return 0;
  p.note_launch();
  if (outcome == 4 || (outcome == 5 && counts_error5)) {
    p.note_give_up();
    ++s.gave_up_row;
    ++s.gave_up;
  } else if (outcome == 0) {
    p.note_success(us);
    s.gave_up_row = 0;
    s.us_max = std::max(0.98 * s.us_max, us);
  }
  CHECK(p.gave_up_row == s.gave_up_row && p.since_off == s.since_off && p.gave_up == s.gave_up && p.us_max == s.us_max);
  return 0;
}

}  // namespace

int main() {
  {  // three give-ups in a row switch the form off; the 64th call after that is asked again
    ResidentPolicy p;
    for (int i = 0; i < 3; ++i) {
      CHECK(p.armed());
      p.note_launch();
      p.note_give_up();
    }
    CHECK(p.gave_up == 3 && p.matches == 3);
    for (int i = 1; i <= 63; ++i) CHECK(!p.armed());
    CHECK(p.armed());  // (call 64)
    CHECK(p.gave_up_row == 0 && p.since_off == 0);
    // one more give-up is one in a row again, not the fourth
    p.note_give_up();
    CHECK(p.armed());
  }
  {  // a success between give-ups clears the row
    ResidentPolicy p;
    p.note_give_up();
    p.note_give_up();
    p.note_success(100.0);
    p.note_give_up();
    p.note_give_up();
    CHECK(p.armed() && p.gave_up == 4);
    p.note_give_up();
    CHECK(!p.armed());
  }
  {  // reset (slamhip_matcher_set_device_chain) asks again at once; the calls counted so far stay counted
    ResidentPolicy p;
    for (int i = 0; i < 3; ++i) p.note_give_up();
    for (int i = 0; i < 10; ++i) CHECK(!p.armed());
    p.reset();
    CHECK(p.armed() && p.since_off == 10);
    for (int i = 0; i < 3; ++i) p.note_give_up();
    for (int i = 1; i <= 53; ++i) CHECK(!p.armed());
    CHECK(p.armed());  // (10 + 54 = 64)
  }
  {  // the spin bound: 25 polls per microsecond of the longest call seen, within [2^12, 2^17]; the maximum decays
    ResidentPolicy p;
    CHECK(p.spin_limit() == (1u << 17));
    p.note_success(100.0);
    CHECK(p.spin_limit() == (1u << 12));
    p.note_success(1000.0);
    CHECK(p.spin_limit() == 25000u);
    p.note_success(10.0);
    CHECK(p.us_max == 0.98 * 1000.0 && p.spin_limit() == (unsigned)(25.0 * 980.0));
    p.note_success(1e5);
    CHECK(p.spin_limit() == (1u << 17));
  }
  // the three users' call patterns, at random, against the rule spelled out
  std::mt19937 rng(7);
  long long calls = 0;
  for (int user = 0; user < 3; ++user) {  // 0 lone HC / MC, 1 K matches per call (shares 0's kind of policy), 2 the filter
    for (int run = 0; run < 200; ++run) {
      ResidentPolicy p;
      SpelledOut s;
      const int p_fail = 1 + (int)(rng() % 90);  // per cent of launches that give up
      for (int i = 0; i < 600; ++i, ++calls) {
        const bool other = rng() % 8 != 0;  // (mode, OOPE, the context's option, a grid that fits)
        const int outcome = (int)(rng() % 100) < p_fail ? (rng() % 4 == 0 ? 5 : 4) : 0;
        if (drive(p, s, other, outcome, 20.0 + (double)(rng() % 5000), user != 0)) return 1;
        if (user != 2 && rng() % 97 == 0) {
          p.reset();
          s.gave_up_row = 0;
        }
      }
    }
  }
  std::printf("ok %lld driver calls\n", calls);
  return 0;
}
