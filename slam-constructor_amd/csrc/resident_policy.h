// resident_policy.h -- when a host driver asks for the co-resident form of its chains (ONE launch whose workgroups all
// stay on the chip), when it stops asking, and how long the kernels may spin.  Plain host C++ (no HIP): the drivers
// of matchers.cpp hold one per matcher / per filter and tests/native/resident_policy_test.cpp walks it on the CPU.
#pragma once

#include <algorithm>

namespace slamhip {

struct ResidentPolicy {
  // after three give-ups in a row a driver stops asking for the co-resident form; 64 calls later it asks again (the
  // other tenant of the device may be gone)
  static constexpr int kGiveUpsToSwitchOff = 3;
  static constexpr int kRearmAfter = 64;

  int gave_up_row = 0;  // give-ups in a row (a success clears it)
  int since_off = 0;    // calls since the form switched itself off
  double us_max = 0;    // the longest co-resident call seen (decaying): sizes the kernels' spin bound
  long long gave_up = 0, matches = 0;  // in total: give-ups / co-resident launches (slamhip_matcher_resident_stats)

  // Asked ONCE per driver call: every call made while the form is switched off counts towards the re-arm,
  // whether or not the caller's other conditions (mode, OOPE, context option) would have allowed the form.
  bool armed() {
    if (gave_up_row >= kGiveUpsToSwitchOff && ++since_off >= kRearmAfter) {
      gave_up_row = 0;  // (re-armed: the device may be ours again)
      since_off = 0;
    }
    return gave_up_row < kGiveUpsToSwitchOff;
  }
  // polls a sweep may take before a chain gives up: ten times the longest match seen (a poll is ~0.4 us), never less
  // than 2^12 (1.6 ms) nor more than 2^17 (~55 ms: the bound of a driver's first launches)
  unsigned spin_limit() const {
    constexpr unsigned kMax = 1u << 17, kMin = 1u << 12;
    if (!(us_max > 0)) return kMax;
    const double polls = 25.0 * us_max;
    return polls >= (double)kMax ? kMax : (polls <= (double)kMin ? kMin : (unsigned)polls);
  }
  void note_launch() { ++matches; }
  void note_give_up() {
    ++gave_up_row;
    ++gave_up;
  }
  void note_success(double us) {
    gave_up_row = 0;
    us_max = std::max(0.98 * us_max, us);
  }
  // slamhip_matcher_set_device_chain: asks again at once (the calls counted towards a re-arm so far stay counted)
  void reset() { gave_up_row = 0; }
};

}  // namespace slamhip
