// Native test of csrc/bf_batch_plan.h (the bookkeeping of K brute-force enumerator streams): plain C++, run as an
// ordinary executable by tests/test_bf_batch_plan_host.py, plainly and under -fsanitize=address,undefined.
#include <cstdio>
#include <cstring>
#include <vector>

#include "bf_batch_plan.h"

using slamhip::BfBatchPlan;
using slamhip::BfStream;
using slamhip::BfStreams;

static int g_failed = 0;
#define CHECK(cond)                                                  \
  do {                                                               \
    if (!(cond)) {                                                   \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);  \
      ++g_failed;                                                    \
    }                                                                \
  } while (0)

static bool same(const BfStreams &a, const BfStreams &b) {
  if (a.s.size() != b.s.size() || a.job_streams != b.job_streams) return false;
  for (size_t k = 0; k < a.s.size(); ++k) {
    if (a.s[k].base_set != b.s[k].base_set || a.s[k].matches != b.s[k].matches) return false;
    if (std::memcmp(a.s[k].base, b.s[k].base, sizeof(a.s[k].base)) != 0) return false;
  }
  return true;
}
static bool base_is(const BfStreams &st, int k, const double *p) {
  return st.s[(size_t)k].base_set && std::memcmp(st.s[(size_t)k].base, p, 3 * sizeof(double)) == 0;
}
static bool plan_base_is(const BfBatchPlan &p, int job, const double *want) {
  return std::memcmp(&p.base[3 * (size_t)job], want, 3 * sizeof(double)) == 0;
}

int main() {
  // ---- latching over several calls, identity mapping
  BfStreams st;
  CHECK(!st.any());
  st.set(3);
  CHECK(st.any() && st.s.size() == 3);
  const double call1[9] = {1.0, 2.0, 0.1, -3.0, 4.0, 0.2, 5.5, -6.5, 0.3};
  const double call2[9] = {1.5, 2.5, 0.4, -3.5, 4.5, 0.5, 6.0, -7.0, 0.6};
  std::vector<int> sid;
  CHECK(st.streams_of(3, &sid) == nullptr);
  CHECK(sid == std::vector<int>({0, 1, 2}));
  {
    const BfStreams before = st;
    const BfBatchPlan p = st.plan(3, sid.data(), call1, nullptr);
    CHECK(same(st, before));  // (a plan is worked out on copies)
    CHECK(p.latches == std::vector<int>({0, 1, 2}));
    for (int c = 0; c < 3; ++c) CHECK(plan_base_is(p, c, call1 + 3 * c));
    st.commit(p);
    for (int c = 0; c < 3; ++c) CHECK(base_is(st, c, call1 + 3 * c));
  }
  {
    const BfBatchPlan p = st.plan(3, sid.data(), call2, nullptr);  // other initial poses: the bases stay call 1's
    CHECK(p.latches.empty());
    for (int c = 0; c < 3; ++c) CHECK(plan_base_is(p, c, call1 + 3 * c));
    st.commit(p);
    for (int c = 0; c < 3; ++c) CHECK(base_is(st, c, call1 + 3 * c));
  }
  // ---- fewer jobs than streams, explicit mappings
  {
    const int map[2] = {2, 0};
    CHECK(st.set_job_streams(2, map) == nullptr);
    CHECK(st.streams_of(2, &sid) == nullptr);
    CHECK(sid == std::vector<int>({2, 0}));
    const BfBatchPlan p = st.plan(2, sid.data(), call2, nullptr);
    CHECK(plan_base_is(p, 0, call1 + 6) && plan_base_is(p, 1, call1));
    CHECK(st.streams_of(1, &sid) == nullptr && sid == std::vector<int>({2}));
    // more jobs than the mapping names
    const BfStreams before = st;
    std::vector<int> keep = sid;
    CHECK(st.streams_of(3, &sid) != nullptr);
    CHECK(sid == keep && same(st, before));
  }
  // ---- every refusal leaves the state as it was
  {
    const BfStreams before = st;
    const int twice[3] = {0, 1, 1}, high[3] = {0, 1, 3}, low[2] = {0, -1}, many[4] = {0, 1, 2, 0};
    CHECK(st.set_job_streams(3, twice) != nullptr);
    CHECK(st.set_job_streams(3, high) != nullptr);
    CHECK(st.set_job_streams(2, low) != nullptr);
    CHECK(st.set_job_streams(4, many) != nullptr);
    CHECK(same(st, before));
    CHECK(st.set_job_streams(0, nullptr) == nullptr && st.job_streams.empty());  // null or 0: identity
    std::vector<int> out;
    CHECK(st.streams_of(4, &out) != nullptr && out.empty());  // more jobs than streams
    CHECK(st.streams_of(3, &out) == nullptr && out.size() == 3);
  }
  // a mapping given before the streams were set anew with fewer of them is refused in the batch call
  {
    BfStreams t;
    t.set(4);
    const int map[2] = {3, 1};
    CHECK(t.set_job_streams(2, map) == nullptr);
    t.s.resize(2);  // (what only a direct edit can do: set() drops the mapping)
    std::vector<int> out;
    CHECK(t.streams_of(2, &out) != nullptr);
    t.set(2);
    CHECK(t.job_streams.empty() && t.streams_of(2, &out) == nullptr);
  }
  // ---- an empty raw job does not latch, and latches in the next call at that call's pose
  {
    BfStreams t;
    t.set(3);
    std::vector<int> id;
    CHECK(t.streams_of(3, &id) == nullptr);
    const unsigned char live[3] = {1, 0, 1};
    BfBatchPlan p = t.plan(3, id.data(), call1, live);
    CHECK(p.latches == std::vector<int>({0, 2}));
    t.commit(p);
    CHECK(base_is(t, 0, call1) && !t.s[1].base_set && base_is(t, 2, call1 + 6));
    p = t.plan(3, id.data(), call2, nullptr);
    CHECK(p.latches == std::vector<int>({1}));
    CHECK(plan_base_is(p, 0, call1) && plan_base_is(p, 1, call2 + 3) && plan_base_is(p, 2, call1 + 6));
    t.commit(p);
    CHECK(base_is(t, 1, call2 + 3));
    // ---- reset keeps the bases
    const BfStreams before = t;
    t.reset();
    CHECK(same(t, before));
    // ---- set anew forgets them and drops the mapping
    const int map[1] = {2};
    CHECK(t.set_job_streams(1, map) == nullptr);
    t.set(3);
    CHECK(t.job_streams.empty());
    for (int k = 0; k < 3; ++k) CHECK(!t.s[(size_t)k].base_set && t.s[(size_t)k].matches == 0);
    t.set(0);
    CHECK(!t.any());
  }
  if (g_failed) return 1;
  std::printf("ok bf batch plan\n");
  return 0;
}
