// hip_block_test.cpp -- csrc/hip_block.h alone, with a host compiler, against tests/native/hip_stub (the runtime's five
// calls on top of malloc, with a switch that makes the k-th allocation fail): the error paths of the owners and of the
// two growth rules.  A failed growth leaves empty blocks under capacity zero -- never an old capacity over a null block,
// never a block freed twice, never one leaked --, a retry succeeds, a request that fits allocates nothing and waits for
// nothing, capacities are the floor doubled, and what the last owner held is gone with it.
#include <hip/hip_runtime.h>  // (the stub: -Itests/native/hip_stub)

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

#include "slamhip.h"

#define SLAMHIP_CHECK(expr)                          \
  do {                                               \
    hipError_t _e = (expr);                          \
    if (_e != hipSuccess) return SLAMHIP_ERR_HIP;    \
  } while (0)

#include "hip_block.h"

using namespace slamhip;

#define CHECK(cond)                                                         \
  do {                                                                      \
    if (!(cond)) {                                                          \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);         \
      std::exit(1);                                                         \
    }                                                                       \
  } while (0)

static const hipStream_t kStream = nullptr, kStreamB = nullptr;

// the shape of a growth site in the library: three blocks under one capacity, one of them pinned, with what clears them
struct Group {
  DeviceBuf<double> a;
  PinnedBuf<int> b;
  DeviceBuf<unsigned char> c;
  int cap = 0;
  long bodies = 0;
  int ensure(size_t need, size_t floor) {
    return grow_blocks({kStream, kStreamB}, cap, need, floor, [&](size_t grown) -> int {
      ++bodies;
      SLAMHIP_CHECK(a.alloc(3 * grown));
      SLAMHIP_CHECK(b.alloc(grown, kPinnedCoherent));
      std::memset(b.get(), 0, sizeof(int) * grown);
      SLAMHIP_CHECK(c.alloc(grown + 8));
      return SLAMHIP_OK;
    });
  }
  // what every use site relies on: blocks of the stored capacity, or none of it
  void check_consistent() const {
    if (cap > 0) CHECK(a && b && c);
  }
};

static void test_failed_grow_block_and_retry() {
  DeviceBuf<double> d;
  size_t cap = 0;
  CHECK(grow_block(kStream, d, cap, 10, 16) == SLAMHIP_OK && cap == 16 && d);
  d.get()[15] = 1.0;
  hip_stub::fail_in() = 1;
  CHECK(grow_block(kStream, d, cap, 17, 16) == SLAMHIP_ERR_HIP);
  CHECK(cap == 0 && !d && d.get() == nullptr && hip_stub::live() == 0);
  CHECK(grow_block(kStream, d, cap, 17, 16) == SLAMHIP_OK && cap == 32 && d && hip_stub::live() == 1);
  d.get()[31] = 2.0;
  // `per` elements a unit, and a pinned block with its flags
  PinnedBuf<int> h;
  int hcap = 0;
  CHECK(grow_block(kStream, h, hcap, 5, 4, 3, kPinnedCoherent) == SLAMHIP_OK && hcap == 8);
  CHECK(hip_stub::last_pinned_flags() == kPinnedCoherent && hip_stub::live_pinned().size() == 1);
  h.get()[3 * 8 - 1] = 7;
  hip_stub::fail_in() = 1;
  CHECK(grow_block(kStream, h, hcap, 9, 4, 3, kPinnedCoherent) == SLAMHIP_ERR_HIP && hcap == 0 && !h);
  CHECK(hip_stub::live_pinned().empty());
}

static void test_group_every_failure_point() {
  const long kAllocs = 3;  // of one growth of a Group
  for (int round = 0; round < 2; ++round) {  // from empty blocks, and from blocks that hold something
    for (long k = 1; k <= kAllocs; ++k) {
      {
        Group g;
        if (round == 1) {
          CHECK(g.ensure(100, 64) == SLAMHIP_OK && g.cap == 128 && hip_stub::live() == 3);
          g.check_consistent();
        }
        hip_stub::fail_in() = k;
        CHECK(g.ensure(1000, 64) == SLAMHIP_ERR_HIP);
        CHECK(hip_stub::fail_in() == 0);
        CHECK(g.cap == 0);
        // the blocks in front of the failed one hold the new size, the failed one nothing, those behind it what they held
        const bool held = round == 1;
        CHECK((bool)g.a == (k > 1) && (bool)g.b == (k > 2 || (held && k < 2)) && (bool)g.c == (held && k < 3));
        CHECK(hip_stub::live() == (size_t)(k - 1) + (round == 1 ? (size_t)(kAllocs - k) : 0));
        // capacity zero sends the next call -- however small -- through a whole growth
        CHECK(g.ensure(1, 64) == SLAMHIP_OK && g.cap == 64 && hip_stub::live() == 3);
        g.check_consistent();
        g.a.get()[3 * 64 - 1] = 1.0;
        g.b.get()[63] = 1;
        g.c.get()[64 + 7] = 1;
      }
      CHECK(hip_stub::live() == 0);  // nothing leaked, and (the stub aborts otherwise) nothing freed twice
    }
  }
}

static void test_fitting_request_does_nothing() {
  Group g;
  CHECK(g.ensure(65, 64) == SLAMHIP_OK && g.cap == 128);
  const long allocs = hip_stub::allocations(), waits = hip_stub::stream_waits(), bodies = g.bodies;
  const double *a = g.a.get();
  CHECK(g.ensure(128, 64) == SLAMHIP_OK && g.ensure(1, 64) == SLAMHIP_OK && g.ensure(0, 64) == SLAMHIP_OK);
  CHECK(hip_stub::allocations() == allocs && hip_stub::stream_waits() == waits && g.bodies == bodies);
  CHECK(g.cap == 128 && g.a.get() == a);
  DeviceBuf<int> d;
  size_t cap = 0;
  CHECK(grow_block(kStream, d, cap, 3, 8) == SLAMHIP_OK);
  const long allocs1 = hip_stub::allocations(), waits1 = hip_stub::stream_waits();
  CHECK(grow_block(kStream, d, cap, 8, 8) == SLAMHIP_OK);
  CHECK(hip_stub::allocations() == allocs1 && hip_stub::stream_waits() == waits1 && cap == 8);
  // a growth waits once for every stream it was given
  CHECK(g.ensure(129, 64) == SLAMHIP_OK && hip_stub::stream_waits() == waits1 + 2);
  CHECK(grow_block(kStream, d, cap, 9, 8) == SLAMHIP_OK && hip_stub::stream_waits() == waits1 + 3);
}

static void test_capacities_are_the_floor_doubled() {
  const size_t floors[] = {1, 64, 256, 1024, 2048, 65536};
  for (size_t floor : floors) {
    const std::pair<size_t, size_t> cases[] = {{floor, 1}, {floor + 1, 2}, {4 * floor + 1, 8}};
    for (const auto &c : cases) {
      DeviceBuf<unsigned char> d;
      size_t cap = 0;
      CHECK(grow_block(kStream, d, cap, c.first, floor) == SLAMHIP_OK && cap == c.second * floor);
      Group g;
      CHECK(g.ensure(c.first, floor) == SLAMHIP_OK && (size_t)g.cap == c.second * floor);
    }
    // growing step by step ends where one growth does: a stored capacity is always the floor doubled
    Group g;
    for (size_t need = 1; need < 4 * floor + 1; need = 2 * need + 1) CHECK(g.ensure(need, floor) == SLAMHIP_OK);
    CHECK(g.ensure(4 * floor + 1, floor) == SLAMHIP_OK && (size_t)g.cap == 8 * floor);
  }
}

static void test_moves() {
  DeviceBuf<int> x, y;
  CHECK(x.alloc(4) == hipSuccess && y.alloc(4) == hipSuccess && hip_stub::live() == 2);
  int *const py = y.get();
  x = std::move(y);  // frees x's old block, once
  CHECK(hip_stub::live() == 1 && x.get() == py && !y);
  DeviceBuf<int> z(std::move(x));
  CHECK(hip_stub::live() == 1 && z.get() == py && !x);
  // owners in a vector that reallocates
  struct Slot {
    DeviceBuf<double> d;
    PinnedBuf<double> h;
    int n = 0;
  };
  std::vector<Slot> slots;
  for (int i = 0; i < 9; ++i) {
    slots.emplace_back();
    CHECK(slots.back().d.alloc(2) == hipSuccess && slots.back().h.alloc(2) == hipSuccess);
  }
  CHECK(hip_stub::live() == 1 + 18);
  slots.resize(20);
  CHECK(hip_stub::live() == 1 + 18);
  slots.resize(3);
  CHECK(hip_stub::live() == 1 + 6);
  z.reset();
  z.reset();
  CHECK(hip_stub::live() == 6);
}

int main() {
  test_failed_grow_block_and_retry();
  CHECK(hip_stub::live() == 0);
  test_group_every_failure_point();
  CHECK(hip_stub::live() == 0);
  test_fitting_request_does_nothing();
  CHECK(hip_stub::live() == 0);
  test_capacities_are_the_floor_doubled();
  CHECK(hip_stub::live() == 0);
  test_moves();
  CHECK(hip_stub::live() == 0);  // the last owner is gone
  std::printf("ok hip block\n");
  return 0;
}
