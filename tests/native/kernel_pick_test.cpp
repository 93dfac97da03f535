// kernel_pick_test.cpp -- csrc/kernel_pick.h, the one place that says which template instantiation of a kernel family
// runs, held against the rules as the launchers spelled them out before the header existed:
//
//   cell model   OCC (0), TBM (1), CREDIBILIST (3) have kernels; GMAPPING (2) and anything else has NONE -- never
//                another model's
//   co-resident hill climbing (hc_resident.hip), grid = 6 x max_inst + 1 workgroups, G = 2 up to 128 of them, 4 up to
//                256, else 7; a workgroup size other than 256 or 1024 means 512
//     window     every size, default sum order, lone chains, at most 256 workgroups; G = 4
//     pair       a batch whose workgroups score two poses: 512 threads only (`pair` means nothing outside a batch)
//     plain      every size x {default order, beam order, batch} -- no batch in beam order --, but not 1024 threads at G = 7
//   GMapping chain LDS   the expression launch_gm (hc_chain.hip) had
#include <cstdio>

#include "gm_score_device.h"
#include "kernel_pick.h"

using namespace slamhip;

#define CHECK(cond)                                                  \
  do {                                                               \
    if (!(cond)) {                                                   \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);    \
      return 1;                                                      \
    }                                                                \
  } while (0)

namespace {

const int kSome = 0;  // (what a dispatcher's lambda returns here: any non-null pointer)

int check_dispatchers() {
  const int with[] = {SLAMHIP_CELL_OCC, SLAMHIP_CELL_TBM, SLAMHIP_CELL_CREDIBILIST};
  CHECK(with[0] == 0 && with[1] == 1 && with[2] == 3);
  for (int model : with) {
    int calls = 0, seen = -100;
    const int *r = pick_cell_model(model, [&](auto m) -> const int * {
      ++calls;
      seen = decltype(m)::value;
      return &kSome;
    });
    CHECK(r == &kSome && calls == 1 && seen == model);
  }
  for (int model : {2, -1, 4}) {
    int calls = 0;
    const int *r = pick_cell_model(model, [&](auto) -> const int * {
      ++calls;
      return &kSome;
    });
    CHECK(r == nullptr && calls == 0);
  }
  CHECK(SLAMHIP_CELL_GMAPPING == 2);
  // the probability plane's two models
  for (int model = -1; model <= 4; ++model) {
    int calls = 0, seen = -100;
    const int *r = pick_belief_model(model, [&](auto m) -> const int * {
      ++calls;
      seen = decltype(m)::value;
      return &kSome;
    });
    if (model == 1 || model == 3) CHECK(r == &kSome && calls == 1 && seen == model);
    else CHECK(r == nullptr && calls == 0);
  }
  // workgroup sizes and flags
  const int nts[] = {0, 64, 128, 256, 384, 512, 1000, 1024, 2048}, hc[] = {512, 512, 512, 256, 512, 512, 512, 1024, 512},
            mc[] = {1024, 1024, 1024, 1024, 1024, 512, 1024, 1024, 1024};
  for (int i = 0; i < 9; ++i) {
    int calls = 0, seen = 0;
    const auto f = [&](auto nt) -> const int * {
      ++calls;
      seen = decltype(nt)::value;
      return &kSome;
    };
    CHECK(pick_hc_nt(nts[i], f) == &kSome && calls == 1 && seen == hc[i] && hc_nt_of(nts[i]) == hc[i]);
    CHECK(pick_mc_nt(nts[i], f) == &kSome && calls == 2 && seen == mc[i] && mc_nt_of(nts[i]) == mc[i]);
  }
  for (int b = 0; b < 2; ++b) {
    int calls = 0, seen = -1;
    CHECK(pick_bool(b != 0, [&](auto v) -> const int * {
            ++calls;
            seen = decltype(v)::value ? 1 : 0;
            return &kSome;
          }) == &kSome);
    CHECK(calls == 1 && seen == b);
  }
  return 0;
}

int check_hc_resident_variants(long *n_accepted) {
  const int nts[] = {64, 256, 512, 1024}, nt_means[] = {512, 256, 512, 1024};
  for (int i = 0; i < 4; ++i)
    for (int max_inst = 1; max_inst <= 64; ++max_inst)
      for (int bits = 0; bits < 16; ++bits) {
        const bool batch = bits & 1, pair = bits & 2, window = bits & 4, seq = bits & 8;
        // the table, literally: max_inst <= 21 is a grid of at most 127 workgroups, <= 42 of at most 253
        const int g_plain = max_inst <= 21 ? 2 : (max_inst <= 42 ? 4 : 7);
        bool want;
        int want_g;
        if (window) {
          want = !seq && !batch && max_inst <= 42;
          want_g = 4;
        } else if (batch && pair) {
          want = !seq && nts[i] == 512;
          want_g = g_plain;
        } else {
          want = !(seq && batch) && !(nt_means[i] == 1024 && g_plain == 7);
          want_g = g_plain;
        }
        int nt = -1, g = -1;
        const bool got = hc_resident_variant(HcResidentKey{nts[i], max_inst, seq, batch, pair, window}, &nt, &g);
        if (got != want || (got && (nt != nt_means[i] || g != want_g))) {
          std::printf("FAIL nt %d max_inst %d batch %d pair %d window %d seq %d: %s <%d, %d>, want %s <%d, %d>\n", nts[i],
                      max_inst, batch, pair, window, seq, got ? "accepted" : "refused", nt, g, want ? "accepted" : "refused",
                      nt_means[i], want_g);
          return 1;
        }
        *n_accepted += got ? 1 : 0;
      }
  CHECK(hc_gran_per_lane(127) == 2 && hc_gran_per_lane(128) == 2 && hc_gran_per_lane(129) == 4 && hc_gran_per_lane(256) == 4 &&
        hc_gran_per_lane(257) == 7 && hc_gran_per_lane(385) == 7);
  return 0;
}

int check_gm_lds() {
  for (int KB = 1; KB <= 5; ++KB)
    for (int nt : {256, 512, 1024}) {
      const size_t shm = (size_t)KB * 256 * sizeof(double) + 4 * KB * sizeof(int2) + 4 * KB * sizeof(int) +
                         2 * (size_t)KB * 256 * sizeof(int) + (nt >= 512 ? (size_t)nt * sizeof(double) : 0);
      CHECK(gm_chain_lds_bytes(KB, nt) == shm);
    }
  CHECK(gm_chain_lds_bytes(5, 1024) == 5 * 2048 + 5 * 32 + 5 * 16 + 5 * 2048 + 8192);
  return 0;
}

}  // namespace

int main() {
  long n_accepted = 0;
  if (check_dispatchers() || check_hc_resident_variants(&n_accepted) || check_gm_lds()) return 1;
  std::printf("ok %ld of %d co-resident variants accepted\n", n_accepted, 4 * 64 * 16);
  return 0;
}
