// tests/native/credibilist_probability_test.cpp -- credibilist_probability (slam-constructor_amd/csrc/slamhip_internal.h:
// the one definition the scorers, the probability plane's writers and the host share) compiled for the host and run
// over the golden cells of tests/golden/credibilist.npz, which the test hands over as a flat file of doubles:
// n records of (u, e, o, c, the reference's 1 - CredibilistCell::discrepancy(scorer's observation)).  Bitwise equality.
//   g++ -std=c++17 -O2 -ffp-contract=off -D__HIP_PLATFORM_AMD__ -I<hip> -I<repo>/include -I<repo>/slam-constructor_amd/csrc
#include <cstdio>
#include <cstring>
#include <vector>

#include "slamhip_internal.h"

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  FILE *f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<double> v;
  double rec[5];
  while (std::fread(rec, sizeof(double), 5, f) == 5) v.insert(v.end(), rec, rec + 5);
  std::fclose(f);
  long n = (long)v.size() / 5, bad = 0, differ_from_tbm = 0;
  for (long i = 0; i < n; ++i) {
    const double *r = &v[5 * i];
    const double got = slamhip::credibilist_probability(r[0], r[1], r[2], r[3]);
    const double via = slamhip::belief_probability(SLAMHIP_CELL_CREDIBILIST, r[0], r[1], r[2], r[3]);
    if (std::memcmp(&got, &r[4], sizeof got) != 0 || std::memcmp(&via, &got, sizeof got) != 0) {
      if (bad < 10) std::printf("cell %ld (%a %a %a %a): got %a want %a\n", i, r[0], r[1], r[2], r[3], got, r[4]);
      ++bad;
    }
    const double tbm = slamhip::belief_probability(SLAMHIP_CELL_TBM, r[0], r[1], r[2], r[3]);
    if (std::memcmp(&tbm, &got, sizeof got) != 0) ++differ_from_tbm;
  }
  std::printf("%ld cells, %ld mismatches, %ld differ from the TBM cell's value\n", n, bad, differ_from_tbm);
  return bad ? 1 : 0;
}
