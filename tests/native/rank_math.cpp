// The host arithmetic of ranked retrieval (findex_amd/csrc/fmx_rank_math.h), built with -fsanitize=address,undefined by
// tests/test_rank_cpu.py: the score key is monotone over negatives, zeros, denormals, neighbours one ulp apart and large
// values; its inverse gives the double back; 1.0 and its successor map to keys that differ by exactly 1; the weight formula.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <limits>
#include <vector>

#include "fmx_rank_math.h"

using namespace fmx;

static int fails = 0;
#define CHECK(cond)                                              \
  do {                                                           \
    if (!(cond)) {                                               \
      printf("FAILED line %d: %s\n", __LINE__, #cond);           \
      fails++;                                                   \
    }                                                            \
  } while (0)

static uint64_t bits(double x) {
  uint64_t u;
  memcpy(&u, &x, 8);
  return u;
}

int main() {
  const double inf = std::numeric_limits<double>::infinity(), dmin = std::numeric_limits<double>::denorm_min();
  const double big = std::numeric_limits<double>::max(), tiny = std::numeric_limits<double>::min();
  // ascending, neighbours one ulp apart among them
  std::vector<double> v = {-inf, -big, nextafter(-big, 0.0), -1e300, -2.0, nextafter(-1.0, -2.0), -1.0, nextafter(-1.0, 0.0), -0.5,
                           -tiny, nextafter(-tiny, 0.0), -2 * dmin, -dmin, -0.0, 0.0, dmin, 2 * dmin, nextafter(tiny, 0.0), tiny,
                           0.5, nextafter(1.0, 0.0), 1.0, nextafter(1.0, 2.0), 2.0, 1e300, nextafter(big, 0.0), big, inf};
  for (size_t i = 0; i < v.size(); i++) {
    CHECK(bits(rank_unkey(rank_key(v[i]))) == bits(v[i]));                   // the round trip, bit for bit (-0.0 too)
    for (size_t j = 0; j < v.size(); j++) {
      if (v[i] < v[j]) CHECK(rank_key(v[i]) < rank_key(v[j]));
      if (v[i] == v[j] && bits(v[i]) == bits(v[j])) CHECK(rank_key(v[i]) == rank_key(v[j]));
    }
    if (i) CHECK(rank_key(v[i - 1]) < rank_key(v[i]));                       // strictly, as listed (-0.0 below +0.0)
  }
  // neighbours: keys one apart, on both sides of the sign branch
  CHECK(rank_key(nextafter(1.0, 2.0)) - rank_key(1.0) == 1);
  CHECK(rank_key(-1.0) - rank_key(nextafter(-1.0, -2.0)) == 1);
  CHECK(rank_key(dmin) - rank_key(0.0) == 1);
  CHECK(rank_key(0.0) - rank_key(-0.0) == 1);
  CHECK(rank_key(-0.0) - rank_key(-dmin) == 1);
  CHECK(rank_key(0.0) == 0x8000000000000000ull);
  // a walk of single ulps keeps the order
  double x = 3.0;
  for (int i = 0; i < 1000; i++) {
    const double y = nextafter(x, 4.0);
    CHECK(rank_key(y) == rank_key(x) + 1);
    CHECK(rank_key(-y) + 1 == rank_key(-x));
    x = y;
  }
  // the weight: log(1 + (N - df + 0.5) / (df + 0.5))
  CHECK(rank_weight(3, 2) == log(1.0 + 1.5 / 2.5));
  CHECK(rank_weight(10, 0) == log(1.0 + 10.5 / 0.5));
  CHECK(rank_weight(10, 10) == log(1.0 + 0.5 / 10.5));
  CHECK(rank_weight(1000000, 1) > rank_weight(1000000, 2));
  // the term, operation by operation, and the case the tests lean on: b = 0, tf = 1 gives c == w exactly
  CHECK(rank_norm(5, 3.0, 1.2, 0.75) == 1.2 * ((1.0 - 0.75) + 0.75 * (5.0 / 3.0)));
  CHECK(rank_norm(5, 0.0, 1.2, 0.75) == 1.2 * ((1.0 - 0.75) + 0.75 * 0.0));
  CHECK(rank_norm(40, 17.5, 1.2, 0.0) == 1.2);
  CHECK((1.0 * (1.2 + 1.0)) / (1.0 + 1.2) == 1.0);
  CHECK(rank_term(1.0, 1, 1.2, 1.2) == 1.0);
  CHECK(rank_term(nextafter(1.0, 2.0), 1, 1.2, 1.2) == nextafter(1.0, 2.0));
  CHECK(rank_term(0.47, 2, 1.2, 1.8) == 0.47 * ((2.0 * (1.2 + 1.0)) / (2.0 + 1.8)));
  CHECK(bits(rank_add(0.0, -0.0)) == bits(0.0));                             // a score is never -0.0
  if (fails) return 1;
  printf("rank math ok\n");
  return 0;
}
