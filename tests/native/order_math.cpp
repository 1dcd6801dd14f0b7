// order_math.cpp -- the host arithmetic of the order step (findex_amd/csrc/fmx_order_math.h) against what the call sites
// computed by hand before there was one definition: the sort workspace's bytes, the scan scratch against the recursion that
// uses it, and bits_for against every loop it replaced.  Built with the sanitizers by tests/test_order_math_cpu.py.
#include <stdint.h>

#include <algorithm>
#include <cstdio>
#include <vector>

#include "fmx_order_math.h"

using namespace fmx;

static int failures = 0;
#define CHECK(cond, ...)                   \
  do {                                     \
    if (!(cond)) {                         \
      std::printf("FAIL %s: ", #cond);     \
      std::printf(__VA_ARGS__);            \
      std::printf("\n");                   \
      failures++;                          \
    }                                      \
  } while (0)

// The scan as ScanSpace::run walks it: a level of `len` elements writes one total per block at partials[at ..], and more than
// one block sends those totals through the next level, whose scratch begins behind them.  Returns the slots touched.
static uint64_t scan_extent(uint64_t len) {
  uint64_t at = 0, end = 0;
  while (len > 0) {
    const uint64_t nb = (len + kScanTile - 1) / kScanTile;
    end = at + nb;
    if (nb == 1) break;
    at += nb;
    len = nb;
  }
  return end;
}

// ---- the loops the call sites had
static int loop_holds(uint64_t v) {                  // occurrences, lines: the bits that hold 0 .. v
  int b = 1;
  while (b < 64 && (v >> b) != 0) b++;
  return b;
}
static int loop_corpus(uint64_t v) {                 // the document listing's doc_bits and k_bits (v < 2^32 there)
  int b = 1;
  while ((v >> b) != 0) b++;
  return b;
}
static int loop_clamped(uint64_t k, int clamp) {     // approx (26) and edit (23): pattern ids 0 .. k - 1
  int b = 1;
  while (b < clamp && ((k - 1) >> b) != 0) b++;
  return b;
}
static int bit_width(uint64_t v) { return v ? 64 - __builtin_clzll((unsigned long long)v) : 0; }      // n-grams

int main() {
  const uint64_t ms[] = {1, 2047, 2048, 2049, 2048ull * 2048, 2048ull * 2048 + 1, (1ull << 32) - 1};
  for (const uint64_t m : ms) {
    // the sort's workspace, as every call site summed it
    const uint64_t tiles = (m + 4095) / 4096;
    CHECK(radix_tiles(m) == tiles, "m = %llu", (unsigned long long)m);
    const uint64_t want = 24 * m + 4 * 256 * radix_tiles(m) + 4 * scan_partials(std::max<uint64_t>(m, 256 * radix_tiles(m)));
    CHECK(sort_space_bytes(m) == want, "m = %llu: %llu, the call sites had %llu", (unsigned long long)m,
          (unsigned long long)sort_space_bytes(m), (unsigned long long)want);
    CHECK(scan_space_bytes(m) == 4 * scan_partials(m), "m = %llu", (unsigned long long)m);
    // the scratch covers the recursion, level by level, with at most one slot to spare
    for (const uint64_t len : {m, 256 * tiles, m + 1, m - 1}) {
      const uint64_t ext = scan_extent(len), have = scan_partials(len);
      CHECK(ext <= have && have <= ext + 1, "len = %llu: the recursion touches %llu slots, scan_partials gives %llu",
            (unsigned long long)len, (unsigned long long)ext, (unsigned long long)have);
    }
    // ... and the sort's allotment covers both scans it serves
    const uint64_t allot = scan_partials(sort_scan_len(m));
    CHECK(scan_extent(m) <= allot && scan_extent(256 * tiles) <= allot, "m = %llu", (unsigned long long)m);
    // the recursion writes what the model says: replay it on a real buffer of the allotted size
    if (m <= 2048ull * 2048 + 1) {
      std::vector<uint32_t> partials(scan_partials(m), 0);
      uint64_t at = 0, len = m;
      while (len > 0) {
        const uint64_t nb = (len + kScanTile - 1) / kScanTile;
        for (uint64_t b = 0; b < nb; b++) partials.at(at + b) += 1;
        if (nb == 1) break;
        at += nb;
        len = nb;
      }
      for (uint64_t i = 0; i < scan_extent(m); i++) CHECK(partials[i] == 1, "m = %llu: slot %llu shared by two levels", (unsigned long long)m, (unsigned long long)i);
    }
  }
  CHECK(scan_partials(0) == 1 && scan_extent(0) == 0, "an empty scan");

  std::vector<uint64_t> vs = {0, 1, 2};
  for (int p = 1; p < 64; p++)
    for (const uint64_t v : {(1ull << p) - 1, 1ull << p, (1ull << p) + 1}) vs.push_back(v);
  vs.push_back(~0ull);
  for (const uint64_t v : vs) {
    CHECK(bits_for(v) == loop_holds(v), "v = %llu", (unsigned long long)v);
    CHECK(bits_for(v) == std::max(1, bit_width(v)), "v = %llu", (unsigned long long)v);
    if (v < (1ull << 63)) CHECK(bits_for(v) == loop_corpus(v), "v = %llu", (unsigned long long)v);
    if (v >= 1) CHECK(bits_for(v) == std::max(1, 64 - __builtin_clzll((unsigned long long)v)), "v = %llu", (unsigned long long)v);
    // the clamped forms take a pattern COUNT k and size the ids 0 .. k - 1; k == 0 wraps and meets the clamp in both
    CHECK(std::min(26, bits_for(v - 1)) == loop_clamped(v, 26), "k = %llu", (unsigned long long)v);
    CHECK(std::min(23, bits_for(v - 1)) == loop_clamped(v, 23), "k = %llu", (unsigned long long)v);
  }
  if (failures) {
    std::printf("%d checks failed\n", failures);
    return 1;
  }
  std::printf("order math ok: %zu sizes, %zu values\n", sizeof ms / sizeof ms[0], vs.size());
  return 0;
}
