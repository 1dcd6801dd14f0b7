// ctx_math.cpp -- fmx_ctx_math.h held to bit-by-bit loops, exhaustively (tests/test_words_cpu.py builds this with
// -fsanitize=address,undefined and runs it).
//   1. ctx_heads / ctx_tails: every 12-bit mask x both carries on either side against a loop over the bits.
//   2. ctx_range_mask / ctx_valid_mask: every lo, hi of 0 .. 40 at widths 1 .. 32.
//   3. chunk cuts: a 64-row chunk of 16-row lanes, every record [base + s, .. + e) with start offset s and end offset e of
//      0 .. 33 over 0 .. 2 further chunks, at two bases and three pass patterns: the heads and tails the lanes report with
//      their carries, summed over the chunks, are the run starts and ends of a loop over the record's rows, in order.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "fmx_ctx_math.h"

using namespace fmx;

static int fails = 0;
#define CHECK(c)                                                    \
  do {                                                              \
    if (!(c)) {                                                     \
      if (fails++ < 20) std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
    }                                                               \
  } while (0)

static void masks_12() {
  const uint32_t W = 12;
  for (uint32_t m = 0; m < (1u << W); m++)
    for (uint32_t cin = 0; cin < 2; cin++)
      for (uint32_t cout = 0; cout < 2; cout++) {
        uint32_t h = 0, t = 0;
        for (uint32_t i = 0; i < W; i++) {
          const uint32_t cur = (m >> i) & 1u;
          const uint32_t prev = i ? (m >> (i - 1)) & 1u : cin;
          const uint32_t next = i + 1 < W ? (m >> (i + 1)) & 1u : cout;
          if (cur && !prev) h |= 1u << i;
          if (cur && !next) t |= 1u << i;
        }
        CHECK(ctx_heads(m, cin) == h);
        CHECK(ctx_tails(m, cout, W) == t);
      }
}

static void ranges() {
  for (uint32_t w = 1; w <= 32; w++)
    for (uint64_t lo = 0; lo <= 40; lo++)
      for (uint64_t hi = 0; hi <= 40; hi++) {
        uint32_t want = 0;
        for (uint32_t i = 0; i < w; i++)
          if (i >= lo && i < hi) want |= 1u << i;
        CHECK(ctx_range_mask(lo, hi, w) == want);
        CHECK(ctx_valid_mask(100, 100 + lo, 100 + hi, w) == want);
      }
  CHECK(ctx_valid_mask(64, 10, 20, 16) == 0u);                       // a record that ends before the lane
  CHECK(ctx_valid_mask(64, 100, 200, 16) == 0u);                     // one that begins behind it
  CHECK(ctx_valid_mask(64, 0, ~0ull, 16) == 0xffffu);
  CHECK(ctx_range_mask(0, ~0ull, 32) == 0xffffffffu);
}

static bool pass_of(int pattern, uint64_t row) {
  switch (pattern) {
    case 0: return true;
    case 1: return (row & 1) != 0;                                   // alternating: a run per two rows
    default: return ((row * 2654435761ull) >> 7) % 3 != 0;           // mixed runs
  }
}

static void chunks() {
  const uint64_t chunk = 64, lanes = chunk / kCtxLane;
  for (int pattern = 0; pattern < 3; pattern++)
    for (uint64_t base : {(uint64_t)0, (uint64_t)(3 * 64 + 16)})
      for (uint64_t s = 0; s <= 33; s++)
        for (uint64_t more = 0; more <= 2; more++)
          for (uint64_t e = 0; e <= 33; e++) {
            const uint64_t a = base + s, b = base + more * chunk + e;
            // the loop: run starts and ends over the rows of [a, b)
            std::vector<uint64_t> want_h, want_t;
            for (uint64_t r = a; r < b; r++) {
              if (!pass_of(pattern, r)) continue;
              if (r == a || !pass_of(pattern, r - 1)) want_h.push_back(r);
              if (r + 1 == b || !pass_of(pattern, r + 1)) want_t.push_back(r + 1);
            }
            // the kernel's way
            std::vector<uint64_t> got_h, got_t;
            const uint64_t nc = ctx_chunk_count(a, b, chunk);
            if (a >= b) CHECK(nc == 0);
            else {
              CHECK(ctx_chunk_base(a) <= a && a - ctx_chunk_base(a) < kCtxLane && ctx_chunk_base(a) % kCtxLane == 0);
              CHECK(ctx_chunk_first(a, nc, chunk) >= b && ctx_chunk_first(a, nc - 1, chunk) < b);
            }
            for (uint64_t c = 0; c < nc; c++) {
              uint32_t m[8];
              for (uint64_t l = 0; l < lanes; l++) {
                const uint64_t row0 = ctx_chunk_first(a, c, chunk) + l * kCtxLane;
                uint32_t bits = 0;
                for (uint32_t i = 0; i < kCtxLane; i++)
                  if (pass_of(pattern, row0 + i)) bits |= 1u << i;
                m[l] = bits & ctx_valid_mask(row0, a, b, kCtxLane);
              }
              for (uint64_t l = 0; l < lanes; l++) {
                const uint64_t row0 = ctx_chunk_first(a, c, chunk) + l * kCtxLane;
                uint32_t cin = l ? m[l - 1] >> (kCtxLane - 1) : (row0 > a ? (uint32_t)pass_of(pattern, row0 - 1) : 0u);
                uint32_t cout = l + 1 < lanes ? m[l + 1] & 1u : (row0 + kCtxLane < b ? (uint32_t)pass_of(pattern, row0 + kCtxLane) : 0u);
                const uint32_t h = ctx_heads(m[l], cin), t = ctx_tails(m[l], cout, kCtxLane);
                for (uint32_t i = 0; i < kCtxLane; i++) {
                  if ((h >> i) & 1u) got_h.push_back(row0 + i);
                  if ((t >> i) & 1u) got_t.push_back(row0 + i + 1);
                }
              }
            }
            CHECK(got_h == want_h);
            CHECK(got_t == want_t);
            CHECK(got_h.size() == got_t.size());
          }
}

int main() {
  masks_12();
  ranges();
  chunks();
  if (fails) {
    std::printf("ctx math: %d failures\n", fails);
    return 1;
  }
  std::printf("ctx math ok\n");
  return 0;
}
