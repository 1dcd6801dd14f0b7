// The host arithmetic of the passages (findex_amd/csrc/fmx_passage_math.h), built with -fsanitize=address,undefined by
// tests/test_passages_cpu.py: the occurrence key packs and unpacks at the narrowest and the widest fields (64 bits in all, a
// shift of 63), its order is (hit, slot, position), the hit key orders by (query, document), the window order is total with
// equal values going to the smaller start, and the value is added up slot by slot without reassociation.
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "fmx_passage_math.h"

using namespace fmx;

static int fails = 0;
#define CHECK(cond)                                              \
  do {                                                           \
    if (!(cond)) {                                               \
      printf("FAILED line %d: %s\n", __LINE__, #cond);           \
      fails++;                                                   \
    }                                                            \
  } while (0)

int main() {
  // the fields: every one holds 0 .. its largest value
  PsgBits b = psg_bits(1, 0, 1);
  CHECK(b.hit_bits == 1 && b.slot_bits == 1 && b.pos_bits == 1 && b.total() == 3);
  b = psg_bits(40960, 3, 1ull << 28);
  CHECK(b.hit_bits == 16 && b.slot_bits == 2 && b.pos_bits == 28 && b.hit_shift() == 30);
  b = psg_bits(3, 64, 0xfffffffeull);
  CHECK(b.hit_bits == 2 && b.slot_bits == 7 && b.pos_bits == 32 && b.total() == 41);
  // the widest key that is accepted: 64 bits, the hit shifted by 39 .. 63
  b = psg_bits((1ull << 25) - 1, 64, 0xfffffffeull);
  CHECK(b.total() == 64);
  const uint64_t top_hit = (1ull << 25) - 1;
  uint64_t k = psg_key(top_hit, 64, 0xfffffffdull, b);
  CHECK(psg_key_hit(k, b) == top_hit && psg_key_slot(k, b) == 64 && psg_key_pos(k, b) == 0xfffffffdull);
  CHECK(psg_bits(1ull << 25, 64, 0xfffffffeull).total() == 65);              // one hit more: refused by the caller
  const PsgBits one{1, 31, 32};                                              // a shift of 63
  k = psg_key(1, 0x7fffffffull, 0xffffffffull, one);
  CHECK(k == ~0ull && psg_key_hit(k, one) == 1 && psg_key_slot(k, one) == 0x7fffffffull && psg_key_pos(k, one) == 0xffffffffull);
  // the order of the keys is (hit, slot, position), and a slot's successor at position 0 bounds its run
  b = psg_bits(100, 5, 1000);
  std::vector<uint64_t> keys;
  for (uint64_t h = 0; h < 3; h++)
    for (uint64_t s = 0; s <= 5; s++)
      for (uint64_t f : {0ull, 1ull, 998ull, 999ull}) keys.push_back(psg_key(h, s, f, b));
  for (size_t i = 1; i < keys.size(); i++) CHECK(keys[i - 1] < keys[i]);
  CHECK(psg_key(2, 3, 999, b) < psg_key(2, 4, 0, b) && psg_key(2, 5, 999, b) < psg_key(3, 0, 0, b));
  // the hit key
  CHECK(psg_hit_key(0, 7, 4) == 7 && psg_hit_key(3, 7, 4) == 55 && psg_hit_key(3, 15, 4) < psg_hit_key(4, 0, 4));
  CHECK(psg_hit_key(0xfffffffeull, 0xfffffffeull, 32) == 0xfffffffefffffffeull);
  // the window order: value first, then the smaller start; an invalid window loses against every valid one, never wins
  const PsgBest none{0.0, 0, 0, 0}, w1{1.0, 50, 1, 1}, w2{1.0, 40, 2, 1}, w3{3.0, 90, 3, 1}, wn{-2.0, 10, 4, 1}, z{0.0, 5, 0, 1};
  CHECK(psg_before(w3, w1) && !psg_before(w1, w3));
  CHECK(psg_before(w2, w1) && !psg_before(w1, w2));                          // equal values: the smaller start
  CHECK(!psg_before(w1, w1));
  CHECK(psg_before(wn, none) && !psg_before(none, wn) && !psg_before(none, none));
  CHECK(psg_before(z, wn) && psg_before(w1, z));
  const PsgBest all[] = {w1, w2, w3, wn, z};
  for (const PsgBest &x : all)
    for (const PsgBest &y : all)
      CHECK(psg_before(x, y) + psg_before(y, x) == (x.a == y.a ? 0 : 1));     // total and antisymmetric
  // the value: slot order is observable
  PsgBest v{0.0, 0, 0, 1};
  psg_cover(v, 0, 1e16);
  psg_cover(v, 1, 1.0);
  psg_cover(v, 2, -1e16);
  CHECK(v.value == 0.0 && v.mask == 7);
  PsgBest u{0.0, 0, 0, 1};
  psg_cover(u, 0, 1e16);
  psg_cover(u, 2, -1e16);
  psg_cover(u, 1, 1.0);
  CHECK(u.value == 1.0 && u.mask == 7);
  PsgBest t{0.0, 0, 0, 1};
  psg_cover(t, 63, 0.5);
  CHECK(t.mask == 1ull << 63 && t.value == 0.5);
  if (fails) return 1;
  printf("passage math ok\n");
  return 0;
}
