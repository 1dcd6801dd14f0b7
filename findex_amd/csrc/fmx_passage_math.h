// fmx_passage_math.h -- the arithmetic of the passages (fmx_passages.hip), for the host and the device alike:
// the two sort keys and their fields, the order in which a window's value is added up (include/fmx.h: no FMA) and the
// total order the best window is chosen by.  Plain functions that need no device: tests/native/passage_math.cpp checks
// them on the host.
#pragma once
#include <stdint.h>

#include "fmx_order_math.h"
#include "fmx_rank_math.h"

namespace fmx {

// ---- the hit table's key: query << doc_bits | document, doc_bits = bits_for(n_docs).  Queries and documents are both
// fewer than 2^32 - 1, so the key always fits.
FMX_RANK_HD uint64_t psg_hit_key(uint64_t query, uint64_t doc, int doc_bits) { return (query << doc_bits) | doc; }

// ---- the occurrence key: hit << (slot_bits + pos_bits) | slot in query << pos_bits | f, sorted over exactly its bits
struct PsgBits {
  int hit_bits, slot_bits, pos_bits;
  FMX_RANK_HD int total() const { return hit_bits + slot_bits + pos_bits; }
  FMX_RANK_HD int hit_shift() const { return slot_bits + pos_bits; }            // < 64 whenever total() <= 64: hit_bits >= 1
};

// n_hits >= 1 hits (0 .. n_hits: a hit's successor is formed for the segment bounds), queries of at most max_slots slots
// (0 .. max_slots: a slot's successor bounds its run) and stream positions 0 .. stream_len - 1
inline PsgBits psg_bits(uint64_t n_hits, uint64_t max_slots, uint64_t stream_len) {
  return PsgBits{bits_for(n_hits), bits_for(max_slots), bits_for(stream_len ? stream_len - 1 : 0)};
}

FMX_RANK_HD uint64_t psg_key(uint64_t hit, uint64_t slot, uint64_t f, const PsgBits &b) {
  return (hit << b.hit_shift()) | (slot << b.pos_bits) | f;
}
FMX_RANK_HD uint64_t psg_key_pos(uint64_t key, const PsgBits &b) { return key & ((1ull << b.pos_bits) - 1); }       // pos_bits <= 32
FMX_RANK_HD uint64_t psg_key_slot(uint64_t key, const PsgBits &b) { return (key >> b.pos_bits) & ((1ull << b.slot_bits) - 1); }
FMX_RANK_HD uint64_t psg_key_hit(uint64_t key, const PsgBits &b) { return key >> b.hit_shift(); }

// ---- a window: its start, value and cover.  An invalid one (no start seen yet) loses against every valid one.
struct PsgBest {
  double value;
  uint64_t a, mask;
  int valid;
};

// x stands before y: the larger value (plain > on doubles), equal values by the smaller start.  Two windows of one start
// have one cover and one value, so this is a total order on the windows of a hit.
FMX_RANK_HD bool psg_before(const PsgBest &x, const PsgBest &y) {
  if (!x.valid || !y.valid) return x.valid && !y.valid;
  return x.value > y.value || (x.value == y.value && x.a < y.a);
}

// value = ((0.0 + w(s0)) + w(s1)) + ..: one slot more, in ascending slot order
FMX_RANK_HD void psg_cover(PsgBest &x, unsigned slot, double w) {
  x.value = rank_add(x.value, w);
  x.mask |= 1ull << slot;
}

}  // namespace fmx
