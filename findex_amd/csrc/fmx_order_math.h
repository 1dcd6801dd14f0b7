// fmx_order_math.h -- the arithmetic of the order step (fmx_order.h): how large the sort's and the scan's workspaces are, and
// the bits a value takes.  Plain functions that need no device: tests/native/order_math.cpp checks them on the host.
#pragma once
#include <stdint.h>

namespace fmx {

constexpr int kScanSum = 0, kScanMax = 1;
constexpr uint32_t kScanTile = 2048;                // elements per scan block: 8 per thread
constexpr uint32_t kRadixTile = 4096;               // keys per radix tile: 16 chunks of 256

inline int bits_for(uint64_t v) {                   // the bits that hold 0 .. v: the significant bits of v, at least 1
  int b = 1;
  while (b < 64 && (v >> b) != 0) b++;
  return b;
}

inline uint64_t radix_tiles(uint64_t m) { return (m + kRadixTile - 1) / kRadixTile; }

// u32 slots the recursive scan of len elements needs for its block totals: level j's totals lie behind those of the levels
// before it, and the last level (one block) writes one
inline uint64_t scan_partials(uint64_t len) {
  uint64_t t = 0;
  while (len > 1) { len = (len + kScanTile - 1) / kScanTile; t += len; }
  return t + 1;
}

inline uint64_t scan_space_bytes(uint64_t len) { return 4 * scan_partials(len); }

// The sort of m (u64 key, u32 value) pairs: two key buffers, two value buffers, one histogram of 256 digits per tile, and
// the block totals of the longer of the two scans the workspace serves (the histograms', and one over m elements)
inline uint64_t sort_hist_words(uint64_t m) { return 256 * radix_tiles(m); }
inline uint64_t sort_scan_len(uint64_t m) { return m > sort_hist_words(m) ? m : sort_hist_words(m); }
inline uint64_t sort_space_bytes(uint64_t m) { return 2 * 8 * m + 2 * 4 * m + 4 * sort_hist_words(m) + scan_space_bytes(sort_scan_len(m)); }

}  // namespace fmx
