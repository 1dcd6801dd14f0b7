// fmx_pool_deal.h -- how k_search4's pool of drawn batches is dealt to its ticket counters (fmx_search4.h, "the pool").
//
// The waves of a launch draw the pool's batches by ticket from up to 64 counters: the 32 waves of group g = wave / 32 draw
// from counter g mod nshards.  The counters do not have equal numbers of drawers -- 160 groups on 64 counters are three
// groups for counters 0..31 and two for the others, and the launch's last group may be short -- so every counter owns a
// share of the pool in proportion to its drawers: with D_c the drawers of the counters before c,
//     first_c = floor(npool * D_c / nwaves),   count_c = first_(c+1) - first_c,
// contiguous ranges that tile [0, npool) and differ from npool * drawers_c / nwaves by less than one batch.
// (Until this rule the counters had equal shares, npool / nshards each: the waves of the short-handed counters drew three
// batches where the others drew one or two, and the launch ended with them -- profiles/pool_c3_ab.md.)
//
// Written for a wave's scalar unit: with 64 counters, a power of two, the only divisions are the two by nwaves, of 32 bits
// whenever the product fits them (a grid of less than 2^16 waves) -- a 64-bit division is a long vector sequence on the
// device, and its registers would be the kernel's high-water mark.
//
// Nothing from HIP is included: the kernel and a host test (tests/test_search_pool_deal.py) compile the same code.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define FMX_POOL_HD __host__ __device__
#else
#define FMX_POOL_HD
#endif

namespace fmx {

constexpr uint32_t kPoolShards = 64;      // counters per ticket area (fmx_device.h, kTixShards): a power of two
constexpr uint32_t kPoolGroupLog = 5;     // waves that share a counter come in groups of 32 consecutive ones

struct PoolDeal {
  uint32_t first;        // this counter's first pool batch (ticket j is pool batch first + j)
  uint32_t count;        // ... how many it owns
  uint32_t drawers;      // the waves that draw from it
};

// The counters a launch of `nwaves` waves uses: one per group of 32 waves, kPoolShards at the most.
FMX_POOL_HD inline uint32_t pool_shards(uint32_t nwaves) {
  const uint32_t groups = (nwaves + (1u << kPoolGroupLog) - 1u) >> kPoolGroupLog;
  return groups < kPoolShards ? groups : kPoolShards;
}

// The counter wave `wave` of `nwaves` draws from: (wave / 32) mod pool_shards(nwaves) -- with fewer groups than counters
// every group has its own.
FMX_POOL_HD inline uint32_t pool_shard_of(uint32_t wave, uint32_t nwaves) {
  const uint32_t g = wave >> kPoolGroupLog;
  return pool_shards(nwaves) == kPoolShards ? g & (kPoolShards - 1u) : g;
}

// floor(a * b / d) for a quotient that fits 32 bits.
FMX_POOL_HD inline uint32_t pool_muldiv(uint32_t a, uint32_t b, uint32_t d) {
  const uint64_t p = (uint64_t)a * b;
  if ((p >> 32) == 0) return (uint32_t)p / d;
  uint64_t rem = 0;     // long division, a bit per turn: grids of 2^16 waves and more only
  uint32_t quo = 0;
  for (int i = 63; i >= 0; i--) {
    rem = (rem << 1) | ((p >> i) & 1u);
    quo <<= 1;
    if (rem >= d) { rem -= d; quo |= 1u; }
  }
  return quo;
}

// Counter `shard`'s share of a pool of `npool` batches in a launch of `nwaves` waves (shard < pool_shards(nwaves)).
FMX_POOL_HD inline PoolDeal pool_deal(uint32_t nwaves, uint32_t shard, uint32_t npool) {
  const uint32_t groups = (nwaves + (1u << kPoolGroupLog) - 1u) >> kPoolGroupLog;      // the last one may be short
  const bool full = groups >= kPoolShards;                                              // all the counters are in use
  const uint32_t q = full ? groups / kPoolShards : 1u, r = full ? groups % kPoolShards : 0u;      // counters 0 .. r-1 have q + 1 groups, the others q
  const uint32_t last = full ? (groups - 1u) % kPoolShards : groups - 1u;               // the counter the last group draws from
  const uint32_t short_by = (groups << kPoolGroupLog) - nwaves;                         // ... and the waves it lacks
  // the drawers of the counters before `shard`, and before `shard + 1`
  const uint32_t d0 = ((shard * q + (shard < r ? shard : r)) << kPoolGroupLog) - (last < shard ? short_by : 0u);
  const uint32_t d1 = (((shard + 1u) * q + (shard + 1u < r ? shard + 1u : r)) << kPoolGroupLog) - (last <= shard ? short_by : 0u);
  PoolDeal d;
  d.first = pool_muldiv(npool, d0, nwaves);
  d.count = pool_muldiv(npool, d1, nwaves) - d.first;
  d.drawers = d1 - d0;
  return d;
}

}  // namespace fmx
