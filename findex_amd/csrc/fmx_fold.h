// fmx_fold.h -- the search under a fold map (fmx_fold.hip) as fmx_context.hip calls it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <fmx.h>

#include "fmx_host.h"

namespace fmx {

struct FoldInfo {
  uint64_t total = 0, steps = 0, requests = 0;
  double search_ms = 0.0, sort_ms = 0.0;        // device events: the search kernel, the ordering step
};

constexpr uint32_t kFoldLeadBit = 0x80000000u;  // in a record's len, per > 1 only: the record's pattern had leading exact steps

// fold_map_check: FMX_ERR_ARG with a message unless `opts` (NULL: ASCII case folding) holds a valid map; map = its 256 bytes.
int fold_map_check(const fmx_fold_opts *opts, uint8_t map[256]);
int fold_handle_check(const Index *h);

// The hits of k patterns under `map`, device pointers throughout; allocates, synchronises `st`, frees its temporaries on
// every path.  d_lead (k bytes or null: all 0): the leading steps of each pattern that are exact whatever the map says.
// Pattern q's hits are reported under group q / per, in CSR over the k / per groups (d_out_off: k / per + 1 words), by
// ascending sp; with per > 1 a record of a pattern with lead != 0 carries kFoldLeadBit in its len and comes behind a record
// of the same sp without.  info->total is the exact number of hits; when it exceeds cap nothing is ordered and d_out_off /
// d_out are unspecified.  max_len (1 .. FMX_FOLD_MAX_LEN, clamped to that): no pattern is longer, as far as the caller knows;
// each wave's stack is sized for it, and the kernel skips a longer pattern and raises its flag.  check_len: such a pattern may
// be among them -- FMX_ERR_ARG then, after the launch.
int fold_search(const Index *h, const void *d_pat, const void *d_off, uint64_t k, const uint8_t map[256], const uint8_t *d_lead,
                uint64_t per, uint32_t max_len, void *d_out_off, void *d_out, uint64_t cap, bool check_len, hipStream_t st,
                FoldInfo *info);

void fold_set_last(const FoldInfo &info);

// The ordering step of fold_search, which the class search (fmx_classes.hip) takes as it is: `rows` staged hits
// {group | len << 32, sp, ep} into d_out by group, then sp, then (tb == 1) the lead bit, and the CSR offsets of the `groups`
// groups into d_out_off; rows == 0 writes the offsets alone.  Enqueues on `st`; its sort space comes from `mem`.
constexpr int kFoldRowBits = 38;                // rows are below 2^38, groups below 2^26: the sort key
int fold_order(DevMem &mem, unsigned long long *stage, uint64_t rows, uint64_t groups, int tb, void *d_out_off, void *d_out,
               hipStream_t st);

}  // namespace fmx
