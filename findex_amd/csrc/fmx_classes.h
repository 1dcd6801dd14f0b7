// fmx_classes.h -- the search under string classes (fmx_classes.hip): the class table as the kernel reads it.
#pragma once
#include <stdint.h>

#include <vector>

#include <fmx.h>

#include "fmx_fold.h"
#include "fmx_host.h"

namespace fmx {

// One class in device memory: a 128-byte line a wave reads with uniform loads.  w[g] holds member g's bytes in the order they
// are stepped -- the member's LAST byte in bits 0 .. 7 -- and len[g] how many of them there are.
struct ClassRec {
  uint32_t w[FMX_CLASS_MAX_MEMBERS];
  uint8_t len[FMX_CLASS_MAX_MEMBERS];
  uint32_t count;
  uint32_t pad[11];
};
static_assert(sizeof(ClassRec) == 128, "a class is one cache line");

// FMX_ERR_ARG with the offending class in the message unless `tab` (NULL: no classes) is a valid table; packed = its classes
// as the kernel takes them, *largest = the members of its largest class (1 for the empty table).
int classes_table_check(const fmx_class_table *tab, std::vector<ClassRec> *packed, uint32_t *largest);

// The hits of k patterns of uint16_t elements, device pointers throughout (the table is host memory); allocates, synchronises
// `st` and frees its temporaries on every path, as fold_search does, whose FoldInfo, output order and overflow rule these are.
// max_len (1 .. FMX_CLASS_MAX_ELEMS): no pattern has more elements, as far as the caller knows; check_flags: one may, or may
// name a class outside the table -- FMX_ERR_ARG then, after the launch.
// per > 1: pattern q reports under group q / per, in CSR over the k / per groups, and a pattern with q % per != 0 carries
// kFoldLeadBit in its records' len and comes behind a record of the same sp without (fold_search's rule; fmx_context.hip).
int classes_search(const Index *h, const void *d_el, const void *d_off, uint64_t k, uint64_t per, const std::vector<ClassRec> &packed,
                   uint32_t largest, uint32_t max_len, void *d_out_off, void *d_out, uint64_t cap, bool check_flags,
                   hipStream_t st, FoldInfo *info);
void classes_set_last(const FoldInfo &info);

}  // namespace fmx
