// fmx_search4_onehot_kx.hip -- the k_search4 instantiations (fmx_search4.h, FMX_SEARCH4_LIST) with level KT + 1 of the k-mer table.
#include "fmx_search4.h"

namespace fmx {

FMX_SEARCH4_ONEHOT_LEVELX(FMX_SEARCH4_INSTANTIATE)

}  // namespace fmx
