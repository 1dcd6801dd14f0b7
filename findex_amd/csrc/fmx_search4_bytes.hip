// fmx_search4_bytes.hip -- the k_search4 instantiations (fmx_search4.h, FMX_SEARCH4_LIST) of the bytes layout.
#include "fmx_search4.h"

namespace fmx {

FMX_SEARCH4_BYTES(FMX_SEARCH4_INSTANTIATE)

}  // namespace fmx
