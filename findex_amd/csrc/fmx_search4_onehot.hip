// fmx_search4_onehot.hip -- the k_search4 instantiations (fmx_search4.h, FMX_SEARCH4_LIST) of the one-hot layout up to 2^32 rows.
#include "fmx_search4.h"

namespace fmx {

FMX_SEARCH4_ONEHOT(FMX_SEARCH4_INSTANTIATE, false)

}  // namespace fmx
