// fmx_search4_onehot_wide.hip -- the k_search4 instantiations (fmx_search4.h, FMX_SEARCH4_LIST) of the one-hot layout above 2^32 rows.
#include "fmx_search4.h"

namespace fmx {

FMX_SEARCH4_ONEHOT(FMX_SEARCH4_INSTANTIATE, true)

}  // namespace fmx
