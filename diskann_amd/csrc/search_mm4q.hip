// beam_search_kernel instantiations for DT_MM4 rows searched with MM8 query images (see search_kernel_impl.h; split per
// row type so the translation units compile in parallel)
#include "search_kernel_impl.h"

namespace dann {
int32_t launch_search_mm4q(const SearchArgs& a, uint32_t qcap, size_t lds, hipStream_t stream, int* regs_out) {
    return launch_row_type<DT_MM4Q>(a, qcap, lds, stream, regs_out);
}
}  // namespace dann
