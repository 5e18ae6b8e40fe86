// beam_search_beta_kernel instantiations for MinMax rows (see search_beta_impl.h; split by row family so
// the translation units compile in parallel)
#include "search_beta_impl.h"

namespace dann {
int32_t launch_search_beta_mm(const SearchArgs& a, uint32_t qcap, size_t lds, hipStream_t stream, int* regs_out) {
    switch (a.ix.dtype) {
        case DT_MM1: return launch_beta_row_type<DT_MM1>(a, qcap, lds, stream, regs_out);
        case DT_MM2: return launch_beta_row_type<DT_MM2>(a, qcap, lds, stream, regs_out);
        case DT_MM4: return launch_beta_row_type<DT_MM4>(a, qcap, lds, stream, regs_out);
        case DT_MM8: return launch_beta_row_type<DT_MM8>(a, qcap, lds, stream, regs_out);
    }
    set_error("bad dtype %d", a.ix.dtype);
    return DANN_EINVAL;
}
}  // namespace dann
