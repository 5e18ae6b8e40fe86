// beam_search_beta_kernel instantiations for one-byte and scalar-quantised rows (see search_beta_impl.h; split by row family so
// the translation units compile in parallel)
#include "search_beta_impl.h"

namespace dann {
int32_t launch_search_beta_int(const SearchArgs& a, uint32_t qcap, size_t lds, hipStream_t stream, int* regs_out) {
    switch (a.ix.dtype) {
        case DT_U8: return launch_beta_row_type<DT_U8>(a, qcap, lds, stream, regs_out);
        case DT_I8: return launch_beta_row_type<DT_I8>(a, qcap, lds, stream, regs_out);
        case DT_SQ8: return launch_beta_row_type<DT_SQ8>(a, qcap, lds, stream, regs_out);
        case DT_SQ4: return launch_beta_row_type<DT_SQ4>(a, qcap, lds, stream, regs_out);
        case DT_SQ1: return launch_beta_row_type<DT_SQ1>(a, qcap, lds, stream, regs_out);
    }
    set_error("bad dtype %d", a.ix.dtype);
    return DANN_EINVAL;
}
}  // namespace dann
