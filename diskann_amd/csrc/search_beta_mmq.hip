// beam_search_beta_kernel instantiations for MinMax rows searched with MM8 queries (see search_beta_impl.h; split by row family so
// the translation units compile in parallel)
#include "search_beta_impl.h"

namespace dann {
int32_t launch_search_beta_mmq(const SearchArgs& a, uint32_t qcap, size_t lds, hipStream_t stream, int* regs_out) {
    switch (a.ix.dtype) {
        case DT_MM1Q: return launch_beta_row_type<DT_MM1Q>(a, qcap, lds, stream, regs_out);
        case DT_MM2Q: return launch_beta_row_type<DT_MM2Q>(a, qcap, lds, stream, regs_out);
        case DT_MM4Q: return launch_beta_row_type<DT_MM4Q>(a, qcap, lds, stream, regs_out);
    }
    set_error("bad dtype %d", a.ix.dtype);
    return DANN_EINVAL;
}
}  // namespace dann
