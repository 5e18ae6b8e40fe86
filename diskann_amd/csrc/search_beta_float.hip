// beam_search_beta_kernel instantiations for f32 / f16 rows and PQ codes (see search_beta_impl.h; split by row family so
// the translation units compile in parallel)
#include "search_beta_impl.h"

namespace dann {
int32_t launch_search_beta_float(const SearchArgs& a, uint32_t qcap, size_t lds, hipStream_t stream, int* regs_out) {
    switch (a.ix.dtype) {
        case DT_F32: return launch_beta_row_type<DT_F32>(a, qcap, lds, stream, regs_out);
        case DT_F16: return launch_beta_row_type<DT_F16>(a, qcap, lds, stream, regs_out);
        case DT_PQ: return launch_beta_row_type<DT_PQ>(a, qcap, lds, stream, regs_out);
    }
    set_error("bad dtype %d", a.ix.dtype);
    return DANN_EINVAL;
}
}  // namespace dann
