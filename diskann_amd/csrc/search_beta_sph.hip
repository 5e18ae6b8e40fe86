// beam_search_beta_kernel instantiations for spherical-quantised rows and the transposed query layout (see search_beta_impl.h; split by row family so
// the translation units compile in parallel)
#include "search_beta_impl.h"

namespace dann {
int32_t launch_search_beta_sph(const SearchArgs& a, uint32_t qcap, size_t lds, hipStream_t stream, int* regs_out) {
    switch (a.ix.dtype) {
        case DT_SPH1: return launch_beta_row_type<DT_SPH1>(a, qcap, lds, stream, regs_out);
        case DT_SPH1T: return launch_beta_row_type<DT_SPH1T>(a, qcap, lds, stream, regs_out);
        case DT_SPH2: return launch_beta_row_type<DT_SPH2>(a, qcap, lds, stream, regs_out);
        case DT_SPH4: return launch_beta_row_type<DT_SPH4>(a, qcap, lds, stream, regs_out);
    }
    set_error("bad dtype %d", a.ix.dtype);
    return DANN_EINVAL;
}
}  // namespace dann
