// pair_search_kernel instantiations (search_pair_impl.h: two queries per wavefront, 128-byte integer rows); its own
// translation unit so that it compiles beside the beam_search_kernel instantiations of search_{u8,i8,sq8}.hip
#include "search_pair_impl.h"

namespace dann {
// the kernel of the launch's row type, metric and pair_qe / pair_re
int32_t launch_search_pair(const SearchArgs& a, size_t lds, hipStream_t stream) {
    const uint32_t grid = (a.nq + 1u) / 2u, qe = pair_qe(a), re = pair_re(a);
    const int32_t rc = dispatch_row_op<kRowsPair>(a.ix.dtype, a.ix.metric, [&](auto r) {
        using R = decltype(r);
#define DANN_PAIR_GO(QE, RE)                                                                                       \
    launch_kernel<pair_search_kernel<R::dt, R::op, R::norm, QE, RE>, kLds160>("pair_search_kernel launch", dim3(grid), \
                                                                              dim3(kWave), lds, stream, a)
        return re == 2u ? (qe == 3u ? DANN_PAIR_GO(3, 2) : DANN_PAIR_GO(2, 2))
             : qe == 3u ? DANN_PAIR_GO(3, 1)
             : qe == 2u ? DANN_PAIR_GO(2, 1)
                        : DANN_PAIR_GO(1, 1);
#undef DANN_PAIR_GO
    });
    if (rc != kNoRow) return rc;
    set_error("internal: two queries per wavefront serve 128-byte integer rows");
    return DANN_EINTERNAL;
}
}  // namespace dann
