// (dtype, metric) -> the kernel instantiation's (DT, OP, NORM): the one place that knows which triples have kernels and
// the one ladder every kernel family's launch walks.  No HIP here: tests/test_row_dispatch_host.py compiles it with g++.
#pragma once
#include "row_types.h"

namespace dann {

// The (DT, OP, NORM) triples that have kernels -- exactly the ones resolve_metric can answer with: NORM folds the
// normalised metric's epilogue into L2 for scalar-quantised rows and into the inner product for float and MinMax rows;
// scalar-quantised rows have no Cosine; PQ rows have L2 and the inner product.
constexpr bool row_op_defined(int dt, int op, bool norm) {
    if (dt == DT_PQ) return !norm && (op == OP_L2 || op == OP_IP);
    if (op == OP_L2) return !norm || dt_is_sq(dt);
    if (op == OP_IP) return !norm || dt == DT_F32 || dt == DT_F16 || dt_mm_rows(dt);
    return op == OP_COS && !norm && !dt_is_sq(dt);
}

// beam search also has a form with the row length fixed at 128 elements: under L2 for every row type but PQ, under the
// inner product and Cosine for every row type but PQ and the float rows; MinMax rows searched with MM8 queries have none
constexpr bool search_dim128_defined(int dt, int op) {
    return dt != DT_PQ && !dt_is_mmq(dt) && (op == OP_L2 || (dt != DT_F32 && dt != DT_F16));
}

// what a visitor hands its functor: read the constants as decltype(r)::dt
template <int DT, int OP, bool NORM>
struct RowOp {
    static constexpr int dt = DT, op = OP;
    static constexpr bool norm = NORM;
};

// The visitors' two refusals (no dann.h code is this small): the metric does not resolve to a defined triple; the
// dtype is outside the row set.  dispatch_row_op (dann_internal.h) turns the first into the caller's error.
enum : int32_t { kNoMetric = INT32_MIN, kNoRow = INT32_MIN + 1 };

// f(RowOp<DT, op, norm>{}) for the (op, norm) that `metric` means on rows of type DT; an undefined triple is never
// instantiated
template <int DT, class F>
int32_t visit_metric(int metric, F&& f) {
    int op;
    bool norm;
    if (!resolve_metric(DT, metric, &op, &norm)) return kNoMetric;
    if (op == OP_L2) {
        if constexpr (row_op_defined(DT, OP_L2, true)) {
            if (norm) return f(RowOp<DT, OP_L2, true>{});
        }
        return f(RowOp<DT, OP_L2, false>{});
    }
    if (op == OP_IP) {
        if constexpr (row_op_defined(DT, OP_IP, true)) {
            if (norm) return f(RowOp<DT, OP_IP, true>{});
        }
        return f(RowOp<DT, OP_IP, false>{});
    }
    if constexpr (row_op_defined(DT, OP_COS, false)) {
        if (op == OP_COS) return f(RowOp<DT, OP_COS, false>{});
    }
    return kNoMetric;
}

// The row types an entry point serves:
//   kRowsStored  the 14 row types an index stores -- entry points that take no query (prune, consolidate, in-place
//                delete, distances between stored or raw rows)
//   kRowsQuery   plus DT_SPH1T, the transposed query layout of DT_SPH1 rows, and DT_MM1Q / MM2Q / MM4Q, MinMax rows
//                searched with MM8 queries -- entry points that take a query (rerank, expand-beam, paged and diverse
//                search, the flat scans)
//   kRowsSearch  plus DT_PQ, which only beam search serves
//   kRowsFloat   f32 / f16, the MFMA pool prune;  kRowsPair  one-byte codes, two queries per wavefront
enum RowSet { kRowsStored, kRowsQuery, kRowsSearch, kRowsFloat, kRowsPair };
constexpr bool row_in_set(RowSet s, int dt) {
    if (s == kRowsFloat) return dt == DT_F32 || dt == DT_F16;
    if (s == kRowsPair) return dt == DT_U8 || dt == DT_I8 || dt == DT_SQ8;
    if (dt == DT_SPH1T || dt_is_mmq(dt)) return s == kRowsQuery || s == kRowsSearch;
    if (dt == DT_PQ) return s == kRowsSearch;
    return dt == DT_F32 || dt == DT_F16 || dt == DT_U8 || dt == DT_I8 || dt_is_sq(dt) || dt_is_sph(dt) || dt_is_mm(dt);
}

// visit_metric for the row type `dtype`, if ROWS holds it
template <RowSet ROWS, class F>
int32_t visit_row_op(int dtype, int metric, F&& f) {
    switch (dtype) {
#define DANN_ROW(DT)                                                          \
    case DT:                                                                  \
        if constexpr (row_in_set(ROWS, DT)) return visit_metric<DT>(metric, f); \
        break;
        DANN_ROW(DT_F32) DANN_ROW(DT_F16) DANN_ROW(DT_U8) DANN_ROW(DT_I8) DANN_ROW(DT_SQ8) DANN_ROW(DT_SQ4) DANN_ROW(DT_SQ1)
        DANN_ROW(DT_SPH1) DANN_ROW(DT_SPH2) DANN_ROW(DT_SPH4) DANN_ROW(DT_MM1) DANN_ROW(DT_MM2) DANN_ROW(DT_MM4)
        DANN_ROW(DT_MM8) DANN_ROW(DT_SPH1T) DANN_ROW(DT_MM1Q) DANN_ROW(DT_MM2Q) DANN_ROW(DT_MM4Q) DANN_ROW(DT_PQ)
#undef DANN_ROW
    }
    return kNoRow;
}

}  // namespace dann
