// The row-type and metric vocabulary shared by the kernels (dann_device.h) and the host-side launch planning
// (launch_plan.h).  No HIP here: tests/test_launch_plan_host.py compiles it with g++.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define DANN_HD __host__ __device__
#else
#define DANN_HD
#endif

namespace dann {

enum : int {
    DT_F32 = 0, DT_F16 = 1, DT_U8 = 2, DT_I8 = 3, DT_SQ8 = 4, DT_PQ = 5, DT_SQ1 = 17, DT_SQ4 = 20,
    // spherically quantised rows (spherical::Data<NBITS>), dtype value 32 + bits
    DT_SPH1 = 33, DT_SPH2 = 34, DT_SPH4 = 36,
    // internal, never a dann_config::dtype: DT_SPH1 rows searched with a FOUR_BIT_TRANSPOSED query (IndexView::dtype
    // of the query-taking entry points; the inner-product routine differs, so the layout is a template argument)
    DT_SPH1T = 97,
    // MinMax-quantised rows (minmax::Data<NBITS>, front-canonical: the 20-byte MinMaxCompensation, then the code
    // bytes), dtype value 48 + bits
    DT_MM1 = 49, DT_MM2 = 50, DT_MM4 = 52, DT_MM8 = 56,
    // internal, never a dann_config::dtype: DT_MM1 / MM2 / MM4 rows searched with MM8 query images
    // (MinMaxQuery::EightBit, dann_set_query_dtype; IndexView::dtype of the query-taking entry points), 112 + the rows' bits
    DT_MM1Q = 113, DT_MM2Q = 114, DT_MM4Q = 116
};
// scalar-quantised rows: SQ-8 (one byte per code) and the packed widths, whose dtype value is 16 + bits
DANN_HD constexpr bool dt_is_sq(int dt) { return dt == DT_SQ8 || dt == DT_SQ4 || dt == DT_SQ1; }
DANN_HD constexpr bool dt_is_sph(int dt) { return dt == DT_SPH1 || dt == DT_SPH2 || dt == DT_SPH4 || dt == DT_SPH1T; }
DANN_HD constexpr bool dt_is_mm(int dt) { return dt == DT_MM1 || dt == DT_MM2 || dt == DT_MM4 || dt == DT_MM8; }
DANN_HD constexpr bool dt_is_mmq(int dt) { return dt == DT_MM1Q || dt == DT_MM2Q || dt == DT_MM4Q; }
// MinMax rows under either query form: what the kernels and the launch shapes ask (dt_is_mm stays the four stored types,
// which is what the entry points validate a caller's dtype with)
DANN_HD constexpr bool dt_mm_rows(int dt) { return dt_is_mm(dt) || dt_is_mmq(dt); }
// rows of sub-byte codes: a 4-lane distance group (MM8 is one byte per code and takes the u8 path's 8 lanes)
DANN_HD constexpr bool dt_is_packed(int dt) {
    return dt == DT_SQ4 || dt == DT_SQ1 || dt_is_sph(dt) || dt == DT_MM1 || dt == DT_MM2 || dt == DT_MM4 || dt_is_mmq(dt);
}
// MinMax rows: bytes of the MinMaxCompensation in front of the codes, and where a query image is staged inside its
// LDS slot.  The codes start at byte 20 of an image: staged at slot + 12 they start at slot + 32, and every 16-, 8- or
// 4-byte LDS read of the lane shapes is naturally aligned; the slot (mm_query_lds_bytes) ends at the 16-byte step that
// covers the last code byte -- the tail step reads whole dwords, masked beyond dim * bits.
constexpr uint32_t kMmHeader = 20u, kMmStageOff = 12u;
DANN_HD constexpr uint32_t query_stage_off(int dt) { return dt_mm_rows(dt) ? kMmStageOff : 0u; }
DANN_HD constexpr uint32_t mm_query_lds_bytes(uint32_t image_bytes) {
    return kMmStageOff + kMmHeader + ((image_bytes - kMmHeader + 15u) & ~15u);
}
// An MM8 query image staged for narrower rows (mmq_stage_query, dann_device.h) takes the slot of the image itself,
// mm_query_lds_bytes(20 + dim): the staged codes are a permutation of the image's, one byte per element.  The one
// exception is DT_MM1Q, whose staged form is eight whole plane dwords per 32 elements: its last block needs 32 bytes
// where the image's rounded codes may end 16 earlier.
DANN_HD constexpr uint32_t mm_slot_bytes(int dt, uint32_t image_bytes) {
    return dt == DT_MM1Q ? kMmStageOff + kMmHeader + ((image_bytes - kMmHeader + 31u) & ~31u) : mm_query_lds_bytes(image_bytes);
}
// bytes of the LDS slot of a query of integer rows staged as raw bytes
DANN_HD constexpr uint32_t int_query_slot_bytes(int dt, uint32_t qbytes) { return dt_mm_rows(dt) ? mm_slot_bytes(dt, qbytes) : qbytes; }
enum : int { M_COSINE = 0, M_IP = 1, M_L2 = 2, M_COSN = 3 };
enum : int { OP_L2 = 0, OP_IP = 1, OP_COS = 2 };

constexpr uint32_t kEmpty = 0xFFFFFFFFu;

// (dtype, metric) -> (OP, NORMALIZED).  Integers treat CosineNormalized as Cosine
// (distance_provider.rs:274-297, full.rs:470,499); SQ-8 / SQ4 / SQ1 CosineNormalized is L2-based.
// Returns false for unsupported combinations (scalar-quantised rows have no plain Cosine).
DANN_HD inline bool resolve_metric(int dtype, int metric, int* op, bool* norm) {
    *norm = false;
    if (dtype == DT_PQ) {
        if (metric == M_L2) { *op = OP_L2; return true; }
        if (metric == M_IP) { *op = OP_IP; return true; }
        return false;
    }
    if (dt_is_sph(dtype)) {  // SupportedMetric (spherical/mod.rs): SquaredL2, InnerProduct, Cosine
        if (metric == M_L2) { *op = OP_L2; return true; }
        if (metric == M_IP) { *op = OP_IP; return true; }
        if (metric == M_COSINE) { *op = OP_COS; return true; }
        return false;
    }
    if (dt_mm_rows(dtype)) {  // distance_comparer (minmax_repr.rs:330-335): the form of the epilogue, finish_minmax
        if (metric == M_L2) { *op = OP_L2; return true; }
        if (metric == M_IP) { *op = OP_IP; return true; }
        if (metric == M_COSINE) { *op = OP_COS; return true; }
        *op = OP_IP;
        *norm = true;  // MinMaxCosineNormalized = 1 - v
        return true;
    }
    if (dt_is_sq(dtype)) {
        if (metric == M_L2) { *op = OP_L2; return true; }
        if (metric == M_IP) { *op = OP_IP; return true; }
        if (metric == M_COSN) { *op = OP_L2; *norm = true; return true; }
        return false;
    }
    if (metric == M_L2) { *op = OP_L2; return true; }
    if (metric == M_IP) { *op = OP_IP; return true; }
    if (metric == M_COSINE) { *op = OP_COS; return true; }
    if (dtype == DT_U8 || dtype == DT_I8) { *op = OP_COS; return true; }
    *op = OP_IP;
    *norm = true;  // CosineNormalized on float rows = 1 - <x, y>
    return true;
}

}  // namespace dann
