// seq_sum.h -- a sequential f64 sum, evaluated in parallel wherever that cannot change a bit.  Shared by the PQ trainer's
// rolling sums (pq_kernels.hip) and the medoid's column sums (medoid_kernels.hip); plain C++ besides the HD marks, so the
// test is unit-tested on the host as well (tests/test_build_finish_host.py).
//
// A floating-point sum is order-independent exactly when no addition rounds.  For a range of values v_i with
// g = the exponent of the lowest set bit over the v_i and the running sum acc at the range's start, and
// A = sum |v_i|: every partial sum the sequential walk forms is a multiple of 2^min(g, lsb(acc)) and at most
// |acc| + A in magnitude; if |acc| + A < 2^(min(g, lsb(acc)) + 53) they are all representable, no addition rounds,
// and the walk's result is acc + (sum of the range in ANY association).  `seq_exact` is that test (A carries a 2^-30
// margin for its own rounding; a non-finite value fails it).  Ranges that fail are walked one element at a time,
// from the carry: a low bit pushed out when acc crosses a power of two, or a value far below the running sum's last
// place -- local events on continuous data.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define DANN_SEQ_HD __host__ __device__ __forceinline__
#else
#define DANN_SEQ_HD inline
#endif

namespace dann {

struct SeqSummary {
    double S, A;
    int g;
};
constexpr int kSeqNone = 0x7FFFFFFF, kSeqBad = (int)0x80000000;

DANN_SEQ_HD int lsb_exp_f64(double v) {  // finite, non-zero
    const uint64_t b = (uint64_t)__builtin_bit_cast(long long, v);
    const int e = (int)((b >> 52) & 0x7FFu);
    uint64_t m = b & ((1ull << 52) - 1u);
    if (e == 0) return -1074 + (int)__builtin_ctzll(m);
    m |= 1ull << 52;
    return e - 1075 + (int)__builtin_ctzll(m);
}
DANN_SEQ_HD void seq_take(SeqSummary& s, double v) {
    s.S += v;
    s.A += __builtin_fabs(v);
    if (!(__builtin_fabs(v) < __builtin_inf())) s.g = kSeqBad;
    else if (v != 0.0 && s.g != kSeqBad) {
        const int g = lsb_exp_f64(v);
        s.g = g < s.g ? g : s.g;
    }
}
DANN_SEQ_HD SeqSummary seq_join(const SeqSummary& a, const SeqSummary& b) {
    SeqSummary r;
    r.S = a.S + b.S;
    r.A = a.A + b.A;
    r.g = (a.g == kSeqBad || b.g == kSeqBad) ? kSeqBad : (a.g < b.g ? a.g : b.g);
    return r;
}
DANN_SEQ_HD bool seq_exact(double acc, const SeqSummary& s) {
    if (s.g == kSeqBad || !(__builtin_fabs(acc) < __builtin_inf())) return false;
    int g = s.g;
    if (acc != 0.0) {
        const int ga = lsb_exp_f64(acc);
        g = ga < g ? ga : g;
    }
    if (g == kSeqNone) return true;  // nothing but zeros on a zero sum
    const double bound = (__builtin_fabs(acc) + s.A) * (1.0 + 0x1p-30);
    const int lim = g + 53;
    if (lim > 1023) return bound < __builtin_inf();
    if (lim < -1021) return false;
    return bound < __builtin_ldexp(1.0, lim);
}

// The medoid's column sums (medoid_kernels.hip): a column of nrows values is cut into ranges of kMedoidRangeRows rows
// and groups of kMedoidGroupRanges ranges.  The walk tests a whole group against the carry first, then each of its
// ranges; a range that fails is walked row by row.
constexpr uint32_t kMedoidRangeRows = 256, kMedoidGroupRanges = 64;

}  // namespace dann
