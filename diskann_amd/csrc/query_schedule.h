// query_schedule.h -- the slot map of a locality-scheduled search launch (query_schedule.hip), shared by the kernels and
// the host test (tests/test_query_schedule_host.py).
//
// A launch's queries are sorted by their nearest pivot; the sorted order is cut into `parts` contiguous chunks whose
// sizes differ by at most one (the first n % parts chunks take one more), and slot s runs chunk s % parts, entry
// s / parts.  One-wave launches deal workgroup s to XCD (s + c) % 8 (an observed dealing, relied on for speed only): with
// parts = 8 each XCD walks its own chunk in sorted order.  Persistent launches (waves draw slots from one counter) use
// parts = 1: slot s runs sorted entry s.  Both directions are bijections on [0, n).
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define DANN_SCHED_FN __host__ __device__ inline
#else
#define DANN_SCHED_FN inline
#endif

namespace dann {

// sorted position that slot s runs
DANN_SCHED_FN uint32_t sched_source(uint32_t s, uint32_t n, uint32_t parts) {
    const uint32_t q = n / parts, r = n % parts, x = s % parts;
    return x * q + (x < r ? x : r) + s / parts;
}

// slot that runs sorted position p (the inverse of sched_source)
DANN_SCHED_FN uint32_t sched_slot(uint32_t p, uint32_t n, uint32_t parts) {
    const uint32_t q = n / parts, r = n % parts, big = r * (q + 1u);  // positions in the r chunks of q + 1
    const uint32_t x = p < big ? p / (q + 1u) : r + (p - big) / q;
    const uint32_t j = p < big ? p % (q + 1u) : (p - big) % q;
    return j * parts + x;
}

}  // namespace dann
