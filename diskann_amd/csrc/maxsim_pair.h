// maxsim_pair.h -- what every multi-vector scoring kernel (maxsim_kernels.hip, maxsim_mm_kernels.hip) does first and last:
// find the workgroup's (query, candidate) pair, settle the cases that take no arithmetic, and sum the Chamfer score.
#pragma once
#include <float.h>

#include "dann_device.h"
#include "dann_internal.h"

namespace dann {
namespace {

constexpr uint32_t kMsThreads = 256;   // four wavefronts: one 32-row query tile each
constexpr uint32_t kMsWaves = kMsThreads / 64;

struct MsPair {
    const uint8_t* q;    // the query's first row
    const uint8_t* d;    // the document's first row
    uint32_t q0;         // the query's first row, as an index into the call's query rows
    uint64_t d0;         // the document's first row, as an index into the set's rows
    uint32_t qn;         // query rows (<= kMaxSimQueryRows)
    uint64_t dn;         // document rows
    float* chamfer;      // the pair's Chamfer cell
    float* scores;       // the pair's qn score cells, or null
    bool live;           // false: nothing more to do for this workgroup (cells already written)
};

// Skipped candidates (0xFFFFFFFF) and ids >= ndocs write +infinity (the latter also raise the status word: DANN_EBOUNDS
// on the host -- an argument check INSTEAD of the read); an empty document writes f32::MAX scores and Chamfer 0.0.
__device__ __forceinline__ MsPair ms_pair(const MaxSimArgs& a) {
    const uint32_t c = blockIdx.x, qi = blockIdx.y;
    const uint32_t q0 = a.qoff[qi], qn = a.qoff[qi + 1] - q0;
    MsPair p;
    p.qn = qn;
    p.q0 = q0;
    p.q = a.qrows + (uint64_t)q0 * a.qstride;
    p.chamfer = a.out_chamfer + (uint64_t)qi * a.cand_stride + c;
    p.scores = a.out_scores ? a.out_scores + (uint64_t)q0 * a.cand_stride + (uint64_t)c * qn : nullptr;
    p.d = a.drows;
    p.d0 = 0;
    p.dn = 0;
    p.live = false;
    const uint32_t id = a.cand[(uint64_t)qi * a.cand_stride + c];
    float fill, cham;
    if (id == kEmpty || id >= a.ndocs) {
        if (id != kEmpty && threadIdx.x == 0) *a.status = 1u;  // (every writer writes the same word)
        fill = cham = __builtin_inff();
    } else {
        const uint64_t d0 = a.doff[id];
        p.d0 = d0;
        p.dn = a.doff[id + 1] - d0;
        p.d = a.drows + d0 * a.stride;
        if (p.dn != 0 && qn != 0) {
            p.live = true;
            return p;
        }
        fill = FLT_MAX;  // (qn == 0: no cell to fill)
        cham = 0.0f;
    }
    if (p.scores)
        for (uint32_t i = threadIdx.x; i < qn; i += blockDim.x) p.scores[i] = fill;
    if (threadIdx.x == 0) *p.chamfer = cham;
    return p;
}

// Chamfer::evaluate (fallback.rs:196-204): one lane, query-row order, from 0.0 -- not a tree, not an atomic
__device__ __forceinline__ void ms_chamfer(const MsPair& p, const float* sc) {
    __syncthreads();
    if (threadIdx.x == 0) {
        float sum = 0.0f;
        for (uint32_t i = 0; i < p.qn; ++i) sum += sc[i];
        *p.chamfer = sum;
    }
}

}  // namespace
}  // namespace dann
