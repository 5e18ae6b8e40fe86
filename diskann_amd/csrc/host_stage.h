// host_stage.h -- the staging loop of the host-pointer entry points.  The per-query inputs of a call go from host memory
// to one block of a context's arena (SearchCtx::stage[4]) in pieces, the caller runs something on the piece's device
// buffers, and the per-query outputs and stats come back to host + off * bytes_per_query; one stream synchronisation per
// piece.  No hipMalloc / hipFree per call: a hipFree synchronises the whole device and would serialise concurrent callers.
#pragma once
#include <string.h>

#include <algorithm>
#include <initializer_list>
#include <vector>

#include "dann_internal.h"

namespace dann {

// a block of a context's arena, carved into 256-byte aligned pieces
struct Carve {
    size_t off = 0;
    size_t take(size_t bytes) {
        const size_t o = off;
        off = (off + bytes + 255) & ~(size_t)255;
        return o;
    }
};

// The arena stays resident between calls only up to this size: a call with per-query filter bitmaps on a large index can
// need gigabytes, and an index that nearly fills HBM would miss them in its next build or search (the pool keeps up to 16
// contexts).  Beyond it the block is released when the call returns (a hipFree synchronises the device: the price of a
// call that large, not of every call).
constexpr size_t kArenaKeepBytes = (size_t)256 << 20;
struct ArenaTrim {
    SearchCtx& ctx;
    ~ArenaTrim() {
        if (ctx.stage_bytes[4] > kArenaKeepBytes) {
            (void)hipStreamSynchronize(ctx.stream);
            (void)hipFree(ctx.stage[4]);
            ctx.stage[4] = nullptr;
            ctx.stage_bytes[4] = 0;
        }
    }
};

struct HostStage {
    struct In {
        const void* host;
        size_t bytes;  // per query
    };
    struct Out {
        void* host;    // null: laid out for the kernels, not copied back
        size_t bytes;  // per query
    };
    // the per-query stats: none; copied to out_stats when the caller passed one; or always fetched, mirrored to out_stats
    // and checked, the walk stopping at the first non-zero status
    enum Stats { kNoStats, kCopyStats, kCheckStats };
    static constexpr size_t kMaxIn = 2, kMaxOut = 3, kMaxExtra = 8;

    // Lay out `inputs | outputs | stats | extras` for pieces of at most `piece` queries and grow the arena to hold them.
    // Every input keeps a 16-byte tail (the kernels read a query's tail with whole vector loads); `extra`: whole-call
    // sizes in bytes.
    int32_t layout(SearchCtx& ctx, uint32_t nq, uint32_t piece, std::initializer_list<In> in, std::initializer_list<Out> out,
                   Stats stats, std::initializer_list<size_t> extra = {}) {
        if (in.size() > kMaxIn || out.size() > kMaxOut || extra.size() > kMaxExtra) return DANN_EINVAL;
        ctx_ = &ctx, nq_ = nq, piece_ = std::max(1u, std::min(piece, nq)), stats_ = stats;
        Carve cv;
        for (const In& i : in) in_[nin_] = i, o_in_[nin_++] = cv.take((size_t)piece_ * i.bytes + 16);
        for (const Out& o : out) out_[nout_] = o, o_out_[nout_++] = cv.take((size_t)piece_ * o.bytes);
        if (stats != kNoStats) o_stats_ = cv.take((size_t)piece_ * sizeof(dann_search_stats));
        size_t* o_x = o_extra_;
        for (size_t bytes : extra) *o_x++ = cv.take(bytes);
        return grow_stage(ctx, 4, cv.off);
    }

    // the device buffers of the piece in flight
    template <class T = void>
    T* in(int i) const { return at<T>(o_in_[i]); }
    template <class T>
    T* out(int i) const { return at<T>(o_out_[i]); }
    template <class T>
    T* extra(int i) const { return at<T>(o_extra_[i]); }
    dann_search_stats* stats() const { return stats_ != kNoStats ? at<dann_search_stats>(o_stats_) : nullptr; }

    // Walk the call: per piece H2D the inputs, run(off, m) on ctx.stream, D2H the outputs and stats, synchronise.
    // kCheckStats: *first_bad = the first query of the call whose status is non-zero (the walk ends with its piece), or
    // nq; what an exhausted query means is the caller's to say.
    template <class Run>
    int32_t walk(dann_search_stats* out_stats, uint32_t* first_bad, Run&& run) {
        hipStream_t st = ctx_->stream;
        std::vector<dann_search_stats> checked(stats_ == kCheckStats ? piece_ : 0);
        for (uint32_t off = 0; off < nq_; off += piece_) {
            const uint32_t m = std::min(piece_, nq_ - off);
            for (int i = 0; i < nin_; ++i)
                DANN_HIP(hipMemcpyAsync(at<void>(o_in_[i]), static_cast<const uint8_t*>(in_[i].host) + (size_t)off * in_[i].bytes,
                                        (size_t)m * in_[i].bytes, hipMemcpyHostToDevice, st));
            if (int32_t rc = run(off, m)) return rc;
            for (int i = 0; i < nout_; ++i)
                if (out_[i].host)
                    DANN_HIP(hipMemcpyAsync(static_cast<uint8_t*>(out_[i].host) + (size_t)off * out_[i].bytes, at<void>(o_out_[i]),
                                            (size_t)m * out_[i].bytes, hipMemcpyDeviceToHost, st));
            dann_search_stats* const h_stats = stats_ == kCheckStats ? checked.data() : out_stats ? out_stats + off : nullptr;
            if (stats_ != kNoStats && h_stats)
                DANN_HIP(hipMemcpyAsync(h_stats, stats(), (size_t)m * sizeof(dann_search_stats), hipMemcpyDeviceToHost, st));
            DANN_HIP(hipStreamSynchronize(st));
            if (stats_ != kCheckStats) continue;
            if (out_stats) memcpy(out_stats + off, checked.data(), (size_t)m * sizeof(dann_search_stats));
            for (uint32_t i = 0; i < m; ++i)
                if (checked[i].status) {
                    *first_bad = off + i;
                    return DANN_OK;
                }
        }
        if (first_bad) *first_bad = nq_;
        return DANN_OK;
    }

  private:
    template <class T>
    T* at(size_t off) const { return reinterpret_cast<T*>(static_cast<uint8_t*>(ctx_->stage[4]) + off); }
    SearchCtx* ctx_ = nullptr;
    uint32_t nq_ = 0, piece_ = 1;
    Stats stats_ = kNoStats;
    int nin_ = 0, nout_ = 0;
    In in_[kMaxIn];
    Out out_[kMaxOut];
    size_t o_in_[kMaxIn] = {}, o_out_[kMaxOut] = {}, o_extra_[kMaxExtra] = {}, o_stats_ = 0;
};

}  // namespace dann
