// build_scratch.h -- the persistent per-index scratch of the build path (idx->build_scratch; created by build_batch.hip's
// scratch_of, which is the only place that allocates it).  prune_gram.hip reaches the buffers of the matrix-core prune and
// the tile clock through it.
#pragma once

#include "dann_internal.h"

namespace dann {

struct BuildScratch {
    uint32_t batch_cap = 0, rec_stride = 0, pend_stride = 0, degree = 0;
    bool bootstrap_too_big = false;  // set when a batch needed the bootstrap with more members than its pool holds
    DevBuf slots, rec_ids, rec_d, rec_n, stats, pending, pending2, keys_in, keys_out, seg_start, seg_len, meta, sort_tmp;
    DevBuf counters;  // kStatStripes x 8 x u64, see PruneCfg::counters (accumulate over the index's lifetime)
    size_t sort_tmp_bytes = 0;
    // MFMA pool prune: sorted pools, Gram blocks and norms of one batch slice (grow-only)
    DevBuf g_sid, g_sd, g_sn, g_loc, g_gram, g_nrm, g_order;
    size_t g_sorted_elems = 0, g_items = 0, g_gram_elems = 0, g_nrm_elems = 0;
    // HIP-event time of the gram_tiles_kernel launches (dann_kernel_time, which = 5): pairs of events around every
    // launch on the build stream, resolved without ever making the build wait (a pair is read once it has completed,
    // or when the ring comes round to it -- hundreds of launches later)
    static constexpr uint32_t kTileEvents = 64;
    hipEvent_t tile_ev[2 * kTileEvents] = {};
    uint32_t tile_head = 0, tile_tail = 0;  // pairs [tail, head) are pending
    double tile_ms = 0.0;
    uint64_t tile_launches = 0;
    void tile_drain(bool all) {
        while (tile_tail != tile_head) {
            hipEvent_t e0 = tile_ev[2 * (tile_tail % kTileEvents)], e1 = tile_ev[2 * (tile_tail % kTileEvents) + 1];
            if (!all && tile_head - tile_tail < kTileEvents && hipEventQuery(e1) != hipSuccess) break;
            float ms = 0.f;
            if (hipEventSynchronize(e1) == hipSuccess && hipEventElapsedTime(&ms, e0, e1) == hipSuccess) {
                tile_ms += ms;
                tile_launches += 1;
            }
            ++tile_tail;
        }
    }
    int32_t tile_begin(hipStream_t st) {
        tile_drain(false);
        hipEvent_t& e0 = tile_ev[2 * (tile_head % kTileEvents)];
        hipEvent_t& e1 = tile_ev[2 * (tile_head % kTileEvents) + 1];
        if (!e0) DANN_HIP(hipEventCreate(&e0));
        if (!e1) DANN_HIP(hipEventCreate(&e1));
        DANN_HIP(hipEventRecord(e0, st));
        return DANN_OK;
    }
    int32_t tile_end(hipStream_t st) {
        DANN_HIP(hipEventRecord(tile_ev[2 * (tile_head % kTileEvents) + 1], st));
        ++tile_head;
        return DANN_OK;
    }
    // second stream of a commit: the few long back-edge lists of a batch (one wavefront each, a serial prune of hundreds
    // of candidates) run beside the short lists instead of holding the chip for themselves
    hipStream_t side = nullptr;
    int32_t side_stream(hipStream_t* out) {
        if (!side) DANN_HIP(hipStreamCreateWithFlags(&side, hipStreamNonBlocking));
        *out = side;
        return DANN_OK;
    }
    ~BuildScratch() {
        for (hipEvent_t e : tile_ev)
            if (e) (void)hipEventDestroy(e);
        if (side) (void)hipStreamDestroy(side);
    }
};

}  // namespace dann
