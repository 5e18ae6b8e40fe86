// The shape of a beam-search launch as host and kernels both compute it: the LDS layouts of the three kernel families
// (search_kernel_impl.h, search_pair_impl.h, search_pq_impl.h), which launches each family serves, and the constants
// they read.  Everything lives in an anonymous namespace, like the kernel headers that include it.  No HIP here:
// tests/test_launch_plan_host.py compiles it with g++.
#pragma once
#include <stdint.h>

#include <algorithm>

#include "row_types.h"
#include "search_args.h"

namespace dann {
namespace {

constexpr int kWave = 64;
constexpr int kMaxBeam = 16;
constexpr uint32_t kTuneRowPrefetch = 1u;  // SearchArgs::tune bits
constexpr uint32_t kTuneNoSpeculation = 2u;  // teams: no speculative expansion of the predicted next node
constexpr uint32_t kTuneNoSelfStart = 4u;    // teams: the visited wave always waits for the control wave's words

constexpr uint32_t kAdjLandBytes = 256u;
struct SearchLds {
    uint32_t ht_off, cand_id_off, cand_d_off, cand2_id_off, cand2_d_off, adj_off, slots_off, mscr_off, mail_off, stage_off, snew_off, beam_off, q_off, total;
};

DANN_HD inline uint32_t round16(uint32_t x) { return (x + 15u) & ~15u; }
// entries of the queue image in LDS: the largest capacity the queue can have during the search
DANN_HD inline uint32_t lds_queue_entries(const SearchArgs& a) {
    const uint32_t q = a.l_value + a.ix.nstart;
    return q > a.qcap_max ? q : a.qcap_max;
}

// bytes of the staged query: f32 vector (float rows), raw bytes (integer rows), lookup table (PQ rows)
DANN_HD inline uint32_t query_lds_bytes(const IndexView& ix) {
    if (ix.dtype == DT_PQ) return ix.pq_chunks * 1024u;
    if (ix.dtype == DT_U8 || ix.dtype == DT_I8 || dt_is_sq(ix.dtype) || dt_is_sph(ix.dtype)) return ix.qbytes;
    if (dt_mm_rows(ix.dtype)) return mm_slot_bytes(ix.dtype, ix.qbytes);
    return ix.dim * 4u;
}

// The queue image and the visited table come last, in that order: every other region then sits at an offset that
// depends only on (cmax, query bytes) -- compile-time constants in the plain fixed-length instantiations, where the
// region pointers cost no SGPRs and the LDS instructions carry immediate offsets; the image is sized by the queue's
// real capacity `qcap` (L + start points, or what AdaptiveL may grow it to), not by its register slots, so the table's
// offset is the one run-time offset.  (Every byte counts: at 1 M x 128-byte rows the table caps the queries per CU.)
DANN_HD inline SearchLds search_lds_layout(uint32_t ht_entries, uint32_t cmax, uint32_t qcap,
                                                       uint32_t qbytes, bool team = false) {
    SearchLds l;
    uint32_t off = 0;
    l.q_off = off;
    off += round16(qbytes);
    l.cand_id_off = off;
    off += round16(cmax * 4u);
    l.cand_d_off = off;
    off += round16(cmax * 4u);
    // teams: a second candidate buffer -- the visited wave fills it with the next hop's candidates while the gather wave
    // still evaluates the current hop's (the speculative expansion of the predicted next node, §3.5 of DESIGN.md)
    l.cand2_id_off = off;
    if (team) off += round16(cmax * 4u);
    l.cand2_d_off = off;
    if (team) off += round16(cmax * 4u);
    // teams: two landing buffers of 64 dwords for adjacency rows requested ahead of their use (length + at most 63
    // neighbours each; the loads write LDS directly, see adj_fetch_lds)
    l.adj_off = off;
    if (team) off += 2u * kAdjLandBytes;
    // teams: the table slots of the visited wave's speculative inserts (wave 0 takes them back through these), and 64
    // (id, distance) words of scratch for wave 0's merge (the candidate buffer it merges from is already being refilled)
    l.slots_off = off;
    if (team) off += 256u;
    l.mscr_off = off;
    if (team) off += 512u;
    l.mail_off = off;  // teams: the mailbox the four waves of a team talk through (64 words, see kMb*)
    if (team) off += 256u;
    l.beam_off = off;
    off += round16(kMaxBeam * 4u);
    l.stage_off = off;  // the queue image, (id, distance bits) pairs: every merge scatters the register-resident queue
    off += round16(qcap * 8u);  // here and reloads it (one 8-byte LDS access per entry).  One buffer is enough: nothing
                                // is read from it between the first scatter write and the reload (ranks come from
                                // registers or were taken before), and one wave's LDS operations retire in order.
    l.snew_off = l.cand_id_off;  // (unused: the slow merge keeps its sorted survivors in the candidates' own buffer)
    l.ht_off = off;        // 16-byte aligned (wiped with 16-byte stores)
    off += ht_entries * 4u;  // any multiple of 64
    l.total = off;
    return l;
}

// what kModePlain assumes (checked by the host for every launch)
inline bool plain_mode(const SearchArgs& a) {
    return !a.filter_mode && a.beam_width == 1 && a.ix.tag_off == 0 && a.ix.max_degree <= (uint32_t)kWave &&
           a.ix.nstart <= (uint32_t)kWave;
}

// does a team instantiation exist for this launch?  (launch_one: plain mode, a fixed-length kernel -- 128-element rows
// of the metric's specialised form --, at most 256 queue entries, not PQ rows; row_dispatch.h search_dim128_defined)
inline bool team_shape(const SearchArgs& a) {
    int op;
    bool norm;
    const int dt = a.ix.dtype;
    if (!plain_mode(a) || dt == DT_PQ || dt_is_packed(dt) || dt_mm_rows(dt) || a.ix.dim != 128u || !resolve_metric(dt, a.ix.metric, &op, &norm)) return false;
    if (std::max(a.l_value + a.ix.nstart, a.qcap_max) > 256u) return false;
    const bool ints = dt == DT_U8 || dt == DT_I8 || dt == DT_SQ8;
    if (op == OP_L2) return true;
    if (op == OP_IP) return ints;  // (float rows: inner product and CosineNormalized run the generic-length kernel)
    return dt == DT_U8 || dt == DT_I8;
}

inline uint32_t cmax_of(const SearchArgs& a) {
    uint32_t c1 = (a.beam_width * a.ix.max_degree + 63u) & ~63u, c2 = (a.ix.nstart + 63u) & ~63u;
    return c1 > c2 ? c1 : c2;
}
inline uint32_t qs_of(uint32_t qcap) { return qcap <= 64 ? 1 : qcap <= 128 ? 2 : qcap <= 256 ? 4 : qcap <= 512 ? 8 : 16; }

// ---- two queries per wavefront (search_pair_impl.h) ----
constexpr uint32_t kPairHalf = 32;
// LDS of one half: candidates (ids, distances), the scatter buffer of the merge ((id, distance) pairs), the queue's
// distances in order (what the lower-bound searches read), the survivors' distances of one merge, a sink for the
// stores of lanes that have nothing to store, the visited table.  QE = queue entries per lane (1: L + start points <=
// 32, 2: <= 64), RE = adjacency ids per lane (1: degree <= 32, 2: <= 64).
struct PairLds {
    uint32_t cand_id_off, cand_d_off, stage_off, qimg_off, qpiv_off, sd_off, sink_off, ht_off, ov_off, half_bytes;
};
// keys of the queue image: a power of two beyond the queue's entries (the lower-bound search needs no bound check)
DANN_HD inline uint32_t pair_qimg_keys(uint32_t qe) { return qe == 1u ? 64u : 128u; }
DANN_HD inline PairLds pair_lds_layout(uint32_t qe, uint32_t re, uint32_t ht_words, uint32_t ov_words) {
    PairLds l;
    l.cand_id_off = 0;
    l.cand_d_off = 128u * re;
    uint32_t off = 256u * re;
    if (re == 1u) {
        // one pass per hop: the scatter buffer of the merge takes the candidates' place -- they are in registers by then
        l.stage_off = 0;
        off = 256u * qe > off ? 256u * qe : off;
    } else {
        // two passes per hop: the second pass's candidates are still in their buffer when the first pass is merged
        l.stage_off = off;
        off += 256u * qe;
    }
    l.qimg_off = off;  // the entries beyond the queue stay "empty" = larger than every distance
    off += 4u * pair_qimg_keys(qe);
    l.qpiv_off = off;  // one queue entry per lane: the last key of each eighth of the queue image (first level of the
    off += 32u;        // lower-bound search); 32 bytes
    l.sd_off = off;
    off += 128u;
    l.sink_off = off;  // one dword per lane (stores of many lanes to ONE address serialise like a bank conflict); the
    off += 128u;       // 8-byte stores of the merge's scatter sink into [sd, sink + 128): the survivors' keys are dead by then
    l.ht_off = off;
    l.ov_off = l.ht_off + ht_words * 4u;  // the overflow table of the 16-bit table (ov_insert; 0 words: none)
    l.half_bytes = l.ov_off + ov_words * 4u;
    return l;
}
// the instantiation a launch takes: queue entries per lane = ceil((L + start points) / 32) (1 .. 3), two adjacency ids per
// lane beyond degree 32 (which comes with at least two queue entries per lane: five instantiations per metric, not six)
DANN_HD inline uint32_t pair_re(const SearchArgs& a) { return a.ix.max_degree > kPairHalf ? 2u : 1u; }
DANN_HD inline uint32_t pair_qe(const SearchArgs& a) {
    const uint32_t q = (a.l_value + a.ix.nstart + kPairHalf - 1u) / kPairHalf;
    return (q < 2u && pair_re(a) == 2u) ? 2u : (q ? q : 1u);
}

// what the pair kernel serves (host side; the table geometry is checked by the caller)
inline bool pair_shape(const SearchArgs& a) {
    const int dt = a.ix.dtype;
    return plain_mode(a) && !a.team && !a.grid && !a.srv.ring && !a.rec_ids && !a.range_ids && !a.qslots && a.out_ids &&
           (dt == DT_U8 || dt == DT_I8 || dt == DT_SQ8) && a.ix.dim == 128u && a.l_value + a.ix.nstart <= 3u * kPairHalf &&
           a.ix.max_degree <= 2u * kPairHalf && a.ix.nstart >= 1u && a.ix.nstart <= kPairHalf && a.ix.row_stride % 16u == 0u;
}

// ---- PQ rows with the lookup table in registers (search_pq_impl.h) ----
constexpr uint32_t kPqLutChunks = 64;  // chunks the register-resident table covers at most (4 registers each)
// groups of 16 chunks = code-row dwordx4 loads = 64 table registers: the instantiation a chunk count takes
DANN_HD inline uint32_t pq_lut_groups(uint32_t chunks) { return (chunks + 15u) / 16u; }

// LDS of one query: the queue image ((id, distance) pairs: the merge scatters the register-resident queue here and
// reloads it), two 64-word buffers of the merge's slow path, the visited table
struct PqLds {
    uint32_t stage_off, cbi_off, cbd_off, ht_off, total;
};
// (ov_words: the overflow table of the 16-bit table directly behind it -- ov_insert, search_pair_impl.h)
DANN_HD inline PqLds pq_lds_layout(uint32_t qs, uint32_t ht_words, uint32_t ov_words) {
    PqLds l;
    l.stage_off = 0;
    l.cbi_off = qs * 64u * 8u;
    l.cbd_off = l.cbi_off + 256u;
    l.ht_off = l.cbd_off + 256u;
    l.total = l.ht_off + (ht_words + ov_words) * 4u;
    return l;
}

// what pq_search_kernel serves (host side; the table geometry is checked by the caller)
inline bool pq_lut_shape(const SearchArgs& a) {
    return a.ix.dtype == DT_PQ && plain_mode(a) && !a.team && !a.grid && !a.srv.ring && !a.rec_ids && !a.range_ids &&
           !a.qslots && a.out_ids && a.ix.pq_chunks <= kPqLutChunks && a.ix.row_stride % 16u == 0u &&
           a.ix.row_stride >= 16u * pq_lut_groups(a.ix.pq_chunks) &&
           std::max(a.l_value + a.ix.nstart, a.qcap_max) <= 4u * (uint32_t)kWave && a.ix.nstart >= 1u &&
           (a.ix.metric == M_L2 || a.ix.metric == M_IP);
}
inline uint32_t pq_lut_qs(const SearchArgs& a) {
    const uint32_t q = a.l_value + a.ix.nstart;
    return q <= 64u ? 1u : q <= 128u ? 2u : 4u;
}
// queries per CU the registers of a table size allow
inline uint32_t pq_lut_waves_per_cu(uint32_t chunks) {
    const uint32_t g = pq_lut_groups(chunks);
    return g <= 1u ? 16u : g <= 3u ? 8u : 4u;
}

}  // namespace
}  // namespace dann
