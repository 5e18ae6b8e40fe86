// wave_lists.h -- wave-level list helpers of the kernels that build, sort and compact id lists: the slot-bitmap test and
// the tag values of the deleted state, the lock-free appends of the mutation kernels (consolidate.hip,
// inplace_delete.hip), and the (distance, payload) sort key with its in-LDS bitonic sort (also prune_rows.hip, prune_gram.hip,
// distance_kernels.hip, maxsim_kernels.hip).  The search kernels keep their own ordered_bits / wave_sort_keys
// (search_kernel_impl.h): no -0.0 fold there, and a sort of global memory.
#pragma once

#include "dann_device.h"

namespace dann {
namespace {

// inline concurrency tags (diskann-inmem/src/tag.rs:81-135)
constexpr uint8_t kTagRetiring = 2;    // Tag::RETIRING: not readable
constexpr uint8_t kTagReadable = 254;  // Tag::can_read: tag >= PUBLISHED

// one bit per slot (the deleted bitmap, a call's own marks): is `id` a slot whose bit is set?  A null bitmap has none.
__device__ __forceinline__ bool in_bitmap(const uint32_t* bm, uint32_t id, uint32_t nslots) {
    return bm && id < nslots && ((bm[id >> 5] >> (id & 31u)) & 1u);
}

// append this lane's value to list[*count ..] with one atomic per wavefront
__device__ __forceinline__ void wave_push(bool p, uint32_t* list, uint32_t* count, uint32_t value) {
    const uint64_t m = ballot64(p);
    if (m == 0) return;
    const uint32_t leader = (uint32_t)__ffsll((unsigned long long)m) - 1u;
    uint32_t base = 0;
    if (lane_id() == leader) base = atomicAdd(count, (uint32_t)__popcll(m));
    base = (uint32_t)__shfl((int)base, (int)leader);
    if (p) list[base + mbcnt(m)] = value;
}

// Appends the lanes' ids (kEmpty = none) that are not yet in the pool -- an id repeated among the lanes goes in once, from
// its lowest lane: list order -- and returns the new length.  `hash` (hmask + 1 entries, kEmpty = free, at most half full)
// is the set of the pool's ids: one probe sequence per new candidate instead of a scan of the pool.
__device__ __forceinline__ uint32_t append_unique(uint32_t* pool, uint32_t* hash, uint32_t hmask, uint32_t cnt, uint32_t pcap,
                                                  uint32_t id, uint32_t* err) {
    const uint32_t lane = lane_id();
    bool take = id != kEmpty;
    for (int k = 0; k < 64; ++k) {
        const uint32_t o = (uint32_t)__shfl((int)id, k);
        take &= !((uint32_t)k < lane && o == id);
    }
    if (take) {
        uint32_t h = (id * 2654435761u) & hmask;
        for (uint32_t probe = 0; probe <= hmask; ++probe) {
            const uint32_t old = atomicCAS(&hash[h], kEmpty, id);
            if (old == kEmpty) break;
            if (old == id) {
                take = false;
                break;
            }
            h = (h + 1u) & hmask;
        }
    }
    const uint64_t tm = ballot64(take);
    const uint32_t pos = cnt + mbcnt(tm);
    if (take) {
        if (pos < pcap) pool[pos] = id;
        else atomicOr(err, 1u);
    }
    return min(cnt + (uint32_t)__popcll(tm), pcap);
}

// 64-bit sort key: the order-preserving bits of d above a payload (a pool position) that breaks ties
__device__ __forceinline__ uint64_t dist_key(float d, uint32_t payload) {
    uint32_t u = __builtin_bit_cast(uint32_t, d + 0.0f);  // -0.0 -> +0.0: `<` treats them as equal
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ((uint64_t)u << 32) | payload;
}

// the distance a key was made of; -0.0 comes back as +0.0, every other non-NaN value as its own bits
__device__ __forceinline__ float key_dist(uint64_t key) {
    const uint32_t u = (uint32_t)(key >> 32);
    return __builtin_bit_cast(float, (u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u);
}

// ascending bitonic sort of the 64-bit keys[0, P) in LDS, P a power of two, by one workgroup of `nthreads` threads (a
// kernel that is only ever launched with one size names it: the stride is then a constant, not a load)
template <class K>
__device__ void block_bitonic(K* keys, uint32_t P, uint32_t nthreads = blockDim.x) {
    for (uint32_t k = 2; k <= P; k <<= 1)
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t t = threadIdx.x; t < (P >> 1); t += nthreads) {
                const uint32_t i = ((t & ~(j - 1u)) << 1) | (t & (j - 1u)), p = i | j;
                const K x = keys[i], y = keys[p];
                if ((x > y) == ((i & k) == 0)) {
                    keys[i] = y;
                    keys[p] = x;
                }
            }
            __syncthreads();
        }
}

}  // namespace
}  // namespace dann
