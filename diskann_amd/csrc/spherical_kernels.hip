// spherical_kernels.hip -- SphericalQuantizer::compress_into on the GPU, device to device: the data side
// (spherical::Data<1 | 2 | 4>) and the two query sides (Query<4, BitTranspose> for 1-bit rows, Query<2 | 4, Dense>),
// byte for byte the reference's code as it runs (diskann-quantization/src/spherical/quantizer.rs: preprocess :338-381,
// data :805-861, the 1-bit finish :596-647, compress_via_maximum_cosine :871-918, maximize_cosine_similarity :991-1100
// over SliceHeap algorithms/heap.rs:69-187, queries :1128-1212).  No operation is fused (-ffp-contract=off) except the
// one the reference fuses (mul_add, written fmaf); divisions and square roots are the correctly rounded ones.
//
// Three stages per chunk of rows:
//   spherical_pre_kernel     a group of 8 lanes per row: mul (cosine: 1 / FastL2Norm(x)), shifted = mul * x - shift,
//                            shifted_norm and <shifted, shift> through the f32 inner product's V3 order (FAcc / finish_vec
//                            of dann_device.h), the row divided by its norm into a packed scratch, {shifted_norm,
//                            metric_specific} beside it
//   launch_transform         transform_kernels.hip (a NullTransform is skipped: the scratch is the transformed row);
//                            spherical_tnorm_kernel then forms FastL2Norm(transformed) where the transform does not
//                            preserve norms
//   spherical_*_kernel       one row per lane, as minmax_compress_kernel: everything that is left is order-bound -- the
//                            sequential f32 sums, the min/max fold, and for 2 and 4 bits the heap walk of the maximiser
// The heap holds an f32 critical value and a u16 position per entry, plus `rounded` (u16 per position): 8 bytes per
// element, interleaved by lane so that the bank of every access is the lane's whatever entry it is at -- dword
// entry * 64 + lane for the values, and for the u16 arrays half (e & 1) of dword (e >> 1) * 64 + lane.  One wavefront per
// block; its 512 * output_dim bytes sit in LDS up to output_dim = kSphLdsDim (128 of the 160 KiB), beyond that in a global
// scratch of the same layout.
#include <math.h>

#include <cmath>

#include <memory>

#include "dann_device.h"
#include "dann_internal.h"
#include "transform.h"

struct dann_spherical {
    int device = 0;
    int32_t metric = 0;
    float pre_scale = 1.0f;
    float shift_norm_sq = 0.0f;
    dann_transform t;  // the handle's own copy of the caller's transform
    float* d_shift = nullptr;
    ~dann_spherical() {
        if (d_shift) (void)hipFree(d_shift);
    }
};

namespace dann {
namespace {

constexpr uint32_t kSphLdsDim = 256u;  // 512 bytes per element and wavefront: 128 of the 160 KiB
constexpr size_t kSphChunkBytes = (size_t)256 << 20;  // scratch of one chunk of rows
enum : uint32_t { kFlagNaN = 1u, kFlagIpc = 2u, kFlagMs = 4u, kFlagBitSum = 8u };
enum : int { kData = 0, kQueryDense = 1, kQueryTransposed = 2 };

// InnerProduct::evaluate(x, y) for f32 slices in the V3 order (Strategy4x1: four f32x8 accumulators), by a group of 8
// lanes: group_distance_raw<4, OP_IP> with the elements taken from functors.  Every lane of the wavefront is here (the
// combine is DPP); valid in lane v == 0 of the group.
template <class FX, class FY>
__device__ __forceinline__ float group_ip_v3(FX&& fx, FY&& fy, uint32_t dim, uint32_t v) {
    const uint32_t full_end = dim & ~7u, rem = dim & 7u;
    FAcc<OP_IP> acc;
    acc.init();
    for (uint32_t e = 4u * v; e < full_end; e += 32u) {
        const F4 a{fx(e), fx(e + 1u), fx(e + 2u), fx(e + 3u)}, b{fy(e), fy(e + 1u), fy(e + 2u), fy(e + 3u)};
        acc.step(a, b);
    }
    return finish_vec<4>(acc.s, [&](float(&a)[4]) {
        if (rem == 0) return;
#pragma unroll
        for (uint32_t i = 0; i < 4u; ++i) {
            const uint32_t l = 4u * (v & 1u) + i;
            float x = 0.0f, y = 0.0f;
            if (l < rem) {
                x = fx(full_end + l);
                y = fy(full_end + l);
            }
            a[i] = __builtin_fmaf(x, y, a[i]);
        }
    });
}
// the group's value (lane v == 0) in every lane of the group
__device__ __forceinline__ float group_bcast(float x) { return __shfl(x, (int)(lane_id() & ~7u), 64); }
__device__ __forceinline__ bool finite_f32(float x) { return __builtin_fabsf(x) < __builtin_inff(); }  // (false for NaN)

// preprocess (quantizer.rs:338-381) and the division by shifted_norm (:823-826 / :1145-1148)
__global__ __launch_bounds__(256) void spherical_pre_kernel(const float* __restrict__ x, uint64_t xs, uint32_t n,
                                                            uint32_t dim, const float* __restrict__ shift,
                                                            float pre_scale, int32_t metric, float* __restrict__ out,
                                                            float2* __restrict__ meta, uint32_t* flag) {
    const uint32_t tid = blockIdx.x * 256u + threadIdx.x, v = tid & 7u;
    uint32_t row = tid >> 3;
    const bool live = row < n;
    if (!live) row = n - 1u;
    const float* xr = x + (uint64_t)row * xs;
    auto xe = [&](uint32_t e) { return xr[e]; };
    auto se = [&](uint32_t e) { return shift[e]; };
    float mul = pre_scale;
    if (metric == M_COSINE) {
        const float norm = __builtin_sqrtf(group_bcast(group_ip_v3(xe, xe, dim, v)));
        mul = norm == 0.0f ? 1.0f : 1.0f / norm;
    }
    auto sh = [&](uint32_t e) { return mul * xr[e] - shift[e]; };
    const float sn = __builtin_sqrtf(group_bcast(group_ip_v3(sh, sh, dim, v)));
    float ms = sn * sn;
    if (metric != M_L2) ms = group_bcast(group_ip_v3(sh, se, dim, v));
    if (!live) return;
    const bool ok = finite_f32(sn);
    const bool zero = !ok || sn == 0.0f;
    float* dst = out + (uint64_t)row * dim;
    for (uint32_t e = v; e < dim; e += 8u) dst[e] = zero ? 0.0f : sh(e) / sn;
    if (v == 0) {
        meta[row] = make_float2(sn, ms);
        if (!ok) atomicOr(flag, kFlagNaN);  // InputContainsNaN
    }
}

// FastL2Norm (root) or FastL2NormSquared of n packed rows
__global__ __launch_bounds__(256) void spherical_tnorm_kernel(const float* __restrict__ t, uint32_t n, uint32_t dim,
                                                              int32_t root, float* __restrict__ out) {
    const uint32_t tid = blockIdx.x * 256u + threadIdx.x, v = tid & 7u;
    uint32_t row = tid >> 3;
    const bool live = row < n;
    if (!live) row = n - 1u;
    const float* tr = t + (uint64_t)row * dim;
    auto te = [&](uint32_t e) { return tr[e]; };
    const float sq = group_ip_v3(te, te, dim, v);
    if (live && v == 0) out[row] = root ? __builtin_sqrtf(sq) : sq;
}

// cast_f32_to_f16 (round to nearest even) and DataMeta::new (vectors.rs:265-290)
__device__ __forceinline__ uint16_t f16_bits(float x, bool* finite) {
    const uint16_t b = __half_as_ushort(__float2half_rn(x));
    *finite = (b & 0x7C00u) != 0x7C00u;
    return b;
}
__device__ __forceinline__ void write_data_meta(uint8_t* at, float ipc, float ms, uint32_t bit_sum, uint32_t* flag) {
    bool ok_ipc, ok_ms;
    const uint16_t m[3] = {f16_bits(ipc, &ok_ipc), f16_bits(ms, &ok_ms), (uint16_t)bit_sum};
    __builtin_memcpy(at, m, 6);
    const uint32_t bad = (ok_ipc ? 0u : kFlagIpc) | (ok_ms ? 0u : kFlagMs) | (bit_sum > 0xFFFFu ? kFlagBitSum : 0u);
    if (bad) atomicOr(flag, bad);
}

struct FinArgs {
    const float* t;      // n packed transformed rows
    const float2* meta;  // {shifted_norm, metric_specific}
    const float* tnorm;  // null: the transform preserves norms (1.0)
    uint32_t n, dim;
    uint8_t* out;  // n zeroed packed images
    uint32_t image_bytes;
    uint32_t* heap;  // null: the heap is in LDS
    uint32_t* flag;
};

// the row of this lane, or null for no row / a row at the centroid / a row whose norm is not finite (its image stays zero)
__device__ __forceinline__ const float* fin_row(const FinArgs& a, uint32_t* r, float2* m) {
    *r = blockIdx.x * 64u + threadIdx.x;
    if (*r >= a.n) return nullptr;
    *m = a.meta[*r];
    if (!finite_f32(m->x) || m->x == 0.0f) return nullptr;
    return a.t + (uint64_t)*r * a.dim;
}

// FinishCompressing for DataMut<1> (quantizer.rs:596-647)
__global__ __launch_bounds__(64) void spherical_data1_kernel(FinArgs a) {
    uint32_t r;
    float2 m;
    const float* t = fin_row(a, &r, &m);
    if (!t) return;
    uint8_t* img = a.out + (uint64_t)r * a.image_bytes;
    float sum = 0.0f;
    uint32_t bit_sum = 0;
    for (uint32_t i = 0; i < a.dim; ++i) {
        const float e = t[i];
        const uint32_t bit = e > 0.0f ? 1u : 0u;
        sum += __builtin_fabsf(e);
        bit_sum += bit;
        img[i >> 3] |= (uint8_t)(bit << (i & 7u));
    }
    const float tn = a.tnorm ? a.tnorm[r] : 1.0f;
    const float ipc = ((2.0f * tn) * m.x) / sum;
    write_data_meta(img + sq_code_bytes(DT_SPH1, a.dim), ipc, m.y, bit_sum, a.flag);
}

// SliceHeap over Pair (heap.rs:69-187, quantizer.rs:933-958) in the lane-interleaved layout.  Pair's Ord is reversed and
// a NaN compares equal: x <= y is !(y.value > x.value), x >= y is !(y.value < x.value), x < y is y.value < x.value.
struct LaneHeap {
    float* val;
    uint16_t* pos;
    uint16_t* rnd;
    uint32_t len, lane;
    __device__ __forceinline__ uint32_t at32(uint32_t e) const { return e * 64u + lane; }
    __device__ __forceinline__ uint32_t at16(uint32_t e) const { return (((e >> 1) * 64u + lane) << 1) | (e & 1u); }
    __device__ __forceinline__ void swap(uint32_t x, uint32_t y) {
        const float v = val[at32(x)];
        val[at32(x)] = val[at32(y)];
        val[at32(y)] = v;
        const uint16_t p = pos[at16(x)];
        pos[at16(x)] = pos[at16(y)];
        pos[at16(y)] = p;
    }
    __device__ __forceinline__ void sift_down(uint32_t p) {
        uint32_t child = 2u * p + 1u;
        const uint32_t lim = len >= 2u ? len - 2u : 0u;  // len.saturating_sub(2)
        while (child <= lim) {
            child += !(val[at32(child + 1u)] > val[at32(child)]) ? 1u : 0u;  // child <= child + 1
            if (!(val[at32(child)] < val[at32(p)])) return;                  // pos >= child
            swap(p, child);
            p = child;
            child = 2u * p + 1u;
        }
        if (child == len - 1u && val[at32(child)] < val[at32(p)]) swap(p, child);  // pos < child: the one-child case
    }
    __device__ __forceinline__ void heapify() {
        if (len <= 1u) return;
        for (uint32_t i = (len - 2u) / 2u + 1u; i-- > 0u;) sift_down(i);
    }
};

// maximize_cosine_similarity (quantizer.rs:991-1100)
template <int BITS>
__device__ __forceinline__ float maximize_cosine(const float* __restrict__ t, uint32_t dim, LaneHeap& h) {
    constexpr float eps = 0.0001f;
    constexpr float one_and_change = 1.0f + eps;
    constexpr uint32_t stop = 1u << (BITS - 1);
    double current_ip = 0.0;
    for (uint32_t i = 0; i < dim; ++i) {
        const float av = __builtin_fabsf(t[i]);
        current_ip += (double)av;
        h.val[h.at32(i)] = one_and_change / av;
        h.pos[h.at16(i)] = (uint16_t)i;
        h.rnd[h.at16(i)] = 1;
    }
    current_ip = 0.5 * current_ip;
    double current_square_norm = 0.25 * (double)dim;
    h.heapify();
    double max_similarity = -__builtin_inf();
    float optimal_scale = 0.0f;
    // every pass but the last one raises one `rounded` below `stop` by one: at most dim * (stop - 1) + 1 passes
    for (uint32_t pass = 0; pass <= dim * stop; ++pass) {
        const float value = h.val[h.at32(0)];
        if (value == 3.40282347e+38f) break;  // f32::MAX
        const uint32_t p = h.pos[h.at16(0)];
        const uint32_t old_r = h.rnd[h.at16(p)], r = old_r + 1u;
        h.rnd[h.at16(p)] = (uint16_t)r;
        const float av = __builtin_fabsf(t[p]);
        current_ip += (double)av;
        current_square_norm += (double)(2u * old_r);
        const double similarity = current_ip / __builtin_sqrt(current_square_norm);
        if (similarity > max_similarity) {
            max_similarity = similarity;
            optimal_scale = value;
        }
        h.val[h.at32(0)] = r < stop ? ((float)r + eps) / av : 3.40282347e+38f;
        h.sift_down(0);
    }
    return optimal_scale;
}

// compress_via_maximum_cosine (quantizer.rs:871-918)
template <int BITS, bool GLOBAL>
__global__ __launch_bounds__(64) void spherical_data_kernel(FinArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t sph_lds[];
    uint32_t r;
    float2 m;
    const float* t = fin_row(a, &r, &m);
    if (!t) return;
    const uint32_t dim = a.dim, half = ((dim + 1u) >> 1) * 64u;  // dwords of one u16 array
    uint32_t* base = sph_lds;
    if constexpr (GLOBAL) base = a.heap + (uint64_t)blockIdx.x * ((uint64_t)dim * 64u + 2u * half);
    LaneHeap h{reinterpret_cast<float*>(base), reinterpret_cast<uint16_t*>(base + dim * 64u),
               reinterpret_cast<uint16_t*>(base + dim * 64u + half), dim, threadIdx.x};
    const float optimal_scale = maximize_cosine<BITS>(t, dim, h);
    uint8_t* img = a.out + (uint64_t)r * a.image_bytes;
    constexpr float maxv = (float)((1 << BITS) - 1), offset = maxv / 2.0f;
    float self_inner_product = 0.0f;
    uint32_t bit_sum = 0;
    for (uint32_t i = 0; i < dim; ++i) {
        const float e = t[i];
        float x = e * optimal_scale + offset;
        x = x < 0.0f ? 0.0f : x > maxv ? maxv : x;  // f32::clamp (a NaN stays)
        const float vv = __builtin_roundf(x);       // half away from zero
        self_inner_product = __builtin_fmaf(vv - offset, e, self_inner_product);
        const uint32_t c = vv == vv ? (uint32_t)vv : 0u;  // (`NaN as u8` is 0)
        bit_sum += c;
        const uint32_t bit = i * BITS;
        img[bit >> 3] |= (uint8_t)(c << (bit & 7u));
    }
    const float tn = a.tnorm ? a.tnorm[r] : 1.0f;
    const float ipc = (tn * m.x) / self_inner_product;
    write_data_meta(img + sq_code_bytes(32 + BITS, dim), ipc, m.y, bit_sum, a.flag);
}

// Query<QBITS, Dense | BitTranspose> (quantizer.rs:1177-1209)
template <int QBITS, bool TRANSPOSED>
__global__ __launch_bounds__(64) void spherical_query_kernel(FinArgs a) {
    uint32_t r;
    float2 m;
    const float* t = fin_row(a, &r, &m);
    if (!t) return;
    const uint32_t dim = a.dim;
    uint8_t* img = a.out + (uint64_t)r * a.image_bytes;
    // fold((f32::MAX, f32::MIN), |(min, max), i| (i.min(min), i.max(max))) as x86-64 runs f32::min / max: minss / maxss
    // of (accumulator, i), which hand back i unless the accumulator is strictly smaller / larger -- of two zeros the
    // later element's sign stays -- and the accumulator when i is a NaN
    float mn = 3.40282347e+38f, mx = -3.40282347e+38f;
    for (uint32_t i = 0; i < dim; ++i) {
        const float e = t[i];
        const float lo = mn < e ? mn : e, hi = mx > e ? mx : e;
        mn = e != e ? mn : lo;
        mx = e != e ? mx : hi;
    }
    constexpr float top = (float)((1 << QBITS) - 1);
    const float scale = (mx - mn) / top;
    float bit_sum = 0.0f;
    for (uint32_t i = 0; i < dim; ++i) {
        float c = __builtin_roundf((t[i] - mn) / scale);
        c = c < 0.0f ? 0.0f : c > top ? top : c;  // f32::clamp (a NaN stays)
        bit_sum += c;
        const uint32_t code = c == c ? (uint32_t)c : 0u;  // (`NaN as i64` is 0)
        if constexpr (TRANSPOSED) {
            const uint32_t at = (i >> 6) * 32u + ((i & 63u) >> 3), sh = i & 7u;
#pragma unroll
            for (uint32_t j = 0; j < 4u; ++j) img[at + 8u * j] |= (uint8_t)(((code >> j) & 1u) << sh);
        } else {
            const uint32_t bit = i * QBITS;
            img[bit >> 3] |= (uint8_t)(code << (bit & 7u));
        }
    }
    const float qm[4] = {m.x * scale, bit_sum, mn / scale, m.y};
    __builtin_memcpy(img + (TRANSPOSED ? sph_plane_bytes(dim) : sq_code_bytes(32 + QBITS, dim)), qm, 16);
}

int32_t launch_finish(int kind, int32_t bits, const FinArgs& a, hipStream_t st) {
    const dim3 grid((a.n + 63u) / 64u), block(64);
    if (kind == kQueryTransposed)
        return launch_kernel<spherical_query_kernel<4, true>>("spherical_query_kernel", grid, block, 0, st, a);
    if (kind == kQueryDense)
        return bits == 2 ? launch_kernel<spherical_query_kernel<2, false>>("spherical_query_kernel", grid, block, 0, st, a)
                         : launch_kernel<spherical_query_kernel<4, false>>("spherical_query_kernel", grid, block, 0, st, a);
    if (bits == 1) return launch_kernel<spherical_data1_kernel>("spherical_data1_kernel", grid, block, 0, st, a);
    const size_t lds = a.heap ? 0 : (size_t)256 * a.dim + (size_t)512 * ((a.dim + 1u) >> 1);
    if (bits == 2)
        return a.heap ? launch_kernel<spherical_data_kernel<2, true>>("spherical_data_kernel", grid, block, 0, st, a)
                      : launch_kernel<spherical_data_kernel<2, false>, kLds160Once>("spherical_data_kernel", grid, block, lds, st, a);
    return a.heap ? launch_kernel<spherical_data_kernel<4, true>>("spherical_data_kernel", grid, block, 0, st, a)
                  : launch_kernel<spherical_data_kernel<4, false>, kLds160Once>("spherical_data_kernel", grid, block, lds, st, a);
}

int32_t invalid(const char* who, const char* what) {
    set_error("%s: %s", who, what);
    return DANN_EINVAL;
}

// bits, and for queries the layout, in the classes of dann_set_query_layout; `kind` and the bytes of one image
int32_t check_form(const char* who, const dann_spherical* q, int32_t bits, bool query, int32_t layout, int* kind,
                   uint32_t* image_bytes) {
    if (!q) return invalid(who, "null handle");
    if (bits != 1 && bits != 2 && bits != 4) {
        set_error("%s: bits must be 1, 2 or 4 (got %d)", who, bits);
        return DANN_EINVAL;
    }
    if (!query) layout = QL_SAME;
    if (layout != QL_EIGHT_BIT && (layout < QL_SAME || layout > QL_FULL)) {
        set_error("%s: unknown layout %d", who, layout);
        return DANN_EINVAL;
    }
    const uint32_t ib = layout == QL_EIGHT_BIT ? 0u : sph_query_bytes(32 + bits, q->t.out_dim, layout);
    if (ib == 0u) {  // UnsupportedQueryLayout, as dann_set_query_layout; FULL_PRECISION is not served
        set_error("%s: query layout %d is not supported for %d-bit rows", who, layout, bits);
        return DANN_EUNSUPPORTED;
    }
    *kind = layout == QL_SAME ? kData : layout == QL_TRANSPOSED ? kQueryTransposed : kQueryDense;
    *image_bytes = ib;
    return DANN_OK;
}

int32_t compress_device(const char* who, const dann_spherical* q, int32_t bits, int kind, uint32_t ib, const float* d_x,
                        uint64_t xs, uint32_t n, void* d_out, uint64_t os) {
    const dann_transform& t = q->t;
    const uint32_t id = t.in_dim, od = t.out_dim;
    if (xs < id || os < ib) {
        set_error("%s: x_stride %llu floats / out_stride %llu bytes are below a row (%u floats) / an image (%u bytes)", who,
                  (unsigned long long)xs, (unsigned long long)os, id, ib);
        return DANN_EINVAL;
    }
    DeviceGuard dev(q->device);
    if (!dev.ok) return hip_fail(hipErrorInvalidDevice, "hipSetDevice");
    const bool heap_global = kind == kData && bits != 1 && od > kSphLdsDim;
    const bool null_tf = t.kind == DANN_TRANSFORM_NULL, tnorm = kind == kData && !t.preserves_norms();
    const size_t heap_row = heap_global ? ((size_t)od * 4 + (size_t)((od + 1u) >> 1) * 8) : 0;  // bytes per row
    const size_t per_row = (size_t)id * 4 + (null_tf ? 0 : (size_t)od * 4) + 8 + 4 + heap_row + (os != ib ? ib : 0);
    uint64_t chunk = kSphChunkBytes / per_row / 64u * 64u;
    if (chunk < 64u) chunk = 64u;
    if (chunk > n) chunk = n;
    const uint32_t cn_max = (uint32_t)chunk, blocks_max = (cn_max + 63u) / 64u;
    DevBuf dsh, dtx, dmeta, dtn, dheap, dimg, dflag;
    DANN_HIP(dsh.alloc((size_t)cn_max * id * 4));
    if (!null_tf) DANN_HIP(dtx.alloc((size_t)cn_max * od * 4));
    DANN_HIP(dmeta.alloc((size_t)cn_max * 8));
    if (tnorm) DANN_HIP(dtn.alloc((size_t)cn_max * 4));
    if (heap_global) DANN_HIP(dheap.alloc((size_t)blocks_max * 64u * heap_row));
    if (os != ib) DANN_HIP(dimg.alloc((size_t)cn_max * ib));  // (the bytes between the caller's images are not ours to clear)
    DANN_HIP(dflag.alloc(4));
    DANN_HIP(hipMemsetAsync(dflag.p, 0, 4, nullptr));
    for (uint64_t c0 = 0; c0 < n; c0 += chunk) {
        const uint32_t cn = (uint32_t)(n - c0 < chunk ? n - c0 : chunk);
        const dim3 ggrid((uint32_t)(((uint64_t)cn * 8u + 255u) / 256u)), gblock(256);
        hipLaunchKernelGGL(spherical_pre_kernel, ggrid, gblock, 0, nullptr, d_x + c0 * xs, xs, cn, id, q->d_shift,
                           q->pre_scale, q->metric, dsh.as<float>(), dmeta.as<float2>(), dflag.as<uint32_t>());
        DANN_HIP(hipGetLastError());
        const float* tx = dsh.as<float>();
        if (!null_tf) {
            if (int32_t rc = launch_transform(t, dsh.as<float>(), id, cn, dtx.as<float>(), od, nullptr)) return rc;
            tx = dtx.as<float>();
        }
        if (tnorm) {
            hipLaunchKernelGGL(spherical_tnorm_kernel, ggrid, gblock, 0, nullptr, tx, cn, od, 1, dtn.as<float>());
            DANN_HIP(hipGetLastError());
        }
        uint8_t* img = os != ib ? dimg.as<uint8_t>() : static_cast<uint8_t*>(d_out) + c0 * ib;
        DANN_HIP(hipMemsetAsync(img, 0, (size_t)cn * ib, nullptr));
        const FinArgs a{tx, dmeta.as<float2>(), tnorm ? dtn.as<float>() : nullptr, cn, od, img, ib,
                        heap_global ? dheap.as<uint32_t>() : nullptr, dflag.as<uint32_t>()};
        if (int32_t rc = launch_finish(kind, bits, a, nullptr)) return rc;
        if (os != ib)
            DANN_HIP(hipMemcpy2DAsync(static_cast<uint8_t*>(d_out) + c0 * os, os, img, ib, ib, cn, hipMemcpyDeviceToDevice,
                                      nullptr));
    }
    uint32_t flag = 0;
    DANN_HIP(hipMemcpy(&flag, dflag.p, 4, hipMemcpyDeviceToHost));
    DANN_HIP(hipStreamSynchronize(nullptr));
    if (flag & kFlagNaN) {
        set_error("%s: the norm of a shifted vector is not finite (InputContainsNaN)", who);
        return DANN_EINVAL;
    }
    if (flag) {
        set_error("%s: EncodingError(DataMetaError::%s): the value does not fit its 16-bit field -- scale the dataset down "
                  "(pre_scale)", who, flag & kFlagIpc ? "InnerProductCorrection" : flag & kFlagMs ? "MetricSpecific" : "BitSum");
        return DANN_EINVAL;
    }
    return DANN_OK;
}

int32_t compress_host(const char* who, const dann_spherical* q, int32_t bits, int kind, uint32_t ib, const float* x, uint32_t n,
                      void* out) {
    DeviceGuard dev(q->device);
    if (!dev.ok) return hip_fail(hipErrorInvalidDevice, "hipSetDevice");
    const size_t xb = (size_t)n * q->t.in_dim * 4, ob = (size_t)n * ib;
    DevBuf dx, dout;
    DANN_HIP(dx.alloc(xb));
    DANN_HIP(dout.alloc(ob));
    DANN_HIP(hipMemcpy(dx.p, x, xb, hipMemcpyHostToDevice));
    const int32_t rc = compress_device(who, q, bits, kind, ib, dx.as<float>(), q->t.in_dim, n, dout.p, ib);
    if (rc != DANN_OK && rc != DANN_EINVAL) return rc;  // (a refused row: the outputs are still handed back, as MinMax does)
    DANN_HIP(hipMemcpy(out, dout.p, ob, hipMemcpyDeviceToHost));
    return rc;
}

int32_t copy_u32(uint32_t** d, const uint32_t* src, uint32_t n) {
    if (!src || n == 0) return DANN_OK;
    DANN_HIP(hipMalloc(reinterpret_cast<void**>(d), (size_t)n * 4));
    DANN_HIP(hipMemcpy(*d, src, (size_t)n * 4, hipMemcpyDeviceToDevice));
    return DANN_OK;
}

}  // namespace
}  // namespace dann

extern "C" int32_t dann_spherical_create(const dann_transform* t, const dann_spherical_parts* parts, dann_spherical** out) try {
    using namespace dann;
    const char* who = "dann_spherical_create";
    if (!t || !parts || !out) return invalid(who, "null pointer");
    *out = nullptr;
    if (parts->metric != DANN_L2 && parts->metric != DANN_INNER_PRODUCT && parts->metric != DANN_COSINE)
        return invalid(who, "metric must be DANN_L2, DANN_INNER_PRODUCT or DANN_COSINE (SupportedMetric)");
    if (!parts->shift) return invalid(who, "null shift");
    for (uint32_t i = 0; i < t->in_dim; ++i)
        if (!std::isfinite(parts->shift[i])) return invalid(who, "the shift is not finite");
    if (!(parts->pre_scale > 0.0f) || !std::isfinite(parts->pre_scale)) return invalid(who, "pre_scale must be positive and finite");
    DeviceGuard dev(t->device);
    if (!dev.ok) return hip_fail(hipErrorInvalidDevice, "hipSetDevice");
    std::unique_ptr<dann_spherical> q(new dann_spherical());
    q->device = t->device;
    q->metric = parts->metric;
    q->pre_scale = parts->pre_scale;
    dann_transform& c = q->t;
    c.device = t->device;
    c.kind = t->kind;
    c.in_dim = t->in_dim;
    c.out_dim = t->out_dim;
    c.work = t->work;
    c.t = t->t;
    c.m = t->m;
    c.rescale = t->rescale;
    if (int32_t rc = copy_u32(&c.d_signs0, t->d_signs0, t->in_dim)) return rc;
    if (int32_t rc = copy_u32(&c.d_signs1, t->d_signs1, t->signs1_len())) return rc;
    if (int32_t rc = copy_u32(&c.d_sub, t->d_sub, t->out_dim)) return rc;
    DANN_HIP(hipMalloc(reinterpret_cast<void**>(&q->d_shift), (size_t)t->in_dim * 4));
    DANN_HIP(hipMemcpy(q->d_shift, parts->shift, (size_t)t->in_dim * 4, hipMemcpyHostToDevice));
    // CompensatedIP::new: FastL2NormSquared(shift), by the kernel every other norm here goes through
    DevBuf dn;
    DANN_HIP(dn.alloc(4));
    hipLaunchKernelGGL(spherical_tnorm_kernel, dim3(1), dim3(256), 0, nullptr, q->d_shift, 1u, t->in_dim, 0, dn.as<float>());
    DANN_HIP(hipGetLastError());
    float norm = 0.0f;
    DANN_HIP(hipMemcpy(&norm, dn.p, 4, hipMemcpyDeviceToHost));
    q->shift_norm_sq = norm;
    *out = q.release();
    return DANN_OK;
} DANN_CATCH_ALL

extern "C" int32_t dann_spherical_destroy(dann_spherical* q) try {
    if (!q) return DANN_OK;
    dann::DeviceGuard dev(q->device);
    delete q;
    return DANN_OK;
} DANN_CATCH_ALL

extern "C" int32_t dann_spherical_shift_norm_sq(const dann_spherical* q, float* out) try {
    if (!q || !out) return dann::invalid("dann_spherical_shift_norm_sq", "null pointer");
    *out = q->shift_norm_sq;
    return DANN_OK;
} DANN_CATCH_ALL

extern "C" int32_t dann_spherical_compress_device(const dann_spherical* q, int32_t bits, const float* d_x, uint64_t x_stride,
                                                  uint32_t n, void* d_out, uint64_t out_stride) try {
    using namespace dann;
    const char* who = "dann_spherical_compress_device";
    int kind;
    uint32_t ib;
    if (int32_t rc = check_form(who, q, bits, false, 0, &kind, &ib)) return rc;
    if (n == 0) return DANN_OK;
    if (!d_x || !d_out) return invalid(who, "null pointer");
    return compress_device(who, q, bits, kind, ib, d_x, x_stride, n, d_out, out_stride);
} DANN_CATCH_ALL

extern "C" int32_t dann_spherical_compress(const dann_spherical* q, int32_t bits, const float* x, uint32_t n, void* out) try {
    using namespace dann;
    const char* who = "dann_spherical_compress";
    int kind;
    uint32_t ib;
    if (int32_t rc = check_form(who, q, bits, false, 0, &kind, &ib)) return rc;
    if (n == 0) return DANN_OK;
    if (!x || !out) return invalid(who, "null pointer");
    return compress_host(who, q, bits, kind, ib, x, n, out);
} DANN_CATCH_ALL

extern "C" int32_t dann_spherical_compress_queries_device(const dann_spherical* q, int32_t bits, int32_t layout,
                                                          const float* d_x, uint64_t x_stride, uint32_t n, void* d_out,
                                                          uint64_t out_stride) try {
    using namespace dann;
    const char* who = "dann_spherical_compress_queries_device";
    int kind;
    uint32_t ib;
    if (int32_t rc = check_form(who, q, bits, true, layout, &kind, &ib)) return rc;
    if (n == 0) return DANN_OK;
    if (!d_x || !d_out) return invalid(who, "null pointer");
    return compress_device(who, q, bits, kind, ib, d_x, x_stride, n, d_out, out_stride);
} DANN_CATCH_ALL

extern "C" int32_t dann_spherical_compress_queries(const dann_spherical* q, int32_t bits, int32_t layout, const float* x,
                                                   uint32_t n, void* out) try {
    using namespace dann;
    const char* who = "dann_spherical_compress_queries";
    int kind;
    uint32_t ib;
    if (int32_t rc = check_form(who, q, bits, true, layout, &kind, &ib)) return rc;
    if (n == 0) return DANN_OK;
    if (!x || !out) return invalid(who, "null pointer");
    return compress_host(who, q, bits, kind, ib, x, n, out);
} DANN_CATCH_ALL
