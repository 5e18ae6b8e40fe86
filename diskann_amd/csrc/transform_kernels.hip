// transform_kernels.hip -- Transform::transform_into on the GPU, device to device (diskann-quantization/src/algorithms/
// transforms: NullTransform, PaddingHadamard padding_hadamard.rs:204-273, DoubleHadamard double_hadamard.rs:238-287), and
// MinMaxQuantizer::compress_into including the transform (dann_minmax_quantize: these kernels, then
// minmax_compress_kernel on a device scratch buffer).  Bit for bit the reference's x86-64 V3 path of hadamard_transform
// (algorithms/hadamard.rs:22-371): for lengths >= 64 the strides 1, 2, 4 are not butterflies but micro_kernel_64's
// eight-term FMA chain (exact +-1 products, one rounding per addition, k ascending, from +0.0); every other stride is the
// butterfly (l, r) -> (l + r, l - r); 1 / sqrt(len) is computed on the host.  Nothing is fused (-ffp-contract=off),
// denormals are kept.
//
// Shape: a lane owns eight consecutive elements (one sub-block of the micro kernel), so the order-sensitive chain is 64
// in-register additions; strides 8 .. 256 are exchanges with lanes l ^ 1 .. l ^ 32 (the lane with the bit clear takes own
// + other, the other one other - own); strides >= 512 are between the 8-groups of a row staged in LDS.
//   hadamard_wave_kernel  PaddingHadamard without subsample, padded_dim 8 .. 512: registers only, 64 / (padded_dim / 8)
//                         rows per wavefront
//   transform_lds_kernel  everything else: the row's working vector lives in LDS (DoubleHadamard's second window starts at
//                         an arbitrary offset, a subsample gathers, rows up to 16384 floats exceed a wavefront's registers)
// Loads are never behind a per-lane branch: the address is clamped and the value discarded.
#include <math.h>

#include <memory>

#include "dann_device.h"
#include "dann_internal.h"
#include "transform.h"

namespace dann {
namespace {

constexpr uint32_t kMaxWork = 16384u;  // floats of one row's working vector: one 64 KB LDS stage

struct TfArgs {
    const uint32_t* s0;
    const uint32_t* s1;   // DoubleHadamard only (length work)
    const uint32_t* sub;  // null: no subsample
    uint32_t in_dim, out_dim, work, t;
    uint32_t off2;    // DoubleHadamard: start of the second window, work - t
    uint32_t gshift;  // log2 of the lanes per row
    int32_t dbl;
    float m, rescale;
};

// micro_kernel_64's process_patch for one sub-block: d[j] = sum_k s(k, j) v[k], s(k, j) = (-1)^popcount(k & j), from +0.0
// (so a -0.0 input gives +0.0, as the FMA does), k ascending, one rounding per addition
__device__ __forceinline__ void chain8(float (&v)[8]) {
    float d[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        float acc = 0.0f;
#pragma unroll
        for (int k = 0; k < 8; ++k) acc = (__builtin_popcount(k & j) & 1) ? acc - v[k] : acc + v[k];
        d[j] = acc;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = d[j];
}

// lengths below 64: the butterflies at strides 1, 2, 4
__device__ __forceinline__ void butterfly8(float (&v)[8]) {
#pragma unroll
    for (int s = 1; s < 8; s <<= 1) {
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int i = ((p & ~(s - 1)) << 1) | (p & (s - 1));
            const float l = v[i], r = v[i + s];
            v[i] = l + r;
            v[i + s] = l - r;
        }
    }
}

// strides 1 .. min(t, 512) / 2 of a row of length t >= 8 whose 8-group q sits in lane q & 63 of its wavefront (rows are
// aligned to their power-of-two lane count; every lane of the wavefront is here)
__device__ __forceinline__ void hadamard_wave_part(float (&v)[8], uint32_t t, uint32_t lane) {
    if (t >= 64u) chain8(v);
    else butterfly8(v);
    const uint32_t lim = t >> 3 < 64u ? t >> 3 : 64u;
    for (uint32_t m = 1; m < lim; m <<= 1) {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const float o = __shfl_xor(v[k], (int)m, 64);
            v[k] = (lane & m) ? o - v[k] : v[k] + o;
        }
    }
}

// elements e0 .. e0 + 7 (e0 a multiple of 8) of the sign-flipped, zero-padded input row.  VEC: in_dim % 4 == 0 and the
// row and the signs are 16-byte aligned.  The address is clamped, never the load skipped.
template <bool VEC>
__device__ __forceinline__ void load8(float (&v)[8], const float* __restrict__ src, const uint32_t* __restrict__ s0,
                                      uint32_t e0, uint32_t in_dim) {
    if constexpr (VEC) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const uint32_t e = e0 + 4u * h;
            const bool in = e < in_dim;
            const uint32_t ec = in ? e : 0u;
            const uint4 f = *reinterpret_cast<const uint4*>(src + ec);
            const uint4 s = *reinterpret_cast<const uint4*>(s0 + ec);
            v[4 * h + 0] = in ? __uint_as_float(f.x ^ s.x) : 0.0f;
            v[4 * h + 1] = in ? __uint_as_float(f.y ^ s.y) : 0.0f;
            v[4 * h + 2] = in ? __uint_as_float(f.z ^ s.z) : 0.0f;
            v[4 * h + 3] = in ? __uint_as_float(f.w ^ s.w) : 0.0f;
        }
    } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const uint32_t e = e0 + k;
            const bool in = e < in_dim;
            const uint32_t ec = in ? e : 0u;
            const uint32_t b = __float_as_uint(src[ec]) ^ s0[ec];
            v[k] = in ? __uint_as_float(b) : 0.0f;
        }
    }
}

template <bool VEC>
__global__ __launch_bounds__(256) void hadamard_wave_kernel(TfArgs a, const float* __restrict__ x, uint64_t xs,
                                                            uint32_t n, float* __restrict__ out, uint64_t os) {
    const uint32_t lane = threadIdx.x & ((1u << a.gshift) - 1u);
    uint64_t row = ((uint64_t)blockIdx.x * 256u + threadIdx.x) >> a.gshift;
    const bool live = row < n;
    if (!live) row = n - 1u;
    const float* src = x + row * xs;
    const uint32_t e0 = lane * 8u;
    float v[8];
    load8<VEC>(v, src, a.s0, e0, a.in_dim);
    hadamard_wave_part(v, a.t, lane);
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] *= a.m;
    if (!live) return;
    float* dst = out + row * os + e0;
    if constexpr (VEC) {
        *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
        *reinterpret_cast<float4*>(dst + 4) = make_float4(v[4], v[5], v[6], v[7]);
    } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) dst[k] = v[k];
    }
}

// LDS index of element i of a row: one pad word per 32, so that lanes reading eight consecutive elements each (a stride
// of eight words) spread over the banks
__device__ __forceinline__ uint32_t lds_at(uint32_t i) { return i + (i >> 5); }
__host__ __device__ constexpr uint32_t lds_row_words(uint32_t work) { return work + (work >> 5) + 1u; }

// hadamard_transform of the t elements of a row's working vector `w` from element `off` on, by the g lanes of the row
// (t / 8 of them, at most 256; one for t < 8).  FIRST: the first transform, off = 0 -- for t >= 8 the window comes straight
// from global memory (sign-flipped, zero-padded) and only the result is written to LDS; else the second one of a
// DoubleHadamard, whose window takes its signs1 flip on the way in.  Every thread of the block takes the same path (t is
// uniform) and has synchronised before a window that is read from LDS.
template <bool FIRST, bool VEC>
__device__ __forceinline__ void hadamard_lds(float* w, uint32_t off, const TfArgs& a, const float* __restrict__ src,
                                             uint32_t lane, uint32_t g) {
    const uint32_t t = a.t;
    const float m = a.m;
    uint32_t s = 1;
    if (t >= 8u) {
        const bool done = t <= 512u;
        for (uint32_t q = lane; q < t >> 3; q += g) {
            float v[8];
            if constexpr (FIRST) {
                load8<VEC>(v, src, a.s0, 8u * q, a.in_dim);
            } else {
#pragma unroll
                for (int k = 0; k < 8; ++k)
                    v[k] = __uint_as_float(__float_as_uint(w[lds_at(off + 8u * q + k)]) ^ a.s1[off + 8u * q + k]);
            }
            hadamard_wave_part(v, t, lane);
#pragma unroll
            for (int k = 0; k < 8; ++k) w[lds_at(off + 8u * q + k)] = done ? v[k] * m : v[k];
        }
        s = done ? t : 512u;
    } else if (!FIRST) {
        for (uint32_t i = lane; i < t; i += g)  // (g == 1: the lane's own elements)
            w[lds_at(off + i)] = __uint_as_float(__float_as_uint(w[lds_at(off + i)]) ^ a.s1[off + i]);
    }
    for (; s < t; s <<= 1) {
        __syncthreads();
        const bool last = 2u * s == t;
        for (uint32_t p = lane; p < t >> 1; p += g) {
            const uint32_t i = off + (((p & ~(s - 1u)) << 1) | (p & (s - 1u)));
            const float l = w[lds_at(i)], r = w[lds_at(i + s)];
            float lo = l + r, hi = l - r;
            if (last) {
                lo *= m;
                hi *= m;
            }
            w[lds_at(i)] = lo;
            w[lds_at(i + s)] = hi;
        }
    }
}

template <bool VEC>
__global__ __launch_bounds__(256) void transform_lds_kernel(TfArgs a, const float* __restrict__ x, uint64_t xs, uint32_t n,
                                                            float* __restrict__ out, uint64_t os) {
    extern __shared__ float tf_lds[];
    const uint32_t g = 1u << a.gshift, lane = threadIdx.x & (g - 1u), slot = threadIdx.x >> a.gshift;
    uint64_t row = (uint64_t)blockIdx.x * (256u >> a.gshift) + slot;
    const bool live = row < n;
    if (!live) row = n - 1u;
    float* w = tf_lds + slot * lds_row_words(a.work);
    const float* src = x + row * xs;
    // what the first transform does not take from global memory itself: everything for t < 8, else the tail [t, work)
    for (uint32_t i = (a.t >= 8u ? a.t : 0u) + lane; i < a.work; i += g) {
        const bool in = i < a.in_dim;
        const uint32_t ic = in ? i : 0u;
        const uint32_t b = __float_as_uint(src[ic]) ^ a.s0[ic];
        w[lds_at(i)] = in ? __uint_as_float(b) : 0.0f;
    }
    hadamard_lds<true, VEC>(w, 0u, a, src, lane, g);
    if (a.dbl) {
        __syncthreads();
        hadamard_lds<false, VEC>(w, a.off2, a, src, lane, g);
    }
    __syncthreads();
    float* dst = out + row * os;
    for (uint32_t i = lane; i < a.out_dim; i += g) {
        const uint32_t j = a.sub ? a.sub[i] : i;
        uint32_t b = __float_as_uint(w[lds_at(j)]);
        if (a.dbl) b ^= j < a.off2 ? a.s1[j] : 0u;  // below the second window: the signs1 flip is all that is left to do
        float v = __uint_as_float(b);
        if (a.sub) v *= a.rescale;
        if (live) dst[i] = v;
    }
}

bool is_pow2(uint32_t v) { return v != 0 && (v & (v - 1u)) == 0; }
bool all_signs(const uint32_t* s, uint32_t n) {
    for (uint32_t i = 0; i < n; ++i)
        if (s[i] != 0u && s[i] != 0x80000000u) return false;
    return true;
}
bool strictly_monotonic(const uint32_t* s, uint32_t n) {
    for (uint32_t i = 1; i < n; ++i)
        if (s[i] <= s[i - 1]) return false;
    return true;
}

int32_t invalid(const char* what) {
    set_error("dann_transform_create: %s", what);
    return DANN_EINVAL;
}

// PaddingHadamard::try_from_parts / DoubleHadamard::try_from_parts: DANN_OK, or the status with the variant's name in
// the message.  Fills kind, dims, work, t, m, rescale of `t`.
int32_t validate_parts(const dann_transform_parts& p, dann_transform& t) {
    t.kind = p.kind;
    if (p.kind == DANN_TRANSFORM_RANDOM_ROTATION) {
        set_error("dann_transform_create: RandomRotation is reserved (its sgemm's summation order is not part of the "
                  "contract)");
        return DANN_EUNSUPPORTED;
    }
    if (p.kind == DANN_TRANSFORM_NULL) {
        if (p.dim == 0) return invalid("NullTransform: dim must be positive");
        t.in_dim = t.out_dim = t.work = p.dim;
        return DANN_OK;
    }
    if (p.kind != DANN_TRANSFORM_PADDING_HADAMARD && p.kind != DANN_TRANSFORM_DOUBLE_HADAMARD)
        return invalid("kind is not a dann_transform_kind");
    const bool has_sub = p.subsample != nullptr || p.subsample_len != 0;
    if ((p.signs0_len && !p.signs0) || (p.kind == DANN_TRANSFORM_DOUBLE_HADAMARD && p.signs1_len && !p.signs1) || (p.subsample_len && !p.subsample))
        return invalid("a null pointer with a non-zero length");
    if (p.kind == DANN_TRANSFORM_PADDING_HADAMARD) {
        if (p.signs0_len == 0) return invalid("PaddingHadamard: signs cannot be empty");
        if (!all_signs(p.signs0, p.signs0_len)) return invalid("PaddingHadamardError::InvalidSignRepresentation");
        if (p.signs0_len > p.padded_dim) return invalid("PaddingHadamardError::SignsTooLong");
        if (!is_pow2(p.padded_dim)) return invalid("PaddingHadamardError::DimNotPowerOfTwo");
        if (has_sub) {
            if (!strictly_monotonic(p.subsample, p.subsample_len)) return invalid("PaddingHadamardError::SubsampleNotMonotonic");
            if (p.subsample_len == 0) return invalid("PaddingHadamardError::SubsampleEmpty");
            if (p.subsample[p.subsample_len - 1] >= p.padded_dim) return invalid("PaddingHadamardError::LastSubsampleTooLarge");
        }
        t.in_dim = p.signs0_len;
        t.work = t.t = p.padded_dim;
        t.out_dim = has_sub ? p.subsample_len : p.padded_dim;
    } else {
        if (p.signs0_len == 0) return invalid("DoubleHadamardError::Signs0Empty");
        if (p.signs1_len < p.signs0_len) return invalid("DoubleHadamardError::Signs1TooSmall");
        if (!all_signs(p.signs0, p.signs0_len)) return invalid("DoubleHadamardError::Signs0Invalid");
        if (!all_signs(p.signs1, p.signs1_len)) return invalid("DoubleHadamardError::Signs1Invalid");
        if (has_sub) {
            if (!strictly_monotonic(p.subsample, p.subsample_len)) return invalid("DoubleHadamardError::SubsampleNotMonotonic");
            if (p.subsample_len == 0) return invalid("DoubleHadamardError::InvalidSubsampleLength");
            if (p.subsample[p.subsample_len - 1] >= p.signs1_len) return invalid("DoubleHadamardError::LastSubsampleTooLarge");
            // DoubleHadamard::new never builds one (signs1 has max(dim, target) = dim entries when it subsamples), and
            // transform_into would index its intermediate vector of signs0_len entries out of bounds
            if (p.signs1_len != p.signs0_len)
                return invalid("DoubleHadamard: with a subsample signs1 must be as long as signs0");
        }
        t.in_dim = p.signs0_len;
        t.out_dim = has_sub ? p.subsample_len : p.signs1_len;
        t.work = p.signs1_len;  // == max(input_dim, output_dim)
        t.t = 1u;
        while (t.t <= t.work / 2u) t.t <<= 1;
    }
    if (t.work > kMaxWork) {
        set_error("dann_transform_create: a working length of %u floats exceeds the %u of one LDS stage", t.work, kMaxWork);
        return DANN_EUNSUPPORTED;
    }
    t.m = 1.0f / sqrtf((float)t.t);
    if (has_sub) t.rescale = sqrtf((float)t.work / (float)p.subsample_len);
    return DANN_OK;
}

int32_t upload(uint32_t** d, const uint32_t* h, uint32_t n) {
    DANN_HIP(hipMalloc(reinterpret_cast<void**>(d), (size_t)n * 4));
    DANN_HIP(hipMemcpy(*d, h, (size_t)n * 4, hipMemcpyHostToDevice));
    return DANN_OK;
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace

// n rows d_x -> d_out on the current device (the transform's), queued on `st`
int32_t launch_transform(const dann_transform& t, const float* d_x, uint64_t xs, uint32_t n, float* d_out, uint64_t os,
                         hipStream_t st) {
    if (t.kind == DANN_TRANSFORM_NULL) {
        DANN_HIP(hipMemcpy2DAsync(d_out, os * 4, d_x, xs * 4, (size_t)t.in_dim * 4, n, hipMemcpyDeviceToDevice, st));
        return DANN_OK;
    }
    TfArgs a{};
    a.s0 = t.d_signs0;
    a.s1 = t.d_signs1;
    a.sub = t.d_sub;
    a.in_dim = t.in_dim;
    a.out_dim = t.out_dim;
    a.work = t.work;
    a.t = t.t;
    a.off2 = t.work - t.t;
    a.dbl = t.kind == DANN_TRANSFORM_DOUBLE_HADAMARD;
    a.m = t.m;
    a.rescale = t.rescale;
    uint32_t g = t.t >> 3 ? t.t >> 3 : 1u;  // lanes per row
    if (g > 256u) g = 256u;
    while ((1u << a.gshift) < g) ++a.gshift;
    const bool vec_in = t.in_dim % 4u == 0 && xs % 4u == 0 && aligned16(d_x);  // 16-byte loads of the rows and their signs
    if (!a.dbl && !a.sub && t.t >= 8u && t.t <= 512u) {
        const bool vec = vec_in && os % 4u == 0 && aligned16(d_out);
        const uint64_t blocks = ((uint64_t)n * g + 255u) / 256u;
        if (vec) hipLaunchKernelGGL(hadamard_wave_kernel<true>, dim3((uint32_t)blocks), dim3(256), 0, st, a, d_x, xs, n, d_out, os);
        else hipLaunchKernelGGL(hadamard_wave_kernel<false>, dim3((uint32_t)blocks), dim3(256), 0, st, a, d_x, xs, n, d_out, os);
    } else {
        const uint32_t rpb = 256u / g;
        const size_t lds = (size_t)rpb * lds_row_words(t.work) * 4;
        auto kern = vec_in ? transform_lds_kernel<true> : transform_lds_kernel<false>;
        if (lds > 65536u)
            DANN_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                         (int)lds));
        hipLaunchKernelGGL(kern, dim3((uint32_t)(((uint64_t)n + rpb - 1u) / rpb)), dim3(256), lds, st, a, d_x, xs, n, d_out, os);
    }
    DANN_HIP(hipGetLastError());
    return DANN_OK;
}

namespace {

bool bad_bits(const char* who, int32_t bits, float grid_scale) {
    if (bits != 1 && bits != 2 && bits != 4 && bits != 8) {
        set_error("%s: bits must be 1, 2, 4 or 8 (got %d)", who, bits);
        return true;
    }
    if (!(grid_scale > 0.0f)) {
        set_error("%s: grid_scale must be positive", who);
        return true;
    }
    return false;
}

}  // namespace
}  // namespace dann

extern "C" int32_t dann_transform_create(int32_t device, const dann_transform_parts* parts, dann_transform** out) try {
    using namespace dann;
    if (!parts || !out) return DANN_EINVAL;
    *out = nullptr;
    std::unique_ptr<dann_transform> t(new dann_transform());
    if (int32_t rc = validate_parts(*parts, *t)) return rc;
    if (device >= 0) DANN_HIP(hipSetDevice(device));
    DANN_HIP(hipGetDevice(&t->device));
    if (t->kind != DANN_TRANSFORM_NULL) {
        if (int32_t rc = upload(&t->d_signs0, parts->signs0, parts->signs0_len)) return rc;
        if (t->kind == DANN_TRANSFORM_DOUBLE_HADAMARD)
            if (int32_t rc = upload(&t->d_signs1, parts->signs1, parts->signs1_len)) return rc;
        if (parts->subsample_len)
            if (int32_t rc = upload(&t->d_sub, parts->subsample, parts->subsample_len)) return rc;
    }
    *out = t.release();
    return DANN_OK;
} DANN_CATCH_ALL

extern "C" int32_t dann_transform_destroy(dann_transform* t) try {
    if (!t) return DANN_OK;
    dann::DeviceGuard dev(t->device);
    delete t;
    return DANN_OK;
} DANN_CATCH_ALL

extern "C" int32_t dann_transform_input_dim(const dann_transform* t) try {
    return t ? (int32_t)t->in_dim : DANN_EINVAL;
} DANN_CATCH_ALL

extern "C" int32_t dann_transform_output_dim(const dann_transform* t) try {
    return t ? (int32_t)t->out_dim : DANN_EINVAL;
} DANN_CATCH_ALL

extern "C" int32_t dann_transform_apply_device(const dann_transform* t, const float* d_x, uint64_t x_stride, uint32_t n,
                                               float* d_out, uint64_t out_stride) try {
    using namespace dann;
    if (!t) return DANN_EINVAL;
    if (n == 0) return DANN_OK;
    if (!d_x || !d_out) return DANN_EINVAL;
    if (x_stride < t->in_dim || out_stride < t->out_dim) {
        set_error("dann_transform_apply_device: strides (%llu, %llu floats) are below the transform's dims (%u, %u)",
                  (unsigned long long)x_stride, (unsigned long long)out_stride, t->in_dim, t->out_dim);
        return DANN_EINVAL;
    }
    DeviceGuard dev(t->device);
    if (!dev.ok) return hip_fail(hipErrorInvalidDevice, "hipSetDevice");
    if (int32_t rc = launch_transform(*t, d_x, x_stride, n, d_out, out_stride, nullptr)) return rc;
    DANN_HIP(hipStreamSynchronize(nullptr));
    return DANN_OK;
} DANN_CATCH_ALL

extern "C" int32_t dann_transform_apply(const dann_transform* t, const float* x, uint32_t n, float* out) try {
    using namespace dann;
    if (!t) return DANN_EINVAL;
    if (n == 0) return DANN_OK;
    if (!x || !out) return DANN_EINVAL;
    DeviceGuard dev(t->device);
    if (!dev.ok) return hip_fail(hipErrorInvalidDevice, "hipSetDevice");
    const size_t xb = (size_t)n * t->in_dim * 4, ob = (size_t)n * t->out_dim * 4;
    DevBuf dx, dout;
    DANN_HIP(dx.alloc(xb));
    DANN_HIP(dout.alloc(ob));
    DANN_HIP(hipMemcpy(dx.p, x, xb, hipMemcpyHostToDevice));
    if (int32_t rc = launch_transform(*t, static_cast<const float*>(dx.p), t->in_dim, n, static_cast<float*>(dout.p),
                                      t->out_dim, nullptr))
        return rc;
    DANN_HIP(hipMemcpy(out, dout.p, ob, hipMemcpyDeviceToHost));
    return DANN_OK;
} DANN_CATCH_ALL

extern "C" int32_t dann_minmax_quantize_device(const dann_transform* t, int32_t bits, float grid_scale, const float* d_x,
                                               uint64_t x_stride, uint32_t n, void* d_out, uint64_t out_stride,
                                               float* d_out_loss) try {
    using namespace dann;
    if (!t) return DANN_EINVAL;
    if (bad_bits("dann_minmax_quantize_device", bits, grid_scale)) return DANN_EINVAL;
    if (n == 0) return DANN_OK;
    if (!d_x || !d_out) return DANN_EINVAL;
    const size_t lb = kMmHeader + sq_code_bytes(48 + bits, t->out_dim);
    if (x_stride < t->in_dim || out_stride < lb) {
        set_error("dann_minmax_quantize_device: x_stride %llu floats / out_stride %llu bytes are below a row (%u floats) / "
                  "an image (%zu bytes)", (unsigned long long)x_stride, (unsigned long long)out_stride, t->in_dim, lb);
        return DANN_EINVAL;
    }
    DeviceGuard dev(t->device);
    if (!dev.ok) return hip_fail(hipErrorInvalidDevice, "hipSetDevice");
    // the transformed rows, packed; images that are not packed in d_out are compressed into a packed scratch first (the
    // compressor ORs codes into zeroed images, and the bytes between the caller's images are not ours to clear)
    DevBuf dtx, dimg, dflag;
    DANN_HIP(dtx.alloc((size_t)n * t->out_dim * 4));
    DANN_HIP(dflag.alloc(4));
    uint8_t* img = static_cast<uint8_t*>(d_out);
    if (out_stride != lb) {
        DANN_HIP(dimg.alloc((size_t)n * lb));
        img = static_cast<uint8_t*>(dimg.p);
    }
    if (int32_t rc = launch_transform(*t, d_x, x_stride, n, static_cast<float*>(dtx.p), t->out_dim, nullptr)) return rc;
    DANN_HIP(hipMemsetAsync(img, 0, (size_t)n * lb, nullptr));
    DANN_HIP(hipMemsetAsync(dflag.p, 0, 4, nullptr));
    if (int32_t rc = launch_minmax_compress(bits, static_cast<const float*>(dtx.p), n, t->out_dim, grid_scale, img,
                                            d_out_loss, static_cast<uint32_t*>(dflag.p), nullptr))
        return rc;
    if (out_stride != lb)
        DANN_HIP(hipMemcpy2DAsync(d_out, out_stride, img, lb, lb, n, hipMemcpyDeviceToDevice, nullptr));
    uint32_t flag = 0;
    DANN_HIP(hipMemcpy(&flag, dflag.p, 4, hipMemcpyDeviceToHost));
    DANN_HIP(hipStreamSynchronize(nullptr));
    if (flag) {
        set_error("dann_minmax_quantize_device: a transformed vector contains a NaN (InputContainsNaN)");
        return DANN_EINVAL;
    }
    return DANN_OK;
} DANN_CATCH_ALL

extern "C" int32_t dann_minmax_quantize(const dann_transform* t, int32_t bits, float grid_scale, const float* x, uint32_t n,
                                        void* out, float* out_loss) try {
    using namespace dann;
    if (!t) return DANN_EINVAL;
    if (bad_bits("dann_minmax_quantize", bits, grid_scale)) return DANN_EINVAL;
    if (n == 0) return DANN_OK;
    if (!x || !out) return DANN_EINVAL;
    DeviceGuard dev(t->device);
    if (!dev.ok) return hip_fail(hipErrorInvalidDevice, "hipSetDevice");
    const size_t lb = kMmHeader + sq_code_bytes(48 + bits, t->out_dim);
    const size_t xb = (size_t)n * t->in_dim * 4, ob = (size_t)n * lb;
    DevBuf dx, dout, dloss;
    DANN_HIP(dx.alloc(xb));
    DANN_HIP(dout.alloc(ob));
    if (out_loss) DANN_HIP(dloss.alloc((size_t)n * 4));
    DANN_HIP(hipMemcpy(dx.p, x, xb, hipMemcpyHostToDevice));
    const int32_t rc = dann_minmax_quantize_device(t, bits, grid_scale, static_cast<const float*>(dx.p), t->in_dim, n, dout.p,
                                                   lb, static_cast<float*>(dloss.p));
    if (rc != DANN_OK && rc != DANN_EINVAL) return rc;  // (a NaN: the outputs are still handed back, as dann_minmax_compress does)
    DANN_HIP(hipMemcpy(out, dout.p, ob, hipMemcpyDeviceToHost));
    if (out_loss) DANN_HIP(hipMemcpy(out_loss, dloss.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    return rc;
} DANN_CATCH_ALL
