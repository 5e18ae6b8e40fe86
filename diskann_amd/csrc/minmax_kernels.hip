// minmax_kernels.hip -- MinMaxQuantizer::compress_into on the GPU (diskann-quantization/src/minmax/quantizer.rs:117-228)
// for vectors that have already been through the quantiser's transform.  Not a hot path: one row per lane, every
// order-dependent f32 chain (the 1-bit range's mean and partial sums, norm_squared, the loss) runs sequentially in that
// lane exactly as the reference's iterators do; no operation is fused (-ffp-contract=off).
#include "dann_device.h"
#include "dann_internal.h"

namespace dann {
namespace {

// f32::min / f32::max: a NaN operand loses
__device__ __forceinline__ float rust_min(float a, float b) { return a != a ? b : b != b ? a : (b < a ? b : a); }
__device__ __forceinline__ float rust_max(float a, float b) { return a != a ? b : b != b ? a : (b > a ? b : a); }

template <int BITS>
__global__ __launch_bounds__(64) void minmax_compress_kernel(const float* __restrict__ x, uint32_t n, uint32_t dim,
                                                             float grid_scale, uint8_t* __restrict__ out,
                                                             float* __restrict__ out_loss, uint32_t* nan_flag) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const float* v = x + (uint64_t)r * dim;
    const uint32_t lb = kMmHeader + sq_code_bytes(48 + BITS, dim);
    uint8_t* img = out + (uint64_t)r * lb;  // (zeroed by the host: the padding bits stay zero)
    float lo, hi;
    if constexpr (BITS == 1) {
        float sum = 0.0f;
        for (uint32_t i = 0; i < dim; ++i) sum += v[i];
        const float mean = sum / (float)dim;
        float mn = 0.0f, mnc = 0.0f, mx = 0.0f, mxc = 0.0f;
        for (uint32_t i = 0; i < dim; ++i) {
            const float e = v[i];
            const float m = e < mean ? 1.0f : 0.0f;
            mn += m * e;
            mnc += m;
            mx += (1.0f - m) * e;
            mxc += 1.0f - m;
        }
        lo = rust_min(mn / mnc, mean);
        hi = rust_max(mx / mxc, mean);
    } else {
        lo = hi = __builtin_nanf("");
        for (uint32_t i = 0; i < dim; ++i) {
            lo = rust_min(lo, v[i]);
            hi = rust_max(hi, v[i]);
        }
    }
    const float width = (hi - lo) / 2.0f;
    const float mid = lo + width;
    const float rmin = mid - width * grid_scale, rmax = mid + width * grid_scale;
    constexpr float top = (float)((1 << BITS) - 1);
    const float inv = rust_max(rmax - rmin, 1e-8f) / top;
    float ns = 0.0f, csum = 0.0f, loss = 0.0f;
    bool nan = false;
    for (uint32_t i = 0; i < dim; ++i) {
        const float e = v[i];
        nan |= e != e;
        float t = (e - rmin) / inv;
        t = t < 0.0f ? 0.0f : t > top ? top : t;  // f32::clamp (a NaN stays)
        const float code = __builtin_roundf(t);   // half away from zero
        const float vr = code * inv + rmin;
        ns += vr * vr;
        csum += code;
        const float d = vr - e;
        loss += d * d;
        const uint32_t c = code == code ? (uint32_t)code : 0u;  // (`NaN as u8` is 0)
        if constexpr (BITS == 8) {
            img[kMmHeader + i] = (uint8_t)c;
        } else {
            const uint32_t bit = i * BITS;
            img[kMmHeader + (bit >> 3)] |= (uint8_t)(c << (bit & 7u));
        }
    }
    const float hdr[4] = {rmin, inv * csum, inv, ns};
    __builtin_memcpy(img, &dim, 4);
    __builtin_memcpy(img + 4, hdr, 16);
    if (out_loss) out_loss[r] = loss > 0.0f ? loss : 0.0f;  // L2Loss::as_f32
    if (nan) atomicOr(nan_flag, 1u);
}

}  // namespace

// minmax_compress_kernel on device buffers: x packed n x dim, out n zeroed packed images, out_loss optional, nan_flag cleared
int32_t launch_minmax_compress(int32_t bits, const float* px, uint32_t n, uint32_t dim, float grid_scale, uint8_t* po,
                               float* pl, uint32_t* pf, hipStream_t st) {
    const dim3 grid((n + 63u) / 64u), block(64);
    switch (bits) {
        case 1: hipLaunchKernelGGL(minmax_compress_kernel<1>, grid, block, 0, st, px, n, dim, grid_scale, po, pl, pf); break;
        case 2: hipLaunchKernelGGL(minmax_compress_kernel<2>, grid, block, 0, st, px, n, dim, grid_scale, po, pl, pf); break;
        case 4: hipLaunchKernelGGL(minmax_compress_kernel<4>, grid, block, 0, st, px, n, dim, grid_scale, po, pl, pf); break;
        default: hipLaunchKernelGGL(minmax_compress_kernel<8>, grid, block, 0, st, px, n, dim, grid_scale, po, pl, pf); break;
    }
    DANN_HIP(hipGetLastError());
    return DANN_OK;
}
}  // namespace dann

extern "C" int32_t dann_minmax_compress(int32_t device, int32_t bits, const float* x, uint32_t n, uint32_t dim,
                                        float grid_scale, void* out, float* out_loss) try {
    using namespace dann;
    if (bits != 1 && bits != 2 && bits != 4 && bits != 8) {
        set_error("dann_minmax_compress: bits must be 1, 2, 4 or 8 (got %d)", bits);
        return DANN_EINVAL;
    }
    if (dim == 0 || !(grid_scale > 0.0f)) {
        set_error("dann_minmax_compress: dim and grid_scale must be positive");
        return DANN_EINVAL;
    }
    if (n == 0) return DANN_OK;
    if (!x || !out) return DANN_EINVAL;
    if (device >= 0) DANN_HIP(hipSetDevice(device));
    const size_t lb = kMmHeader + sq_code_bytes(48 + bits, dim);
    const size_t xb = (size_t)n * dim * 4, ob = (size_t)n * lb;
    DevBuf dx, dout, dloss, dflag;
    DANN_HIP(dx.alloc(xb));
    DANN_HIP(dout.alloc(ob));
    DANN_HIP(dloss.alloc((size_t)n * 4));
    DANN_HIP(dflag.alloc(4));
    DANN_HIP(hipMemcpy(dx.p, x, xb, hipMemcpyHostToDevice));
    DANN_HIP(hipMemset(dout.p, 0, ob));
    DANN_HIP(hipMemset(dflag.p, 0, 4));
    if (int32_t rc = launch_minmax_compress(bits, static_cast<const float*>(dx.p), n, dim, grid_scale,
                                            static_cast<uint8_t*>(dout.p), static_cast<float*>(dloss.p),
                                            static_cast<uint32_t*>(dflag.p), nullptr))
        return rc;
    uint32_t flag = 0;
    DANN_HIP(hipMemcpy(&flag, dflag.p, 4, hipMemcpyDeviceToHost));
    DANN_HIP(hipMemcpy(out, dout.p, ob, hipMemcpyDeviceToHost));
    if (out_loss) DANN_HIP(hipMemcpy(out_loss, dloss.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    if (flag) {
        set_error("dann_minmax_compress: the input contains a NaN");
        return DANN_EINVAL;
    }
    return DANN_OK;
} DANN_CATCH_ALL
