// transform.h -- the device-resident Transform (transform_kernels.hip) as the units that apply one see it
// (dann_minmax_quantize there, the spherical compressor in spherical_kernels.hip).
#pragma once
#include "dann_internal.h"

struct dann_transform {
    int device = 0;
    int32_t kind = 0;
    uint32_t in_dim = 0, out_dim = 0;
    uint32_t work = 0;  // PaddingHadamard: padded_dim; DoubleHadamard: max(input_dim, output_dim)
    uint32_t t = 0;     // length of one Hadamard transform (DoubleHadamard: the largest power of two <= work)
    float m = 1.0f, rescale = 1.0f;
    uint32_t *d_signs0 = nullptr, *d_signs1 = nullptr, *d_sub = nullptr;
    dann_transform() = default;
    dann_transform(const dann_transform&) = delete;  // (owns its device arrays)
    dann_transform& operator=(const dann_transform&) = delete;
    ~dann_transform() {
        if (d_signs0) (void)hipFree(d_signs0);
        if (d_signs1) (void)hipFree(d_signs1);
        if (d_sub) (void)hipFree(d_sub);
    }
    // Transform::preserves_norms: NullTransform always, the Hadamard ones without a subsample
    bool preserves_norms() const { return d_sub == nullptr; }
    uint32_t signs1_len() const { return kind == DANN_TRANSFORM_DOUBLE_HADAMARD ? work : 0u; }
};

namespace dann {
// n rows d_x -> d_out on the current device (the transform's), queued on `st`; strides in floats
int32_t launch_transform(const dann_transform& t, const float* d_x, uint64_t xs, uint32_t n, float* d_out, uint64_t os,
                         hipStream_t st);
}  // namespace dann
