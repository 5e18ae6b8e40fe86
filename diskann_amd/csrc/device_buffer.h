// device_buffer.h -- the owner of one device allocation and the pool-size rounding, shared by every translation unit's
// host code (dann_internal.h includes it).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dann {

// One device allocation, freed when the object goes or is allocated again.  (The grow-only staging of a search context,
// SearchCtx::stage, and the pieces carved from it are a different mechanism.)
struct DevBuf {
    void* p = nullptr;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { reset(); }
    void reset() {
        if (p) (void)hipFree(p);
        p = nullptr;
    }
    hipError_t alloc(size_t bytes) {  // (at least one byte: a buffer that was allocated is never null)
        reset();
        return hipMalloc(&p, bytes ? bytes : 1);
    }
    template <class T>
    T* as() const {
        return reinterpret_cast<T*>(p);
    }
};

// smallest power of two >= x, at least 64 (one wavefront): the capacity of a candidate pool
inline uint32_t pow2_at_least(uint32_t x) {
    uint32_t p = 64;
    while (p < x) p <<= 1;
    return p;
}

}  // namespace dann
