// bn_buffer.hpp -- owners of the host side's device memory, page-locked memory and function-local streams and events.  Host code
// only: no .hip file includes it.  A handle converts to the raw pointer, so it goes straight into kernel arguments and HIP calls;
// it frees what it holds when it is reset, assigned over or destroyed.  Release happens on the CURRENT device: an owner of
// device memory is destroyed inside its DeviceGuard (free_engine, ~bn_info_table).
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstddef>

namespace bnmi {

template <class H, class R, hipError_t (*Release)(R)>
class HipOwner {
public:
    HipOwner() = default;
    HipOwner(const HipOwner&) = delete;
    HipOwner& operator=(const HipOwner&) = delete;
    HipOwner(HipOwner&& o) noexcept : h_(o.h_) { o.h_ = nullptr; }
    HipOwner& operator=(HipOwner&& o) noexcept {
        if (this != &o) { reset(o.h_); o.h_ = nullptr; }
        return *this;
    }
    ~HipOwner() { reset(); }

    operator H() const { return h_; }
    H operator->() const { return h_; }
    H get() const { return h_; }
    void reset(H h = nullptr) {
        if (h_) (void)Release(h_);
        h_ = h;
    }
    // the out-parameter of a creating call (hipStreamCreate...): empties the owner first
    H* put() { reset(); return &h_; }
    // allocate(void**) is hipMalloc or one of its kin; what was held is freed first, and a failure leaves the owner empty
    template <class F>
    hipError_t alloc(F allocate) {
        reset();
        void* p = nullptr;
        const hipError_t e = allocate(&p);
        if (e == hipSuccess) h_ = static_cast<H>(p);
        return e;
    }

private:
    H h_ = nullptr;
};

template <class T> using DeviceBuf = HipOwner<T*, void*, hipFree>;
template <class T> using PinnedBuf = HipOwner<T*, void*, hipHostFree>;
using StreamOwner = HipOwner<hipStream_t, hipStream_t, hipStreamDestroy>;
using EventOwner = HipOwner<hipEvent_t, hipEvent_t, hipEventDestroy>;

template <class T>
inline hipError_t dev_malloc(DeviceBuf<T>& b, size_t bytes) {
    return b.alloc([&](void** p) { return hipMalloc(p, bytes); });
}
// fine-grained (system-coherent) device memory: peers store into it from their kernels
template <class T>
inline hipError_t dev_malloc_fine(DeviceBuf<T>& b, size_t bytes) {
    return b.alloc([&](void** p) { return hipExtMallocWithFlags(p, bytes, hipDeviceMallocFinegrained); });
}
template <class T>
inline hipError_t host_malloc(PinnedBuf<T>& b, size_t bytes, unsigned flags) {
    return b.alloc([&](void** p) { return hipHostMalloc(p, bytes, flags); });
}

}  // namespace bnmi
