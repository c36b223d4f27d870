// bn_buffer.hpp -- owners of the host side's device memory, page-locked memory and function-local streams and events.  Host code
// only: no .hip file includes it.  A handle converts to the raw pointer, so it goes straight into kernel arguments and HIP calls;
// it frees what it holds when it is reset, assigned over or destroyed.  Release happens on the CURRENT device: an owner of
// device memory is destroyed inside its DeviceGuard (free_engine, ~bn_info_table).  MappedBuf is the owner of page-locked memory
// that kernels read and write in place: the block, the address the device sees it at and the number of elements it holds, kept
// together so that none of the three can outlive the others.
#pragma once

#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstddef>
#include <utility>

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


// A block of mapped page-locked memory (hipHostMallocMapped).  Converts to and indexes as the host pointer; dev() is the same memory
// as the device sees it.  Memory comes from alloc() or reserve() alone, and both end with the capacity: a failure on the way leaves
// the object empty -- no pointer, no alias, capacity 0 -- so the next call allocates again.
template <class T>
class MappedBuf {
public:
    MappedBuf() = default;
    MappedBuf(const MappedBuf&) = delete;
    MappedBuf& operator=(const MappedBuf&) = delete;
    MappedBuf(MappedBuf&& o) noexcept : host_(std::move(o.host_)), dev_(o.dev_), cap_(o.cap_) { o.dev_ = nullptr; o.cap_ = 0; }
    MappedBuf& operator=(MappedBuf&& o) noexcept {
        if (this != &o) {
            host_ = std::move(o.host_);
            dev_ = o.dev_; cap_ = o.cap_;
            o.dev_ = nullptr; o.cap_ = 0;
        }
        return *this;
    }

    operator T*() const { return host_; }
    T* operator->() const { return host_; }
    T* get() const { return host_; }
    T* dev() const { return dev_; }
    size_t capacity() const { return cap_; }   // elements
    // a buffer sized once: exactly max(count, 1) elements
    hipError_t alloc(size_t count) { return take(std::max<size_t>(count, 1) * sizeof(T)); }
    // a buffer that grows with the calls: nothing at or below the capacity, else twice what is asked for (4096 bytes at least)
    hipError_t reserve(size_t count) { return count <= cap_ ? hipSuccess : take(std::max<size_t>(2 * count * sizeof(T), 4096)); }

private:
    hipError_t take(size_t bytes) {
        cap_ = 0;
        dev_ = nullptr;
        hipError_t e = host_malloc(host_, bytes, hipHostMallocMapped);   // (frees the block held before)
        if (e != hipSuccess) return e;
        void* d = nullptr;
        e = hipHostGetDevicePointer(&d, host_, 0);
        if (e != hipSuccess) { host_.reset(); return e; }
        dev_ = static_cast<T*>(d);
        cap_ = bytes / sizeof(T);
        return hipSuccess;
    }
    PinnedBuf<T> host_;
    T* dev_ = nullptr;
    size_t cap_ = 0;
};

}  // namespace bnmi
