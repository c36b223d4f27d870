// bn_item_launch.hpp -- host side of launching an item kernel (bn_small.hip, bn_em.hip, bn_mid.hip, bn_maxprod.hip): every one is a
// template over ROUNDS = items of one kind per thread, instantiated for 1, 2 and kSmallMaxRounds.  A kernel family is handed over as a
// generic lambda  [](auto R) { return some_kernel<decltype(R)::value>; }  (a function template cannot be a template argument).
#pragma once

#include <hip/hip_runtime.h>

#include <initializer_list>
#include <type_traits>

#include "bn_small.hpp"

namespace bnmi {

inline int item_rounds(int re, int rb, int rc) { return re > rb ? (re > rc ? re : rc) : (rb > rc ? rb : rc); }

// f(integral_constant<int, R>) for the instantiation that holds `rounds` rounds of items
template <class F>
auto with_item_rounds(int rounds, F&& f) {
    if (rounds <= 1) return f(std::integral_constant<int, 1>{});
    if (rounds <= 2) return f(std::integral_constant<int, 2>{});
    return f(std::integral_constant<int, kSmallMaxRounds>{});
}

// once per device before the first launch: a kernel's dynamic LDS may exceed the 64 KiB default.  0 or the hipError_t.
template <class... Families>
int prepare_item_kernels(Families... kernel_of) {
    (void)hipGetLastError();
    hipError_t e = hipSuccess;
    auto set = [&](auto family) {
        for (const int rounds : {1, 2, kSmallMaxRounds})
            if (e == hipSuccess)
                e = with_item_rounds(rounds, [&](auto R) {
                    return hipFuncSetAttribute(reinterpret_cast<const void*>(family(R)), hipFuncAttributeMaxDynamicSharedMemorySize, kSmallLdsBytes);
                });
    };
    (set(kernel_of), ...);
    return e == hipSuccess ? 0 : int(e);
}

// 0 or the hipError_t of the launch
template <class Family, class... Args>
int launch_item_kernel(int rounds, Family kernel_of, dim3 grid, dim3 block, size_t lds_bytes, void* stream, const Args&... args) {
    (void)hipGetLastError();  // drop any stale error of this thread
    with_item_rounds(rounds, [&](auto R) { hipLaunchKernelGGL(kernel_of(R), grid, block, lds_bytes, (hipStream_t)stream, args...); });
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : int(e);
}

}  // namespace bnmi
