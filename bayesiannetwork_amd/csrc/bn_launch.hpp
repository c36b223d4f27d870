// bn_launch.hpp -- the host side of a plain kernel launch, for the .hip files that report a launch's error to their caller.
#pragma once

#include <hip/hip_runtime.h>

namespace bnmi {

// drop any stale error of this thread, launch, 0 or the hipError_t
template <class F>
inline int launched(F launch) {
    (void)hipGetLastError();
    launch();
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : int(e);
}

}  // namespace bnmi
