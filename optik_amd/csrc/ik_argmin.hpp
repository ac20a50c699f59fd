// ik_argmin.hpp -- the (key, restart index) order of the selection kernels (ik_select.hip, ik_solutions.hip):
// the smaller key first, ties to the smaller index; index ~0 = no entry.
#pragma once

#include <hip/hip_runtime.h>

namespace optik {
namespace host {

// Does (okey, oidx) come before (key, idx)?
__device__ __forceinline__ bool argmin_takes(double key, unsigned long long idx, double okey, unsigned long long oidx) {
    return (oidx != ~0ull) && (idx == ~0ull || okey < key || (okey == key && oidx < idx));
}

// (key, idx) argmin across the wave: smaller key wins, ties -> smaller idx; idx ~0 = none.  Every lane ends with it.
__device__ __forceinline__ void wave_argmin(double &key, unsigned long long &idx) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const double okey = __shfl_xor(key, off, 64);
        const unsigned long long oidx = __shfl_xor(idx, off, 64);
        if (argmin_takes(key, idx, okey, oidx)) { key = okey; idx = oidx; }
    }
}

}  // namespace host
}  // namespace optik
