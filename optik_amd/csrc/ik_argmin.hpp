// ik_argmin.hpp -- the (key, restart index) order of the selection kernels (ik_select.hip, ik_solutions.hip,
// ik_path.hip): the smaller key first, ties to the smaller index; index ~0 = no entry.
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

// The argmin of a BLOCK-thread block (BLOCK / 64 waves); every thread ends with it.  s_key / s_idx: BLOCK / 64
// shared entries, free again on return.
template <int BLOCK>
__device__ __forceinline__ void block_argmin(double &key, unsigned long long &idx, double *s_key,
                                             unsigned long long *s_idx) {
    wave_argmin(key, idx);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { s_key[wave] = key; s_idx[wave] = idx; }
    __syncthreads();
    key = s_key[0];
    idx = s_idx[0];
    for (int w = 1; w < BLOCK / 64; ++w)
        if (argmin_takes(key, idx, s_key[w], s_idx[w])) { key = s_key[w]; idx = s_idx[w]; }
    __syncthreads();
}

}  // namespace host
}  // namespace optik
