// ik_path.hip -- the per-waypoint selection of optik_hip_ik_path: P paths, each waypoint solved from the seed its path
// carries (the last accepted solution, or the path's start), over the per-restart keys, x and f a solver launch
// leaves behind.
//
// The candidates of a path at a waypoint are its restarts with a finite key (the successes, lib.rs:376-379) whose
// L-infinity joint distance to the seed is <= max_step (max_step = +inf admits every success).  The accepted one is
// their (key, restart index) minimum, the order of ik_argmin.hpp.
//
//   ik_path_select_kernel   one 256-thread block per path, its R <= 4096 restarts in one tile: the filtered argmin,
//                           the waypoint's outputs, and the path's next seed (the accepted solution, else the seed)
// Distances use subtraction, fabs and comparisons only: the result is exact and does not depend on the launch shape.
// The kernel also puts the launch's work-item counter back to 0 and, after a launch with early exit, the paths'
// first-success words back to ~0, so that the next waypoint's launch needs no fill commands in front of it.
#include "ik_argmin.hpp"
#include "ik_host.hpp"

namespace optik {
namespace host {
namespace {

constexpr int PATH_BLOCK = 256;

// max_i |x_i(col) - c_i|.  (NaN terms are skipped by the comparison; the successes the distance is taken of are finite.)
__device__ __forceinline__ double path_linf(const PathSelectLaunch &a, size_t col, const double *s_c) {
    double d = 0.0;
    for (int i = 0; i < a.n; ++i) {
        const double e = fabs(a.out_x[(size_t)i * a.ld + col] - s_c[i]);
        if (e > d) d = e;
    }
    return d;
}

__global__ __launch_bounds__(PATH_BLOCK) void ik_path_select_kernel(const PathSelectLaunch a) {
    __shared__ double s_key[PATH_BLOCK / WAVE];
    __shared__ unsigned long long s_idx[PATH_BLOCK / WAVE];
    __shared__ double s_c[WIDE_MAX_DOF];  // the seed this waypoint was solved from
    const int p = blockIdx.x;
    // (every read of the seed happens before the barrier: `carry` may be `seed`, and it is written after it)
    if ((int)threadIdx.x < a.n) s_c[threadIdx.x] = a.seed[(size_t)p * a.n + threadIdx.x];
    __syncthreads();
    const size_t base = (size_t)p * a.n_restarts;
    double key = 0.0;
    unsigned long long idx = ~0ull;
    for (unsigned long long r = threadIdx.x; r < a.n_restarts; r += PATH_BLOCK) {
        const double k = a.out_key[base + r];
        if (!(k < __builtin_huge_val())) continue;
        if (a.filter && !(path_linf(a, base + r, s_c) <= a.max_step)) continue;
        const unsigned long long i = a.restart_begin + r;
        if (argmin_takes(key, idx, k, i)) { key = k; idx = i; }
    }
    block_argmin<PATH_BLOCK>(key, idx, s_key, s_idx);
    const bool found = idx != ~0ull;
    const size_t col = base + (found ? (size_t)(idx - a.restart_begin) : 0);
    if ((int)threadIdx.x < a.n) {
        const int i = threadIdx.x;
        const size_t o = (size_t)p * a.n + i;
        const double v = found ? a.out_x[(size_t)i * a.ld + col] : __builtin_nan("");
        if (a.x) a.x[o] = v;
        const double next = found ? v : s_c[i];
        a.carry[o] = next;
        if (a.last) a.last[o] = next;
    }
    if (threadIdx.x == 0) {
        double step = __builtin_nan("");
        if (found) {
            step = 0.0;
            for (int i = 0; i < a.n; ++i) {
                const double e = fabs(a.out_x[(size_t)i * a.ld + col] - s_c[i]);
                if (e > step) step = e;
            }
        }
        if (a.f) a.f[p] = (found && a.out_f) ? a.out_f[col] : __builtin_nan("");
        if (a.idx) a.idx[p] = idx;
        if (a.key) a.key[p] = found ? key : __builtin_huge_val();
        if (a.step) a.step[p] = step;
        if (a.reset_fs) a.reset_fs[p] = ~0ull;
        if (a.reset_queue && p == 0) *a.reset_queue = 0ull;
    }
}

}  // namespace

hipError_t path_select_launch(const PathSelectLaunch &s, int P, hipStream_t stream) {
    hipLaunchKernelGGL(ik_path_select_kernel, dim3(P), dim3(PATH_BLOCK), 0, stream, s);
    return hipGetLastError();
}

}  // namespace host
}  // namespace optik
