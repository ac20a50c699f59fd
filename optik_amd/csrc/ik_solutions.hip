// ik_solutions.hip -- up to K distinct solutions per target (optik_hip_ik_solutions) over the per-restart keys, x and
// f a solver launch leaves behind.
//
// The candidates of a target are its restarts with a finite key (the successes, lib.rs:376-379), ordered by (key,
// restart index).  They are taken greedily in that order: one is accepted if its L-infinity joint distance to every
// solution accepted before it is > min_dist, up to K of them.  The same set comes from K rounds of
//     accept the (key, index)-minimum of the surviving candidates; eliminate every survivor within min_dist of it
// (the minimum survivor is never within min_dist of an earlier acceptance).  A candidate is alive while its key in
// the launch's scratch key array is finite: an eliminated one's key is set to +inf there.
//
//   ik_solutions_small_kernel   every round of one target in one 256-thread block, when its restarts fit one
//                               4096-restart tile (the keys stay in registers; one launch for the whole selection)
//   ik_solutions_tile_kernel    per tile and round: eliminate against the previous round's acceptance, then the
//                               (key, index) argmin of the tile's survivors -> one 16-byte record
//   ik_solutions_pick_kernel    per target and round: the minimum of its tile records, published to slot k
// Distances use subtraction, fabs and comparisons only: the result is exact and does not depend on the launch shape.
// The last kernel of the selection puts the launch's work-item counter back to 0 (the first-success words are not
// used: every restart runs to its end).
#include "ik_argmin.hpp"
#include "ik_host.hpp"

namespace optik {
namespace host {
namespace {

constexpr int SOL_BLOCK = 256;
constexpr int SOL_PER_THREAD = SEL_TILE / SOL_BLOCK;  // restarts of a tile per thread

// max_i |x_i(col) - a_i|.  (NaN terms are skipped by the comparison; the successes the distance is taken of are finite.)
__device__ __forceinline__ double linf_dist(const SolutionsLaunch &a, size_t col, const double *s_a) {
    double d = 0.0;
    for (int i = 0; i < a.n; ++i) {
        const double e = fabs(a.out_x[(size_t)i * a.ld + col] - s_a[i]);
        if (e > d) d = e;
    }
    return d;
}

// Slot k of target t gets the solution in column col (lanes < n write x, lane 0 the rest).
__device__ __forceinline__ void put_solution(const SolutionsLaunch &a, int t, int k, size_t col, double key,
                                             unsigned long long idx) {
    const size_t s = (size_t)t * a.K + k;
    if (a.x && (int)threadIdx.x < a.n) a.x[s * a.n + threadIdx.x] = a.out_x[(size_t)threadIdx.x * a.ld + col];
    if (threadIdx.x == 0) {
        if (a.f) a.f[s] = a.out_f[col];
        if (a.idx) a.idx[s] = idx;
        if (a.key) a.key[s] = key;
    }
}

// Slots [k0, k1) of target t are padding: x and f NaN, index ~0, key +inf (the whole block writes).
__device__ __forceinline__ void pad_slots(const SolutionsLaunch &a, int t, int k0, int k1) {
    const size_t s0 = (size_t)t * a.K;
    for (int k = k0 + (int)threadIdx.x; k < k1; k += blockDim.x) {
        if (a.f) a.f[s0 + k] = __builtin_nan("");
        if (a.idx) a.idx[s0 + k] = ~0ull;
        if (a.key) a.key[s0 + k] = __builtin_huge_val();
    }
    if (a.x)
        for (int e = k0 * a.n + (int)threadIdx.x; e < k1 * a.n; e += blockDim.x) a.x[s0 * a.n + e] = __builtin_nan("");
}

// One target per block, its restarts in one tile: all K rounds here.
__global__ __launch_bounds__(SOL_BLOCK) void ik_solutions_small_kernel(const SolutionsLaunch a) {
    __shared__ double s_key[SOL_BLOCK / WAVE];
    __shared__ unsigned long long s_idx[SOL_BLOCK / WAVE];
    __shared__ double s_a[WIDE_MAX_DOF];  // the solution accepted last
    const int t = blockIdx.x;
    const size_t base = (size_t)t * a.n_restarts;
    double kk[SOL_PER_THREAD];  // this thread's keys: +inf = not (or no longer) a candidate
#pragma unroll
    for (int j = 0; j < SOL_PER_THREAD; ++j) {
        const unsigned long long r = threadIdx.x + (unsigned long long)j * SOL_BLOCK;
        kk[j] = r < a.n_restarts ? a.out_key[base + r] : __builtin_huge_val();
    }
    int count = 0;
    for (int k = 0; k < a.K; ++k) {
        double key = 0.0;
        unsigned long long idx = ~0ull;
#pragma unroll
        for (int j = 0; j < SOL_PER_THREAD; ++j) {
            const unsigned long long i = a.restart_begin + threadIdx.x + (unsigned long long)j * SOL_BLOCK;
            if (kk[j] < __builtin_huge_val() && argmin_takes(key, idx, kk[j], i)) { key = kk[j]; idx = i; }
        }
        block_argmin<SOL_BLOCK>(key, idx, s_key, s_idx);
        if (idx == ~0ull) break;  // (the same for the whole block)
        const size_t col = base + (size_t)(idx - a.restart_begin);
        if ((int)threadIdx.x < a.n) s_a[threadIdx.x] = a.out_x[(size_t)threadIdx.x * a.ld + col];
        put_solution(a, t, k, col, key, idx);
        count = k + 1;
        __syncthreads();
        if (count == a.K) break;  // (nothing to eliminate for)
#pragma unroll
        for (int j = 0; j < SOL_PER_THREAD; ++j) {
            if (kk[j] < __builtin_huge_val()) {
                const size_t c = base + threadIdx.x + (size_t)j * SOL_BLOCK;
                if (!(linf_dist(a, c, s_a) > a.min_dist)) kk[j] = __builtin_huge_val();
            }
        }
        // (s_a is written again only after the next round's block_argmin, whose barriers every thread passes after
        // its eliminations)
    }
    pad_slots(a, t, count, a.K);
    if (threadIdx.x == 0) {
        if (a.count) a.count[t] = count;
        if (a.reset_queue && t == 0) *a.reset_queue = 0ull;
    }
}

// Round k, one tile of one target: eliminate the survivors within min_dist of round k-1's acceptance (their keys go
// to +inf in the scratch array), then the argmin of what is left.
__global__ __launch_bounds__(SOL_BLOCK) void ik_solutions_tile_kernel(const SolutionsLaunch a, int k) {
    __shared__ double s_key[SOL_BLOCK / WAVE];
    __shared__ unsigned long long s_idx[SOL_BLOCK / WAVE];
    __shared__ double s_a[WIDE_MAX_DOF];
    // (one-dimensional grid over target-major tiles, as ik_tile_argmin_kernel)
    const int t = (int)(blockIdx.x / (unsigned)a.tiles_per_target);
    const int tile = (int)(blockIdx.x % (unsigned)a.tiles_per_target);
    TileRec *rec = a.tile_recs + (size_t)t * a.tiles_per_target + tile;
    const unsigned long long prev = k > 0 ? a.pick[t] : ~0ull;
    if (k > 0 && prev == ~0ull) {  // the target ran out of candidates in an earlier round
        if (threadIdx.x == 0) { TileRec r; r.idx = ~0ull; r.key = 0.0; *rec = r; }
        return;
    }
    if (k > 0 && (int)threadIdx.x < a.n) s_a[threadIdx.x] = a.out_x[(size_t)threadIdx.x * a.ld + prev];
    __syncthreads();
    const unsigned long long lo = (unsigned long long)tile * (unsigned long long)a.tile;
    const size_t base = (size_t)t * a.n_restarts;
    double key = 0.0;
    unsigned long long idx = ~0ull;
#pragma unroll
    for (int j = 0; j < SOL_PER_THREAD; ++j) {
        const unsigned long long r = lo + threadIdx.x + (unsigned long long)j * SOL_BLOCK;
        if (r >= a.n_restarts) break;
        double kr = a.out_key[base + r];
        if (!(kr < __builtin_huge_val())) continue;
        if (k > 0 && !(linf_dist(a, base + r, s_a) > a.min_dist)) {
            a.out_key[base + r] = __builtin_huge_val();
            continue;
        }
        const unsigned long long i = a.restart_begin + r;
        if (argmin_takes(key, idx, kr, i)) { key = kr; idx = i; }
    }
    block_argmin<SOL_BLOCK>(key, idx, s_key, s_idx);
    if (threadIdx.x == 0) { TileRec r; r.idx = idx; r.key = key; *rec = r; }
}

// Round k, one 64-lane block per target: the minimum of the tile records is accepted into slot k.
__global__ __launch_bounds__(WAVE) void ik_solutions_pick_kernel(const SolutionsLaunch a, int k) {
    const int t = blockIdx.x;
    double key = 0.0;
    unsigned long long idx = ~0ull;
    for (int i = threadIdx.x; i < a.tiles_per_target; i += WAVE) {
        const TileRec r = a.tile_recs[(size_t)t * a.tiles_per_target + i];
        if (argmin_takes(key, idx, r.key, r.idx)) { key = r.key; idx = r.idx; }
    }
    wave_argmin(key, idx);
    if (idx != ~0ull) {
        const size_t col = (size_t)t * a.n_restarts + (size_t)(idx - a.restart_begin);
        put_solution(a, t, k, col, key, idx);
        if (threadIdx.x == 0) {
            a.pick[t] = col;
            if (a.count) a.count[t] = k + 1;
        }
    } else {
        pad_slots(a, t, k, k + 1);
        if (threadIdx.x == 0) {
            a.pick[t] = ~0ull;
            if (a.count && k == 0) a.count[t] = 0;
        }
    }
    if (a.reset_queue && k + 1 == a.K && t == 0 && threadIdx.x == 0) *a.reset_queue = 0ull;
}

}  // namespace

hipError_t solutions_launch(const SolutionsLaunch &s, int T, hipStream_t stream) {
    if (s.tiles_per_target == 1) {
        hipLaunchKernelGGL(ik_solutions_small_kernel, dim3(T), dim3(SOL_BLOCK), 0, stream, s);
        return hipGetLastError();
    }
    const unsigned tiles = (unsigned)(s.tiles_per_target * (long long)T);
    for (int k = 0; k < s.K; ++k) {
        hipLaunchKernelGGL(ik_solutions_tile_kernel, dim3(tiles), dim3(SOL_BLOCK), 0, stream, s, k);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
        hipLaunchKernelGGL(ik_solutions_pick_kernel, dim3(T), dim3(WAVE), 0, stream, s, k);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace host
}  // namespace optik
