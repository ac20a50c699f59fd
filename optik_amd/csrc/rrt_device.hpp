// rrt_device.hpp -- what the two tree-planner units share on the device side: the launch record of ik_rrt.hip's
// kernels and the host loop over the iterations (ik_rrt.hip defines it; ik_rrt_goals.hip runs the same loop, and so
// the same rrt_step_kernel, on trees that its own begin kernel has rooted: DESIGN.md sections 5.26 and 5.28).
#pragma once

#include "collision_device.hpp"
#include "rrt_measure.hpp"

namespace optik {
namespace rrtdev {

constexpr int RRT_BLOCK = 256, RRT_WAVE = 64;
constexpr long long MAX_QUERIES = 1ll << 30;

struct RrtLaunch {
    long long Q, q0, Qc;         // the call's queries; the chunk's first and its count
    int n, M, Lmax, I, iter;
    double eta;
    const double *start, *goal;  // [n][Q] the caller's
    const double *lo, *hi;       // [n] the joint limits (the chain's table)
    const double *samples;       // [n][I]
    double *s, *g;               // [n][Qc] the chunk's ends
    const uint8_t *flags;        // begin: [3][Qc] start free, goal free, direct free; step: [3][Qc] the segments' flags
    double *conf;                // [Qc][2][n][M]
    int32_t *parent;             // [Qc][2][M]
    int32_t *count;              // [2][Qc]
    int32_t *state;              // [Qc] rrt::RUNNING or how the query ended
    int32_t *junction;           // [2][Qc]
    int32_t *used;               // [Qc]
    int32_t *pend;               // [3][Qc] the iteration in flight: p (-1: none), m, whether tree b extends
    double *qa, *qb;             // [n][3 Qc] the segments, column s * Qc + q
    int32_t *unfinished;         // [1]
    double *path;                // [Lmax][Q][n] or null
    int32_t *len, *status, *iters, *nodes;  // [Q], nodes [2][Q]; or null
    double *cost;
};

__device__ __forceinline__ double *tree_conf(const RrtLaunch &a, long long q, int t) {
    return a.conf + ((size_t)q * 2 + t) * (size_t)a.n * a.M;
}
__device__ __forceinline__ int32_t *tree_parent(const RrtLaunch &a, long long q, int t) {
    return a.parent + ((size_t)q * 2 + t) * (size_t)a.M;
}

// every segment of query q is "not sampled" from here on
__device__ __forceinline__ void clear_segments(const RrtLaunch &a, long long q, int i) {
    const long long B = 3 * a.Qc;
    for (int s = 0; s < 3; ++s) {
        a.qa[(long long)i * B + s * a.Qc + q] = roadmap::nan_value();
        a.qb[(long long)i * B + s * a.Qc + q] = roadmap::nan_value();
    }
}

inline unsigned blocks(long long work) { return (unsigned)((work + RRT_BLOCK - 1) / RRT_BLOCK); }
inline size_t align16(size_t bytes) { return (bytes + 15) & ~(size_t)15; }

// what optik_hip_rrt_plan refuses before any device work; 0 to go on
int check_args(const optik_hip_chain *ch, int64_t Q, int32_t iters, double step, double resolution, int32_t max_nodes,
               int32_t Lmax, int32_t poll);

// The iterations of the chunk a.q0, a.Qc whose begin kernel has run on `stream`: rrt_step_kernel and the motion check
// over the 3 a.Qc segments per iteration, one read of *a.unfinished every `poll` iterations, and the last commit with
// rule 6.  d_flags is a.flags.  The caller's walk kernel comes next on the stream.
int run_iterations(optik_hip_chain *ch, const double *ee_offset7, RrtLaunch &a, int32_t iters, int32_t poll,
                   double resolution, uint8_t *d_flags, hipStream_t stream);

}  // namespace rrtdev
}  // namespace optik
