// ik_spherefit.hip -- a greedy sphere cover of a solid from its distance field and surface points
// (spherefit_measure.hpp): optik_hip_sphere_fit (include/optik_hip.h).
//
//   fit_init_kernel     the outputs to "nothing chosen", the covered flags and the round state to zero.
//   fit_gain_kernel<false>  the initial gains: one candidate slot (node) per lane in memory order, every lane walks ALL
//                       points and counts the ones its sphere covers.
//   fit_pick_kernel     stage 1 of a round's argmax over (gain, node): a grid-stride block each, one record per block.
//   fit_choose_kernel   stage 2: one block reduces the records, writes the round's outputs and the pick, or, at gain 0,
//                       raises the `done` word; every later kernel of the call then returns at once.
//   fit_mark_kernel     tests the points still uncovered against the picked sphere, flags the newly covered ones and
//                       appends them to a list.  (The list's order depends on the run; only its set is used.)
//   fit_gain_kernel<true>   the update: the same shape as the gain pass over that list only, subtracting.  A slot whose
//                       gain is 0 can lose nothing and sits the loop out.  Over a call the updates test every
//                       (slot, point) pair at most once more, so the work is about 2 * C * P pair tests, not K * C * P.
//
// The points (the list's points) are staged through LDS in tiles of FIT_TILE (512 x 24 B = 12 KiB per block of 256
// lanes), as ik_mesh.hip stages triangles: the block loads a tile with lane-consecutive reads, then every lane reads
// point t of the tile at a wave-uniform address (a broadcast).  A lane past the last node of its launch computes the
// launch's last node again and stores nothing: it takes part in every tile load and every barrier.  A wave without a
// live candidate skips a tile's tests, not its barriers.
//
// All K rounds are enqueued on the stream without a host synchronisation: what a round decides (the pick, the length
// of the list, `done`) stays in device memory and the next kernels read it.  No kernel waits for another workgroup;
// every trip count is bounded by C, P or K.  The gain pass and the updates are cut by candidates into launches of at
// most FIT_PAIRS_PER_LAUNCH pair tests (an update's bound is taken with the whole P, since the host does not know the
// list's length).
#include <atomic>

#include "collision_model.hpp"
#include "ik_argmin.hpp"
#include "ik_host.hpp"
#include "spherefit_measure.hpp"

using namespace optik;
using namespace optik::host;

namespace {

constexpr int FIT_BLOCK = 256;
using coll::FIT_PAIRS_PER_LAUNCH;
using coll::FIT_PICK_BLOCKS;
using coll::FIT_TILE;
static_assert(FIT_PICK_BLOCKS <= FIT_BLOCK, "fit_choose_kernel reads one record per thread");

std::atomic<long long> g_pairs_per_launch{FIT_PAIRS_PER_LAUNCH};

// the round state (int32 words at the workspace's end)
enum { ST_NEW = 0, ST_DONE = 1, ST_PICK = 2, ST_COVERED = 3, ST_COUNT = 4, ST_WORDS = 16 };

struct FitLaunch {
    double origin[3], voxel, pad, slack;
    int32_t n[3];
    int32_t C, P, K;
    int32_t node_begin, node_end;  // this launch's slots (the gain kernels)
    int32_t round;                 // fit_choose_kernel's j
    int32_t pick_blocks;           // the grid of fit_pick_kernel
    const float *values;           // [C]
    const double *points;          // [P][3]
    int32_t *gain;                 // [C]
    int32_t *covered;              // [P]
    int32_t *list;                 // [P]
    int32_t *rec_gain, *rec_node;  // [FIT_PICK_BLOCKS]
    int32_t *state;                // [ST_WORDS]
    int32_t *chosen, *gains, *count_uncovered;
    double *centers, *radii;
};

__global__ __launch_bounds__(FIT_BLOCK) void fit_init_kernel(const FitLaunch a) {
    const int gid = (int)(blockIdx.x * FIT_BLOCK + threadIdx.x), stride = (int)(gridDim.x * FIT_BLOCK);
    for (int p = gid; p < a.P; p += stride) a.covered[p] = 0;
    for (int j = gid; j < a.K; j += stride) {
        a.chosen[j] = -1;
        a.gains[j] = 0;
        a.radii[j] = a.centers[3 * j] = a.centers[3 * j + 1] = a.centers[3 * j + 2] = NAN;
    }
    for (int k = gid; k < ST_WORDS; k += stride) a.state[k] = 0;
    if (gid == 0) {
        a.count_uncovered[0] = 0;
        a.count_uncovered[1] = a.P;
    }
}

template <bool UPDATE>
__global__ __launch_bounds__(FIT_BLOCK) void fit_gain_kernel(const FitLaunch a) {
    __shared__ double sp[3 * FIT_TILE];
    // (an update without newly covered points -- a round after `done` included -- has nothing to do; the word is the
    // same for every lane of the launch, so a block leaves as a whole, before any barrier)
    const int total = UPDATE ? a.state[ST_NEW] : a.P;
    if (UPDATE && total == 0) return;
    const int node = a.node_begin + (int)(blockIdx.x * FIT_BLOCK + threadIdx.x);
    const bool live = node < a.node_end;
    const int q = live ? node : a.node_end - 1;  // (node_begin < node_end: a slot of this launch)
    coll::FitSlot s = coll::fit_slot(a.origin, a.voxel, a.n, q, a.values[q], a.pad, a.slack);
    const int before = UPDATE ? a.gain[q] : 0;
    if (UPDATE) s.ok = s.ok && before > 0;
    int g = 0;
    for (int t0 = 0; t0 < total; t0 += FIT_TILE) {
        const int cnt = total - t0 < FIT_TILE ? total - t0 : FIT_TILE;
        __syncthreads();  // (the previous tile has been read by every lane)
        // (k < 3 * cnt <= 3 * FIT_TILE: inside sp; t0 + k / 3 < total <= P: inside points, resp. list, whose entries
        // are point indices in 0 .. P - 1)
        for (int k = threadIdx.x; k < 3 * cnt; k += FIT_BLOCK)
            sp[k] = UPDATE ? a.points[3 * (size_t)a.list[t0 + k / 3] + k % 3] : a.points[3 * (size_t)t0 + k];
        __syncthreads();
        if (__any(s.ok))
            for (int t = 0; t < cnt; ++t) g += coll::fit_covers(s, a.slack, sp + 3 * t) ? 1 : 0;
    }
    if (live) a.gain[node] = UPDATE ? before - g : g;
}

__global__ __launch_bounds__(FIT_BLOCK) void fit_pick_kernel(const FitLaunch a) {
    __shared__ double s_key[FIT_BLOCK / 64];
    __shared__ unsigned long long s_idx[FIT_BLOCK / 64];
    if (a.state[ST_DONE]) return;
    // the order of spherefit_measure.hpp's fit_takes as ik_argmin.hpp's: key = -gain (exact), ties to the lower node
    double key = 0.0;
    unsigned long long idx = ~0ull;
    for (long long c = (long long)blockIdx.x * FIT_BLOCK + threadIdx.x; c < a.C; c += (long long)gridDim.x * FIT_BLOCK) {
        const int g = a.gain[c];
        if (g > 0 && argmin_takes(key, idx, -(double)g, (unsigned long long)c)) { key = -(double)g; idx = (unsigned long long)c; }
    }
    block_argmin<FIT_BLOCK>(key, idx, s_key, s_idx);
    if (threadIdx.x == 0) {
        a.rec_gain[blockIdx.x] = idx == ~0ull ? 0 : (int32_t)(-key);
        a.rec_node[blockIdx.x] = idx == ~0ull ? -1 : (int32_t)idx;
    }
}

__global__ __launch_bounds__(FIT_BLOCK) void fit_choose_kernel(const FitLaunch a) {
    __shared__ double s_key[FIT_BLOCK / 64];
    __shared__ unsigned long long s_idx[FIT_BLOCK / 64];
    if (a.state[ST_DONE]) return;
    double key = 0.0;
    unsigned long long idx = ~0ull;
    if ((int)threadIdx.x < a.pick_blocks && a.rec_node[threadIdx.x] >= 0) {
        key = -(double)a.rec_gain[threadIdx.x];
        idx = (unsigned long long)a.rec_node[threadIdx.x];
    }
    block_argmin<FIT_BLOCK>(key, idx, s_key, s_idx);
    if (threadIdx.x != 0) return;
    a.state[ST_NEW] = 0;
    if (idx == ~0ull) {
        a.state[ST_DONE] = 1;
        return;
    }
    const int32_t node = (int32_t)idx, g = (int32_t)(-key), j = a.round;
    const coll::FitSlot s = coll::fit_slot(a.origin, a.voxel, a.n, node, a.values[node], a.pad, a.slack);
    a.chosen[j] = node;
    a.gains[j] = g;
    a.radii[j] = s.r;
    for (int k = 0; k < 3; ++k) a.centers[3 * j + k] = s.c[k];
    a.state[ST_PICK] = node;
    a.state[ST_COVERED] += g;
    a.state[ST_COUNT] += 1;
    a.count_uncovered[0] = a.state[ST_COUNT];
    a.count_uncovered[1] = a.P - a.state[ST_COVERED];
}

__global__ __launch_bounds__(FIT_BLOCK) void fit_mark_kernel(const FitLaunch a) {
    if (a.state[ST_DONE]) return;
    const int32_t node = a.state[ST_PICK];
    const coll::FitSlot s = coll::fit_slot(a.origin, a.voxel, a.n, node, a.values[node], a.pad, a.slack);
    for (long long p = (long long)blockIdx.x * FIT_BLOCK + threadIdx.x; p < a.P; p += (long long)gridDim.x * FIT_BLOCK) {
        if (a.covered[p] || !coll::fit_covers(s, a.slack, a.points + 3 * (size_t)p)) continue;
        a.covered[p] = 1;
        // (a point is appended at most once a round and the word is 0 at the round's start: the slot is below P)
        a.list[atomicAdd(&a.state[ST_NEW], 1)] = (int32_t)p;
    }
}

template <bool UPDATE>
void gain_launches(const optik_hip_chain *ch, FitLaunch a, hipStream_t stream) {
    long long per = g_pairs_per_launch.load() / a.P;
    if (per < 1) per = 1;
    for (long long b = 0; b < a.C; b += per) {
        a.node_begin = (int32_t)b;
        a.node_end = (int32_t)(b + per < a.C ? b + per : a.C);
        const int grid = (a.node_end - a.node_begin + FIT_BLOCK - 1) / FIT_BLOCK;
        hipLaunchKernelGGL(fit_gain_kernel<UPDATE>, dim3(grid), dim3(FIT_BLOCK), 0, stream, a);
    }
}

}  // namespace

extern "C" {

int optik_hip_sphere_fit(const optik_hip_chain *ch, const double *origin3, double voxel, int32_t nx, int32_t ny,
                         int32_t nz, const float *d_values, const double *d_points3, int64_t P, double pad,
                         double slack, int32_t K, int32_t *d_chosen, double *d_centers3, double *d_radii,
                         int32_t *d_gains, int32_t *d_count_uncovered, void *d_workspace, int64_t workspace_bytes,
                         void *stream) {
    if (!ch) return fail(OPTIK_HIP_EINVAL, "bad argument");
    std::string err;
    if (int rc = coll::check_grid(origin3, voxel, nx, ny, nz, nullptr, false, err)) return fail(rc, err);
    if (coll::check_fit(P, pad, slack, K, nullptr, err)) return fail(OPTIK_HIP_EINVAL, err);
    if (!d_values || !d_points3 || !d_chosen || !d_centers3 || !d_radii || !d_gains || !d_count_uncovered
        || !d_workspace)
        return fail(OPTIK_HIP_EINVAL, "sphere fit: null buffer");
    const long long nodes = (long long)nx * ny * nz;
    if (workspace_bytes < (int64_t)coll::fit_workspace_bytes(nodes, P))
        return fail(OPTIK_HIP_EINVAL, "sphere fit: the workspace is smaller than optik_hip_sphere_fit_workspace_bytes");
    BIND_DEVICE(ch);
    hipStream_t st = (hipStream_t)stream;
    FitLaunch a;
    std::memset(&a, 0, sizeof a);
    for (int k = 0; k < 3; ++k) a.origin[k] = origin3[k];
    a.voxel = voxel; a.pad = pad; a.slack = slack;
    a.n[0] = nx; a.n[1] = ny; a.n[2] = nz;
    a.C = (int32_t)nodes; a.P = (int32_t)P; a.K = K;
    a.values = d_values;
    a.points = d_points3;
    a.gain = static_cast<int32_t *>(d_workspace);
    a.covered = a.gain + nodes;
    a.list = a.covered + P;
    a.rec_gain = a.list + P;
    a.rec_node = a.rec_gain + FIT_PICK_BLOCKS;
    a.state = a.rec_node + FIT_PICK_BLOCKS;
    a.chosen = d_chosen; a.gains = d_gains; a.count_uncovered = d_count_uncovered;
    a.centers = d_centers3; a.radii = d_radii;
    a.pick_blocks = stride_grid((unsigned long long)nodes, FIT_BLOCK, FIT_PICK_BLOCKS, opt().grid_cap);
    const int row_grid = grid_for(ch, P > K ? P : K, FIT_BLOCK, 8);
    hipLaunchKernelGGL(fit_init_kernel, dim3(row_grid), dim3(FIT_BLOCK), 0, st, a);
    gain_launches<false>(ch, a, st);
    for (int32_t j = 0; j < K; ++j) {
        a.round = j;
        hipLaunchKernelGGL(fit_pick_kernel, dim3(a.pick_blocks), dim3(FIT_BLOCK), 0, st, a);
        hipLaunchKernelGGL(fit_choose_kernel, dim3(1), dim3(FIT_BLOCK), 0, st, a);
        if (j + 1 == K) break;  // (nothing reads the gains after the last pick)
        hipLaunchKernelGGL(fit_mark_kernel, dim3(row_grid), dim3(FIT_BLOCK), 0, st, a);
        gain_launches<true>(ch, a, st);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

int64_t optik_hip_sphere_fit_workspace_bytes(int32_t nx, int32_t ny, int32_t nz, int64_t P) {
    if (nx < 0 || ny < 0 || nz < 0 || P < 0) return 0;
    return (int64_t)coll::fit_workspace_bytes((int64_t)nx * ny * nz, P);
}

int32_t optik_hip_fit_tile(void) { return FIT_TILE; }

int64_t optik_hip_fit_pairs_per_launch(int64_t pairs) {
    if (pairs > 0) g_pairs_per_launch.store(pairs);
    else if (pairs == 0) g_pairs_per_launch.store(FIT_PAIRS_PER_LAUNCH);
    return g_pairs_per_launch.load();
}

}  // extern "C"
