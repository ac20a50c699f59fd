// ik_mesh.hip -- from a triangle mesh to a distance-field world (mesh_measure.hpp):
// optik_hip_world_grid_from_mesh (include/optik_hip.h).
//
//   mesh_field_kernel   one node per lane in memory order: the lanes of a wave run along z and the value stores are
//                       lane-consecutive.  Every lane walks ALL triangles in index order (step 7's serial sum), so the
//                       launch shape cannot change a bit of the result.
//
// The triangles are staged through LDS in tiles of MESH_TILE (256 x 72 B = 18 KiB per block of 256 lanes): the block
// loads a tile with lane-consecutive reads, then every lane reads triangle t of the tile at a wave-uniform address (a
// broadcast, no bank conflicts).  Distance and winding share A, B, C in one loop (mesh_accumulate); a lane's state
// across the loop is its node and two doubles.  A lane past the last node of its launch computes the launch's last
// node again and stores nothing: it takes part in every tile load and every barrier, and there is no return before
// a __syncthreads.
//
// No culling: a field costs nodes * M pair evaluations.  The host therefore splits the nodes into stream-ordered
// launches of at most MESH_PAIRS_PER_LAUNCH pairs each, so that no single launch holds the device for long; the split
// is by nodes, which leaves every node's triangle order untouched.
#include <atomic>

#include "collision_model.hpp"
#include "ik_host.hpp"
#include "mesh_measure.hpp"

using namespace optik;
using namespace optik::host;

static_assert(coll::MESH_MAX_TRIANGLES == OPTIK_HIP_MAX_MESH_TRIANGLES, "mesh_measure.hpp restates optik_hip.h's limit");

namespace {

constexpr int MESH_BLOCK = 256;
using coll::MESH_PAIRS_PER_LAUNCH;
using coll::MESH_TILE;

std::atomic<long long> g_pairs_per_launch{MESH_PAIRS_PER_LAUNCH};

struct MeshLaunch {
    double origin[3], voxel, max_distance;
    int32_t n[3];
    int32_t node_begin, node_end;  // this launch's nodes, in memory order (node_end <= nx * ny * nz <= 2^24)
    const double *tris;            // [M][9]
    int32_t M;
    float *values;                 // [nx][ny][nz]
};

__global__ __launch_bounds__(MESH_BLOCK) void mesh_field_kernel(const MeshLaunch a) {
    __shared__ double st[9 * MESH_TILE];
    const int node = a.node_begin + (int)(blockIdx.x * MESH_BLOCK + threadIdx.x);
    const bool live = node < a.node_end;
    const int q = live ? node : a.node_end - 1;  // (node_begin < node_end: a node of this launch)
    const int sx = a.n[1] * a.n[2];
    double p[3];
    coll::grid_node(a.origin, a.voxel, q / sx, q / a.n[2] % a.n[1], q % a.n[2], p);
    coll::MeshAcc acc = coll::mesh_acc_start();
    for (int t0 = 0; t0 < a.M; t0 += MESH_TILE) {
        const int cnt = a.M - t0 < MESH_TILE ? a.M - t0 : MESH_TILE;
        __syncthreads();  // (the previous tile has been read by every lane)
        // (k < 9 * cnt <= 9 * MESH_TILE: inside st; 9 * t0 + k < 9 * M: inside tris)
        for (int k = threadIdx.x; k < 9 * cnt; k += MESH_BLOCK) st[k] = a.tris[9 * (size_t)t0 + k];
        __syncthreads();
        for (int t = 0; t < cnt; ++t) coll::mesh_accumulate(p, st + 9 * t, acc);
    }
    if (live) a.values[node] = coll::mesh_value(acc, a.max_distance);
}

}  // namespace

extern "C" {

int optik_hip_world_grid_from_mesh(const optik_hip_chain *ch, const double *origin3, double voxel, int32_t nx,
                                   int32_t ny, int32_t nz, const double *d_tris9, int32_t M, double max_distance,
                                   float *d_values_out, void *stream) {
    if (!ch) return fail(OPTIK_HIP_EINVAL, "bad argument");
    std::string err;
    if (int rc = coll::check_grid(origin3, voxel, nx, ny, nz, nullptr, false, err)) return fail(rc, err);
    if (coll::check_mesh(M, max_distance, nullptr, err)) return fail(OPTIK_HIP_EINVAL, err);
    if (!d_tris9 || !d_values_out) return fail(OPTIK_HIP_EINVAL, "world grid from mesh: null buffer");
    BIND_DEVICE(ch);
    MeshLaunch a;
    std::memset(&a, 0, sizeof a);
    for (int k = 0; k < 3; ++k) a.origin[k] = origin3[k];
    a.voxel = voxel;
    a.max_distance = max_distance;
    a.n[0] = nx; a.n[1] = ny; a.n[2] = nz;
    a.tris = d_tris9;
    a.M = M;
    a.values = d_values_out;
    const long long nodes = (long long)nx * ny * nz;
    long long per = g_pairs_per_launch.load() / M;
    if (per < 1) per = 1;
    for (long long b = 0; b < nodes; b += per) {
        a.node_begin = (int32_t)b;
        a.node_end = (int32_t)(b + per < nodes ? b + per : nodes);
        const int grid = (a.node_end - a.node_begin + MESH_BLOCK - 1) / MESH_BLOCK;
        hipLaunchKernelGGL(mesh_field_kernel, dim3(grid), dim3(MESH_BLOCK), 0, (hipStream_t)stream, a);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

int32_t optik_hip_mesh_tile(void) { return MESH_TILE; }

int64_t optik_hip_mesh_pairs_per_launch(int64_t pairs) {
    if (pairs > 0) g_pairs_per_launch.store(pairs);
    else if (pairs == 0) g_pairs_per_launch.store(MESH_PAIRS_PER_LAUNCH);
    return g_pairs_per_launch.load();
}

}  // extern "C"
