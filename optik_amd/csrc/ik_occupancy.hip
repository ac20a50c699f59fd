// ik_occupancy.hip -- from sensor data to a distance-field world (collision_measure.hpp, steps 8 and 9; DESIGN.md
// section 5.15): optik_hip_world_grid_from_occupancy and optik_hip_occupancy_from_points (include/optik_hip.h).
//
//   edt_pass_kernel<AXIS>   one pass of the exact Euclidean distance transform along z (AXIS 2, reads the occupancy
//                           bytes), y (AXIS 1) or x (AXIS 0, which also applies step 8 and writes the float values)
//   voxelize_kernel         one point per lane: its node, the exclusion spheres, a byte store
//
// The transform: one node per lane in memory order, so the lanes of a wave run along z in EVERY pass -- a pass along y or
// x reads, at step t, the nodes t lines away, which are again consecutive in z.  All three passes therefore load and
// store lane-consecutive addresses.  Each lane walks outward from its node (coll::edt_scan) and stops when t^2 reaches
// its minimum: O(distance to the nearest node of the other set) steps on a real scene, O(n) on a line that holds none.
// Both fields (to the nearest occupied and to the nearest free node) travel together, two words per node: at every node
// one of the two is 0 from the first pass on and ends its scan at once, so one walk serves both at the length the
// other alone would need, the occupancy is read once and a transform is three launches instead of six; the price is a
// workspace of 16 bytes per node (two ping-pong buffers of 8) instead of 8.
//
// Voxelize: grid-stride, 256 threads; the exclusion spheres are staged in LDS (32 KiB at the limit of 1024) and read at
// wave-uniform addresses.  Lanes that hit one node all store the same 1: plain byte stores, no atomics.
#include "collision_measure.hpp"
#include "collision_model.hpp"
#include "ik_host.hpp"

using namespace optik;
using namespace optik::host;

namespace {

struct EdtLaunch {
    const uint8_t *occupied;  // [nx][ny][nz]
    const coll::EdtPair *in;  // the previous pass (AXIS 2: unused)
    coll::EdtPair *out;       // this pass (AXIS 0: unused)
    float *values;            // AXIS 0: the field
    int n[3];
    double voxel, max_distance;
};

template <int AXIS>
__global__ __launch_bounds__(256) void edt_pass_kernel(const EdtLaunch a) {
    const int sy = a.n[2], sx = a.n[1] * a.n[2];
    const int nodes = a.n[0] * sx;  // <= 2^24
    for (int p = (int)(blockIdx.x * blockDim.x + threadIdx.x); p < nodes; p += (int)(gridDim.x * blockDim.x)) {
        // (every index a scan forms is base + j * stride with 0 <= j < n_AXIS: a node of p's own line)
        if (AXIS == 2) {
            const int i = p % sy;
            const uint8_t *line = a.occupied + (p - i);
            a.out[p] = coll::edt_scan([line](int j) { return coll::edt_source(line[j]); }, i, a.n[2]);
        } else if (AXIS == 1) {
            const int i = p / sy % a.n[1];
            const coll::EdtPair *line = a.in + (p - i * sy);
            a.out[p] = coll::edt_scan([line, sy](int j) { return line[j * sy]; }, i, a.n[1]);
        } else {
            const int i = p / sx;
            const coll::EdtPair *line = a.in + (p - i * sx);
            const coll::EdtPair d2 = coll::edt_scan([line, sx](int j) { return line[j * sx]; }, i, a.n[0]);
            a.values[p] = coll::occupancy_value(a.occupied[p], d2, a.voxel, a.max_distance);
        }
    }
}

struct VoxLaunch {
    double origin[3], inv;
    int32_t n[3];
    const double *points;   // [N][3]
    long long N;
    const double *exclude;  // [E][4]
    int E;
    uint8_t *occupied;
};

__global__ __launch_bounds__(256) void voxelize_kernel(const VoxLaunch a) {
    __shared__ double sex[4 * OPTIK_HIP_MAX_EXCLUDE_SPHERES];
    for (int k = threadIdx.x; k < 4 * a.E; k += blockDim.x) sex[k] = a.exclude[k];
    __syncthreads();
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < a.N;
         i += (long long)gridDim.x * blockDim.x) {
        const double p[3] = {a.points[3 * i], a.points[3 * i + 1], a.points[3 * i + 2]};
        int ijk[3];
        if (!coll::point_node(p, a.origin, a.inv, a.n, ijk)) continue;
        bool drop = false;
        for (int e = 0; e < a.E; ++e) drop = drop || coll::point_excluded(p, sex + 4 * e);
        // (0 <= ijk[a] < n[a]: inside the nx * ny * nz bytes)
        if (!drop) a.occupied[((size_t)ijk[0] * a.n[1] + ijk[1]) * a.n[2] + ijk[2]] = 1;
    }
}

const double kZero3[3] = {0.0, 0.0, 0.0};

int edt_reserve(optik_hip_chain *ch, size_t nodes) {
    HIP_TRY(ch->edt_ws.reserve(2 * sizeof(coll::EdtPair) * nodes));
    return 0;
}

}  // namespace

extern "C" {

int optik_hip_world_grid_from_occupancy(optik_hip_chain *ch, double voxel, int32_t nx, int32_t ny, int32_t nz,
                                        const uint8_t *d_occupied, double max_distance, float *d_values_out,
                                        void *stream) {
    if (!ch) return fail(OPTIK_HIP_EINVAL, "bad argument");
    std::string err;
    if (int rc = coll::check_grid(kZero3, voxel, nx, ny, nz, nullptr, false, err)) return fail(rc, err);
    if (int rc = coll::check_max_distance(max_distance, err)) return fail(rc, err);
    if (!d_occupied || !d_values_out) return fail(OPTIK_HIP_EINVAL, "world grid from occupancy: null buffer");
    std::lock_guard<std::mutex> lock(ch->mu);
    BIND_DEVICE(ch);
    const size_t nodes = (size_t)nx * (size_t)ny * (size_t)nz;
    if (int rc = edt_reserve(ch, nodes)) return rc;
    // (every pass writes all nodes of its output before the next reads them: what an earlier call left in the
    // workspace is never read)
    EdtLaunch a;
    std::memset(&a, 0, sizeof a);
    a.occupied = d_occupied;
    a.values = d_values_out;
    a.n[0] = nx; a.n[1] = ny; a.n[2] = nz;
    a.voxel = voxel;
    a.max_distance = max_distance;
    coll::EdtPair *w0 = reinterpret_cast<coll::EdtPair *>(ch->edt_ws.get()), *w1 = w0 + nodes;
    const int grid = grid_for(ch, (long long)nodes, 256, 8);
    a.out = w0;
    hipLaunchKernelGGL(edt_pass_kernel<2>, dim3(grid), dim3(256), 0, (hipStream_t)stream, a);
    a.in = w0; a.out = w1;
    hipLaunchKernelGGL(edt_pass_kernel<1>, dim3(grid), dim3(256), 0, (hipStream_t)stream, a);
    a.in = w1; a.out = nullptr;
    hipLaunchKernelGGL(edt_pass_kernel<0>, dim3(grid), dim3(256), 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

int optik_hip_occupancy_from_points(const optik_hip_chain *ch, const double *origin3, double voxel, int32_t nx,
                                    int32_t ny, int32_t nz, const double *d_points3, int64_t N,
                                    const double *d_exclude4, int32_t E, uint8_t *d_occupied, void *stream) {
    if (!ch) return fail(OPTIK_HIP_EINVAL, "bad argument");
    std::string err;
    if (int rc = coll::check_grid(origin3, voxel, nx, ny, nz, nullptr, false, err)) return fail(rc, err);
    if (int rc = coll::check_cloud(N, E, err)) return fail(rc, err);
    if (N == 0) return 0;
    if (!d_points3 || !d_occupied || (E > 0 && !d_exclude4))
        return fail(OPTIK_HIP_EINVAL, "occupancy from points: null buffer");
    BIND_DEVICE(ch);
    VoxLaunch a;
    std::memset(&a, 0, sizeof a);
    for (int k = 0; k < 3; ++k) a.origin[k] = origin3[k];
    a.inv = 1.0 / voxel;
    a.n[0] = nx; a.n[1] = ny; a.n[2] = nz;
    a.points = d_points3;
    a.N = N;
    a.exclude = d_exclude4;
    a.E = E;
    a.occupied = d_occupied;
    const int grid = grid_for(ch, N, 256, 8);
    hipLaunchKernelGGL(voxelize_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"
