// ik_depth.hip -- depth-image worlds: the evidence map with free-space carving (depth_measure.hpp; DESIGN.md section
// 5.23): optik_hip_depth_integrate and optik_hip_occupancy_from_map (include/optik_hip.h).
//
//   depth_clean_kernel          one pixel per lane: validity, back-projection, the exclusion spheres, a float store
//   depth_integrate_kernel      one node per lane: projection, one gathered pixel per frame, an int16 load and store
//   occupancy_from_map_kernel   one node per lane: a threshold, a byte store
//
// Clean: grid-stride over the pixels of a frame, 256 threads, blockIdx.y = the frame of the launch, so the camera is
// one set of scalar loads per block; the exclusion spheres are staged in LDS (32 KiB at the limit of 1024) and read at
// wave-uniform addresses, as voxelize_kernel does (ik_occupancy.hip).
//
// Integrate: one node per lane in memory order, so the lanes of a wave are consecutive in z and load and store
// lane-consecutive 2-byte words of the map.  The cameras of the launch travel in the kernel arguments (wave-uniform:
// scalar registers); the frame loop runs inside the kernel with the evidence in a register, so the map is read and
// written once per launch whatever the frame count.  A wave's 64 nodes are a segment of one grid line, 63 voxels
// long: its projections are a short segment of the image, and the gathered pixels neighbours in it.  A launch takes up
// to FRAMES_PER_LAUNCH frames (the kernel arguments hold that many cameras, 128 bytes each); more frames are more
// launches on the same stream, which is the same arithmetic (depth_measure.hpp, step 3).
#include "collision_model.hpp"
#include "depth_measure.hpp"
#include "ik_host.hpp"

using namespace optik;
using namespace optik::host;

namespace {

constexpr int FRAMES_PER_LAUNCH = 8;
constexpr size_t WS_MAX_FLOATS = (size_t)1 << 26;  // 256 MiB of cleaned images per launch (one 4096 x 4096 frame: 64 MiB)

struct CleanLaunch {
    const float *depth;  // [frames][H][W]
    float *cleaned;      // [frames][H][W]
    int32_t H, W;
    double z_near, z_far;
    const double *exclude;  // [E][4]
    int32_t E;
    depth::Camera cam[FRAMES_PER_LAUNCH];
};

__global__ __launch_bounds__(256) void depth_clean_kernel(const CleanLaunch a) {
    __shared__ double sex[4 * OPTIK_HIP_MAX_EXCLUDE_SPHERES];
    for (int k = threadIdx.x; k < 4 * a.E; k += blockDim.x) sex[k] = a.exclude[k];
    __syncthreads();
    const int pixels = a.H * a.W;  // <= 2^24
    const depth::Camera &c = a.cam[blockIdx.y];
    const float *in = a.depth + (size_t)blockIdx.y * (size_t)pixels;
    float *out = a.cleaned + (size_t)blockIdx.y * (size_t)pixels;
    for (int i = (int)(blockIdx.x * blockDim.x + threadIdx.x); i < pixels; i += (int)(gridDim.x * blockDim.x)) {
        double p[3];
        float cv;
        if (depth::pixel_point(in[i], i / a.W, i % a.W, c, a.z_near, a.z_far, &cv, p)) {
            bool masked = false;
            for (int e = 0; e < a.E; ++e) masked = masked || coll::point_excluded(p, sex + 4 * e);
            if (masked) cv = -cv;
        }
        out[i] = cv;  // (i < H * W: inside this frame's block of the workspace)
    }
}

struct IntegrateLaunch {
    double origin[3], voxel;
    int32_t n[3];
    int16_t *map;          // [nx][ny][nz]
    const float *cleaned;  // [frames][H][W]
    int32_t frames, H, W;
    depth::Params P;
    depth::Camera cam[FRAMES_PER_LAUNCH];
};

__global__ __launch_bounds__(256) void depth_integrate_kernel(const IntegrateLaunch a) {
    const int sy = a.n[2], sx = a.n[1] * a.n[2];
    const int nodes = a.n[0] * sx;  // <= 2^24
    const size_t pixels = (size_t)a.H * (size_t)a.W;
    for (int p = (int)(blockIdx.x * blockDim.x + threadIdx.x); p < nodes; p += (int)(gridDim.x * blockDim.x)) {
        const double px = a.origin[0] + a.voxel * (double)(p / sx);
        const double py = a.origin[1] + a.voxel * (double)(p / sy % a.n[1]);
        const double pz = a.origin[2] + a.voxel * (double)(p % sy);
        int e = a.map[p];
        for (int f = 0; f < a.frames; ++f)
            e = depth::integrate_frame(e, px, py, pz, a.cam[f], a.cleaned + (size_t)f * pixels, a.H, a.W, a.P);
        a.map[p] = (int16_t)e;
    }
}

__global__ __launch_bounds__(256) void occupancy_from_map_kernel(const int16_t *map, int nodes, int threshold,
                                                                 bool unknown_occupied, bool accumulate,
                                                                 uint8_t *occupied) {
    for (int p = (int)(blockIdx.x * blockDim.x + threadIdx.x); p < nodes; p += (int)(gridDim.x * blockDim.x)) {
        const uint8_t o = depth::map_occupied(map[p], threshold, unknown_occupied);
        occupied[p] = accumulate ? (uint8_t)(occupied[p] | o) : o;
    }
}

}  // namespace

extern "C" {

int optik_hip_depth_integrate(optik_hip_chain *ch, const double *origin3, double voxel, int32_t nx, int32_t ny,
                              int32_t nz, int16_t *d_map, const float *d_depth, int32_t F, int32_t H, int32_t W,
                              const double *intrinsics4, const double *poses16, const double *d_exclude4, int32_t E,
                              double z_near, double z_far, double band, int32_t hit, int32_t miss, int32_t e_min,
                              int32_t e_max, void *stream) {
    if (!ch) return fail(OPTIK_HIP_EINVAL, "bad argument");
    std::string err;
    if (int rc = coll::check_grid(origin3, voxel, nx, ny, nz, nullptr, false, err)) return fail(rc, err);
    if (int rc = coll::check_depth(F, H, W, E, z_near, z_far, band, hit, miss, e_min, e_max, err)) return fail(rc, err);
    if (int rc = coll::check_cameras(F, intrinsics4, poses16, err)) return fail(rc, err);
    if (!d_map || !d_depth || (E > 0 && !d_exclude4)) return fail(OPTIK_HIP_EINVAL, "depth integrate: null buffer");
    std::lock_guard<std::mutex> lock(ch->mu);
    BIND_DEVICE(ch);
    const size_t pixels = (size_t)H * (size_t)W, nodes = (size_t)nx * (size_t)ny * (size_t)nz;
    int per = (int)(WS_MAX_FLOATS / pixels);  // >= 4
    if (per > FRAMES_PER_LAUNCH) per = FRAMES_PER_LAUNCH;
    if (per > F) per = F;
    HIP_TRY(ch->depth_ws.reserve(pixels * (size_t)per));
    CleanLaunch c;
    std::memset(&c, 0, sizeof c);
    c.cleaned = ch->depth_ws.get();
    c.H = H; c.W = W;
    c.z_near = z_near; c.z_far = z_far;
    c.exclude = d_exclude4;
    c.E = E;
    IntegrateLaunch a;
    std::memset(&a, 0, sizeof a);
    for (int k = 0; k < 3; ++k) a.origin[k] = origin3[k];
    a.voxel = voxel;
    a.n[0] = nx; a.n[1] = ny; a.n[2] = nz;
    a.map = d_map;
    a.cleaned = ch->depth_ws.get();
    a.H = H; a.W = W;
    a.P.z_near = z_near; a.P.z_far = z_far; a.P.band = band;
    a.P.hit = hit; a.P.miss = miss; a.P.e_min = e_min; a.P.e_max = e_max;
    const int grid_px = grid_for(ch, (long long)pixels, 256, 8), grid_nodes = grid_for(ch, (long long)nodes, 256, 8);
    // (a launch's clean kernel overwrites the workspace only after the integrate kernel before it on the stream has
    // read it)
    for (int f0 = 0; f0 < F; f0 += per) {
        const int frames = F - f0 < per ? F - f0 : per;
        for (int f = 0; f < frames; ++f)
            c.cam[f] = a.cam[f] = depth::camera_from(intrinsics4 + 4 * (f0 + f), poses16 + 16 * (f0 + f));
        c.depth = d_depth + (size_t)f0 * pixels;
        a.frames = frames;
        hipLaunchKernelGGL(depth_clean_kernel, dim3(grid_px, frames), dim3(256), 0, (hipStream_t)stream, c);
        hipLaunchKernelGGL(depth_integrate_kernel, dim3(grid_nodes), dim3(256), 0, (hipStream_t)stream, a);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

int optik_hip_occupancy_from_map(const optik_hip_chain *ch, int32_t nx, int32_t ny, int32_t nz, const int16_t *d_map,
                                 int32_t threshold, int32_t unknown_occupied, int32_t accumulate, uint8_t *d_occupied,
                                 void *stream) {
    if (!ch) return fail(OPTIK_HIP_EINVAL, "bad argument");
    std::string err;
    const double zero3[3] = {0.0, 0.0, 0.0};
    if (int rc = coll::check_grid(zero3, 1.0, nx, ny, nz, nullptr, false, err)) return fail(rc, err);
    if (int rc = coll::check_map_threshold(threshold, err)) return fail(rc, err);
    if (!d_map || !d_occupied) return fail(OPTIK_HIP_EINVAL, "occupancy from map: null buffer");
    BIND_DEVICE(ch);
    const long long nodes = (long long)nx * ny * nz;
    hipLaunchKernelGGL(occupancy_from_map_kernel, dim3(grid_for(ch, nodes, 256, 8)), dim3(256), 0, (hipStream_t)stream,
                       d_map, (int)nodes, (int)threshold, unknown_occupied != 0, accumulate != 0, d_occupied);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"
