// ik_collision.hip -- the collision filter on the device (collision_measure.hpp, collision_model.hpp): the model and
// world of a chain, the key pass of a filtered solver launch, and the stand-alone evaluations
// optik_hip_link_frames_batch / optik_hip_collision_batch (include/optik_hip.h).
//
//   link_frames_batch_kernel<N, TIP>  all n + 2 frames of arbitrary configurations, [B][n + 2][7]
//   collision_batch_kernel<N, TIP>    clearance (and free flag) of arbitrary configurations
//   collision_key_kernel<N, TIP>      after a solver launch (and the key pass of modes 3 and 4), before its selection:
//                                     every success (key < +inf) that is not free gets key +inf
//   wide_link_frames_batch_kernel, wide_collision_batch_kernel, wide_collision_key_kernel
//                                     the same for chains of 9 .. 16 joint positions (run-time n)
// One configuration per lane, grid-stride, 256 threads.  The chain table, the robot spheres and the self pairs are
// staged in LDS; the world obstacles are read from global memory at wave-uniform addresses (one scalar load serves the
// wave).  FK is forward_kinematics / wide_forward as fk_batch_kernel runs it, so frame n + 1 is fk_batch's pose bit for
// bit; the frames stay in registers (n <= 8; the wide form keeps them in a per-lane array).  Spheres are grouped by
// frame and pairs by frame pair (collision_model.hpp), so a frame is selected once per group.  The key form reads
// only the restarts that succeeded and leaves a wave's loop as soon as none of its lanes is still free: stopping at
// the first term below the margin decides exactly what the full minimum decides.
#include "collision_device.hpp"

using namespace optik;
using namespace optik::host;
using namespace optik::hostparams;
using namespace optik::colldev;

namespace {

// What one configuration's result becomes.
template <int FORM>
__device__ __forceinline__ void coll_store(const CollLaunch &a, long long b, double c, bool free_) {
    if (FORM == FORM_KEY) {
        if (!free_) a.key[b] = __builtin_huge_val();
    } else {
        if (a.clearance) a.clearance[b] = c;
        if (a.free_flag) a.free_flag[b] = free_ ? 1 : 0;
    }
}

template <int N, bool TIP, int FORM>
__device__ __forceinline__ void coll_body(const CollLaunch &a) {
    __shared__ ChainDev sch;
    __shared__ ModelDev sm;
    stage_chain(sch, a.chain);
    if (FORM != FORM_FRAMES && a.model) stage_model(sm, a);
    for (long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x; b < a.B;
         b += (long long)gridDim.x * blockDim.x) {
        if (FORM == FORM_KEY && !(a.key[b] < __builtin_huge_val())) continue;  // a failed restart keeps its key
        double q[N];
#pragma unroll
        for (int i = 0; i < N; ++i) q[i] = a.q[(size_t)i * a.B + b];
        if (FORM == FORM_FRAMES) {
            Kin<N, TIP> kin;
            forward_kinematics<N, TIP>(sch, a.ep, q, kin);
            double *dst = a.frames + (size_t)b * (size_t)(N + 2) * 7;
            const Pose id{V3{0.0, 0.0, 0.0}, Q4{0.0, 0.0, 0.0, 1.0}};
            store_pose7(dst, id);
#pragma unroll
            for (int k = 0; k < N; ++k) store_pose7(dst + 7 * (k + 1), kin.tf[k]);
            store_pose7(dst + 7 * (N + 1), kin.ee);
            continue;
        }
        bool free_ = true;
        const double c = config_clearance<N, TIP, FORM == FORM_KEY ? FORM_KEY : FORM_BATCH>(sch, sm, a, q, free_);
        coll_store<FORM>(a, b, c, free_);
    }
}

template <int N, bool TIP>
__global__ __launch_bounds__(256) void link_frames_batch_kernel(const CollLaunch a) { coll_body<N, TIP, FORM_FRAMES>(a); }
template <int N, bool TIP>
__global__ __launch_bounds__(256) void collision_batch_kernel(const CollLaunch a) { coll_body<N, TIP, FORM_BATCH>(a); }
template <int N, bool TIP>
__global__ __launch_bounds__(256) void collision_key_kernel(const CollLaunch a) { coll_body<N, TIP, FORM_KEY>(a); }

// 9 .. 16 joint positions (run-time n).
template <int FORM>
__device__ __forceinline__ void wide_coll_body(const CollLaunch &a) {
    __shared__ WideChainDev sch;
    __shared__ ModelDev sm;
    stage_wide_chain(sch, a.wchain);
    if (FORM != FORM_FRAMES && a.model) stage_model(sm, a);
    const int n = sch.n_pos;
    for (long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x; b < a.B;
         b += (long long)gridDim.x * blockDim.x) {
        if (FORM == FORM_KEY && !(a.key[b] < __builtin_huge_val())) continue;
        double q[WIDE_MAX_DOF];
        for (int i = 0; i < n; ++i) q[i] = a.q[(size_t)i * a.B + b];
        if (FORM == FORM_FRAMES) {
            double tf[7 * WIDE_MAX_DOF];
            const Pose ee = wide_forward(sch, a.ep, n, q, tf);
            double *dst = a.frames + (size_t)b * (size_t)(n + 2) * 7;
            const Pose id{V3{0.0, 0.0, 0.0}, Q4{0.0, 0.0, 0.0, 1.0}};
            store_pose7(dst, id);
            for (int k = 0; k < 7 * n; ++k) dst[7 + k] = tf[k];
            store_pose7(dst + 7 * (n + 1), ee);
            continue;
        }
        bool free_ = true;
        const double c = wide_config_clearance<FORM == FORM_KEY ? FORM_KEY : FORM_BATCH>(sch, sm, a, n, q, free_);
        coll_store<FORM>(a, b, c, free_);
    }
}

__global__ __launch_bounds__(256) void wide_link_frames_batch_kernel(const CollLaunch a) { wide_coll_body<FORM_FRAMES>(a); }
__global__ __launch_bounds__(256) void wide_collision_batch_kernel(const CollLaunch a) { wide_coll_body<FORM_BATCH>(a); }
__global__ __launch_bounds__(256) void wide_collision_key_kernel(const CollLaunch a) { wide_coll_body<FORM_KEY>(a); }

// The bake (collision_measure.hpp, step 7): one lane per node, grid-stride; the primitives are read at wave-uniform
// addresses, as the key pass reads them.
struct BakeLaunch {
    const double *wsph, *wbox;
    int Ms, Mb;
    double origin[3], voxel;
    int n[3];
    float *out;
};

__global__ __launch_bounds__(256) void grid_bake_kernel(const BakeLaunch a) {
    const long long nodes = (long long)a.n[0] * a.n[1] * a.n[2];
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < nodes;
         i += (long long)gridDim.x * blockDim.x) {
        const int iz = (int)(i % a.n[2]), iy = (int)(i / a.n[2] % a.n[1]), ix = (int)(i / ((long long)a.n[1] * a.n[2]));
        double p[3];
        coll::grid_node(a.origin, a.voxel, ix, iy, iz, p);
        a.out[i] = (float)coll::primitive_field(p, a.wsph, a.Ms, a.wbox, a.Mb);
    }
}

const char *const kCollPrismaticMsg = prismatic_msg();

int coll_launch(const optik_hip_chain *ch, const CollLaunch &a, int form, hipStream_t stream) {
    const int grid = grid_for(ch, a.B, 256, 8);
    if (ch->wide) {
        if (form == FORM_FRAMES) hipLaunchKernelGGL(wide_link_frames_batch_kernel, dim3(grid), dim3(256), 0, stream, a);
        else if (form == FORM_BATCH) hipLaunchKernelGGL(wide_collision_batch_kernel, dim3(grid), dim3(256), 0, stream, a);
        else hipLaunchKernelGGL(wide_collision_key_kernel, dim3(grid), dim3(256), 0, stream, a);
        HIP_TRY(hipGetLastError());
        return 0;
    }
    if (form == FORM_FRAMES) {
#define CALL(NN, TT) hipLaunchKernelGGL((link_frames_batch_kernel<NN, TT>), dim3(grid), dim3(256), 0, stream, a)
        OPTIK_DISPATCH(ch, CALL);
#undef CALL
    } else if (form == FORM_BATCH) {
#define CALL(NN, TT) hipLaunchKernelGGL((collision_batch_kernel<NN, TT>), dim3(grid), dim3(256), 0, stream, a)
        OPTIK_DISPATCH(ch, CALL);
#undef CALL
    } else {
#define CALL(NN, TT) hipLaunchKernelGGL((collision_key_kernel<NN, TT>), dim3(grid), dim3(256), 0, stream, a)
        OPTIK_DISPATCH(ch, CALL);
#undef CALL
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

// Before a model or world is replaced: nothing queued on the chain's device may still read the old buffers.
int drain_chain(optik_hip_chain *ch) {
    HIP_TRY(hipDeviceSynchronize());
    ch->claim_pending = false;
    return 0;
}

}  // namespace

namespace optik {
namespace host {

int collision_key_launch(const optik_hip_chain *ch, const double *ee_offset7, const double *x, double *key,
                         size_t cols, hipStream_t stream) {
    if (ch->prismatic) return fail(OPTIK_HIP_EUNSUPPORTED, kCollPrismaticMsg);
    CollLaunch a;
    fill_launch(ch, ee_offset7, x, (long long)cols, a);
    a.key = key;
    return coll_launch(ch, a, FORM_KEY, stream);
}

}  // namespace host
}  // namespace optik

extern "C" {

int optik_hip_chain_set_collision_model(optik_hip_chain *ch, const int32_t *frames, const double *centers3,
                                        const double *radii, int32_t S, const int32_t *pairs2, int32_t P,
                                        double margin) {
    if (!ch) return fail(OPTIK_HIP_EINVAL, "bad argument");
    std::string err;
    if (int rc = coll::check_model(ch->n, frames, centers3, radii, S, pairs2, P, margin, err)) return fail(rc, err);
    if (S > 0 && ch->prismatic) return fail(OPTIK_HIP_EUNSUPPORTED, kCollPrismaticMsg);
    std::lock_guard<std::mutex> lock(ch->mu);
    BIND_DEVICE(ch);
    if (int rc = drain_chain(ch)) return rc;
    if (S == 0) {
        ch->coll_S = 0; ch->coll_P = 0; ch->coll_groups = 0; ch->coll_margin = 0.0;
        return 0;
    }
    std::vector<ModelDev> packed(1);
    std::vector<uint16_t> orig;
    const int groups = coll::pack_model(ch->n, frames, centers3, radii, S, pairs2, P, packed[0], &orig);
    ch->coll_S = 0;  // (no model until both uploads are through: never old counts over new data)
    if (!ch->coll_dev) HIP_TRY(hipMalloc(&ch->coll_dev, sizeof(ModelDev)));
    HIP_TRY(hipMemcpy(ch->coll_dev, packed.data(), sizeof(ModelDev), hipMemcpyHostToDevice));
    HIP_TRY(ch->coll_orig.reserve(orig.size()));
    HIP_TRY(hipMemcpy(ch->coll_orig.get(), orig.data(), sizeof(uint16_t) * orig.size(), hipMemcpyHostToDevice));
    ch->coll_S = S; ch->coll_P = P; ch->coll_groups = groups; ch->coll_margin = margin;
    return 0;
}

int optik_hip_chain_set_world(optik_hip_chain *ch, const double *spheres4, int32_t Ms, const double *boxes10,
                              int32_t Mb) {
    if (!ch) return fail(OPTIK_HIP_EINVAL, "bad argument");
    std::string err;
    if (int rc = coll::check_world(spheres4, Ms, boxes10, Mb, err)) return fail(rc, err);
    std::lock_guard<std::mutex> lock(ch->mu);
    BIND_DEVICE(ch);
    if (int rc = drain_chain(ch)) return rc;
    const size_t need = 4 * (size_t)Ms + 10 * (size_t)Mb;
    if (need > ch->world_dev.capacity()) ch->world_Ms = ch->world_Mb = 0;  // (no world while the block is replaced)
    HIP_TRY(ch->world_dev.reserve(need));
    if (Ms > 0) HIP_TRY(hipMemcpy(ch->world_dev.get(), spheres4, sizeof(double) * 4 * (size_t)Ms, hipMemcpyHostToDevice));
    if (Mb > 0)
        HIP_TRY(hipMemcpy(ch->world_dev.get() + 4 * (size_t)Ms, boxes10, sizeof(double) * 10 * (size_t)Mb,
                          hipMemcpyHostToDevice));
    ch->world_Ms = Ms; ch->world_Mb = Mb;
    return 0;
}

int optik_hip_chain_set_world_grid(optik_hip_chain *ch, const double *origin3, double voxel, int32_t nx, int32_t ny,
                                   int32_t nz, const float *values) {
    if (!ch) return fail(OPTIK_HIP_EINVAL, "bad argument");
    const bool clear = !values && nx == 0 && ny == 0 && nz == 0;
    std::string err;
    if (!clear)
        if (int rc = coll::check_grid(origin3, voxel, nx, ny, nz, values, true, err)) return fail(rc, err);
    std::lock_guard<std::mutex> lock(ch->mu);
    BIND_DEVICE(ch);
    if (int rc = drain_chain(ch)) return rc;
    ch->grid_n[0] = ch->grid_n[1] = ch->grid_n[2] = 0;
    if (clear) return 0;
    const size_t need = (size_t)nx * (size_t)ny * (size_t)nz;
    HIP_TRY(ch->grid_dev.reserve(need));
    HIP_TRY(hipMemcpy(ch->grid_dev.get(), values, sizeof(float) * need, hipMemcpyHostToDevice));
    for (int k = 0; k < 3; ++k) ch->grid_origin[k] = origin3[k];
    ch->grid_inv = 1.0 / voxel;
    ch->grid_n[0] = nx; ch->grid_n[1] = ny; ch->grid_n[2] = nz;
    return 0;
}

int optik_hip_world_grid_bake(const optik_hip_chain *ch, const double *origin3, double voxel, int32_t nx, int32_t ny,
                              int32_t nz, float *d_values_out, void *stream) {
    if (!ch) return fail(OPTIK_HIP_EINVAL, "bad argument");
    std::string err;
    if (int rc = coll::check_grid(origin3, voxel, nx, ny, nz, nullptr, false, err)) return fail(rc, err);
    if (ch->world_Ms + ch->world_Mb == 0) return fail(OPTIK_HIP_EINVAL, coll::bake_empty_msg());
    if (!d_values_out) return fail(OPTIK_HIP_EINVAL, "bad argument");
    BIND_DEVICE(ch);
    BakeLaunch a;
    std::memset(&a, 0, sizeof a);
    a.wsph = ch->world_dev.get();
    a.wbox = ch->world_dev.get() + 4 * (size_t)ch->world_Ms;
    a.Ms = ch->world_Ms; a.Mb = ch->world_Mb;
    for (int k = 0; k < 3; ++k) a.origin[k] = origin3[k];
    a.voxel = voxel;
    a.n[0] = nx; a.n[1] = ny; a.n[2] = nz;
    a.out = d_values_out;
    const int grid = grid_for(ch, (long long)nx * ny * nz, 256, 8);
    hipLaunchKernelGGL(grid_bake_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

int optik_hip_link_frames_batch(const optik_hip_chain *ch, const double *ee_offset7, const double *d_q, int64_t B,
                                double *d_frames, void *stream) {
    if (!ch || B < 0) return fail(OPTIK_HIP_EINVAL, "bad argument");
    if (ch->prismatic) return fail(OPTIK_HIP_EUNSUPPORTED, kCollPrismaticMsg);
    if (B == 0) return 0;
    if (!d_q || !d_frames) return fail(OPTIK_HIP_EINVAL, "bad argument");
    BIND_DEVICE(ch);
    CollLaunch a;
    fill_launch(ch, ee_offset7, d_q, B, a);
    a.model = nullptr;
    a.frames = d_frames;
    return coll_launch(ch, a, FORM_FRAMES, (hipStream_t)stream);
}

int optik_hip_collision_batch(const optik_hip_chain *ch, const double *ee_offset7, const double *d_q, int64_t B,
                              double *d_clearance, uint8_t *d_free, void *stream) {
    if (!ch || B < 0) return fail(OPTIK_HIP_EINVAL, "bad argument");
    if (ch->prismatic) return fail(OPTIK_HIP_EUNSUPPORTED, kCollPrismaticMsg);
    if (B == 0 || (!d_clearance && !d_free)) return 0;
    if (!d_q) return fail(OPTIK_HIP_EINVAL, "bad argument");
    BIND_DEVICE(ch);
    CollLaunch a;
    fill_launch(ch, ee_offset7, d_q, B, a);
    a.clearance = d_clearance;
    a.free_flag = d_free;
    return coll_launch(ch, a, FORM_BATCH, (hipStream_t)stream);
}

}  // extern "C"
