// ik_manip.hip -- the manipulability / condition measures on the device (manip_measure.hpp): the selection keys of
// solution modes 3 and 4, and the stand-alone evaluation optik_hip_manip_batch (include/optik_hip.h).
//
//   manip_key_kernel<N, TIP>   after a solver launch, before its selection: every successful restart's key (< +inf)
//                              becomes -w (mode 3) or -c (mode 4) of its x; failed restarts keep +inf
//   manip_batch_kernel<N, TIP> w and c of arbitrary configurations
//   wide_manip_key_kernel, wide_manip_batch_kernel   the same for chains of 9 .. 16 joint positions (run-time n)
// One configuration per lane, grid-stride, chain table staged in LDS.  FK and the body Jacobian are fk_batch_kernel's
// code (ik_eval.hpp, ik_wide.hpp, ik_jacobian.hpp), so the measures are those of the Jacobian fk_batch returns, bit for
// bit.  The key kernel reads only the restarts that succeeded; the lanes of a wave whose restarts failed idle.
#include "ik_host.hpp"
#include "ik_jacobian.hpp"
#include "ik_wide.hpp"
#include "manip_measure.hpp"

using namespace optik;
using namespace optik::host;
using namespace optik::hostparams;

namespace {

struct ManipLaunch {
    const ChainDev *chain;       // n <= 8
    const WideChainDev *wchain;  // 9 .. 16 joint positions
    EvalParams ep;               // only the ee_offset part is used
    const double *q;             // [n][B]: the configurations (key form: the launch's per-restart x)
    long long B;
    double *key;                 // key form: [B], read and overwritten where < +inf
    int condition;               // key form: 1 -> -c, 0 -> -w
    double *w, *c;               // evaluation form: [B] each, either may be null
};

// What one configuration's measures become: the key form overwrites the key, the evaluation form writes w / c.
__device__ __forceinline__ void manip_store(const ManipLaunch &a, bool key_form, long long b, double w, double c) {
    if (key_form) {
        a.key[b] = -(a.condition ? c : w);
    } else {
        if (a.w) a.w[b] = w;
        if (a.c) a.c[b] = c;
    }
}

template <int N, bool TIP, bool KEY>
__device__ __forceinline__ void manip_body(const ManipLaunch &a) {
    __shared__ ChainDev sch;
    stage_chain(sch, a.chain);
    const bool want_c = KEY ? a.condition != 0 : a.c != nullptr;
    for (long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x; b < a.B;
         b += (long long)gridDim.x * blockDim.x) {
        if (KEY && !(a.key[b] < __builtin_huge_val())) continue;  // a failed restart keeps its key
        double q[N];
#pragma unroll
        for (int i = 0; i < N; ++i) q[i] = a.q[(size_t)i * a.B + b];
        Kin<N, TIP> kin;
        forward_kinematics<N, TIP>(sch, a.ep, q, kin);
        double jac[6 * N];
        const Q4 eeqc = qconj(kin.ee.q);
#pragma unroll
        for (int k = 0; k < N; ++k) {
            double c6[6];
            jacobian_column<N, TIP>(sch, kin, eeqc, k, c6);
#pragma unroll
            for (int r = 0; r < 6; ++r) jac[k * 6 + r] = c6[r];
        }
        double w = 0.0, c = 0.0;
        manip::manip_measures_m<(N < 6 ? N : 6)>(N, jac, &w, want_c ? &c : nullptr);
        manip_store(a, KEY, b, w, c);
    }
}

template <int N, bool TIP>
__global__ __launch_bounds__(256) void manip_key_kernel(const ManipLaunch a) { manip_body<N, TIP, true>(a); }

template <int N, bool TIP>
__global__ __launch_bounds__(256) void manip_batch_kernel(const ManipLaunch a) { manip_body<N, TIP, false>(a); }

// 9 .. 16 joint positions: G = J J^T is always 6 x 6.
template <bool KEY>
__device__ __forceinline__ void wide_manip_body(const ManipLaunch &a) {
    __shared__ WideChainDev sch;
    stage_wide_chain(sch, a.wchain);
    const int n = sch.n_pos;
    const bool want_c = KEY ? a.condition != 0 : a.c != nullptr;
    for (long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x; b < a.B;
         b += (long long)gridDim.x * blockDim.x) {
        if (KEY && !(a.key[b] < __builtin_huge_val())) continue;
        double q[WIDE_MAX_DOF], tf[7 * WIDE_MAX_DOF], jac[6 * WIDE_MAX_DOF];
        for (int i = 0; i < n; ++i) q[i] = a.q[(size_t)i * a.B + b];
        const Pose ee = wide_forward(sch, a.ep, n, q, tf);
        const Q4 eeqc = qconj(ee.q);
        for (int k = 0; k < n; ++k) {
            double c6[6];
            wide_jacobian_column(sch, tf, ee, eeqc, k, c6);
#pragma unroll
            for (int r = 0; r < 6; ++r) jac[k * 6 + r] = c6[r];
        }
        double w = 0.0, c = 0.0;
        manip::manip_measures_m<6>(n, jac, &w, want_c ? &c : nullptr);
        manip_store(a, KEY, b, w, c);
    }
}

__global__ __launch_bounds__(256) void wide_manip_key_kernel(const ManipLaunch a) { wide_manip_body<true>(a); }
__global__ __launch_bounds__(256) void wide_manip_batch_kernel(const ManipLaunch a) { wide_manip_body<false>(a); }

const char *const kManipPrismaticMsg =
    "manipulability: prismatic joints are not supported (the reference's Jacobian panics: kinematics.rs:185 todo!())";

int manip_launch(const optik_hip_chain *ch, const ManipLaunch &a, bool key_form, hipStream_t stream) {
    const int grid = grid_for(ch, a.B, 256, 8);
    if (ch->wide) {
        if (key_form) hipLaunchKernelGGL(wide_manip_key_kernel, dim3(grid), dim3(256), 0, stream, a);
        else hipLaunchKernelGGL(wide_manip_batch_kernel, dim3(grid), dim3(256), 0, stream, a);
        HIP_TRY(hipGetLastError());
        return 0;
    }
    if (key_form) {
#define CALL(NN, TT) hipLaunchKernelGGL((manip_key_kernel<NN, TT>), dim3(grid), dim3(256), 0, stream, a)
        OPTIK_DISPATCH(ch, CALL);
#undef CALL
    } else {
#define CALL(NN, TT) hipLaunchKernelGGL((manip_batch_kernel<NN, TT>), dim3(grid), dim3(256), 0, stream, a)
        OPTIK_DISPATCH(ch, CALL);
#undef CALL
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace

namespace optik {
namespace host {

int manip_key_launch(const optik_hip_chain *ch, int mode, const double *ee_offset7, const double *x, double *key,
                     size_t cols, hipStream_t stream) {
    if (ch->prismatic) return fail(OPTIK_HIP_EUNSUPPORTED, kManipPrismaticMsg);
    ManipLaunch a;
    std::memset(&a, 0, sizeof a);
    a.chain = ch->dev;
    a.wchain = ch->wdev;
    const double one[3] = {1, 1, 1};
    make_eval_params(one, one, ee_offset7, a.ep);
    a.q = x;
    a.B = (long long)cols;
    a.key = key;
    a.condition = mode == OPTIK_MODE_CONDITION ? 1 : 0;
    return manip_launch(ch, a, true, stream);
}

}  // namespace host
}  // namespace optik

extern "C" {

int optik_hip_manip_batch(const optik_hip_chain *ch, const double *ee_offset7, const double *d_q, int64_t B,
                          double *d_w, double *d_c, void *stream) {
    if (!ch || B < 0) return fail(OPTIK_HIP_EINVAL, "bad argument");
    if (ch->prismatic) return fail(OPTIK_HIP_EUNSUPPORTED, kManipPrismaticMsg);
    if (B == 0 || (!d_w && !d_c)) return 0;
    if (!d_q) return fail(OPTIK_HIP_EINVAL, "bad argument");
    BIND_DEVICE(ch);
    ManipLaunch a;
    std::memset(&a, 0, sizeof a);
    a.chain = ch->dev;
    a.wchain = ch->wdev;
    const double one[3] = {1, 1, 1};
    make_eval_params(one, one, ee_offset7, a.ep);
    a.q = d_q;
    a.B = B;
    a.w = d_w;
    a.c = d_c;
    return manip_launch(ch, a, false, (hipStream_t)stream);
}

}  // extern "C"
