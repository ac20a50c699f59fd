// ik_avoid.hip -- which way is out: the witnesses and joint-space gradients of the clearance, and diff_ik with
// velocity dampers (collision_gradient.hpp, diff_ik_lp.hpp: diff_ik_lp_damped).
//
//   collision_witness_kernel<N, TIP>  per configuration the n + 2 witness rows: dist, witness, grad
//   diff_ik_avoid_kernel<N, TIP>      FK and the body Jacobian as diff_ik_batch_kernel forms them, the same distance
//                                     pass, up to 4 damper rows from the closest frames, then the damped LP
// One configuration per lane, grid-stride, 256 threads; the chain table and the model are staged in LDS as
// collision_key_kernel stages them, the obstacles are read at wave-uniform addresses.  The distance pass keeps one
// running (dist, witness) pair per frame and lane -- n + 2 doubles and as many packed words -- and nothing else: the
// gradients are formed afterwards, from the witnesses, by recomputing the witness point (a few dozen flops per row
// against the hundreds of terms the pass visits).  The witness's obstacle differs from lane to lane, so that one read
// is a gather.  The LP's runtime-indexed matrices live in scratch, as diff_ik_batch_kernel's do.
#include "collision_witness_device.hpp"
#include "diff_ik_lp.hpp"

using namespace optik;
using namespace optik::host;
using namespace optik::hostparams;
using namespace optik::colldev;

static_assert(lp::MAX_DAMPER_ROWS == OPTIK_HIP_MAX_DAMPER_ROWS, "optik_hip.h states the cap of diff_ik_lp.hpp");

namespace {

struct AvoidLaunch {
    CollLaunch c;          // chain, ee_offset, model, world, q [n][B], B
    const uint16_t *orig;  // [S + P]: the caller's index of the sphere in a slot, of the pair at a position
    // witness form; any may be null
    double *dist;          // [F][B]
    double *grad;          // [F][n][B]
    int32_t *witness;      // [F][3][B]
    // diff_ik form, laid out as DiffIkLaunch (ik_batch_ops.hip)
    const double *V, *vmax;
    long long ld_V, ld_vmax;
    double influence, safety, gain;
    double *alpha, *v;
    int32_t *status;
};

template <int N, bool TIP>
__global__ __launch_bounds__(256) void collision_witness_kernel(const AvoidLaunch a) {
    __shared__ ChainDev sch;
    __shared__ ModelDev sm;
    stage_chain(sch, a.c.chain);
    if (a.c.model) stage_model(sm, a.c);
    const size_t B = (size_t)a.c.B;
    for (long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x; b < a.c.B;
         b += (long long)gridDim.x * blockDim.x) {
        double q[N];
#pragma unroll
        for (int i = 0; i < N; ++i) q[i] = a.c.q[(size_t)i * B + b];
        Kin<N, TIP> kin;
        forward_kinematics<N, TIP>(sch, a.c.ep, q, kin);
        const bool nan = kin_has_nan<N, TIP>(kin);
        Rows<N> rows;
#pragma unroll
        for (int k = 0; k < N + 2; ++k) { rows.dist[k] = __builtin_huge_val(); rows.wit[k] = -1; }
        if (a.c.model) witness_pass<N, TIP>(sm, a, kin, rows);
        for (int f = 0; f < N + 2; ++f) {
            double d;
            int32_t w;
            row_get<N>(rows, __builtin_amdgcn_readfirstlane(f), d, w);
            if (nan) { d = __builtin_nan(""); w = -1; }
            if (a.dist) a.dist[(size_t)f * B + b] = d;
            if (a.witness) {
                int32_t w3[3] = {-1, -1, -1};
                if (w >= 0) {
                    const int kind = (w >> 16) & 3, idx = w & 0xffff;
                    w3[0] = a.orig[w >> 18];
                    w3[1] = kind;
                    w3[2] = kind == coll::WIT_PAIR ? (int32_t)a.orig[a.c.S + idx] : idx;
                }
#pragma unroll
                for (int k = 0; k < 3; ++k) a.witness[((size_t)f * 3 + k) * B + b] = w3[k];
            }
            if (a.grad) {
                double *g = a.grad + (size_t)f * N * B + b;
                if (w >= 0) {
                    row_gradient<N, TIP>(sch, sm, a, kin, f, w, [&](int j, double v) { g[(size_t)j * B] = v; });
                } else {
                    const double fill = nan ? __builtin_nan("") : 0.0;
                    for (int j = 0; j < N; ++j) g[(size_t)j * B] = fill;
                }
            }
        }
    }
}

template <int N, bool TIP>
__global__ __launch_bounds__(256) void diff_ik_avoid_kernel(const AvoidLaunch a) {
    __shared__ ChainDev sch;
    __shared__ ModelDev sm;
    stage_chain(sch, a.c.chain);
    if (a.c.model) stage_model(sm, a.c);
    const size_t B = (size_t)a.c.B;
    for (long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x; b < a.c.B;
         b += (long long)gridDim.x * blockDim.x) {
        double q[N];
#pragma unroll
        for (int i = 0; i < N; ++i) q[i] = a.c.q[(size_t)i * B + b];
        Kin<N, TIP> kin;
        forward_kinematics<N, TIP>(sch, a.c.ep, q, kin);
        double jac[6 * N];
        const Q4 eeqc = qconj(kin.ee.q);
#pragma unroll
        for (int k = 0; k < N; ++k) {
            double c6[6];
            jacobian_column<N, TIP>(sch, kin, eeqc, k, c6);
#pragma unroll
            for (int r = 0; r < 6; ++r) jac[k * 6 + r] = c6[r];
        }
        const long long bV = a.ld_V ? b : 0, bM = a.ld_vmax ? b : 0;
        const long long sV = a.ld_V ? a.ld_V : 1, sM = a.ld_vmax ? a.ld_vmax : 1;
        double V[6], vmax[N];
#pragma unroll
        for (int r = 0; r < 6; ++r) V[r] = a.V[(size_t)r * sV + bV];
#pragma unroll
        for (int i = 0; i < N; ++i) vmax[i] = a.vmax[(size_t)i * sM + bM];
        // the damper rows: the closest frames inside the influence distance (a NaN frame makes the rows NaN: no
        // solution; without a model there are no rows and the row is diff_ik_batch_kernel's, NaN or not)
        const bool nan = a.c.model && kin_has_nan<N, TIP>(kin);
        Rows<N> rows;
#pragma unroll
        for (int k = 0; k < N + 2; ++k) { rows.dist[k] = __builtin_huge_val(); rows.wit[k] = -1; }
        if (a.c.model) witness_pass<N, TIP>(sm, a, kin, rows);
        int sel[4];
        const int m = coll::select_damper_rows(N + 2, a.influence, [&](int f) {
            double d;
            int32_t w;
            row_get<N>(rows, __builtin_amdgcn_readfirstlane(f), d, w);
            return d;
        }, sel);
        double G[lp::MAX_DAMPER_ROWS * N], h[lp::MAX_DAMPER_ROWS];
#pragma unroll
        for (int r = 0; r < lp::MAX_DAMPER_ROWS; ++r) {
            h[r] = 0.0;
            if (r < m && !nan) {
                double d;
                int32_t w;
                row_get<N>(rows, sel[r], d, w);
                h[r] = coll::damper_rhs(d, a.influence, a.safety, a.gain);
                row_gradient<N, TIP>(sch, sm, a, kin, sel[r], w, [&](int j, double v) { G[r * N + j] = v; });
            }
        }
        const double quat[4] = {kin.ee.q.i, kin.ee.q.j, kin.ee.q.k, kin.ee.q.w};
        double alpha = 0.0, v[N];
        const int st = nan ? 1 : lp::diff_ik_lp_damped<N>(N, quat, jac, V, vmax, m, G, h, &alpha, v);
        if (st) {
            alpha = 0.0;
#pragma unroll
            for (int i = 0; i < N; ++i) v[i] = 0.0;
        }
        a.alpha[b] = alpha;
#pragma unroll
        for (int i = 0; i < N; ++i) a.v[(size_t)i * B + b] = v[i];
        a.status[b] = st;
    }
}

const char *const kAvoidWideMsg =
    "collision witnesses and diff_ik_avoid: chains of more than 8 joint positions are not supported";
const char *const kAvoidPrismaticMsg = prismatic_msg();

void avoid_fill(const optik_hip_chain *ch, const double *ee_offset7, const double *d_q, int64_t B, AvoidLaunch &a) {
    std::memset(&a, 0, sizeof a);
    fill_launch(ch, ee_offset7, d_q, B, a.c);
    a.orig = ch->coll_orig.get();
}

}  // namespace

extern "C" {

int optik_hip_collision_witness_batch(const optik_hip_chain *ch, const double *ee_offset7, const double *d_q, int64_t B,
                                      double *d_dist, double *d_grad, int32_t *d_witness, void *stream) {
    if (!ch || B < 0) return fail(OPTIK_HIP_EINVAL, "bad argument");
    if (ch->wide || ch->n > 8) return fail(OPTIK_HIP_EUNSUPPORTED, kAvoidWideMsg);
    if (ch->prismatic) return fail(OPTIK_HIP_EUNSUPPORTED, kAvoidPrismaticMsg);
    if (B == 0 || (!d_dist && !d_grad && !d_witness)) return 0;
    if (!d_q) return fail(OPTIK_HIP_EINVAL, "bad argument");
    BIND_DEVICE(ch);
    AvoidLaunch a;
    avoid_fill(ch, ee_offset7, d_q, B, a);
    a.dist = d_dist; a.grad = d_grad; a.witness = d_witness;
    const int grid = grid_for(ch, B, 256, 8);
#define CALL(NN, TT) hipLaunchKernelGGL((collision_witness_kernel<NN, TT>), dim3(grid), dim3(256), 0, (hipStream_t)stream, a)
    OPTIK_DISPATCH(ch, CALL);
#undef CALL
    HIP_TRY(hipGetLastError());
    return 0;
}

int optik_hip_diff_ik_avoid_batch(const optik_hip_chain *ch, const double *ee_offset7, const double *d_q,
                                  const double *d_V, int64_t ld_V, const double *d_vmax, int64_t ld_vmax, int64_t B,
                                  double influence, double safety, double gain, double *d_alpha, double *d_v,
                                  int32_t *d_status, void *stream) {
    // (the chain's refusals come first, as optik_hip_diff_ik_batch has them)
    if (!ch || B < 0) return fail(OPTIK_HIP_EINVAL, "bad argument");
    if (ch->wide || ch->n > 8) return fail(OPTIK_HIP_EUNSUPPORTED, kAvoidWideMsg);
    if (ch->prismatic) return fail(OPTIK_HIP_EUNSUPPORTED, kAvoidPrismaticMsg);
    if (!(std::isfinite(influence) && std::isfinite(safety) && std::isfinite(gain) && influence > safety
          && safety >= 0.0 && gain > 0.0))
        return fail(OPTIK_HIP_EINVAL, "diff_ik_avoid: needs influence > safety >= 0 and gain > 0, all finite");
    if (B == 0) return 0;
    if (!d_q || !d_V || !d_vmax || !d_alpha || !d_v || !d_status) return fail(OPTIK_HIP_EINVAL, "bad argument");
    if ((ld_V != 0 && ld_V < B) || (ld_vmax != 0 && ld_vmax < B))
        return fail(OPTIK_HIP_EINVAL, "ld_V / ld_vmax: 0 (one vector for every row) or at least B");
    BIND_DEVICE(ch);
    AvoidLaunch a;
    avoid_fill(ch, ee_offset7, d_q, B, a);
    a.V = d_V; a.vmax = d_vmax; a.ld_V = ld_V; a.ld_vmax = ld_vmax;
    a.influence = influence; a.safety = safety; a.gain = gain;
    a.alpha = d_alpha; a.v = d_v; a.status = d_status;
    const int grid = grid_for(ch, B, 256, 8);
#define CALL(NN, TT) hipLaunchKernelGGL((diff_ik_avoid_kernel<NN, TT>), dim3(grid), dim3(256), 0, (hipStream_t)stream, a)
    OPTIK_DISPATCH(ch, CALL);
#undef CALL
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"
