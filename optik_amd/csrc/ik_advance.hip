// ik_advance.hip -- the certified motion check on the device (advance_measure.hpp):
// conservative advancement along the straight joint-space segment qa -> qb, for many segments at once.
// optik_hip_collision_motion_certify_batch (include/optik_hip.h).
//
// The samples of a segment are sequential -- each step's length comes from the sample before -- so the parallelism is
// over the distance terms of ONE sample, not over samples as in ik_motion.hip:
//
//   advance_kernel<N, TIP>, wide_advance_kernel
//       256 threads = 4 waves, one wave per segment, grid-stride over the segments (ik_grid.hpp).  The model, the
//       reach table, |c_s| and the frame of every sphere are staged in LDS once per block.  Per segment the wave
//       keeps qa, qb, a_j and lam(s) in its own LDS slab.  Per step every lane runs the FK of q(t) redundantly (the
//       values are wave-uniform; forward_kinematics / wide_forward as the collision kernels call them, so the frames
//       have link_frames_batch's bits) and the frames go to the slab; lanes s < S turn them into sphere centres in
//       the slab and take the grid term of their sphere on the way; then, per robot sphere (a wave-uniform loop), the
//       lanes stride over the world spheres and over the boxes (lane-consecutive loads), and at last over the self
//       pairs.  Each lane keeps a running (c, A); two wave minima give the sample's.  The walk's branch is
//       wave-uniform; no atomics, no workspace.
#include "advance_measure.hpp"
#include "collision_device.hpp"
#include "ik_lane.hpp"

using namespace optik;
using namespace optik::host;
using namespace optik::hostparams;
using namespace optik::colldev;

namespace {

constexpr int ABLOCK = 256, AWAVES = ABLOCK / 64;
constexpr int ABLOCKS_PER_CU = 2;  // (what the block's LDS leaves room for)

struct AdvanceLaunch {
    CollLaunch c;          // chain, ee_offset, model, world (c.q, c.B and the outputs of its forms are not used)
    const double *qa, *qb;  // [n][B]
    long long B;
    int n, max_steps;
    double tol, G;
    // outputs, any may be null
    int32_t *status, *steps;
    double *t_stop, *clearance;
    advance::Reach reach;
};
static_assert(sizeof(AdvanceLaunch) <= 4096, "kernel arguments");
static_assert(advance::FREE == OPTIK_HIP_CERTIFY_FREE && advance::BLOCKED == OPTIK_HIP_CERTIFY_BLOCKED
                  && advance::LIMIT == OPTIK_HIP_CERTIFY_LIMIT && advance::NOT_A_NUMBER == OPTIK_HIP_CERTIFY_NAN,
              "advance_measure.hpp's statuses are optik_hip.h's");

// What a wave keeps of its segment and of the current sample.
struct WaveSlab {
    double frames[advance::MAX_FRAMES * 7];
    double cen[coll::MAX_SPHERES][3];
    double lam[coll::MAX_SPHERES];
    double qa[advance::MAX_JOINTS], qb[advance::MAX_JOINTS], a[advance::MAX_JOINTS], q[advance::MAX_JOINTS];
};

struct AdvanceShared {
    ModelDev sm;
    double reach[advance::MAX_JOINTS * advance::MAX_FRAMES];
    double cnorm[coll::MAX_SPHERES];   // |c_s|
    uint8_t sframe[coll::MAX_SPHERES];  // the frame of sphere slot s
    WaveSlab w[AWAVES];
};

__device__ __forceinline__ double wave_min(double v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = fmin(v, __shfl_xor(v, o, 64));
    return __shfl(v, 0, 64);
}

__device__ __forceinline__ void stage_advance(AdvanceShared &sh, const AdvanceLaunch &a) {
    if (a.c.model) stage_model(sh.sm, a.c);
    const double *r = &a.reach.r[0][0];
    for (int i = threadIdx.x; i < advance::MAX_JOINTS * advance::MAX_FRAMES; i += blockDim.x) sh.reach[i] = r[i];
    for (int s = threadIdx.x; s < a.c.S; s += blockDim.x) {
        sh.cnorm[s] = advance::norm3(sh.sm.sph[s]);
        int f = 0;
        while (f + 1 < a.c.nf && sh.sm.frame_begin[f + 1] <= s) ++f;
        sh.sframe[s] = (uint8_t)f;
    }
    __syncthreads();
}

// The segments of a wave.  fk(ws, t): every lane; leaves the n + 2 frames of q(t) in ws.frames.
template <class FkFn>
__device__ __forceinline__ void advance_segments(const AdvanceLaunch &a, AdvanceShared &sh, FkFn &&fk) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    WaveSlab &ws = sh.w[wave];
    const int n = a.n, nf = n + 2, S = a.c.S, P = a.c.P, Ms = a.c.Ms, Mb = a.c.Mb;
    const double m = a.c.margin, mp = m - a.tol;
    const bool has_grid = a.c.grid.values != nullptr;
    for (long long b = (long long)blockIdx.x * AWAVES + wave; b < a.B; b += (long long)gridDim.x * AWAVES) {
        bool ok = true;
        if (lane < n) {
            const double x = a.qa[(size_t)lane * a.B + b], y = a.qb[(size_t)lane * a.B + b];
            ws.qa[lane] = x;
            ws.qb[lane] = y;
            ws.a[lane] = fabs(y - x);
            ok = advance::finite(x) && advance::finite(y);
        }
        advance::Walk w;
        if (__ballot(!ok) != 0ull) {
            advance::walk_refuse(w);
        } else {
            lds_sync();
            for (int s = lane; s < S; s += 64)
                ws.lam[s] = advance::lam_sphere(n, sh.sframe[s], ws.a, sh.reach, sh.cnorm[s]);
            advance::walk_begin(w);
            bool go = true;
            while (go) {
                lds_sync();  // (the sample before has been read)
                fk(ws, w.t);
                lds_sync();
                bool nan = false;
                for (int i = lane; i < 7 * nf; i += 64) nan = nan || ws.frames[i] != ws.frames[i];
                nan = __ballot(nan) != 0ull;
                double c = advance::inf(), A = advance::inf();
                if (!nan) {
                    for (int s = lane; s < S; s += 64) {
                        double p[3];
                        coll::sphere_centre(ws.frames + 7 * sh.sframe[s], sh.sm.sph[s], p);
                        ws.cen[s][0] = p[0];
                        ws.cen[s][1] = p[1];
                        ws.cen[s][2] = p[2];
                        if (has_grid) {
                            double d, adv;
                            advance::grid_term(p, sh.sm.sph[s][3], a.c.grid, m, mp, a.G, ws.lam[s], d, adv);
                            c = fmin(c, d);
                            A = fmin(A, adv);
                        }
                    }
                    lds_sync();
                    if (Ms + Mb > 0) {
                        for (int s = 0; s < S; ++s) {
                            const double p[3] = {ws.cen[s][0], ws.cen[s][1], ws.cen[s][2]};
                            const double r = sh.sm.sph[s][3], lam = ws.lam[s];
                            for (int k = lane; k < Ms; k += 64) {
                                const double *o = a.c.wsph + 4 * k;
                                const double d = coll::sphere_sphere(p, r, o, o[3]);
                                c = fmin(c, d);
                                A = fmin(A, advance::term_advance(d, m, mp, lam));
                            }
                            for (int k = lane; k < Mb; k += 64) {
                                const double d = coll::sphere_box(p, r, a.c.wbox + 10 * k);
                                c = fmin(c, d);
                                A = fmin(A, advance::term_advance(d, m, mp, lam));
                            }
                        }
                    }
                    for (int k = lane; k < P; k += 64) {
                        const int ia = sh.sm.pair[k] & 0xff, ib = sh.sm.pair[k] >> 8;
                        const double d = coll::sphere_sphere(ws.cen[ia], sh.sm.sph[ia][3], ws.cen[ib], sh.sm.sph[ib][3]);
                        const double lam = advance::pair_lam(n, sh.sframe[ia], sh.cnorm[ia], sh.sframe[ib],
                                                             sh.cnorm[ib], ws.a, sh.reach);
                        c = fmin(c, d);
                        A = fmin(A, advance::term_advance(d, m, mp, lam));
                    }
                    c = wave_min(c);
                    A = wave_min(A);
                }
                go = advance::walk_take(w, nan, c, A, m, a.max_steps);
            }
        }
        if (lane == 0) {
            if (a.status) a.status[b] = w.status;
            if (a.steps) a.steps[b] = w.steps;
            if (a.t_stop) a.t_stop[b] = w.t_stop;
            if (a.clearance) a.clearance[b] = w.clearance;
        }
        lds_sync();  // (the slab has been read before the next segment overwrites it)
    }
}

__device__ __forceinline__ void store_identity7(double *dst) {
    dst[0] = 0.0; dst[1] = 0.0; dst[2] = 0.0; dst[3] = 0.0; dst[4] = 0.0; dst[5] = 0.0; dst[6] = 1.0;
}

template <int N, bool TIP>
__global__ __launch_bounds__(ABLOCK) void advance_kernel(const AdvanceLaunch a) {
    __shared__ ChainDev sch;
    __shared__ AdvanceShared sh;
    stage_chain(sch, a.c.chain);
    stage_advance(sh, a);
    advance_segments(a, sh, [&](WaveSlab &ws, double t) {
        double q[N];
#pragma unroll
        for (int i = 0; i < N; ++i) q[i] = advance::sample(ws.qa[i], ws.qb[i], t);
        Kin<N, TIP> kin;
        forward_kinematics<N, TIP>(sch, a.c.ep, q, kin);
        if ((threadIdx.x & 63) == 0) {
            store_identity7(ws.frames);
#pragma unroll
            for (int k = 0; k < N; ++k) store_pose7(ws.frames + 7 * (k + 1), kin.tf[k]);
            store_pose7(ws.frames + 7 * (N + 1), kin.ee);
        }
    });
}

// 9 .. 16 joint positions (run-time n): wide_forward writes the joint frames straight into the slab (every lane the
// same values to the same words).
__global__ __launch_bounds__(ABLOCK) void wide_advance_kernel(const AdvanceLaunch a) {
    __shared__ WideChainDev sch;
    __shared__ AdvanceShared sh;
    stage_wide_chain(sch, a.c.wchain);
    stage_advance(sh, a);
    const int n = sch.n_pos;
    advance_segments(a, sh, [&](WaveSlab &ws, double t) {
        const int lane = threadIdx.x & 63;
        if (lane < n) ws.q[lane] = advance::sample(ws.qa[lane], ws.qb[lane], t);
        lds_sync();
        const Pose ee = wide_forward(sch, a.c.ep, n, (const double *)ws.q, (double *)(ws.frames + 7));
        if (lane == 0) {
            store_identity7(ws.frames);
            store_pose7(ws.frames + 7 * (n + 1), ee);
        }
    });
}

}  // namespace

extern "C" {

int optik_hip_collision_motion_certify_batch(const optik_hip_chain *ch, const double *ee_offset7, const double *d_qa,
                                             const double *d_qb, int64_t B, double tol, double grid_lipschitz,
                                             int32_t max_steps, int32_t *d_status, int32_t *d_steps, double *d_t_stop,
                                             double *d_clearance, void *stream) {
    if (!ch || B < 0) return fail(OPTIK_HIP_EINVAL, "bad argument");
    if (!(tol > 0.0) || !std::isfinite(tol)) return fail(OPTIK_HIP_EINVAL, "motion certify: tol must be finite and > 0");
    if (!(grid_lipschitz > 0.0) || !std::isfinite(grid_lipschitz))
        return fail(OPTIK_HIP_EINVAL, "motion certify: grid_lipschitz must be finite and > 0");
    if (max_steps < 2 || max_steps > OPTIK_HIP_CERTIFY_MAX_STEPS)
        return fail(OPTIK_HIP_EINVAL, "motion certify: max_steps must be in 2 .. 65536");
    if (B > ((int64_t)1 << 30)) return fail(OPTIK_HIP_EINVAL, "motion certify: more than 2^30 segments in one launch");
    if (ch->prismatic) return fail(OPTIK_HIP_EUNSUPPORTED, prismatic_msg());
    if (B == 0 || (!d_status && !d_steps && !d_t_stop && !d_clearance)) return 0;
    if (!d_qa || !d_qb) return fail(OPTIK_HIP_EINVAL, "bad argument");
    BIND_DEVICE(ch);
    AdvanceLaunch a;
    std::memset(&a, 0, sizeof a);
    fill_launch(ch, ee_offset7, nullptr, B, a.c);
    a.qa = d_qa;
    a.qb = d_qb;
    a.B = B;
    a.n = ch->n;
    a.max_steps = max_steps;
    a.tol = tol;
    a.G = grid_lipschitz;
    a.status = d_status; a.steps = d_steps; a.t_stop = d_t_stop; a.clearance = d_clearance;
    if (ch->wide) advance::build_reach(ch->n, ch->whost.origin, ch->whost.has_tip != 0, ee_offset7, a.reach);
    else advance::build_reach(ch->n, ch->host.origin, ch->host.has_tip != 0, ee_offset7, a.reach);
    const int grid = grid_for(ch, B, AWAVES, ABLOCKS_PER_CU);
    if (ch->wide) {
        hipLaunchKernelGGL(wide_advance_kernel, dim3(grid), dim3(ABLOCK), 0, (hipStream_t)stream, a);
    } else {
#define CALL(NN, TT) hipLaunchKernelGGL((advance_kernel<NN, TT>), dim3(grid), dim3(ABLOCK), 0, (hipStream_t)stream, a)
        OPTIK_DISPATCH(ch, CALL);
#undef CALL
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"
