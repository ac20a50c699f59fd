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
#include "collision_device.hpp"
#include "collision_gradient.hpp"
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

// A witness in one word: slot << 18 | kind << 16 | index (a world obstacle's, or the pair's position); -1: none.
__device__ __forceinline__ int32_t pack_witness(int slot, int kind, int idx) {
    return (slot << 18) | (kind << 16) | idx;
}

template <int N>
struct Rows {
    double dist[N + 2];
    int32_t wit[N + 2];
};

template <int N, bool TIP>
__device__ __forceinline__ bool kin_has_nan(const Kin<N, TIP> &kin) {
    bool nan = false;
#pragma unroll
    for (int k = 0; k < N; ++k) {
        nan = nan || kin.tf[k].t.x != kin.tf[k].t.x || kin.tf[k].t.y != kin.tf[k].t.y
              || kin.tf[k].t.z != kin.tf[k].t.z || kin.tf[k].q.i != kin.tf[k].q.i || kin.tf[k].q.j != kin.tf[k].q.j
              || kin.tf[k].q.k != kin.tf[k].q.k || kin.tf[k].q.w != kin.tf[k].q.w;
    }
    return nan || kin.ee.t.x != kin.ee.t.x || kin.ee.t.y != kin.ee.t.y || kin.ee.t.z != kin.ee.t.z
           || kin.ee.q.i != kin.ee.q.i || kin.ee.q.j != kin.ee.q.j || kin.ee.q.k != kin.ee.q.k
           || kin.ee.q.w != kin.ee.q.w;
}

// Frame f of the configuration: f wave-uniform (a scalar-predicated selection), or a per-lane f (selects).
template <int N, bool TIP>
__device__ __forceinline__ void frame_lane(const Kin<N, TIP> &kin, int f, double (&o)[7]) {
    identity7(o);
#pragma unroll
    for (int k = 0; k < N; ++k)
        if (f == k + 1) pose7_of(kin.tf[k], o);
    if (f == N + 1) pose7_of(kin.ee, o);
}
template <int N, bool TIP>
__device__ __forceinline__ void frame_uniform(const Kin<N, TIP> &kin, int f, double (&o)[7]) {
    frame_lane<N, TIP>(kin, __builtin_amdgcn_readfirstlane(f), o);
}

template <int N>
__device__ __forceinline__ void row_get(const Rows<N> &rows, int f, double &d, int32_t &w) {
    d = __builtin_huge_val(); w = -1;
#pragma unroll
    for (int k = 0; k < N + 2; ++k)
        if (f == k) { d = rows.dist[k]; w = rows.wit[k]; }
}
template <int N>
__device__ __forceinline__ void row_set(Rows<N> &rows, int f, double d, int32_t w) {
#pragma unroll
    for (int k = 0; k < N + 2; ++k)
        if (f == k) { rows.dist[k] = d; rows.wit[k] = w; }
}

// The distance pass: every term once, each into the row of its frame (collision_gradient.hpp: the enumeration and its
// tie rule).  The spheres of a frame keep the caller's order in their slots, so d < best alone gives the first of equal
// terms; the pairs are grouped by frame pair, so among equal pair terms the caller's lower index is looked up.
template <int N, bool TIP>
__device__ __forceinline__ void witness_pass(const ModelDev &m, const AvoidLaunch &a, const Kin<N, TIP> &kin,
                                             Rows<N> &rows) {
    const CollLaunch &c = a.c;
    const bool has_grid = c.grid.values != nullptr;
    const bool world = c.Ms + c.Mb > 0 || has_grid;
    for (int f = 0; f < N + 2; ++f) {
        double best = __builtin_huge_val();
        int32_t bw = -1;
        const int s0 = m.frame_begin[f], s1 = m.frame_begin[f + 1];
        if (world && s0 != s1) {
            double fp[7];
            frame_uniform<N, TIP>(kin, f, fp);
            for (int s = s0; s < s1; ++s) {
                double p[3];
                coll::sphere_centre(fp, m.sph[s], p);
                const double r = m.sph[s][3];
                for (int k = 0; k < c.Ms; ++k) {
                    const double *w = c.wsph + 4 * k;
                    const double d = coll::sphere_sphere(p, r, w, w[3]);
                    if (d < best) { best = d; bw = pack_witness(s, coll::WIT_SPHERE, k); }
                }
                for (int k = 0; k < c.Mb; ++k) {
                    const double d = coll::sphere_box(p, r, c.wbox + 10 * k);
                    if (d < best) { best = d; bw = pack_witness(s, coll::WIT_BOX, k); }
                }
                if (has_grid) {
                    const double d = coll::grid_distance(p, r, c.grid);
                    if (d < best) { best = d; bw = pack_witness(s, coll::WIT_GRID, 0); }
                }
            }
        }
        row_set<N>(rows, __builtin_amdgcn_readfirstlane(f), best, bw);
    }
    for (int g = 0; g < c.groups; ++g) {
        const int fa = m.group_fa[g], fb = m.group_fb[g];
        const int f = __builtin_amdgcn_readfirstlane(fa > fb ? fa : fb);
        double pa7[7], pb7[7];
        frame_uniform<N, TIP>(kin, fa, pa7);
        frame_uniform<N, TIP>(kin, fb, pb7);
        double best;
        int32_t bw;
        row_get<N>(rows, f, best, bw);
        const int k1 = m.group_begin[g + 1];
        for (int k = m.group_begin[g]; k < k1; ++k) {
            const int ia = m.pair[k] & 0xff, ib = m.pair[k] >> 8;
            double pa[3], pb[3];
            coll::sphere_centre(pa7, m.sph[ia], pa);
            coll::sphere_centre(pb7, m.sph[ib], pb);
            const double d = coll::sphere_sphere(pa, m.sph[ia][3], pb, m.sph[ib][3]);
            bool take = d < best;
            if (d == best && bw >= 0 && ((bw >> 16) & 3) == coll::WIT_PAIR)  // equal pair terms: the caller's first
                take = a.orig[c.S + k] < a.orig[c.S + (bw & 0xffff)];
            if (take) { best = d; bw = pack_witness(ia, coll::WIT_PAIR, k); }
        }
        row_set<N>(rows, f, best, bw);
    }
}

__device__ __forceinline__ int frame_of_slot(const ModelDev &m, int slot, int nf) {
    int f = 0;
    for (int k = 1; k < nf; ++k) f += (int)m.frame_begin[k] <= slot ? 1 : 0;
    return f;
}

// The gradient of row f from its witness w >= 0 (collision_gradient.hpp, steps 1 - 4): gsink(j, d dist / d q_j).
template <int N, bool TIP, class GSink>
__device__ __forceinline__ void row_gradient(const ChainDev &sch, const ModelDev &m, const AvoidLaunch &a,
                                             const Kin<N, TIP> &kin, int f, int32_t w, GSink &&gsink) {
    const int slot = w >> 18, kind = (w >> 16) & 3, idx = w & 0xffff;
    auto joint_of = [&](int j, double *ax, double *o) {
        double fp[7];
        frame_uniform<N, TIP>(kin, j, fp);
        coll::qrot3(fp + 3, sch.axis[j - 1], ax);
        o[0] = fp[0]; o[1] = fp[1]; o[2] = fp[2];
    };
    if (kind == coll::WIT_PAIR) {
        const int ia = m.pair[idx] & 0xff, ib = m.pair[idx] >> 8;
        const int fa = frame_of_slot(m, ia, N + 2), fb = frame_of_slot(m, ib, N + 2);
        double pa7[7], pb7[7];
        frame_lane<N, TIP>(kin, fa, pa7);
        frame_lane<N, TIP>(kin, fb, pb7);
        coll::pair_term_gradient(N, fa, pa7, m.sph[ia], fb, pb7, m.sph[ib], joint_of, gsink);
    } else {
        double fp[7];
        frame_lane<N, TIP>(kin, f, fp);  // (the damper rows of diff_ik_avoid_kernel differ from lane to lane)
        const double *obstacle = kind == coll::WIT_SPHERE ? a.c.wsph + 4 * idx
                                                          : (kind == coll::WIT_BOX ? a.c.wbox + 10 * idx : nullptr);
        coll::world_term_gradient(N, f, fp, m.sph[slot], kind, obstacle, a.c.grid, joint_of, gsink);
    }
}

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
