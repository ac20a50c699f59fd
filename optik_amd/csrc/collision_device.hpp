// collision_device.hpp -- the device side of the collision filter that its translation units share: the launch
// arguments, the staging of the model in LDS and the clearance of ONE configuration held in a lane's registers.
//
//   ik_collision.hip   one configuration per lane from memory: link frames, clearance batch, the collision key pass
//   ik_motion.hip      one (segment, sample) item per lane, the configuration interpolated in registers
//
// Both run config_clearance / wide_config_clearance below, so a sample of a motion has the bits collision_batch gives
// the same configuration (collision_measure.hpp: one source, one operation order).
#pragma once

#include "collision_measure.hpp"
#include "collision_model.hpp"
#include "ik_host.hpp"
#include "ik_jacobian.hpp"
#include "ik_wide.hpp"

namespace optik {
namespace colldev {

using namespace optik::host;
using namespace optik::hostparams;
using optik::coll::ModelDev;

enum : int { FORM_FRAMES = 0, FORM_BATCH = 1, FORM_KEY = 2 };

struct CollLaunch {
    const ChainDev *chain;       // n <= 8
    const WideChainDev *wchain;  // 9 .. 16 joint positions
    EvalParams ep;               // only the ee_offset part is used
    const ModelDev *model;       // null: no model (S = 0)
    int S, P, groups, nf;        // spheres, pairs, pair groups, frames (n + 2)
    double margin;
    const double *wsph;          // [Ms][4]
    const double *wbox;          // [Mb][10]
    int Ms, Mb;
    coll::Grid grid;             // the distance-field world (values null: none)
    const double *q;             // [n][B]: the configurations (key form: the launch's per-restart x)
    long long B;
    double *key;                 // key form: [B], read, and set to +inf where the success is not free
    double *clearance;           // batch form: [B] or null
    uint8_t *free_flag;          // batch form: [B] or null
    double *frames;              // frames form: [B][nf][7]
};

// The model's S spheres, P pairs and group tables into LDS (whole words; the struct is 8-byte aligned).
__device__ __forceinline__ void stage_model(ModelDev &dst, const CollLaunch &a) {
    {
        const double *s = &a.model->sph[0][0];
        double *d = &dst.sph[0][0];
        for (int i = threadIdx.x; i < 4 * a.S; i += blockDim.x) d[i] = s[i];
    }
    {
        const uint32_t *s = reinterpret_cast<const uint32_t *>(a.model->pair);
        uint32_t *d = reinterpret_cast<uint32_t *>(dst.pair);
        for (int i = threadIdx.x; i < (a.P + 1) / 2; i += blockDim.x) d[i] = s[i];
    }
    {
        constexpr int off = (int)(offsetof(ModelDev, frame_begin) / sizeof(double));
        constexpr int nd = (int)(sizeof(ModelDev) / sizeof(double)) - off;
        static_assert(offsetof(ModelDev, frame_begin) % sizeof(double) == 0, "tables start on a double");
        const double *s = reinterpret_cast<const double *>(a.model) + off;
        double *d = reinterpret_cast<double *>(&dst) + off;
        for (int i = threadIdx.x; i < nd; i += blockDim.x) d[i] = s[i];
    }
    __syncthreads();
}

__device__ __forceinline__ bool wave_any_lane(bool p) { return __ballot(p) != 0ull; }

// The clearance of one configuration (FORM_BATCH) or whether it is free (FORM_KEY: the return value is 0.0 for free,
// anything else for not free; a wave stops once none of its lanes is free).  frame_of(f, pose7) gives frame f.
template <int FORM, class FrameFn>
__device__ __forceinline__ double clearance_of(const ModelDev &m, const CollLaunch &a, bool nan, FrameFn &&frame_of,
                                               bool &free_out) {
    double c = __builtin_huge_val();
    bool ok = !nan;
    const double margin = a.margin;
    const bool has_grid = a.grid.values != nullptr;  // (a launch argument: wave-uniform)
    if (a.Ms + a.Mb > 0 || has_grid) {
        for (int f = 0; f < a.nf; ++f) {
            const int s0 = m.frame_begin[f], s1 = m.frame_begin[f + 1];
            if (s0 == s1) continue;
            double fp[7];
            frame_of(f, fp);
            for (int s = s0; s < s1; ++s) {
                double p[3];
                coll::sphere_centre(fp, m.sph[s], p);
                const double r = m.sph[s][3];
                for (int k = 0; k < a.Ms; ++k) {
                    const double *w = a.wsph + 4 * k;
                    const double d = coll::sphere_sphere(p, r, w, w[3]);
                    if (FORM == FORM_KEY) ok = ok && d >= margin;
                    else c = fmin(c, d);
                }
                for (int k = 0; k < a.Mb; ++k) {
                    const double d = coll::sphere_box(p, r, a.wbox + 10 * k);
                    if (FORM == FORM_KEY) ok = ok && d >= margin;
                    else c = fmin(c, d);
                }
                if (has_grid) {
                    const double d = coll::grid_distance(p, r, a.grid);
                    if (FORM == FORM_KEY) ok = ok && d >= margin;
                    else c = fmin(c, d);
                }
                if (FORM == FORM_KEY && !wave_any_lane(ok)) { free_out = false; return 0.0; }
            }
        }
    }
    for (int g = 0; g < a.groups; ++g) {
        double pa7[7], pb7[7];
        frame_of(m.group_fa[g], pa7);
        frame_of(m.group_fb[g], pb7);
        const int k1 = m.group_begin[g + 1];
        for (int k = m.group_begin[g]; k < k1; ++k) {
            const int ia = m.pair[k] & 0xff, ib = m.pair[k] >> 8;
            double pa[3], pb[3];
            coll::sphere_centre(pa7, m.sph[ia], pa);
            coll::sphere_centre(pb7, m.sph[ib], pb);
            const double d = coll::sphere_sphere(pa, m.sph[ia][3], pb, m.sph[ib][3]);
            if (FORM == FORM_KEY) ok = ok && d >= margin;
            else c = fmin(c, d);
        }
        if (FORM == FORM_KEY && !wave_any_lane(ok)) { free_out = false; return 0.0; }
    }
    if (FORM == FORM_KEY) { free_out = ok; return 0.0; }
    if (nan) c = __builtin_nan("");
    free_out = c >= margin;
    return c;
}

__device__ __forceinline__ void store_pose7(double *dst, const Pose &p) {
    dst[0] = p.t.x; dst[1] = p.t.y; dst[2] = p.t.z;
    dst[3] = p.q.i; dst[4] = p.q.j; dst[5] = p.q.k; dst[6] = p.q.w;
}

__device__ __forceinline__ void pose7_of(const Pose &p, double (&o)[7]) {
    o[0] = p.t.x; o[1] = p.t.y; o[2] = p.t.z; o[3] = p.q.i; o[4] = p.q.j; o[5] = p.q.k; o[6] = p.q.w;
}

__device__ __forceinline__ void identity7(double (&o)[7]) {
    o[0] = 0.0; o[1] = 0.0; o[2] = 0.0; o[3] = 0.0; o[4] = 0.0; o[5] = 0.0; o[6] = 1.0;
}

// One configuration q of a chain of N <= 8 joints, frames in registers: its clearance and free flag (FORM_BATCH), or
// the free flag alone (FORM_KEY).  It may be called from divergent lanes: clearance_of's vote (__ballot) counts the
// active lanes only, so lanes without work simply do not call it (the key pass skips failed restarts that way).
template <int N, bool TIP, int FORM>
__device__ __forceinline__ double config_clearance(const ChainDev &sch, const ModelDev &sm, const CollLaunch &a,
                                                   const double (&q)[N], bool &free_) {
    Kin<N, TIP> kin;
    forward_kinematics<N, TIP>(sch, a.ep, q, kin);
    bool nan = false;
#pragma unroll
    for (int k = 0; k < N; ++k) {
        nan = nan || kin.tf[k].t.x != kin.tf[k].t.x || kin.tf[k].t.y != kin.tf[k].t.y
              || kin.tf[k].t.z != kin.tf[k].t.z || kin.tf[k].q.i != kin.tf[k].q.i || kin.tf[k].q.j != kin.tf[k].q.j
              || kin.tf[k].q.k != kin.tf[k].q.k || kin.tf[k].q.w != kin.tf[k].q.w;
    }
    nan = nan || kin.ee.t.x != kin.ee.t.x || kin.ee.t.y != kin.ee.t.y || kin.ee.t.z != kin.ee.t.z
          || kin.ee.q.i != kin.ee.q.i || kin.ee.q.j != kin.ee.q.j || kin.ee.q.k != kin.ee.q.k
          || kin.ee.q.w != kin.ee.q.w;
    // frame f of the configuration: a wave-uniform index, so the selection is a scalar-predicated one
    auto frame_of = [&](int f, double (&o)[7]) {
        f = __builtin_amdgcn_readfirstlane(f);
        identity7(o);
#pragma unroll
        for (int k = 0; k < N; ++k)
            if (f == k + 1) pose7_of(kin.tf[k], o);
        if (f == N + 1) pose7_of(kin.ee, o);
    };
    free_ = true;
    double c = __builtin_huge_val();
    if (a.model) c = clearance_of<FORM>(sm, a, nan, frame_of, free_);
    else if (nan) { c = __builtin_nan(""); free_ = false; }
    return c;
}

// The same for 9 .. 16 joint positions: the joint frames wide_forward writes (7 per joint) in a per-lane array.
template <int FORM>
__device__ __forceinline__ double wide_config_clearance(const WideChainDev &sch, const ModelDev &sm,
                                                        const CollLaunch &a, int n, const double *q, bool &free_) {
    double tf[7 * WIDE_MAX_DOF];
    const Pose ee = wide_forward(sch, a.ep, n, q, tf);
    bool nan = false;
    for (int k = 0; k < 7 * n; ++k) nan = nan || tf[k] != tf[k];
    nan = nan || ee.t.x != ee.t.x || ee.t.y != ee.t.y || ee.t.z != ee.t.z || ee.q.i != ee.q.i
          || ee.q.j != ee.q.j || ee.q.k != ee.q.k || ee.q.w != ee.q.w;
    auto frame_of = [&](int f, double (&o)[7]) {
        f = __builtin_amdgcn_readfirstlane(f);
        if (f == 0) identity7(o);
        else if (f == n + 1) pose7_of(ee, o);
        else
            for (int i = 0; i < 7; ++i) o[i] = tf[7 * (f - 1) + i];
    };
    free_ = true;
    double c = __builtin_huge_val();
    if (a.model) c = clearance_of<FORM>(sm, a, nan, frame_of, free_);
    else if (nan) { c = __builtin_nan(""); free_ = false; }
    return c;
}

inline const char *prismatic_msg() {
    return "collision: prismatic joints are not supported (IK refuses such chains; the reference's Jacobian panics: "
           "kinematics.rs:185 todo!())";
}

// The chain's tables, model and world as a launch sees them (q [n][B]).
inline void fill_launch(const optik_hip_chain *ch, const double *ee_offset7, const double *q, long long B,
                        CollLaunch &a) {
    std::memset(&a, 0, sizeof a);
    a.chain = ch->dev;
    a.wchain = ch->wdev;
    const double one[3] = {1, 1, 1};
    make_eval_params(one, one, ee_offset7, a.ep);
    a.q = q;
    a.B = B;
    a.nf = ch->n + 2;
    if (ch->coll_S > 0) {
        a.model = ch->coll_dev;
        a.S = ch->coll_S;
        a.P = ch->coll_P;
        a.groups = ch->coll_groups;
        a.margin = ch->coll_margin;
        a.Ms = ch->world_Ms;
        a.Mb = ch->world_Mb;
        a.wsph = ch->world_dev.get();
        a.wbox = a.wsph ? a.wsph + 4 * (size_t)ch->world_Ms : nullptr;
        if (ch->grid_n[0] > 0) {
            a.grid.values = ch->grid_dev.get();
            a.grid.inv = ch->grid_inv;
            for (int k = 0; k < 3; ++k) {
                a.grid.origin[k] = ch->grid_origin[k];
                a.grid.n[k] = ch->grid_n[k];
            }
        }
    }
}

}  // namespace colldev
}  // namespace optik
