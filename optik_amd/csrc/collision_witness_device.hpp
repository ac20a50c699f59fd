// collision_witness_device.hpp -- the device side of the witness table that its translation units share: the distance
// pass that keeps one running (dist, witness) pair per frame and lane, and the gradient of a row from its witness
// (collision_gradient.hpp).
//
//   ik_avoid.hip           collision_witness_kernel, diff_ik_avoid_kernel: one configuration per lane
//   ik_path_optimize.hip   path_optimize_kernel: one waypoint per lane, the rows feeding the obstacle cost of a path
//
// A launch type `Launch` has  CollLaunch c  (chain, ee_offset, model, world) and  const uint16_t *orig  ([S + P]: the
// caller's index of the sphere in a slot, of the pair at a position).
#pragma once

#include "collision_device.hpp"
#include "collision_gradient.hpp"

namespace optik {
namespace colldev {

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
template <int N, bool TIP, class Launch>
__device__ __forceinline__ void witness_pass(const ModelDev &m, const Launch &a, const Kin<N, TIP> &kin,
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
template <int N, bool TIP, class Launch, class GSink>
__device__ __forceinline__ void row_gradient(const ChainDev &sch, const ModelDev &m, const Launch &a,
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

}  // namespace colldev
}  // namespace optik
