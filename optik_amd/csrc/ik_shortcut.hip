// ik_shortcut.hip -- path shortcutting and equal-spacing resampling on the device (shortcut_measure.hpp: the arithmetic
// and its operation order).  optik_hip_path_shortcut / _path_resample (include/optik_hip.h).
//
//   shortcut_gather_kernel     one block of 256 per path.  Its first wave builds the path's vertices in LDS (lane s
//                              holds segment s; the serial sums of the subdivision are lane 0's, in the order the
//                              header fixes); then one thread per (i, j) of the V x V square writes the segments vertex
//                              i -> vertex j, i < j, into the chain's workspace as the motion check takes them.  Pairs
//                              beyond the path's vertex count get NaN endpoints: the motion check does not sample them.
//   (optik_hip_collision_motion_batch, classify form, on the same stream: the motion check's own code)
//   shortcut_route_kernel      one wave per path.  It builds the same vertices again (LDS, [joint][64]: lane j reads its
//                              own column without a bank conflict, vertex i is a broadcast), then i runs serially from
//                              the end while the lanes cover j: lane j keeps d[j] in a register, the minimum over
//                              (value, -j) is a butterfly over the wave -- a total order, so exact in any order -- and
//                              lane i takes the result.  Lane 0 walks the route and the wave writes the path.
//   shortcut_resample_kernel   one thread per (path, output waypoint); no LDS, no workspace.
//
// Under a pose constraint (shortcut_constrained_measure.hpp; optik_hip_path_shortcut_constrained /
// _path_resample_constrained) the same chunk loop (shortcut_chunks) runs four kernels per chunk:
//   shortcut_cgather_kernel<CH>       one block of 256 per path, the chain table staged in LDS (stage_table,
//                                     ik_launch.hpp).  The first wave builds the vertices as above, then lane u projects
//                                     vertex u unless it is one of the input's waypoints (constraint::project, the
//                                     header's own function; lanes whose loops differ in length cost the wave the
//                                     longest of them and nothing else); a vertex that did not project becomes NaN.
//                                     The block stores the final vertices [n][Pc * V] behind the segments in the
//                                     workspace, counts the projections and writes the pair segments as above.
//   (the motion check, classify form, as above)
//   (constraint_mask_launch, ik_host.hpp: ik_constraint.hip's check along a motion in its mask form -- a pair whose
//   flag is 0 already is not sampled, every other flag becomes constraint::motion's ok)
//   shortcut_route_stored_kernel      shortcut_route_kernel's body (route_path) with the vertices read from the
//                                     stored block: nothing is projected twice.
//   shortcut_cresample_kernel<CH>     one wave per path, lane j = output waypoint j: resample, project, then the
//                                     wave's ballots give the status and the two counts.
// CH is ChainDev (n <= 8) or WideChainDev (9 .. 16); the head of the constraint's record, its refusals and the dispatch
// on CH are constraint_device.hpp's.
//
// The paths of a call are processed in chunks of at most OPTIK_HIP_PATH_SHORTCUT_CHUNK_BYTES of workspace, launched
// one after the other on the stream; a path's blocks see only that path, so nothing depends on P or on the chunking.
#include "constraint_device.hpp"
#include "shortcut_constrained_measure.hpp"

using namespace optik;
using namespace optik::host;
using namespace optik::hostparams;
using namespace optik::colldev;
using namespace optik::condev;

static_assert(shortcut::MAX_POINTS == OPTIK_HIP_PATH_OPTIMIZE_MAX_WAYPOINTS && shortcut::MAX_POINTS == 64,
              "a shortcut path is a path path_optimize takes; one lane of a wave per vertex");
static_assert(shortcut::MAX_JOINTS == WIDE_MAX_DOF, "shortcut_measure.hpp states the cap on the joint positions");
static_assert(shortcut::PROJECTION_OK == constraint::PROJECTED && constraint::PROJECTED == OPTIK_HIP_CONSTRAINT_PROJECTED,
              "shortcut_constrained_measure.hpp names the projection's status without including constraint_measure.hpp");
static_assert(shortcut::UNPROJECTED == OPTIK_HIP_PATH_RESAMPLE_UNPROJECTED, "optik_hip.h states the status");
static_assert(shortcut::MAX_JOINTS == constraint::MAXN, "a vertex is a configuration the projection takes");

namespace {

constexpr int GATHER_BLOCK = 256, SC_WAVE = 64, RESAMPLE_BLOCK = 256;
constexpr int MP = shortcut::MAX_POINTS;
constexpr long long MAX_PATHS = 1ll << 30;

struct ShortcutLaunch {
    const double *path;  // [Lin][P][n], the whole call's
    const int32_t *len;  // [P] or null: Lin
    long long P;         // the call's paths (the stride of a waypoint)
    long long p0, Pc;    // this chunk: paths p0 .. p0 + Pc - 1
    int n, Lin, V, Lout;
    double hop;
    double *qa, *qb;           // [n][Pc * pairs] the gathered segments
    const uint8_t *free_flag;  // [Pc * pairs]
    double *out;         // [Lout][P][n] or null
    int32_t *len_out;    // [P] or null
    double *cost, *cost_in;  // [P] or null
    int32_t *status;     // [P] or null
};

// What both kernels hold of a path in LDS.
struct PathLds {
    double v[shortcut::MAX_JOINTS * MP];  // vertex u's joint i at v[i * MP + u]
    double w[MP];                         // the input's segment weights
    int m[MP], off[MP];
    shortcut::Prepared prep;
};

// Steps 1 and 2 of the header by the first wave of the block; every thread of the block calls it.  STORED: the
// vertices are not interpolated but read from `stored` [n][Pc * V], where shortcut_cgather_kernel left them.
template <bool STORED>
__device__ __forceinline__ void build_vertices(const ShortcutLaunch &a, long long p, PathLds &s,
                                               const double *stored = nullptr) {
    const int tid = threadIdx.x;
    const double *path = a.path + p * a.n;
    const long long st = a.P * a.n;
    const int len = a.len ? a.len[p] : a.Lin;
    const int le = shortcut::read_length(len, a.Lin);
    bool fin = true;
    if (tid < le) fin = shortcut::waypoint_finite(a.n, path, st, tid);
    if (tid < le - 1) s.w[tid] = shortcut::segment_weight(a.n, path, st, tid);
    const bool all_finite = __syncthreads_and(fin) != 0;
    if (tid == 0) s.prep = shortcut::prepare(len, a.Lin, a.V, all_finite, s.w, s.m, s.off);
    __syncthreads();
    if (tid < s.prep.nv) {
        if constexpr (STORED) {
            const long long SV = a.Pc * a.V, u = (p - a.p0) * a.V + tid;
            for (int i = 0; i < a.n; ++i) s.v[i * MP + tid] = stored[(long long)i * SV + u];
        } else {
            const int seg = shortcut::vertex_segment(le, s.off, tid);
            for (int i = 0; i < a.n; ++i) s.v[i * MP + tid] = shortcut::vertex_joint(path, st, s.m, s.off, seg, tid, i);
        }
    }
    __syncthreads();
}

// The segments vertex i -> vertex j, i < j, of the path in LDS into the workspace (every thread of the block).
__device__ __forceinline__ void write_pairs(const ShortcutLaunch &a, long long pc, const PathLds &s) {
    const int V = a.V, nv = s.prep.nv, pairs = shortcut::pair_count(V);
    const long long B = a.Pc * pairs;
    for (int e = threadIdx.x; e < V * V; e += GATHER_BLOCK) {
        const int i = e / V, j = e % V;
        if (i >= j) continue;
        const long long b = pc * pairs + shortcut::pair_index(V, i, j);
        const bool real = j < nv;
        for (int k = 0; k < a.n; ++k) {
            a.qa[(long long)k * B + b] = real ? s.v[k * MP + i] : __builtin_nan("");
            a.qb[(long long)k * B + b] = real ? s.v[k * MP + j] : __builtin_nan("");
        }
    }
}

__global__ __launch_bounds__(GATHER_BLOCK) void shortcut_gather_kernel(const ShortcutLaunch a) {
    __shared__ PathLds s;
    const long long pc = blockIdx.x;
    build_vertices<false>(a, a.p0 + pc, s);
    write_pairs(a, pc, s);
}

// The route of one path by one wave (steps 4 to 6); STORED as build_vertices takes it.
template <bool STORED>
__device__ __forceinline__ void route_path(const ShortcutLaunch &a, const double *stored) {
    __shared__ PathLds s;
    __shared__ int s_succ[MP], s_route[MP];
    __shared__ shortcut::Result s_res;
    const long long pc = blockIdx.x, p = a.p0 + pc;
    const int lane = threadIdx.x;
    build_vertices<STORED>(a, p, s, stored);
    const shortcut::Prepared prep = s.prep;
    const int V = a.V, nv = prep.nv;
    double d_lane = shortcut::inf();  // d[lane]
    if (prep.status == shortcut::GO_ON) {
        const uint8_t *free_flag = a.free_flag + pc * shortcut::pair_count(V);
        if (lane == nv - 1) d_lane = 0.0;
        for (int i = nv - 2; i >= 0; --i) {
            double c = shortcut::inf();
            int j = -1;
            if (lane > i && lane < nv) {
                const double w = shortcut::pair_weight(a.n, s.v, MP, i, lane,
                                                       free_flag[shortcut::pair_index(V, i, lane)] != 0);
                c = shortcut::hop_cost(w, a.hop, d_lane);
                if (c < shortcut::inf()) j = lane;
            }
            // (the minimum of the candidates over (value, -j): every lane ends with it)
#pragma unroll
            for (int o = SC_WAVE / 2; o >= 1; o >>= 1) {
                const double oc = __shfl_xor(c, o, SC_WAVE);
                const int oj = __shfl_xor(j, o, SC_WAVE);
                if (oj >= 0 && shortcut::beats(oc, oj, c, j)) { c = oc; j = oj; }
            }
            if (lane == i) {
                d_lane = j >= 0 ? c : shortcut::inf();
                s_succ[i] = j;
            }
        }
    }
    const double d0 = __shfl(d_lane, 0, SC_WAVE);
    __syncthreads();
    if (lane == 0) {
        int count;
        s_res = shortcut::finish(prep, a.n, s.v, MP, d0, s_succ, a.Lout, shortcut::input_cost(prep.le, s.w), s_route,
                                 &count);
        if (a.len_out) a.len_out[p] = s_res.len;
        if (a.cost) a.cost[p] = s_res.cost;
        if (a.cost_in) a.cost_in[p] = s_res.cost_in;
        if (a.status) a.status[p] = s_res.status;
    }
    __syncthreads();
    if (!a.out) return;
    const shortcut::Result r = s_res;
    const double *path = a.path + p * a.n;
    const long long st = a.P * a.n;
    for (int e = lane; e < a.Lout * a.n; e += SC_WAVE) {
        const int t = e / a.n, i = e % a.n;
        a.out[((long long)t * a.P + p) * a.n + i] = shortcut::output_joint(r, prep.le, path, st, s.v, MP, s_route, t, i);
    }
}

__global__ __launch_bounds__(SC_WAVE) void shortcut_route_kernel(const ShortcutLaunch a) { route_path<false>(a, nullptr); }

__global__ __launch_bounds__(SC_WAVE) void shortcut_route_stored_kernel(const ShortcutLaunch a, const double *stored) {
    route_path<true>(a, stored);
}

struct ResampleLaunch {
    const double *path;  // [Lin][P][n]
    const int32_t *len;  // [P] or null: Lin
    long long P;
    int n, Lin, Lout;
    double *out;         // [Lout][P][n]
    int32_t *status;     // [P] or null
};

__global__ __launch_bounds__(RESAMPLE_BLOCK) void shortcut_resample_kernel(const ResampleLaunch a) {
    const long long g = (long long)blockIdx.x * RESAMPLE_BLOCK + threadIdx.x;
    if (g >= a.P * a.Lout) return;
    const long long p = g / a.Lout;
    const int j = (int)(g % a.Lout);
    const int len = a.len ? a.len[p] : a.Lin;
    const int st = shortcut::resample_waypoint(a.n, a.path + p * a.n, a.P * a.n, len, a.Lin, a.Lout, j,
                                               a.out + ((long long)j * a.P + p) * a.n, 1);
    if (j == 0 && a.status) a.status[p] = st;
}

// ---- under a pose constraint (shortcut_constrained_measure.hpp) -------------------------------------------------

// The constraint's side of a launch: it travels with the call, the chain handle keeps nothing of it.
struct ConLaunch {
    ConstraintDev d;
    ProjectArgs p;
    double *verts;               // [n][Pc * V] the chunk's final vertices (shortcut)
    int32_t *projected;          // [2][P] or null
};

template <class CH>
__global__ __launch_bounds__(GATHER_BLOCK) void shortcut_cgather_kernel(const ShortcutLaunch a, const ConLaunch k) {
    __shared__ PathLds s;
    __shared__ CH sch;
    const long long pc = blockIdx.x, p = a.p0 + pc;
    const int tid = threadIdx.x, n = a.n;
    stage_table(sch, table_of<CH>(k.d));
    build_vertices<false>(a, p, s);
    const int nv = s.prep.nv;
    // rule 2': lane u projects vertex u, in its own column of the LDS block
    bool tried = false, ended = false;
    if (tid < nv && !shortcut::is_waypoint(s.off, shortcut::vertex_segment(s.prep.le, s.off, tid), tid)) {
        double x[constraint::MAXN];
        for (int i = 0; i < n; ++i) x[i] = s.v[i * MP + tid];
        const constraint::Projected pr = project(sch, k.d, k.p, n, x);
        tried = true;
        ended = pr.status == constraint::PROJECTED;
        for (int i = 0; i < n; ++i) s.v[i * MP + tid] = shortcut::vertex_after(pr.status, x[i]);
    }
    // (the barriers also publish the projected columns)
    const int n_tried = __syncthreads_count(tried), n_ended = __syncthreads_count(ended);
    if (tid == 0 && k.projected) {
        k.projected[p] = n_tried;
        k.projected[a.P + p] = n_ended;
    }
    const long long SV = a.Pc * a.V;
    for (int e = tid; e < a.V * n; e += GATHER_BLOCK) {
        const int i = e / a.V, u = e % a.V;
        k.verts[(long long)i * SV + pc * a.V + u] = u < nv ? s.v[i * MP + u] : __builtin_nan("");
    }
    write_pairs(a, pc, s);
}

template <class CH>
__global__ __launch_bounds__(SC_WAVE) void shortcut_cresample_kernel(const ResampleLaunch a, const ConLaunch k) {
    __shared__ CH sch;
    stage_table(sch, table_of<CH>(k.d));
    const long long p = blockIdx.x;
    const int j = threadIdx.x, n = a.n;
    bool tried = false, ended = false;
    int st = 0;
    if (j < a.Lout) {
        const int len = a.len ? a.len[p] : a.Lin;
        double x[constraint::MAXN], y[constraint::MAXN];
        st = shortcut::resample_waypoint(n, a.path + p * n, a.P * n, len, a.Lin, a.Lout, j, x, 1);
        if (shortcut::projects(st, a.Lout, j)) {
            for (int i = 0; i < n; ++i) y[i] = x[i];
            const constraint::Projected pr = project(sch, k.d, k.p, n, y);
            tried = true;
            ended = pr.status == constraint::PROJECTED;
            if (ended)
                for (int i = 0; i < n; ++i) x[i] = y[i];
        }
        double *out = a.out + ((long long)j * a.P + p) * n;
        for (int i = 0; i < n; ++i) out[i] = x[i];
    }
    // rule 7' and 8 over the wave (lane 0 holds the path's status: it does not depend on j)
    const int n_tried = __popcll(__ballot(tried)), n_ended = __popcll(__ballot(ended));
    if (j == 0) {
        if (a.status) a.status[p] = shortcut::resample_status(st, n_tried != n_ended);
        if (k.projected) {
            k.projected[p] = n_tried;
            k.projected[a.P + p] = n_ended;
        }
    }
}

// The refusals of the constraint entries, in ik_constraint.hip's order (B = 0 there): the constraint, tol and the
// chain with with_tol; then ptol, piters, damping and max_step.
int check_con(const optik_hip_chain *ch, const double *ref7, const double *lo6, const double *hi6, bool with_tol,
              double resolution, double tol, double ptol, int32_t piters, double damping, double max_step) {
    if (with_tol)
        if (int rc = optik_hip_constraint_motion_batch(ch, nullptr, ref7, lo6, hi6, nullptr, nullptr, 0, resolution, tol,
                                                       nullptr, nullptr, nullptr, nullptr, nullptr))
            return rc;
    return optik_hip_constraint_project_batch(ch, nullptr, ref7, lo6, hi6, nullptr, 0, ptol, piters, damping, max_step,
                                              nullptr, nullptr, nullptr, nullptr, nullptr);
}

bool points_ok(int v) { return v >= shortcut::MIN_POINTS && v <= shortcut::MAX_POINTS; }

// per path: the gathered segments, their free flags, and the motion check's own words; under a constraint the stored
// vertices too
size_t bytes_per_path(int n, int V, bool constrained) {
    return (size_t)shortcut::pair_count(V) * (sizeof(double) * 2 * (size_t)n + 1 + 24)
           + (constrained ? sizeof(double) * (size_t)n * V : 0);
}

long long chunk_paths(int n, int V, bool constrained) {
    const long long c = (long long)((size_t)OPTIK_HIP_PATH_SHORTCUT_CHUNK_BYTES / bytes_per_path(n, V, constrained));
    return c < 1 ? 1 : c;
}

// The host's side of a constrained call: the pointers the constraint entries take, and the device's record.
struct ConCall {
    const double *ref7, *lo6, *hi6;
    double tol;
    ConLaunch k;
};

// The chunk loop of both shortcut entries, their arguments checked and `a` filled but for the chunk and the workspace.
// cc null: no constraint.
int shortcut_chunks(optik_hip_chain *ch, const double *ee_offset7, ShortcutLaunch &a, double resolution, ConCall *cc,
                    hipStream_t stream) {
    const size_t n = (size_t)ch->n;
    const long long P = a.P, pairs = shortcut::pair_count(a.V), V = cc ? a.V : 0;  // (V: the stored vertices per path)
    const long long cap = chunk_paths(ch->n, a.V, cc != nullptr), chunk = P < cap ? P : cap;
    {
        std::lock_guard<std::mutex> lock(ch->mu);
        BIND_DEVICE(ch);
        // (every chunk is at most the first one's size: neither this block nor the motion check's grows in between;
        // the doubles first: the segments twice, then the vertices)
        HIP_TRY(ch->shortcut_ws.reserve((sizeof(double) * 2 * n + 1) * (size_t)(chunk * pairs)
                                        + sizeof(double) * n * (size_t)(chunk * V)));
        a.qa = reinterpret_cast<double *>(ch->shortcut_ws.get());
    }
    for (long long p0 = 0; p0 < P; p0 += chunk) {
        const long long Pc = P - p0 < chunk ? P - p0 : chunk, B = Pc * pairs;
        a.p0 = p0; a.Pc = Pc;
        a.qb = a.qa + n * (size_t)B;
        double *verts = a.qb + n * (size_t)B;
        uint8_t *d_free = reinterpret_cast<uint8_t *>(verts + n * (size_t)(Pc * V));
        a.free_flag = d_free;
        {
            BIND_DEVICE(ch);
            if (cc) {
                cc->k.verts = verts;
                CONSTRAINT_LAUNCH(shortcut_cgather_kernel, ch, (unsigned)Pc, GATHER_BLOCK, stream, a, cc->k);
            } else {
                hipLaunchKernelGGL(shortcut_gather_kernel, dim3((unsigned)Pc), dim3(GATHER_BLOCK), 0, stream, a);
                HIP_TRY(hipGetLastError());
            }
        }
        if (int rc = optik_hip_collision_motion_batch(ch, ee_offset7, a.qa, a.qb, B, resolution, nullptr, d_free,
                                                      nullptr, nullptr, stream))
            return rc;
        if (cc)
            if (int rc = constraint_mask_launch(ch, ee_offset7, cc->ref7, cc->lo6, cc->hi6, a.qa, a.qb, B, resolution,
                                                cc->tol, d_free, stream))
                return rc;
        BIND_DEVICE(ch);
        if (cc)
            hipLaunchKernelGGL(shortcut_route_stored_kernel, dim3((unsigned)Pc), dim3(SC_WAVE), 0, stream, a,
                               (const double *)verts);
        else hipLaunchKernelGGL(shortcut_route_kernel, dim3((unsigned)Pc), dim3(SC_WAVE), 0, stream, a);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

// What both shortcut entries put into the record before the chunk loop.
ShortcutLaunch make_launch(const optik_hip_chain *ch, const double *d_path, const int32_t *d_len, int32_t Lin, int64_t P,
                           int32_t V, double hop_penalty, int32_t Lout, double *d_out, int32_t *d_len_out,
                           double *d_cost, double *d_cost_in, int32_t *d_status) {
    ShortcutLaunch a;
    std::memset(&a, 0, sizeof a);
    a.path = d_path; a.len = d_len; a.P = P;
    a.n = ch->n; a.Lin = Lin; a.V = V; a.Lout = Lout;
    a.hop = hop_penalty;
    a.out = d_out; a.len_out = d_len_out; a.cost = d_cost; a.cost_in = d_cost_in; a.status = d_status;
    return a;
}

}  // namespace

extern "C" {

int64_t optik_hip_path_shortcut_chunk(const optik_hip_chain *ch, int32_t V) {
    if (!ch || !points_ok(V)) return fail(OPTIK_HIP_EINVAL, "bad argument");
    return chunk_paths(ch->n, V, false);
}

int optik_hip_path_shortcut(optik_hip_chain *ch, const double *ee_offset7, const double *d_path, const int32_t *d_len,
                            int32_t Lin, int64_t P, int32_t V, double resolution, double hop_penalty, int32_t Lout,
                            double *d_out, int32_t *d_len_out, double *d_cost, double *d_cost_in, int32_t *d_status,
                            void *stream) {
    if (!ch || P < 0) return fail(OPTIK_HIP_EINVAL, "bad argument");
    if (!points_ok(V) || !points_ok(Lin) || !points_ok(Lout))
        return fail(OPTIK_HIP_EINVAL, "path_shortcut: the vertices and the waypoints of a path are 2 .. 64");
    if (!(hop_penalty >= 0.0) || !std::isfinite(hop_penalty))
        return fail(OPTIK_HIP_EINVAL, "path_shortcut: hop_penalty must be finite and >= 0");
    if (P > MAX_PATHS) return fail(OPTIK_HIP_EINVAL, "path_shortcut: more than 2^30 paths in one launch");
    // (B = 0: the motion check's own refusals -- the resolution, prismatic joints)
    if (int rc = optik_hip_collision_motion_batch(ch, nullptr, nullptr, nullptr, 0, resolution, nullptr, nullptr,
                                                  nullptr, nullptr, nullptr))
        return rc;
    if (P == 0 || (!d_out && !d_len_out && !d_cost && !d_cost_in && !d_status)) return 0;
    if (!d_path) return fail(OPTIK_HIP_EINVAL, "bad argument");
    ShortcutLaunch a =
        make_launch(ch, d_path, d_len, Lin, P, V, hop_penalty, Lout, d_out, d_len_out, d_cost, d_cost_in, d_status);
    return shortcut_chunks(ch, ee_offset7, a, resolution, nullptr, (hipStream_t)stream);
}

int optik_hip_path_resample(const optik_hip_chain *ch, const double *d_path, const int32_t *d_len, int32_t Lin,
                            int64_t P, int32_t Lout, double *d_out, int32_t *d_status, void *stream) {
    if (!ch || P < 0) return fail(OPTIK_HIP_EINVAL, "bad argument");
    if (!points_ok(Lin) || !points_ok(Lout))
        return fail(OPTIK_HIP_EINVAL, "path_resample: a path has 2 .. 64 waypoints");
    if (P > MAX_PATHS) return fail(OPTIK_HIP_EINVAL, "path_resample: more than 2^30 paths in one launch");
    if (ch->prismatic) return fail(OPTIK_HIP_EUNSUPPORTED, prismatic_msg());
    if (P == 0 || (!d_out && !d_status)) return 0;
    if (!d_path || !d_out) return fail(OPTIK_HIP_EINVAL, "bad argument");
    BIND_DEVICE(ch);
    ResampleLaunch a{d_path, d_len, P, ch->n, Lin, Lout, d_out, d_status};
    const unsigned grid = (unsigned)((P * Lout + RESAMPLE_BLOCK - 1) / RESAMPLE_BLOCK);
    hipLaunchKernelGGL(shortcut_resample_kernel, dim3(grid), dim3(RESAMPLE_BLOCK), 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

// ---- under a pose constraint ------------------------------------------------------------------------------------

int64_t optik_hip_path_shortcut_constrained_chunk(const optik_hip_chain *ch, int32_t V) {
    if (!ch || !points_ok(V)) return fail(OPTIK_HIP_EINVAL, "bad argument");
    return chunk_paths(ch->n, V, true);
}

int optik_hip_path_shortcut_constrained(optik_hip_chain *ch, const double *ee_offset7, const double *d_path,
                                        const int32_t *d_len, int32_t Lin, int64_t P, int32_t V, double resolution,
                                        double hop_penalty, int32_t Lout, const double *ref7, const double *lo6,
                                        const double *hi6, double tol, double ptol, int32_t piters, double damping,
                                        double max_step, double *d_out, int32_t *d_len_out, double *d_cost,
                                        double *d_cost_in, int32_t *d_status, int32_t *d_projected, void *stream) {
    if (!ch || P < 0) return fail(OPTIK_HIP_EINVAL, "bad argument");
    if (P > MAX_PATHS) return fail(OPTIK_HIP_EINVAL, "path_shortcut: more than 2^30 paths in one launch");
    // (P = 0: optik_hip_path_shortcut's own refusals -- the sizes, the penalty, the resolution, prismatic joints)
    if (int rc = optik_hip_path_shortcut(ch, nullptr, nullptr, nullptr, Lin, 0, V, resolution, hop_penalty, Lout, nullptr,
                                         nullptr, nullptr, nullptr, nullptr, nullptr))
        return rc;
    if (int rc = check_con(ch, ref7, lo6, hi6, true, resolution, tol, ptol, piters, damping, max_step)) return rc;
    if (P == 0 || (!d_out && !d_len_out && !d_cost && !d_cost_in && !d_status && !d_projected)) return 0;
    if (!d_path) return fail(OPTIK_HIP_EINVAL, "bad argument");
    ShortcutLaunch a =
        make_launch(ch, d_path, d_len, Lin, P, V, hop_penalty, Lout, d_out, d_len_out, d_cost, d_cost_in, d_status);
    ConCall cc{ref7, lo6, hi6, tol, {}};
    fill_constraint(ch, ee_offset7, ref7, lo6, hi6, cc.k.d);
    cc.k.p = ProjectArgs{ptol, damping, max_step, piters};
    cc.k.projected = d_projected;
    return shortcut_chunks(ch, ee_offset7, a, resolution, &cc, (hipStream_t)stream);
}

int optik_hip_path_resample_constrained(const optik_hip_chain *ch, const double *ee_offset7, const double *d_path,
                                        const int32_t *d_len, int32_t Lin, int64_t P, int32_t Lout, const double *ref7,
                                        const double *lo6, const double *hi6, double ptol, int32_t piters,
                                        double damping, double max_step, double *d_out, int32_t *d_status,
                                        int32_t *d_projected, void *stream) {
    if (!ch || P < 0) return fail(OPTIK_HIP_EINVAL, "bad argument");
    if (P > MAX_PATHS) return fail(OPTIK_HIP_EINVAL, "path_resample: more than 2^30 paths in one launch");
    // (P = 0: optik_hip_path_resample's own refusals -- the sizes, prismatic joints)
    if (int rc = optik_hip_path_resample(ch, nullptr, nullptr, Lin, 0, Lout, nullptr, nullptr, nullptr)) return rc;
    if (int rc = check_con(ch, ref7, lo6, hi6, false, 0.0, 0.0, ptol, piters, damping, max_step)) return rc;
    if (P == 0 || (!d_out && !d_status && !d_projected)) return 0;
    if (!d_path || !d_out) return fail(OPTIK_HIP_EINVAL, "bad argument");
    BIND_DEVICE(ch);
    ResampleLaunch a{d_path, d_len, P, ch->n, Lin, Lout, d_out, d_status};
    ConLaunch k{};
    fill_constraint(ch, ee_offset7, ref7, lo6, hi6, k.d);
    k.p = ProjectArgs{ptol, damping, max_step, piters};
    k.projected = d_projected;
    CONSTRAINT_LAUNCH(shortcut_cresample_kernel, ch, (unsigned)P, SC_WAVE, (hipStream_t)stream, a, k);
    return 0;
}

}  // extern "C"
