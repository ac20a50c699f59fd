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
// The paths of a call are processed in chunks of at most OPTIK_HIP_PATH_SHORTCUT_CHUNK_BYTES of workspace, launched
// one after the other on the stream; a path's blocks see only that path, so nothing depends on P or on the chunking.
#include "collision_device.hpp"
#include "shortcut_measure.hpp"

using namespace optik;
using namespace optik::host;
using namespace optik::colldev;

static_assert(shortcut::MAX_POINTS == OPTIK_HIP_PATH_OPTIMIZE_MAX_WAYPOINTS && shortcut::MAX_POINTS == 64,
              "a shortcut path is a path path_optimize takes; one lane of a wave per vertex");
static_assert(shortcut::MAX_JOINTS == WIDE_MAX_DOF, "shortcut_measure.hpp states the cap on the joint positions");

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

// Steps 1 and 2 of the header by the first wave of the block; every thread of the block calls it.
__device__ __forceinline__ void build_vertices(const ShortcutLaunch &a, long long p, PathLds &s) {
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
        const int seg = shortcut::vertex_segment(le, s.off, tid);
        for (int i = 0; i < a.n; ++i) s.v[i * MP + tid] = shortcut::vertex_joint(path, st, s.m, s.off, seg, tid, i);
    }
    __syncthreads();
}

__global__ __launch_bounds__(GATHER_BLOCK) void shortcut_gather_kernel(const ShortcutLaunch a) {
    __shared__ PathLds s;
    const long long pc = blockIdx.x;
    build_vertices(a, a.p0 + pc, s);
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

__global__ __launch_bounds__(SC_WAVE) void shortcut_route_kernel(const ShortcutLaunch a) {
    __shared__ PathLds s;
    __shared__ int s_succ[MP], s_route[MP];
    __shared__ shortcut::Result s_res;
    const long long pc = blockIdx.x, p = a.p0 + pc;
    const int lane = threadIdx.x;
    build_vertices(a, p, s);
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

bool points_ok(int v) { return v >= shortcut::MIN_POINTS && v <= shortcut::MAX_POINTS; }

// per path: the gathered segments, their free flags, and the motion check's own words
size_t bytes_per_path(int n, int V) {
    return (size_t)shortcut::pair_count(V) * (sizeof(double) * 2 * (size_t)n + 1 + 24);
}

long long chunk_paths(int n, int V) {
    const long long c = (long long)((size_t)OPTIK_HIP_PATH_SHORTCUT_CHUNK_BYTES / bytes_per_path(n, V));
    return c < 1 ? 1 : c;
}

}  // namespace

extern "C" {

int64_t optik_hip_path_shortcut_chunk(const optik_hip_chain *ch, int32_t V) {
    if (!ch || !points_ok(V)) return fail(OPTIK_HIP_EINVAL, "bad argument");
    return chunk_paths(ch->n, V);
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
    const size_t n = (size_t)ch->n;
    const long long pairs = shortcut::pair_count(V);
    const long long chunk = P < chunk_paths(ch->n, V) ? P : chunk_paths(ch->n, V);
    ShortcutLaunch a;
    std::memset(&a, 0, sizeof a);
    {
        std::lock_guard<std::mutex> lock(ch->mu);
        BIND_DEVICE(ch);
        // (every chunk is at most the first one's size: neither this block nor the motion check's grows in between)
        HIP_TRY(ch->shortcut_ws.reserve((sizeof(double) * 2 * n + 1) * (size_t)(chunk * pairs)));
        a.qa = reinterpret_cast<double *>(ch->shortcut_ws.get());
    }
    a.path = d_path; a.len = d_len; a.P = P;
    a.n = ch->n; a.Lin = Lin; a.V = V; a.Lout = Lout;
    a.hop = hop_penalty;
    a.out = d_out; a.len_out = d_len_out; a.cost = d_cost; a.cost_in = d_cost_in; a.status = d_status;
    for (long long p0 = 0; p0 < P; p0 += chunk) {
        const long long Pc = P - p0 < chunk ? P - p0 : chunk, B = Pc * pairs;
        a.p0 = p0; a.Pc = Pc;
        a.qb = a.qa + n * (size_t)B;
        uint8_t *d_free = reinterpret_cast<uint8_t *>(a.qb + n * (size_t)B);
        a.free_flag = d_free;
        {
            BIND_DEVICE(ch);
            hipLaunchKernelGGL(shortcut_gather_kernel, dim3((unsigned)Pc), dim3(GATHER_BLOCK), 0, (hipStream_t)stream, a);
            HIP_TRY(hipGetLastError());
        }
        if (int rc = optik_hip_collision_motion_batch(ch, ee_offset7, a.qa, a.qb, B, resolution, nullptr, d_free,
                                                      nullptr, nullptr, stream))
            return rc;
        BIND_DEVICE(ch);
        hipLaunchKernelGGL(shortcut_route_kernel, dim3((unsigned)Pc), dim3(SC_WAVE), 0, (hipStream_t)stream, a);
        HIP_TRY(hipGetLastError());
    }
    return 0;
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

}  // extern "C"
