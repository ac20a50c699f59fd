// ik_motion.hip -- the motion check on the device (motion_measure.hpp): is the straight
// joint-space segment qa -> qb free at resolution h, for many segments at once.  optik_hip_collision_motion_batch and
// the motion key pass of optik_hip_ik_path (include/optik_hip.h).
//
// A segment has K + 1 samples, K from 1 to 4096, so neither a lane nor a wave per segment keeps the chip busy.  The
// (segment, sample) items of a call are flattened instead:
//
//   motion_prep_kernel     one thread per segment: d, K (motion_measure.hpp steps 1, 2), the segment's reduction words
//                          at their neutral values, and the exclusive prefix of the sample counts inside its block
//   motion_scan_kernel     one block: the exclusive prefix of the blocks' totals, and the call's total
//   motion_flatten_kernel  G[s] = the flat index of segment s's sample 0; G[B] = the total
//   motion_kernel<N, TIP, CLASSIFY>, wide_motion_kernel<CLASSIFY>
//                          256 threads, one item per lane and chunk of 256 consecutive items; a block walks a
//                          contiguous run of chunks in ascending order.  The lane finds its segment in G (a window of
//                          it in LDS), interpolates the sample in registers (step 3) and runs the per-configuration
//                          body of collision_batch (collision_device.hpp).  Per segment the chunk reduces in LDS and
//                          then in global memory with integer minima only: the clearance as an order-preserving
//                          64-bit key, `first` as the sample index.  Integer minima commute, so no result depends on
//                          the order of arrival, the launch shape or the hand-out.
//   motion_finish_kernel   one thread per segment: the outputs, or (key form) the key +inf for a motion not free
//
// CLASSIFY (no clearance wanted; always in the key form): a sample whose k lies above a non-free k already recorded
// for its segment is skipped -- it cannot lower the minimum -- and the body stops a wave at the first term below the
// margin, as the collision key pass does.  Chunks of one segment are ascending in every block, so a blocked segment
// stops at the first chunk that holds a non-free sample, and that chunk still yields the exact lowest k.
#include "collision_device.hpp"
#include "motion_measure.hpp"

using namespace optik;
using namespace optik::host;
using namespace optik::hostparams;
using namespace optik::colldev;

namespace {

constexpr int MBLOCK = 256;        // threads per block = items per chunk = segments per prefix block
constexpr int WINDOW = 256;        // segments of a chunk held in LDS (a chunk of non-empty segments spans <= 129)
constexpr int NO_FIRST = 0x7fffffff;
constexpr int NOT_SAMPLED = -1, NOT_A_CANDIDATE = -2;
constexpr unsigned long long KEY_NEUTRAL = ~0ull, KEY_NAN = 0ull;

struct MotionLaunch {
    CollLaunch c;          // chain, ee_offset, model, world (c.q, c.B and the outputs of its forms are not used)
    // joint i of segment b: qa[i * qa_si + (b / qa_div) * qa_sb], qb[i * qb_si + b]
    const double *qa, *qb;
    long long qa_si, qa_sb, qa_div, qb_si;
    long long B;
    int n;
    double h;
    // the key form (null: the batch form): [B], a candidate is a key < +inf within max_step of its qa
    double *key;
    int filter;
    double max_step;
    // workspace
    unsigned long long *G;     // [B + 1]
    unsigned long long *bsum;  // [blocks + 1]
    unsigned long long *mkey;  // [B] min of the samples' clearance keys
    int *mfirst;               // [B] lowest non-free k
    int *msteps;               // [B] K, NOT_SAMPLED or NOT_A_CANDIDATE
    // outputs of the batch form, any may be null
    double *clearance;
    uint8_t *free_flag;
    int32_t *first, *steps;
};

// double -> unsigned key with the same order (-inf lowest, -0 below +0); a NaN below all of them
__device__ __forceinline__ unsigned long long clearance_key(double c) {
    if (c != c) return KEY_NAN;
    const unsigned long long u = (unsigned long long)__double_as_longlong(c);
    return (u >> 63) ? ~u : (u | (1ull << 63));
}
__device__ __forceinline__ double key_clearance(unsigned long long k) {
    if (k == KEY_NAN) return __builtin_nan("");
    return __longlong_as_double((long long)((k >> 63) ? (k & ~(1ull << 63)) : ~k));
}

// exclusive prefix of v over the block's 256 threads; *total = the block's sum
__device__ __forceinline__ unsigned long long block_exclusive(unsigned long long v, unsigned long long *s,
                                                              unsigned long long *total) {
    const int t = threadIdx.x;
    s[t] = v;
    __syncthreads();
    for (int o = 1; o < MBLOCK; o <<= 1) {
        const unsigned long long add = t >= o ? s[t - o] : 0ull;
        __syncthreads();
        s[t] += add;
        __syncthreads();
    }
    const unsigned long long incl = s[t];
    *total = s[MBLOCK - 1];
    __syncthreads();
    return incl - v;
}

__global__ __launch_bounds__(MBLOCK) void motion_prep_kernel(const MotionLaunch a) {
    __shared__ unsigned long long s[MBLOCK];
    const long long b = (long long)blockIdx.x * MBLOCK + threadIdx.x;
    unsigned long long count = 0;
    if (b < a.B) {
        int st = NOT_A_CANDIDATE;
        if (!a.key || a.key[b] < __builtin_huge_val()) {
            const double d = motion::motion_distance(a.n, a.qa + (b / a.qa_div) * a.qa_sb, a.qa_si, a.qb + b, a.qb_si);
            // (beyond max_step: the selection rejects the success anyway)
            if (!a.key || !a.filter || d <= a.max_step) st = motion::motion_steps(d, a.h);
        }
        a.msteps[b] = st;
        a.mkey[b] = KEY_NEUTRAL;
        a.mfirst[b] = NO_FIRST;
        if (st >= 1) count = (unsigned long long)st + 1ull;
    }
    unsigned long long total;
    const unsigned long long ex = block_exclusive(count, s, &total);
    if (b < a.B) a.G[b] = ex;
    if (threadIdx.x == 0) a.bsum[blockIdx.x] = total;
}

__global__ __launch_bounds__(MBLOCK) void motion_scan_kernel(unsigned long long *bsum, long long blocks) {
    __shared__ unsigned long long s[MBLOCK];
    unsigned long long carry = 0;
    for (long long t0 = 0; t0 < blocks; t0 += MBLOCK) {
        const long long i = t0 + threadIdx.x;
        const unsigned long long v = i < blocks ? bsum[i] : 0ull;
        unsigned long long total;
        const unsigned long long ex = block_exclusive(v, s, &total);
        if (i < blocks) bsum[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) bsum[blocks] = carry;
}

__global__ __launch_bounds__(MBLOCK) void motion_flatten_kernel(const MotionLaunch a, long long blocks) {
    const long long b = (long long)blockIdx.x * MBLOCK + threadIdx.x;
    if (b < a.B) a.G[b] += a.bsum[blockIdx.x];
    if (b == 0) a.G[a.B] = a.bsum[blocks];
}

// the last segment s of [lo, hi] with G[s] <= i (G[lo] <= i holds)
__device__ __forceinline__ long long segment_of(const unsigned long long *G, unsigned long long i, long long lo,
                                                long long hi) {
    while (lo < hi) {
        const long long mid = lo + (hi - lo + 1) / 2;
        if (G[mid] <= i) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// Whether this block owns a chunk at all (block-uniform; the same split as motion_chunks).
__device__ __forceinline__ bool block_has_chunks(const MotionLaunch &a) {
    const unsigned long long chunks = (a.G[a.B] + MBLOCK - 1) / MBLOCK;
    const unsigned long long per_block = (chunks + gridDim.x - 1) / gridDim.x;
    return (unsigned long long)blockIdx.x * per_block < chunks;
}

// What the chunks of a block share; Eval(seg, k, K, free_) gives the sample's clearance (CLASSIFY: the flag only).
template <bool CLASSIFY, class Eval>
__device__ __forceinline__ void motion_chunks(const MotionLaunch &a, Eval &&eval) {
    __shared__ unsigned long long s_G[WINDOW + 1];
    __shared__ unsigned long long s_key[WINDOW];
    __shared__ int s_first[WINDOW];
    __shared__ long long s_rng[2];
    const unsigned long long total = a.G[a.B];
    const unsigned long long chunks = (total + MBLOCK - 1) / MBLOCK;
    const unsigned long long per_block = (chunks + gridDim.x - 1) / gridDim.x;
    const unsigned long long c0 = (unsigned long long)blockIdx.x * per_block;
    const unsigned long long c1 = c0 + per_block < chunks ? c0 + per_block : chunks;
    const int tid = threadIdx.x;
    for (unsigned long long ch = c0; ch < c1; ++ch) {
        const unsigned long long i0 = ch * MBLOCK;
        __syncthreads();  // (the slots of the chunk before are flushed)
        if (tid < 2) {
            unsigned long long i = i0 + (tid ? MBLOCK - 1 : 0);
            if (i > total - 1) i = total - 1;
            s_rng[tid] = segment_of(a.G, i, 0, a.B - 1);
        }
        __syncthreads();
        const long long s0 = s_rng[0], s1 = s_rng[1];
        const bool window = s1 - s0 < WINDOW;  // (always, unless segments without samples lie in between)
        if (window) {
            for (long long t = tid; t <= s1 - s0; t += MBLOCK) {
                s_G[t] = a.G[s0 + t];
                s_key[t] = KEY_NEUTRAL;
                s_first[t] = NO_FIRST;
            }
        }
        __syncthreads();
        const unsigned long long i = i0 + tid;
        if (i < total) {
            long long seg;
            unsigned long long g;
            if (window) {
                const long long t = segment_of(s_G, i, 0, s1 - s0);
                seg = s0 + t;
                g = s_G[t];
            } else {
                seg = segment_of(a.G, i, s0, s1);
                g = a.G[seg];
            }
            const int k = (int)(i - g);
            const int K = a.msteps[seg];
            // (a sample above a non-free one that is already known cannot lower the segment's first)
            const bool skip = CLASSIFY && k > __atomic_load_n(&a.mfirst[seg], __ATOMIC_RELAXED);
            if (!skip) {
                bool free_ = true;
                const double c = eval(seg, k, K, free_);
                if (window) {
                    if (!free_) atomicMin(&s_first[seg - s0], k);
                    if (!CLASSIFY) atomicMin(&s_key[seg - s0], clearance_key(c));
                } else {
                    if (!free_) atomicMin(&a.mfirst[seg], k);
                    if (!CLASSIFY) atomicMin(&a.mkey[seg], clearance_key(c));
                }
            }
        }
        __syncthreads();
        if (window) {
            for (long long t = tid; t <= s1 - s0; t += MBLOCK) {
                if (s_first[t] != NO_FIRST) atomicMin(&a.mfirst[s0 + t], s_first[t]);
                if (!CLASSIFY && s_key[t] != KEY_NEUTRAL) atomicMin(&a.mkey[s0 + t], s_key[t]);
            }
        }
    }
}

template <int N, bool TIP, bool CLASSIFY>
__global__ __launch_bounds__(MBLOCK) void motion_kernel(const MotionLaunch a) {
    __shared__ ChainDev sch;
    __shared__ ModelDev sm;
    if (!block_has_chunks(a)) return;  // (before anything is staged: the grid is sized from a bound on the items)
    stage_chain(sch, a.c.chain);
    if (a.c.model) stage_model(sm, a.c);
    motion_chunks<CLASSIFY>(a, [&](long long seg, int k, int K, bool &free_) {
        const double *pa = a.qa + (seg / a.qa_div) * a.qa_sb, *pb = a.qb + seg;
        double q[N];
#pragma unroll
        for (int i = 0; i < N; ++i) q[i] = motion::motion_sample(pa[i * a.qa_si], pb[i * a.qb_si], k, K);
        return config_clearance<N, TIP, CLASSIFY ? FORM_KEY : FORM_BATCH>(sch, sm, a.c, q, free_);
    });
}

template <bool CLASSIFY>
__global__ __launch_bounds__(MBLOCK) void wide_motion_kernel(const MotionLaunch a) {
    __shared__ WideChainDev sch;
    __shared__ ModelDev sm;
    if (!block_has_chunks(a)) return;
    stage_wide_chain(sch, a.c.wchain);
    if (a.c.model) stage_model(sm, a.c);
    const int n = sch.n_pos;
    motion_chunks<CLASSIFY>(a, [&](long long seg, int k, int K, bool &free_) {
        const double *pa = a.qa + (seg / a.qa_div) * a.qa_sb, *pb = a.qb + seg;
        double q[WIDE_MAX_DOF];
        for (int i = 0; i < n; ++i) q[i] = motion::motion_sample(pa[i * a.qa_si], pb[i * a.qb_si], k, K);
        return wide_config_clearance<CLASSIFY ? FORM_KEY : FORM_BATCH>(sch, sm, a.c, n, q, free_);
    });
}

__global__ __launch_bounds__(MBLOCK) void motion_finish_kernel(const MotionLaunch a) {
    const long long b = (long long)blockIdx.x * MBLOCK + threadIdx.x;
    if (b >= a.B) return;
    const int st = a.msteps[b];
    const int mf = a.mfirst[b];
    if (a.key) {
        if (st != NOT_A_CANDIDATE && (st == NOT_SAMPLED || mf != NO_FIRST)) a.key[b] = __builtin_huge_val();
        return;
    }
    motion::Result r = motion::not_sampled();
    if (st >= 1) {
        r.steps = st;
        r.first = mf == NO_FIRST ? -1 : mf;
        r.free_flag = mf == NO_FIRST ? 1 : 0;
        if (a.clearance) r.clearance = key_clearance(a.mkey[b]);
    }
    if (a.clearance) a.clearance[b] = r.clearance;
    if (a.free_flag) a.free_flag[b] = (uint8_t)r.free_flag;
    if (a.first) a.first[b] = r.first;
    if (a.steps) a.steps[b] = r.steps;
}

size_t ws_bytes(long long B) {
    const size_t blocks = ((size_t)B + MBLOCK - 1) / MBLOCK;
    return sizeof(unsigned long long) * ((size_t)B + 1 + blocks + 1 + (size_t)B) + sizeof(int) * 2 * (size_t)B;
}

// The five launches of one call.  `items_bound`: no call has more (segment, sample) items; it sizes the grid, since the
// true total is only known on the device.
int motion_launch(const optik_hip_chain *ch, MotionLaunch &a, bool classify, unsigned long long items_bound,
                  hipStream_t stream) {
    const long long B = a.B;
    const long long blocks = (B + MBLOCK - 1) / MBLOCK;
    unsigned long long *w = reinterpret_cast<unsigned long long *>(ch->motion_ws.get());
    a.G = w; w += B + 1;
    a.bsum = w; w += blocks + 1;
    a.mkey = w; w += B;
    a.mfirst = reinterpret_cast<int *>(w);
    a.msteps = a.mfirst + B;
    hipLaunchKernelGGL(motion_prep_kernel, dim3((unsigned)blocks), dim3(MBLOCK), 0, stream, a);
    hipLaunchKernelGGL(motion_scan_kernel, dim3(1), dim3(MBLOCK), 0, stream, a.bsum, blocks);
    hipLaunchKernelGGL(motion_flatten_kernel, dim3((unsigned)blocks), dim3(MBLOCK), 0, stream, a, blocks);
    const int grid = grid_for(ch, (long long)items_bound, MBLOCK, 8);  // (items_bound < 2^43: motion_reserve)
    if (ch->wide) {
        if (classify) hipLaunchKernelGGL(wide_motion_kernel<true>, dim3(grid), dim3(MBLOCK), 0, stream, a);
        else hipLaunchKernelGGL(wide_motion_kernel<false>, dim3(grid), dim3(MBLOCK), 0, stream, a);
    } else if (classify) {
#define CALL(NN, TT) hipLaunchKernelGGL((motion_kernel<NN, TT, true>), dim3(grid), dim3(MBLOCK), 0, stream, a)
        OPTIK_DISPATCH(ch, CALL);
#undef CALL
    } else {
#define CALL(NN, TT) hipLaunchKernelGGL((motion_kernel<NN, TT, false>), dim3(grid), dim3(MBLOCK), 0, stream, a)
        OPTIK_DISPATCH(ch, CALL);
#undef CALL
    }
    hipLaunchKernelGGL(motion_finish_kernel, dim3((unsigned)blocks), dim3(MBLOCK), 0, stream, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

bool resolution_ok(double h) { return h > 0.0 && std::isfinite(h); }

}  // namespace

namespace optik {
namespace host {

int motion_reserve(optik_hip_chain *ch, long long segments) {
    if (segments > (1ll << 30)) return fail(OPTIK_HIP_EINVAL, "motion check: more than 2^30 segments in one launch");
    HIP_TRY(ch->motion_ws.reserve(ws_bytes(segments)));
    return 0;
}

int motion_key_launch(const optik_hip_chain *ch, const double *ee_offset7, const double *seed, const double *x,
                      double *key, int P, size_t R, int filter, double max_step, hipStream_t stream) {
    if (ch->prismatic) return fail(OPTIK_HIP_EUNSUPPORTED, prismatic_msg());
    const long long B = (long long)P * (long long)R;
    if (ws_bytes(B) > ch->motion_ws.capacity()) return fail(OPTIK_HIP_EINVAL, "motion check: workspace not reserved");
    MotionLaunch a;
    std::memset(&a, 0, sizeof a);
    fill_launch(ch, ee_offset7, nullptr, B, a.c);
    a.qa = seed; a.qa_si = 1; a.qa_sb = ch->n; a.qa_div = (long long)R;
    a.qb = x; a.qb_si = B;
    a.B = B;
    a.n = ch->n;
    a.h = ch->motion_h;
    a.key = key;
    a.filter = filter;
    a.max_step = max_step;
    // (within max_step a candidate has at most ceil(max_step / h) steps)
    double per = (double)(motion::MAX_STEPS + 1);
    if (filter && std::ceil(max_step / a.h) + 1.0 < per) per = std::fmax(2.0, std::ceil(max_step / a.h) + 1.0);
    return motion_launch(ch, a, true, (unsigned long long)B * (unsigned long long)per, stream);
}

}  // namespace host
}  // namespace optik

extern "C" {

int optik_hip_chain_set_motion_resolution(optik_hip_chain *ch, double h) {
    if (!ch) return fail(OPTIK_HIP_EINVAL, "bad argument");
    if (!(h >= 0.0) || !std::isfinite(h))
        return fail(OPTIK_HIP_EINVAL, "motion resolution must be finite and >= 0 (0: no motion check)");
    std::lock_guard<std::mutex> lock(ch->mu);
    BIND_DEVICE(ch);
    // (as set_world: nothing queued on the chain's device runs across the change)
    HIP_TRY(hipDeviceSynchronize());
    ch->claim_pending = false;
    ch->motion_h = h;
    return 0;
}

int optik_hip_collision_motion_batch(optik_hip_chain *ch, const double *ee_offset7, const double *d_qa,
                                     const double *d_qb, int64_t B, double resolution, double *d_clearance,
                                     uint8_t *d_free, int32_t *d_first, int32_t *d_steps, void *stream) {
    if (!ch || B < 0) return fail(OPTIK_HIP_EINVAL, "bad argument");
    if (!resolution_ok(resolution))
        return fail(OPTIK_HIP_EINVAL, "motion resolution must be finite and > 0");
    if (ch->prismatic) return fail(OPTIK_HIP_EUNSUPPORTED, prismatic_msg());
    if (B == 0 || (!d_clearance && !d_free && !d_first && !d_steps)) return 0;
    if (!d_qa || !d_qb) return fail(OPTIK_HIP_EINVAL, "bad argument");
    std::lock_guard<std::mutex> lock(ch->mu);
    BIND_DEVICE(ch);
    if (int rc = motion_reserve(ch, B)) return rc;
    MotionLaunch a;
    std::memset(&a, 0, sizeof a);
    fill_launch(ch, ee_offset7, nullptr, B, a.c);
    a.qa = d_qa; a.qa_si = B; a.qa_sb = 1; a.qa_div = 1;
    a.qb = d_qb; a.qb_si = B;
    a.B = B;
    a.n = ch->n;
    a.h = resolution;
    a.clearance = d_clearance; a.free_flag = d_free; a.first = d_first; a.steps = d_steps;
    return motion_launch(ch, a, d_clearance == nullptr,
                         (unsigned long long)B * (unsigned long long)(motion::MAX_STEPS + 1), (hipStream_t)stream);
}

}  // extern "C"
