// intersect.hip -- sfm_intersect_tracks (gfx950): every track of a fused table intersected over all its views under a given camera
// table.  Arithmetic: intersect_math.hpp (shared with the host build of the CPU tests) over fuse_math.hpp's point LM.
//
// Two launches on the context's stream behind two small memsets, no host synchronisation, no float atomics:
//   intersect_lane_kernel   one lane per track, the list walked with counted loops as fuse_points_kernel walks it: the tracks that
//                           are copied through and the tracks of fewer than wave_min_views views.  A longer track is only
//                           appended to a list in the context's work buffer, one integer atomic per wavefront that has any (the
//                           order of the list does not reach the outputs).
//   intersect_wave_kernel   a fixed grid of one-wavefront blocks that strides over the list's device-side count, one wavefront per
//                           long track.  Lane l forms the per-view terms of views l, l + 64, ... with the header's functions and
//                           puts them into LDS; the lanes that own one accumulator each add them IN LIST ORDER, 64 dependent adds
//                           per chunk instead of 64 whole views.  Without contraction the ordered sum of the per-view terms is the
//                           serial walk's bytes, so the split between the kernels is a pure performance choice.  LmControl runs
//                           in every lane on the same broadcast sums: the control flow is wavefront-uniform, and the sums are
//                           moved to scalar registers to say so.
// The term buffer is [accumulator][lane] with a stride of 65 words: lane l's store of accumulator q goes to bank (q + l) % 32 and
// owner q's read of term i to bank (q + i) % 32, both free of conflicts (a stride of 64 would put all owners on one bank, a
// [lane][accumulator] layout at stride 10 the stores on five).
// The eight counts are integer atomics on the caller's d_counts, one per wavefront and count that is not zero.
#include "common.hpp"
#include "device_math.hpp"
#include "intersect_math.hpp"

namespace sfm {

constexpr int kIntersectBlock = 256;      // tracks per block of the lane kernel
constexpr int kIntersectWaveGrid = 1024;  // the wavefront kernel's blocks at the most: four per compute unit
constexpr int kIntersectStride = 65;      // words between two accumulators' terms in LDS
constexpr int kIntersectTerms = 10;       // the most accumulators of one sum: fuse_lm's V (6), g (3) and cost

struct IntersectArgs {
    const FusePair *pairs;
    int k, N, wave_min;
    sfm_intersect_params p;
    sfm_intersect_in in;
    sfm_intersect_out out;
    // the context's work buffer
    int *list;                            // N: the long tracks, in no order
    int *list_count;
};

// view o of a track whose observations start at `cam` / `rec`, under the caller's cameras
struct IntersectViews {
    const IntersectArgs &a;
    const int32_t *cam, *rec;
    __device__ __forceinline__ FuseView operator()(int o) const
    {
        const int c = cam[o];
        return fuse_view(a.pairs[c >> 1], a.in.d_cams, c >> 1, c & 1, rec[o]);
    }
};

// the number of tracks: d_counts[0], never more than the nodes the buffers were sized for
__device__ __forceinline__ int intersect_tracks(const IntersectArgs &a) { return min(a.in.d_counts[0], a.N); }

__device__ __forceinline__ void intersect_store(const IntersectArgs &a, int t, const IntersectResult &r)
{
#pragma unroll
    for (int c = 0; c < 4; ++c) a.out.d_points[(size_t)c * a.N + t] = r.out[c];
    a.out.d_flags[t] = r.flag;
    if (a.out.d_err) a.out.d_err[t] = r.err;
}

// entries 1 .. 7 of d_counts that a finished track adds to, as bits
__device__ __forceinline__ unsigned intersect_count_bits(const IntersectResult &r)
{
    if (r.copied) return 1u << 4;
    if (r.start == kIntersectNone) return (1u << 1) | (1u << 6);
    const bool refined = r.flag == SFM_FUSE_REFINED || r.flag == SFM_FUSE_SEAM_REFINED;
    return (1u << 1) | (refined ? 1u << 2 : 1u << 3) | (r.start == kIntersectL ? 1u << 5 : 0u) | (r.promoted ? 1u << 7 : 0u);
}

__global__ __launch_bounds__(kIntersectBlock)
void intersect_lane_kernel(IntersectArgs a)
{
    const int t = blockIdx.x * kIntersectBlock + threadIdx.x, lane = threadIdx.x & 63;
    const int T = intersect_tracks(a);
    bool deferred = false;
    unsigned bits = 0;
    if (t < T) {
        const int o0 = a.in.d_track_offset[t], count = a.in.d_track_offset[t + 1] - o0;
        const int flag = a.in.d_flags[t];
        const bool skip = a.in.d_skip && a.in.d_skip[t] != 0;
        deferred = count >= a.wave_min && !intersect_copied(flag, count, skip);
        if (!deferred) {
            const IntersectViews view = { a, a.in.d_obs_cam + o0, a.in.d_obs_record + o0 };
            float Xin[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) Xin[c] = a.in.d_points[(size_t)c * a.N + t];
            IntersectResult r;
            intersect_track(flag, count, skip, Xin, view, a.p, r);
            intersect_store(a, t, r);
            bits = intersect_count_bits(r);
        }
    }
    // the long tracks go to the list: one atomic per wavefront that has any
    const unsigned long long longs = __ballot(deferred);
    if (longs) {
        int base = 0;
        if (lane == 0) base = atomicAdd(a.list_count, __popcll(longs));
        base = __shfl(base, 0);
        if (deferred) a.list[base + __popcll(longs & ((1ull << lane) - 1ull))] = t;
    }
#pragma unroll
    for (int q = 1; q < kIntersectCounts; ++q) {
        const unsigned long long m = __ballot((bits >> q) & 1u);
        if (lane == 0 && m) atomicAdd(&a.out.d_counts[q], __popcll(m));
    }
    if (t == 0) a.out.d_counts[0] = T;
}

// a value that every lane of the wavefront holds, moved to scalar registers
__device__ __forceinline__ float wave_uniform(float v) { return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v))); }
__device__ __forceinline__ int wave_uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ double wave_uniform(double v)
{
    const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)u), hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(u >> 32));
    return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}

// NQ reductions over a track's views in list order by one wavefront (the block).  term(o, v): view o's NQ terms; first(q): the
// start of accumulator q; fold(q, acc, x): what the serial walk does with a term.  Lane l forms the terms of view base + l into
// s[q * kIntersectStride + l]; lane q < NQ folds them in order; every lane returns all NQ results.
template <int NQ, class T, class Term, class First, class Fold>
__device__ __forceinline__ void wave_ordered(int count, int lane, T *s, T *tot, Term &&term, First &&first, Fold &&fold, T out[NQ])
{
    static_assert(NQ <= kIntersectTerms, "more accumulators than the term buffer has rows");
    T acc = first(lane < NQ ? lane : 0);
    for (int base = 0; base < count; base += 64) {
        const int m = min(64, count - base);
        if (lane < m) {
            T v[NQ];
            term(base + lane, v);
#pragma unroll
            for (int q = 0; q < NQ; ++q) s[q * kIntersectStride + lane] = v[q];
        }
        __syncthreads();
        if (lane < NQ)
            for (int i = 0; i < m; ++i) acc = fold(lane, acc, s[lane * kIntersectStride + i]);
        __syncthreads();
    }
    if (lane < NQ) tot[lane] = acc;
    __syncthreads();
#pragma unroll
    for (int q = 0; q < NQ; ++q) out[q] = wave_uniform(tot[q]);
    __syncthreads();
}

__global__ __launch_bounds__(64)
void intersect_wave_kernel(IntersectArgs a)
{
    // the term buffer serves the fp64 terms of the normal equations (9 rows) and the fp32 terms of every other sum (10 rows at the most)
    __shared__ double s_terms[9 * kIntersectStride + kIntersectTerms];
    double *sd = s_terms, *sd_tot = s_terms + 9 * kIntersectStride;
    float *sf = reinterpret_cast<float *>(s_terms), *sf_tot = sf + kIntersectTerms * kIntersectStride;
    static_assert(sizeof(float) * (kIntersectTerms * kIntersectStride + kIntersectTerms) <= sizeof(s_terms), "the fp32 rows fit the fp64 buffer");
    const int lane = threadIdx.x;
    const int T = intersect_tracks(a);
    const int n_long = min(*a.list_count, T);
    const float huber = a.p.huber_px;
    const auto zero = [](int) { return 0.0f; };
    const auto add = [](int, float acc, float x) { return acc + x; };
    for (int i = blockIdx.x; i < n_long; i += gridDim.x) {
        const int t = wave_uniform(a.list[i]);
        const int o0 = wave_uniform(a.in.d_track_offset[t]), count = wave_uniform(a.in.d_track_offset[t + 1]) - o0;
        const int flag = wave_uniform((int)a.in.d_flags[t]);
        const IntersectViews view = { a, a.in.d_obs_cam + o0, a.in.d_obs_record + o0 };
        float Xin[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) Xin[c] = wave_uniform(a.in.d_points[(size_t)c * a.N + t]);
        // ---- candidate L: the normal equations in list order ----
        double Ab[9];
        wave_ordered<9>(count, lane, sd, sd_tot, [&](int o, double v[9]) { intersect_rows(view(o), v, v + 6); },
                        [](int) { return 0.0; }, [](int, double acc, double x) { return acc + x; }, Ab);
        float C[3], L[3];
        bool c_ok = intersect_dehom(Xin, C);
        intersect_solve(Ab, Ab + 6, L);
        bool l_ok = intersect_finite(L);
        // ---- both candidates' front tests and costs in one pass: the serial walk reads a cost only where the candidate is eligible ----
        float fc[4];
        wave_ordered<4>(count, lane, sf, sf_tot, [&](int o, float v[4]) {
                            const FuseView w = view(o);
                            v[0] = intersect_depth(w, C) > 0.0f ? 1.0f : 0.0f; v[1] = intersect_depth(w, L) > 0.0f ? 1.0f : 0.0f;
                            v[2] = intersect_cost_term(w, huber, C); v[3] = intersect_cost_term(w, huber, L);
                        },
                        [](int q) { return q < 2 ? 1.0f : 0.0f; }, [](int q, float acc, float x) { return q < 2 ? fminf(acc, x) : acc + x; }, fc);
        c_ok = c_ok && fc[0] != 0.0f;
        l_ok = l_ok && fc[1] != 0.0f;
        const int start = intersect_choose(c_ok, fc[2], l_ok, fc[3]);
        IntersectResult r;
        if (start == kIntersectNone) {
            intersect_no_start(flag, Xin, r);
        } else {
            const float S[3] = { start == kIntersectL ? L[0] : C[0], start == kIntersectL ? L[1] : C[1], start == kIntersectL ? L[2] : C[2] };
            float X[3] = { S[0], S[1], S[2] };
            const auto cost_at = [&](const float *Y) {
                float c[1];
                wave_ordered<1>(count, lane, sf, sf_tot, [&](int o, float v[1]) { v[0] = intersect_cost_term(view(o), huber, Y); }, zero, add, c);
                return c[0];
            };
            // ---- fuse_lm, its sums by the wavefront ----
            const float cost0 = cost_at(X);
            LmControl lm((double)a.p.initial_lambda, (double)cost0, (double)cost0, false);
            while (lm.running(a.p.max_iterations)) {
                float s[10], Vi[6];
                wave_ordered<10>(count, lane, sf, sf_tot, [&](int o, float v[10]) { intersect_lm_terms(view(o), huber, X, v); }, zero, add, s);
                const float *V = s, *g = s + 6;
                refine_damped_inverse3(V, (float)lm.lambda, Vi);
                float Xt[3];
#pragma unroll
                for (int p = 0; p < 3; ++p) Xt[p] = X[p] - (Vi[sym3(p, 0)] * g[0] + Vi[sym3(p, 1)] * g[1] + Vi[sym3(p, 2)] * g[2]);
                if (!(isfinite(Xt[0]) && isfinite(Xt[1]) && isfinite(Xt[2]))) {      // a singular system: more damping
                    if (!lm.solve_failed()) break;
                    continue;
                }
                const float nc = cost_at(Xt);
                bool stop;
                if (lm.tentative((double)nc, (double)nc, (double)a.p.min_rel_decrease, stop)) { X[0] = Xt[0]; X[1] = Xt[1]; X[2] = Xt[2]; }
                if (stop) break;
            }
            // ---- fuse_accept: the largest squared error, every view an inlier ----
            float acc[2];
            wave_ordered<2>(count, lane, sf, sf_tot, [&](int o, float v[2]) {
                                bool ok;
                                v[0] = intersect_accept_term(view(o), a.p.threshold_px, X, ok);
                                v[1] = ok ? 1.0f : 0.0f;
                            },
                            [](int q) { return q ? 1.0f : 0.0f; }, [](int q, float m, float x) { return q ? fminf(m, x) : fmaxf(m, x); }, acc);
            intersect_finish(flag, start, S, X, acc[1] != 0.0f, sqrtf(acc[0]), r);
        }
        if (lane == 0) {
            intersect_store(a, t, r);
            const unsigned bits = intersect_count_bits(r);
#pragma unroll
            for (int q = 1; q < kIntersectCounts; ++q)
                if ((bits >> q) & 1u) atomicAdd(&a.out.d_counts[q], 1);
        }
    }
}

int launch_intersect_tracks(sfm_ctx *ctx, const FusePair *h_pairs, int num_pairs, const sfm_intersect_in &in, const sfm_intersect_params &p,
                            const sfm_intersect_out &out)
{
    hipStream_t st = ctx->stream;
    JobArray &ja = ctx->chain_jobs;
    int rc = job_array_reserve(ja, (size_t)num_pairs, sizeof(FusePair), st);
    if (rc != SFM_OK) return rc;
    FusePair *jobs = static_cast<FusePair *>(ja.pinned);
    int N = 0;
    for (int i = 0; i < num_pairs; ++i) {
        jobs[i] = h_pairs[i];
        jobs[i].offset = N;
        N += h_pairs[i].n;
    }
    IntersectArgs a;
    a.pairs = static_cast<const FusePair *>(ja.dev);
    a.k = num_pairs; a.N = N;
    a.wave_min = p.wave_min_views ? p.wave_min_views : kIntersectWaveMinViews;
    a.p = p; a.in = in; a.out = out;
    const auto layout = [&](void *buffer) {
        Carver w(buffer);
        a.list = w.take<int>((size_t)N, 4);
        a.list_count = w.take<int>(1, 4);
        return w.used;
    };
    rc = grow(&ctx->chain_ws, &ctx->chain_ws_bytes, layout(nullptr), st);
    if (rc != SFM_OK) return rc;
    layout(ctx->chain_ws);
    rc = job_array_upload(ja, (size_t)num_pairs, sizeof(FusePair), st);
    if (rc != SFM_OK) return rc;
    SFM_HIP_TRY(hipMemsetAsync(out.d_counts, 0, kIntersectCounts * sizeof(int32_t), st));
    SFM_HIP_TRY(hipMemsetAsync(a.list_count, 0, sizeof(int), st));
    if (N == 0) return SFM_OK;                            // no records anywhere: no tracks
    hipLaunchKernelGGL(intersect_lane_kernel, dim3((N + kIntersectBlock - 1) / kIntersectBlock), dim3(kIntersectBlock), 0, st, a);      // T <= N stays on the device
    SFM_HIP_TRY(hipGetLastError());
    // a long track has at least wave_min views and the table 2N observations at the most
    const int most = (int)((2ll * N + a.wave_min - 1) / a.wave_min);
    hipLaunchKernelGGL(intersect_wave_kernel, dim3(most < 1 ? 1 : (most > kIntersectWaveGrid ? kIntersectWaveGrid : most)), dim3(64), 0, st, a);
    SFM_HIP_TRY(hipGetLastError());
    return SFM_OK;
}

} // namespace sfm
