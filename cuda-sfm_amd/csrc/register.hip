// register.hip -- registering a further view against the pair's 3-D points (gfx950): P3P RANSAC, then a pose-only
// Levenberg-Marquardt.  Arithmetic: register_math.hpp (shared with the host build of the CPU tests).
//
// Four launches on the pair's stream, no host synchronisation:
//   register_gate_kernel    ONE block of 1024 threads: the candidates (matched, gated, usable 3-D point) compacted in point
//                           order -- a contiguous range of points per thread and block_scan (block_ops.hpp), as in
//                           homo_gate_kernel, so the order does not depend on scheduling -- as X / W (float4) and the normalised
//                           observation (float2), the point -> candidate map and the candidate count.
//   register_solve_kernel   one lane per hypothesis: sample4, Lambda Twist on three samples, the 4th chooses; the 12-float pose
//                           into a per-hypothesis array (zero for a degenerate sample); the lane also clears the hypothesis'
//                           accumulator (and hypothesis 0 the key) for the scoring launch behind it.
//   register_score_kernel   grid (hypotheses / 256) x splits: each block scores its 256 hypotheses against one contiguous share
//                           of the candidates, staged through LDS.  At the default 4096 hypotheses one lane per hypothesis is
//                           only 64 wavefronts: the split over the candidates gives the GPU enough blocks.  One 64-bit atomic
//                           per hypothesis adds the share's count to the low word and 1 to the high word (the pre-filter
//                           kernel's count | arrived accumulator); the lane that finds all other shares arrived holds the final
//                           count, stores it and folds (count << 32) | (0xFFFFFFFF - hyp) into the key (first maximum wins).
//                           Integer atomics only: the counts do not depend on the split or on the order of arrival.
//   register_refine_kernel  ONE block of 256 threads: the winner's pose and inliers, the 6-parameter LM chain (fp32 per-point
//                           terms, fp64 sums in a fixed order by block_sum, Cholesky on one lane; damping, accept test and
//                           stop rules are LmControl's, refine_math.hpp, as in refine.hip), then every point's error and
//                           final flag and the report.  The candidate set of a view is at most the pair's points (thousands): one block
//                           runs an iteration in a few microseconds, less than a grid launch per iteration would cost.
//
// Many views in one call (launch_register_views): the same four bodies over an array of RegisterArgs in device memory, one per
// pair -- gate and LM chain one block per job, solve grid (hypothesis blocks, jobs), scoring grid (hypothesis blocks, shares, jobs)
// with ONE share count for the launch.  Every block works on its own pair's buffers: a pair ends bit for bit as its single call.
#include "common.hpp"
#include "device_math.hpp"
#include "block_ops.hpp"
#include "register_math.hpp"

namespace sfm {

constexpr int kRegGateThreads = 1024;
constexpr int kRegHypBlock = 256;         // hypotheses per scoring block (one per lane)
constexpr int kRegTile = 1024;            // candidates per LDS stage of the scoring kernel (24 KiB)
constexpr int kRegThreads = 256;          // the LM block
constexpr int kRegWaves = kRegThreads / 64;
constexpr int kRegMinInliers = 6;         // a winner with fewer inliers is SFM_REFINE_DEGENERATE
constexpr int kRegSysValues = 27;         // J^T W J (21 packed), J^T W r (6)

// word offsets inside pair->d_vstate
constexpr int kVsPose = 0;                // refined pose (16), the RANSAC winner's pose (16)   (SFM_BUF_VIEW_POSE)
constexpr int kVsReport = 32;             // sfm_register_report (11 words)
constexpr int kVsKey = 48;                // uint64 packed arg-max key (8-byte aligned)
constexpr int kVsCount = 50;              // int number of candidates
constexpr int kVsWords = 64;

struct RegisterArgs {
    const sfm_sift_point *sift;
    const float *points;                  // 4 x n
    const uint8_t *valid;                 // n or null
    const float *K, *Kinv;
    int n;
    float min_score, max_ambiguity, thr;
    uint32_t seed, H;
    int max_iter;
    float huber, min_rel, lambda0;
    float *state;                         // kVsWords
    float4 *Xc;                           // per candidate: X / W
    float2 *Oc;                           // per candidate: normalised observation
    int *slot;                            // point j -> candidate k or -1
    uint8_t *inl;                         // per candidate: inlier of the winner
    float *poses;                         // 12 x H
    unsigned long long *acc;              // H: (arrived << 32) | count
    int *counts;                          // H
    float *reproj;                        // outputs: err[n], then uint8 inlier[n]
};

__device__ __forceinline__ bool register_gate(const RegisterArgs &a, int j)
{
    const sfm_sift_point &s = a.sift[j];
    if (!(s.match >= 0 && s.score > a.min_score && s.ambiguity < a.max_ambiguity)) return false;
    if (a.valid && !a.valid[j]) return false;
    const float X = a.points[j], Y = a.points[(size_t)a.n + j], Z = a.points[2 * (size_t)a.n + j], W = a.points[3 * (size_t)a.n + j];
    return isfinite(X) && isfinite(Y) && isfinite(Z) && isfinite(W) && W != 0.0f && Z / W > 0.0f;
}

__device__ __forceinline__ void register_gate_block(const RegisterArgs &a)
{
    __shared__ int wsum[kRegGateThreads / 64 + 1];
    const int per = (a.n + kRegGateThreads - 1) / kRegGateThreads;
    const int lo = min(a.n, (int)threadIdx.x * per), hi = min(a.n, lo + per);
    int mine = 0;
    for (int j = lo; j < hi; ++j) mine += register_gate(a, j) ? 1 : 0;
    int k = block_scan<kRegGateThreads / 64>(mine, wsum);
    if (threadIdx.x == 0) reinterpret_cast<int *>(a.state)[kVsCount] = wsum[kRegGateThreads / 64];
    const float *ki = a.Kinv;
    for (int j = lo; j < hi; ++j) {
        if (!register_gate(a, j)) { a.slot[j] = -1; continue; }
        const float W = a.points[3 * (size_t)a.n + j];
        a.Xc[k] = make_float4(a.points[j] / W, a.points[(size_t)a.n + j] / W, a.points[2 * (size_t)a.n + j] / W, 0.0f);
        const float u = a.sift[j].match_xpos, v = a.sift[j].match_ypos;
        float x[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) x[r] = fmaf(ki[3 * r + 2], 1.0f, fmaf(ki[3 * r + 1], v, ki[3 * r] * u));     // fill_xu_kernel's K^-1 u
        a.Oc[k] = make_float2(x[0] / x[2], x[1] / x[2]);
        a.slot[j] = k++;
    }
}

__device__ __forceinline__ void register_solve_block(const RegisterArgs &a)
{
    const uint32_t h = blockIdx.x * kRegHypBlock + threadIdx.x;
    if (h == 0) *reinterpret_cast<unsigned long long *>(a.state + kVsKey) = 0ull;
    if (h >= a.H) return;
    a.acc[h] = 0ull;
    const int m = reinterpret_cast<const int *>(a.state)[kVsCount];
    const RefineCam K = { a.K[0], a.K[1], a.K[4] };
    float P[12];
    register_hypothesis(a.seed, h, m, K, a.Xc, a.Oc, P);
#pragma unroll
    for (int q = 0; q < 12; ++q) a.poses[(size_t)q * a.H + h] = P[q];
}

// blockIdx.y of gridDim.y candidate shares (a share that is empty -- a job with few candidates -- still adds its arrival)
__device__ __forceinline__ void register_score_block(const RegisterArgs &a)
{
    __shared__ float4 sX[kRegTile];
    __shared__ float2 sO[kRegTile];
    const uint32_t h = blockIdx.x * kRegHypBlock + threadIdx.x;
    const int m = reinterpret_cast<const int *>(a.state)[kVsCount];
    const int splits = gridDim.y;
    const int chunk = (m + splits - 1) / splits;
    const int lo = min(m, (int)blockIdx.y * chunk), hi = min(m, lo + chunk);
    const RefineCam K = { a.K[0], a.K[1], a.K[4] };
    float P[12];
#pragma unroll
    for (int q = 0; q < 12; ++q) P[q] = h < a.H ? a.poses[(size_t)q * a.H + h] : 0.0f;
    int cnt = 0;
    for (int base = lo; base < hi; base += kRegTile) {
        const int len = min(kRegTile, hi - base);
        __syncthreads();
        for (int k = threadIdx.x; k < len; k += kRegHypBlock) { sX[k] = a.Xc[base + k]; sO[k] = a.Oc[base + k]; }
        __syncthreads();
        for (int k = 0; k < len; ++k) {
            const float4 X4 = sX[k];
            const float2 o = sO[k];
            const float X[3] = { X4.x, X4.y, X4.z };
            cnt += register_inlier(K, a.thr, P, X, o.x, o.y) ? 1 : 0;
        }
    }
    unsigned long long key = 0ull;
    if (h < a.H) {
        const unsigned long long old = atomicAdd(&a.acc[h], (1ull << 32) | (unsigned long long)cnt);
        if ((uint32_t)(old >> 32) == (uint32_t)(splits - 1)) {
            const uint32_t total = (uint32_t)old + (uint32_t)cnt;
            a.counts[h] = (int)total;
            key = pack_key(total, h);
        }
    }
    key = wave_max(key);
    if ((threadIdx.x & 63) == 0 && key) atomicMax(reinterpret_cast<unsigned long long *>(a.state + kVsKey), key);
}

__device__ __forceinline__ void register_refine_block(const RegisterArgs &a)
{
    __shared__ double s_part[kRegWaves * kRegSysValues];
    __shared__ double s_tot[kRegSysValues];
    __shared__ float s_pose[12], s_try[12];
    __shared__ int s_go, s_degen, s_cnt[kRegWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const RefineCam K = { uniform(a.K[0]), uniform(a.K[1]), uniform(a.K[4]) };
    const int m = reinterpret_cast<const int *>(a.state)[kVsCount];
    const unsigned long long key = *reinterpret_cast<const unsigned long long *>(a.state + kVsKey);
    const uint32_t best = 0xFFFFFFFFu - (uint32_t)key;
    const int wcount = (int)(key >> 32);

    // ---- the winner: its pose ([I|0] when no sample gave one), whether there is anything to refine ----
    if (tid == 0) {
        float P[12];
        bool any = false;
#pragma unroll
        for (int q = 0; q < 12; ++q) { P[q] = best < a.H ? a.poses[(size_t)q * a.H + best] : 0.0f; any = any || P[q] != 0.0f; }
        if (!any) {
#pragma unroll
            for (int q = 0; q < 12; ++q) P[q] = (q == 0 || q == 4 || q == 8) ? 1.0f : 0.0f;
        }
#pragma unroll
        for (int q = 0; q < 12; ++q) s_pose[q] = P[q];
        refine_store_pose(P, a.state + kVsPose + 16);
        s_degen = (m < 4 || wcount < kRegMinInliers) ? 1 : 0;
    }
    __syncthreads();
    const bool degen = s_degen != 0;
    float P[12];
#pragma unroll
    for (int q = 0; q < 12; ++q) P[q] = uniform(s_pose[q]);

    // ---- the winner's inliers: the points the LM runs over ----
    for (int k = tid; k < m; k += kRegThreads) {
        const float4 X4 = a.Xc[k];
        const float2 o = a.Oc[k];
        const float X[3] = { X4.x, X4.y, X4.z };
        a.inl[k] = (!degen && register_inlier(K, a.thr, P, X, o.x, o.y)) ? 1 : 0;
    }
    __syncthreads();
    const float huber = a.huber;
    auto cost_at = [&](const float *Q, double v[2]) {
        v[0] = 0.0; v[1] = 0.0;
        for (int k = tid; k < m; k += kRegThreads) {
            if (!a.inl[k]) continue;
            const float4 X4 = a.Xc[k];
            const float2 o = a.Oc[k];
            const float X[3] = { X4.x, X4.y, X4.z };
            float r[2], J[12], rho;
            register_jacobian(K, Q, X, o.x, o.y, r, J);
            refine_huber(r[0], r[1], huber, rho);
            v[0] += (double)rho;
            v[1] += (double)(r[0] * r[0] + r[1] * r[1]);
        }
    };
    {
        double v[2];
        cost_at(P, v);
        block_sum<kRegWaves>(v, s_part, s_tot);
    }
    LmControl lm(a.lambda0, s_tot[0], s_tot[1], degen);
    const int nin = degen ? 0 : wcount;
    const float initial_rms = nin > 0 ? (float)sqrt(lm.sq / (2.0 * nin)) : 0.0f;

    while (lm.running(a.max_iter)) {
        // ---- the weighted normal equations at P ----
        double sys[kRegSysValues];
#pragma unroll
        for (int q = 0; q < kRegSysValues; ++q) sys[q] = 0.0;
        for (int k = tid; k < m; k += kRegThreads) {
            if (!a.inl[k]) continue;
            const float4 X4 = a.Xc[k];
            const float2 o = a.Oc[k];
            const float X[3] = { X4.x, X4.y, X4.z };
            float r[2], J[12], rho;
            register_jacobian(K, P, X, o.x, o.y, r, J);
            const float w = refine_huber(r[0], r[1], huber, rho);
            register_terms(r, J, w, [&](int q, float v) { sys[q] += (double)v; });
        }
        block_sum<kRegWaves>(sys, s_part, s_tot);
        // ---- the step on one lane: (H + lambda diag H) d = -g, R <- exp([w]x) R, t <- t + dt ----
        if (tid == 0) {
            double S[21], d[6];
#pragma unroll
            for (int q = 0; q < 21; ++q) S[q] = s_tot[q];
#pragma unroll
            for (int q = 0; q < 6; ++q) { S[symn<6>(q, q)] += lm.lambda * s_tot[symn<6>(q, q)]; d[q] = -s_tot[21 + q]; }
            const bool ok = refine_cholesky<6>(S, d);
            s_go = ok ? 1 : 0;
            if (ok) {
                float Rn[9];
                refine_rotate(d, s_pose, Rn);
#pragma unroll
                for (int q = 0; q < 9; ++q) s_try[q] = Rn[q];
#pragma unroll
                for (int r = 0; r < 3; ++r) s_try[9 + r] = (float)((double)s_pose[9 + r] + d[3 + r]);
            }
        }
        __syncthreads();
        if (!s_go) {                                      // not positive definite: more damping
            if (!lm.solve_failed()) break;
            continue;
        }
        // ---- the cost of the tentative pose ----
        float Pt[12];
#pragma unroll
        for (int q = 0; q < 12; ++q) Pt[q] = uniform(s_try[q]);
        double v[2];
        cost_at(Pt, v);
        block_sum<kRegWaves>(v, s_part, s_tot);
        bool stop;
        if (lm.tentative(s_tot[0], s_tot[1], (double)a.min_rel, stop)) {     // accepted: commit the pose
#pragma unroll
            for (int q = 0; q < 12; ++q) P[q] = Pt[q];
            __syncthreads();                              // every lane has read s_pose / s_try for this iteration
            if (tid < 12) s_pose[tid] = s_try[tid];
            __syncthreads();
        }
        if (stop) break;
    }

    // ---- every point under the final pose: pixel error, final inlier flag ----
    int mine = 0;
    uint8_t *flag = reinterpret_cast<uint8_t *>(a.reproj + a.n);
    for (int j = tid; j < a.n; j += kRegThreads) {
        const int k = a.slot[j];
        float e = __builtin_inff();
        bool in = false;
        if (k >= 0) {
            const float4 X4 = a.Xc[k];
            const float2 o = a.Oc[k];
            const float X[3] = { X4.x, X4.y, X4.z };
            e = sqrtf(register_sq_error(K, P, X, o.x, o.y));
            in = !degen && register_inlier(K, a.thr, P, X, o.x, o.y);
        }
        a.reproj[j] = e;
        flag[j] = in ? 1 : 0;
        mine += in ? 1 : 0;
    }
    for (int off = 32; off > 0; off >>= 1) mine += __shfl_xor(mine, off);
    if (lane == 0) s_cnt[wave] = mine;
    __syncthreads();
    if (tid == 0) {
        int nfin = 0;
        for (int w = 0; w < kRegWaves; ++w) nfin += s_cnt[w];
        refine_store_pose(P, a.state + kVsPose);
        sfm_register_report rep;
        rep.status = lm.status;
        rep.num_candidates = m;
        rep.ransac_inliers = nin;
        rep.num_inliers = nfin;
        rep.best_hypothesis = best;
        rep.iterations = lm.iters; rep.accepted = lm.accepted;
        rep.initial_rms_px = initial_rms;
        rep.final_rms_px = nin > 0 ? (float)sqrt(lm.sq / (2.0 * nin)) : 0.0f;
        rep.final_cost = (float)lm.cost;
        rep.lambda = (float)lm.lambda;
        *reinterpret_cast<sfm_register_report *>(a.state + kVsReport) = rep;
    }
}

__global__ __launch_bounds__(kRegGateThreads)
void register_gate_kernel(RegisterArgs a) { register_gate_block(a); }

__global__ __launch_bounds__(kRegHypBlock)
void register_solve_kernel(RegisterArgs a) { register_solve_block(a); }

__global__ __launch_bounds__(kRegHypBlock)
void register_score_kernel(RegisterArgs a) { register_score_block(a); }

__global__ __launch_bounds__(kRegThreads)
void register_refine_kernel(RegisterArgs a) { register_refine_block(a); }

// ---- many views: job blockIdx.x (gate, refine) / blockIdx.y (solve) / blockIdx.z (score) of `jobs` ----
// the block's job, through a uniform address (scalar loads), every pointer marked global (block_ops.hpp)
__device__ __forceinline__ RegisterArgs load_job(const RegisterArgs *__restrict__ jobs, const unsigned int job)
{
    RegisterArgs a = jobs[job];
    a.sift = global_ptr(a.sift); a.points = global_ptr(a.points); a.valid = global_ptr(a.valid); a.K = global_ptr(a.K); a.Kinv = global_ptr(a.Kinv);
    a.state = global_ptr(a.state); a.Xc = global_ptr(a.Xc); a.Oc = global_ptr(a.Oc); a.slot = global_ptr(a.slot); a.inl = global_ptr(a.inl);
    a.poses = global_ptr(a.poses); a.acc = global_ptr(a.acc); a.counts = global_ptr(a.counts); a.reproj = global_ptr(a.reproj);
    return a;
}

// Every block of the four runs its body to the end (the solve body's lanes past H leave on their own, behind no barrier): no
// block is cut short in front of a barrier or a ballot.
__global__ __launch_bounds__(kRegGateThreads)
void register_gate_views_kernel(const RegisterArgs *__restrict__ jobs)
{
    const RegisterArgs a = load_job(jobs, blockIdx.x);
    register_gate_block(a);
}

__global__ __launch_bounds__(kRegHypBlock)
void register_solve_views_kernel(const RegisterArgs *__restrict__ jobs)
{
    const RegisterArgs a = load_job(jobs, blockIdx.y);
    register_solve_block(a);
}

__global__ __launch_bounds__(kRegHypBlock)
void register_score_views_kernel(const RegisterArgs *__restrict__ jobs)
{
    const RegisterArgs a = load_job(jobs, blockIdx.z);
    register_score_block(a);
}

__global__ __launch_bounds__(kRegThreads)
void register_refine_views_kernel(const RegisterArgs *__restrict__ jobs)
{
    const RegisterArgs a = load_job(jobs, blockIdx.x);
    register_refine_block(a);
}

// pair->d_vwork for cap_points points: the arrays of `a` inside it; returns its size in bytes
static size_t register_work_layout(void *buffer, int cap_points, RegisterArgs &a)
{
    const size_t cap = (size_t)cap_points;
    Carver w(buffer);
    a.Xc = w.take<float4>(cap);
    a.Oc = w.take<float2>(cap);
    a.slot = w.take<int>(cap);
    a.inl = w.take<uint8_t>(cap);
    return w.used;
}

// pair->d_vhyp for `hyps` hypotheses, likewise
static size_t register_hyp_layout(void *buffer, size_t hyps, RegisterArgs &a)
{
    Carver h(buffer);
    a.acc = h.take<unsigned long long>(hyps);
    a.poses = h.take<float>(12 * hyps);
    return h.used;
}

static void register_args(sfm_pair *pair, const sfm_sift_point *d_sift, const sfm_register_params &p, const float *d_points, const uint8_t *d_valid,
                          RegisterArgs &a)
{
    a.sift = d_sift; a.points = d_points; a.valid = d_valid;
    a.K = pair->d_K; a.Kinv = pair->d_Kinv;
    a.n = pair->n;
    a.min_score = p.min_score; a.max_ambiguity = p.max_ambiguity; a.thr = p.threshold_px;
    a.seed = p.seed; a.H = p.num_hypotheses;
    a.max_iter = p.max_iterations; a.huber = p.huber_px; a.min_rel = p.min_rel_decrease; a.lambda0 = p.initial_lambda;
    a.state = pair->d_vstate;
    a.reproj = pair->d_vreproj;
    register_work_layout(pair->d_vwork, pair->cap_points, a);
    register_hyp_layout(pair->d_vhyp, pair->cap_vhyps, a);       // sized for the largest num_hypotheses seen
    a.counts = pair->d_vcounts;
}

// candidate shares of a scoring launch: about four blocks per CU over all its jobs, each share at least 128 candidates when every
// point of the largest job is one
static int register_splits(int num_cus, int hblocks, int num_jobs, int nmax)
{
    const long long blocks = (long long)hblocks * num_jobs;
    int splits = (int)((4LL * num_cus + blocks - 1) / blocks);
    const int max_splits = nmax / 128 > 1 ? nmax / 128 : 1;
    if (splits > max_splits) splits = max_splits;
    if (splits < 1) splits = 1;
    return splits;
}

int launch_register(sfm_pair *pair, const sfm_sift_point *d_sift, const sfm_register_params &p, const float *d_points, const uint8_t *d_valid)
{
    RegisterArgs a;
    register_args(pair, d_sift, p, d_points, d_valid, a);
    hipStream_t st = pair->ctx->stream;
    const int hblocks = (int)((p.num_hypotheses + kRegHypBlock - 1) / kRegHypBlock);
    const int splits = register_splits(pair->ctx->num_cus, hblocks, 1, pair->n);
    hipLaunchKernelGGL(register_gate_kernel, dim3(1), dim3(kRegGateThreads), 0, st, a);
    SFM_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(register_solve_kernel, dim3(hblocks), dim3(kRegHypBlock), 0, st, a);
    SFM_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(register_score_kernel, dim3(hblocks, splits), dim3(kRegHypBlock), 0, st, a);
    SFM_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(register_refine_kernel, dim3(1), dim3(kRegThreads), 0, st, a);
    SFM_HIP_TRY(hipGetLastError());
    return SFM_OK;
}

int launch_register_views(sfm_ctx *ctx, sfm_pair *const *pairs, int num_pairs, const sfm_sift_point *const *d_sifts, const sfm_register_params &p,
                          const float *const *d_points, const uint8_t *const *d_valid)
{
    hipStream_t st = ctx->stream;
    const RegisterArgs *d_jobs = nullptr;
    int nmax = 0;                                         // large views first: the one-block gates and LM chains are dispatched in job order
    const int rc = job_array_stage(ctx->register_jobs, num_pairs, st, [&](int i) { return pairs[i]->n; },
                                   [&](RegisterArgs &job, int i) { register_args(pairs[i], d_sifts[i], p, d_points[i], d_valid[i], job); }, &d_jobs, &nmax);
    if (rc != SFM_OK) return rc;
    const int hblocks = (int)((p.num_hypotheses + kRegHypBlock - 1) / kRegHypBlock);
    const int splits = register_splits(ctx->num_cus, hblocks, num_pairs, nmax);              // ONE for the launch: counts do not depend on it
    hipLaunchKernelGGL(register_gate_views_kernel, dim3(num_pairs), dim3(kRegGateThreads), 0, st, d_jobs);
    SFM_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(register_solve_views_kernel, dim3(hblocks, num_pairs), dim3(kRegHypBlock), 0, st, d_jobs);
    SFM_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(register_score_views_kernel, dim3(hblocks, splits, num_pairs), dim3(kRegHypBlock), 0, st, d_jobs);
    SFM_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(register_refine_views_kernel, dim3(num_pairs), dim3(kRegThreads), 0, st, d_jobs);
    SFM_HIP_TRY(hipGetLastError());
    return SFM_OK;
}

size_t register_work_bytes(int cap_points)
{
    RegisterArgs a;
    return register_work_layout(nullptr, cap_points, a);
}

size_t register_hyp_bytes(size_t num_hypotheses)
{
    RegisterArgs a;
    return register_hyp_layout(nullptr, num_hypotheses, a);
}

int register_state_words() { return kVsWords; }
int register_pose_offset() { return kVsPose; }
int register_report_offset() { return kVsReport; }

} // namespace sfm
