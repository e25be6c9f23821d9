// refine.hip -- two-view bundle adjustment after estimateE (gfx950): Levenberg-Marquardt over camera 2's pose and the used
// points, Huber loss on pixel residuals, Schur complement on the 5 pose parameters.  Per-point arithmetic: refine_math.hpp.
//
// Three launches on the pair's stream, no host synchronisation:
//   refine_start_kernel   grid over points, 4 lanes per point: the SFM_POSE_CORRECT candidates of E, every masked point
//                         triangulated against all four (triangulate_point, kSweeps4 -- the DLT sfm_triangulate runs), the
//                         cheirality votes per block.  The 4x4 Jacobi DLT is ~4k instructions per point: spread over the GPU.
//   refine_solve_kernel   ONE block of 512 threads: picks the candidate (first maximum of the votes), compacts the used points,
//                         runs the whole LM chain -- every iteration a block reduction of the reduced camera system, a 5x5
//                         Cholesky on one lane, the back substitution and the cost of the tentative step -- and writes the
//                         refined pose, E and the report.
//   refine_finish_kernel  grid over points: refined point or DLT against the refined pose, reprojection errors, used flags.
// Many pairs in one call (launch_refine_pairs): the same three bodies over an array of RefineArgs in device memory, one per pair --
//   refine_start_pairs_kernel / refine_finish_pairs_kernel   grid (blocks of the largest pair, pairs): blocks past a pair's own
//                         count leave as a whole;  refine_solve_pairs_kernel   grid (pairs), one solve block each.
// A block copies its job into registers through a uniform address (scalar loads), then runs the body the single-pair kernel runs:
// the arithmetic exists once, and a pair's result is the same bit for bit whichever entry point computed it.
// Reductions: per-thread fp64 sums in a fixed point order, then block_sum (block_ops.hpp: wave butterflies, the wave partials in
// wave order) -- no float atomics, so the result is the same bit for bit on every run.
// The damping schedule, the accept test, the stop rules and the report's bookkeeping are LmControl's (refine_math.hpp), which
// register.hip's pose-only LM drives too; the rotation update and the 4 x 4 pose store are shared the same way.  The system,
// its solve, the translation update and the commit are this kernel's own.
#include "common.hpp"
#include "device_math.hpp"
#include "block_ops.hpp"
#include "refine_math.hpp"

namespace sfm {

constexpr int kRefineSweeps = 8;          // = kSweeps4 of pose.hip: the start points are sfm_triangulate(CORRECT)'s
constexpr int kRefineThreads = 512;      // 1024 needs > 128 VGPRs (the fp64 sums of the system + one point's Jacobians): it spilled
constexpr int kRefineWaves = kRefineThreads / 64;
constexpr int kStartPoints = 64;          // points per block of refine_start_kernel (4 lanes each)
constexpr int kFinishPoints = 256;        // points (= threads) per block of refine_finish_kernel
constexpr int kRefineMinPoints = 16;
constexpr int kSysValues = 25;            // S (15), b (5), diag U (5)

// word offsets inside pair->d_rstate
constexpr int kStP = 0;                   // 4 x 16 candidates
constexpr int kStPose = 64;               // refined P (16) + E (9)  (SFM_BUF_REFINED_POSE)
constexpr int kStReport = 96;             // sfm_refine_report
constexpr int kStWords = 128;

struct RefineArgs {
    const float *X0, *X1;
    int ld, n, cap;
    const float *E, *K;
    const uint8_t *mask;
    float huber, min_rel, lambda0;
    int max_iter;
    float *state;                         // kStWords
    int *votes;                           // 4 per start block
    float4 *cand;                         // 4 x cap start points
    float4 *obs, *Xa, *Xb;                // per used point (compact order)
    int *idx, *slot;                      // used point k -> j; j -> k or -1
    float *points, *reproj;               // outputs: 4 x n; err[n] then uint8 used[n]
};

// The three bodies.  `a` is uniform over the block: the kernel's argument, or the block's copy of its job.
__device__ __forceinline__ void refine_start_block(const RefineArgs &a, const int block)
{
    __shared__ int s_votes[4][4];
    const int i = threadIdx.x & 3;
    const int wave = threadIdx.x >> 6;
    const int j = block * kStartPoints + (int)(threadIdx.x >> 2);
    float e[9], p[64];
#pragma unroll
    for (int k = 0; k < 9; ++k) e[k] = a.E[k];
    pose_candidates(e, SFM_POSE_CORRECT, p);
    float Pm[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) Pm[k] = i == 0 ? p[k] : i == 1 ? p[16 + k] : i == 2 ? p[32 + k] : p[48 + k];
    bool pass = false;
    if (j < a.n && a.mask[j]) {
        float pt[4];
        // the rays as the residuals see them: x / z, y / z (z = 1 after fillXU, where the division changes nothing; sfm_set_points
        // takes any z)
        const float z0 = a.X0[2 * (size_t)a.ld + j], z1 = a.X1[2 * (size_t)a.ld + j];
        triangulate_point(a.X0[j] / z0, a.X0[(size_t)a.ld + j] / z0, a.X1[j] / z1, a.X1[(size_t)a.ld + j] / z1, Pm, kRefineSweeps, pt);
        float z2 = Pm[8] * pt[0];
#pragma unroll
        for (int k = 1; k < 4; ++k) z2 = fmaf(Pm[8 + k], pt[k], z2);
        pass = (pt[2] > 0.0f) && (z2 > 0.0f);             // choose_pose_vote_kernel's test
        a.cand[(size_t)i * a.cap + j] = make_float4(pt[0], pt[1], pt[2], pt[3]);
    }
    const unsigned long long m = __ballot(pass);
    if ((threadIdx.x & 63) < 4) {
        const unsigned long long lanes = 0x1111111111111111ull << i;
        s_votes[wave][i] = __builtin_popcountll(m & lanes);
    }
    __syncthreads();
    if (threadIdx.x < 4) a.votes[4 * block + threadIdx.x] = s_votes[0][i] + s_votes[1][i] + s_votes[2][i] + s_votes[3][i];
    if (block == 0 && threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < 64; ++k) a.state[kStP + k] = p[k];
    }
}

__device__ __forceinline__ void load_pose(const float *s, RefinePose &P)
{
#pragma unroll
    for (int k = 0; k < 9; ++k) P.R[k] = uniform(s[k]);
#pragma unroll
    for (int k = 0; k < 3; ++k) { P.t[k] = uniform(s[9 + k]); P.b1[k] = uniform(s[12 + k]); P.b2[k] = uniform(s[15 + k]); }
}

// one lane: the tangent basis of the pose in s (R 9, t 3) into s[12..17]
__device__ void set_basis(float *s)
{
    const double t[3] = { s[9], s[10], s[11] };
    double b1[3], b2[3];
    refine_tangent_basis(t, b1, b2);
#pragma unroll
    for (int k = 0; k < 3; ++k) { s[12 + k] = (float)b1[k]; s[15 + k] = (float)b2[k]; }
}

__device__ __forceinline__ void refine_solve_block(const RefineArgs &a)
{
    __shared__ double s_part[kRefineWaves * kSysValues];
    __shared__ double s_tot[kSysValues];
    __shared__ float s_pose[18], s_try[18], s_dc[5];
    __shared__ int s_wcount[kRefineWaves];
    __shared__ int s_pi, s_used, s_go, s_cur;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const RefineCam K = { uniform(a.K[0]), uniform(a.K[1]), uniform(a.K[4]) };

    // ---- start: the candidate most masked points see in front of both cameras (first maximum) ----
    if (tid == 0) {
        const int nb = (a.n + kStartPoints - 1) / kStartPoints;
        int v0 = 0, v1 = 0, v2 = 0, v3 = 0;
        for (int b = 0; b < nb; ++b) {
            const int4 q = reinterpret_cast<const int4 *>(a.votes)[b];
            v0 += q.x; v1 += q.y; v2 += q.z; v3 += q.w;
        }
        int best = v0, arg = 0;                           // first maximum
        if (v1 > best) { best = v1; arg = 1; }
        if (v2 > best) { best = v2; arg = 2; }
        if (v3 > best) { best = v3; arg = 3; }
        s_pi = arg;
        const float *P = a.state + kStP + 16 * arg;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
#pragma unroll
            for (int c = 0; c < 3; ++c) s_pose[3 * r + c] = P[4 * r + c];
            s_pose[9 + r] = P[4 * r + 3];
        }
        set_basis(s_pose);
        s_used = 0;
    }
    __syncthreads();
    const int pi = s_pi;
    RefinePose P;
    load_pose(s_pose, P);

    // ---- used set, compacted in point order (block prefix scan per round of kRefineThreads points) ----
    for (int base = 0; base < a.n; base += kRefineThreads) {
        const int j = base + tid;
        bool use = false;
        float4 X = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (j < a.n && a.mask[j]) {
            X = a.cand[(size_t)pi * a.cap + j];
            const float Xv[3] = { X.x, X.y, X.z };
            float q[3], Y[3];
            refine_to_cam2(P, Xv, q, Y);
            use = isfinite(X.x) && isfinite(X.y) && isfinite(X.z) && X.z > 0.0f && Y[2] > 0.0f;
        }
        const unsigned long long m = __ballot(use);
        if (lane == 0) s_wcount[wave] = __builtin_popcountll(m);
        __syncthreads();
        int off = s_used;
        for (int w = 0; w < wave; ++w) off += s_wcount[w];
        const int k = off + __builtin_popcountll(m & ((1ull << lane) - 1ull));
        if (j < a.n) {
            a.slot[j] = use ? k : -1;
            if (use) {
                const float z1 = a.X0[2 * (size_t)a.ld + j], z2 = a.X1[2 * (size_t)a.ld + j];
                a.obs[k] = make_float4(a.X0[j] / z1, a.X0[(size_t)a.ld + j] / z1, a.X1[j] / z2, a.X1[(size_t)a.ld + j] / z2);
                a.Xa[k] = X;
                a.idx[k] = j;
            }
        }
        __syncthreads();
        if (tid == 0) { int t = s_used; for (int w = 0; w < kRefineWaves; ++w) t += s_wcount[w]; s_used = t; }
        __syncthreads();
    }
    const int m = s_used;
    const float huber = a.huber;

    // ---- cost of the start ----
    {
        double v[2] = { 0.0, 0.0 };
        for (int k = tid; k < m; k += kRefineThreads) {
            const float4 o4 = a.obs[k], X4 = a.Xa[k];
            const float o[4] = { o4.x, o4.y, o4.z, o4.w }, X[3] = { X4.x, X4.y, X4.z };
            float r[4], z1, z2, rho1, rho2;
            refine_residual(K, P, o, X, r, z1, z2);
            refine_huber(r[0], r[1], huber, rho1);
            refine_huber(r[2], r[3], huber, rho2);
            v[0] += (double)rho1 + (double)rho2;
            v[1] += (double)(r[0] * r[0] + r[1] * r[1]) + (double)(r[2] * r[2] + r[3] * r[3]);
        }
        block_sum<kRefineWaves>(v, s_part, s_tot);
    }
    LmControl lm(a.lambda0, s_tot[0], s_tot[1], m < kRefineMinPoints);
    const float initial_rms = m > 0 ? (float)sqrt(lm.sq / (4.0 * m)) : 0.0f;
    int cur = 0;                                          // Xa (0) or Xb (1) holds the committed points

    while (lm.running(a.max_iter)) {
        const float lam = uniform((float)lm.lambda);
        const float4 *Xc = cur ? a.Xb : a.Xa;
        float4 *Xn = cur ? a.Xa : a.Xb;
        // ---- pass A: the reduced camera system ----
        double sys[kSysValues];
#pragma unroll
        for (int q = 0; q < kSysValues; ++q) sys[q] = 0.0;
        for (int k = tid; k < m; k += kRefineThreads) {
            const float4 o4 = a.obs[k], X4 = Xc[k];
            const float o[4] = { o4.x, o4.y, o4.z, o4.w }, X[3] = { X4.x, X4.y, X4.z };
            RefineJac J;
            refine_jacobian(K, P, o, X, J);
            float rho, Vi[6], Wm[15], gp[3];
            const float w1 = refine_huber(J.r[0], J.r[1], huber, rho), w2 = refine_huber(J.r[2], J.r[3], huber, rho);
            refine_point_block(J, w1, w2, lam, Vi, Wm, gp);
            refine_schur(J, w2, Vi, Wm, gp, [&](int q, float v) { sys[q] += (double)v; });
        }
        block_sum<kRefineWaves>(sys, s_part, s_tot);
        // ---- the pose step on one lane ----
        if (tid == 0) {
            double Sd[15], dc[5];
#pragma unroll
            for (int q = 0; q < 15; ++q) Sd[q] = s_tot[q];
#pragma unroll
            for (int q = 0; q < 5; ++q) { Sd[sym5(q, q)] += lm.lambda * s_tot[20 + q]; dc[q] = -s_tot[15 + q]; }
            const bool ok = refine_solve5(Sd, dc);
            s_go = ok ? 1 : 0;
            if (ok) {
                double t[3], nn = 0.0;
                float Rn[9];
                refine_rotate(dc, s_pose, Rn);
#pragma unroll
                for (int q = 0; q < 9; ++q) s_try[q] = Rn[q];
#pragma unroll
                for (int q = 0; q < 3; ++q) { t[q] = (double)s_pose[9 + q] + (double)s_pose[12 + q] * dc[3] + (double)s_pose[15 + q] * dc[4]; nn += t[q] * t[q]; }
                nn = sqrt(nn);
#pragma unroll
                for (int q = 0; q < 3; ++q) s_try[9 + q] = (float)(t[q] / nn);
#pragma unroll
                for (int q = 0; q < 5; ++q) s_dc[q] = (float)dc[q];
                set_basis(s_try);
            }
        }
        __syncthreads();
        if (!s_go) {                                      // not positive definite: more damping
            if (!lm.solve_failed()) break;
            continue;
        }
        // ---- pass B: point steps and the cost of the tentative state ----
        RefinePose Pt;
        load_pose(s_try, Pt);
        const float dc[5] = { uniform(s_dc[0]), uniform(s_dc[1]), uniform(s_dc[2]), uniform(s_dc[3]), uniform(s_dc[4]) };
        double v[2] = { 0.0, 0.0 };
        for (int k = tid; k < m; k += kRefineThreads) {
            const float4 o4 = a.obs[k], X4 = Xc[k];
            const float o[4] = { o4.x, o4.y, o4.z, o4.w }, X[3] = { X4.x, X4.y, X4.z };
            RefineJac J;
            refine_jacobian(K, P, o, X, J);
            float rho1, rho2, Vi[6], Wm[15], gp[3], dp[3];
            const float w1 = refine_huber(J.r[0], J.r[1], huber, rho1), w2 = refine_huber(J.r[2], J.r[3], huber, rho2);
            refine_point_block(J, w1, w2, lam, Vi, Wm, gp);
            refine_point_step(Vi, Wm, gp, dc, dp);
            const float Xt[3] = { X[0] + dp[0], X[1] + dp[1], X[2] + dp[2] };
            Xn[k] = make_float4(Xt[0], Xt[1], Xt[2], 1.0f);
            float r[4], z1, z2;
            refine_residual(K, Pt, o, Xt, r, z1, z2);
            refine_huber(r[0], r[1], huber, rho1);
            refine_huber(r[2], r[3], huber, rho2);
            v[0] += (double)rho1 + (double)rho2;
            v[1] += (double)(r[0] * r[0] + r[1] * r[1]) + (double)(r[2] * r[2] + r[3] * r[3]);
        }
        block_sum<kRefineWaves>(v, s_part, s_tot);
        bool stop;
        if (lm.tentative(s_tot[0], s_tot[1], (double)a.min_rel, stop)) {     // accepted: commit pose and points
            cur ^= 1;
            P = Pt;
            __syncthreads();                              // every lane has read s_pose / s_try for this iteration
            if (tid < 18) s_pose[tid] = s_try[tid];
            __syncthreads();
        }
        if (stop) break;
    }

    // ---- refined pose, E = [t]x R, report; the used points into slot order for the finish kernel ----
    if (tid == 0) {
        float *Po = a.state + kStPose;
        const float *R = s_pose, *t = s_pose + 9;
        refine_store_pose(s_pose, Po);
        const float tx[9] = { 0.0f, -t[2], t[1], t[2], 0.0f, -t[0], -t[1], t[0], 0.0f };
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) Po[16 + 3 * r + c] = tx[3 * r] * R[c] + tx[3 * r + 1] * R[3 + c] + tx[3 * r + 2] * R[6 + c];
        sfm_refine_report rep;
        rep.status = lm.status; rep.iterations = lm.iters; rep.accepted = lm.accepted; rep.num_used = m; rep.pose_index = pi;
        rep.initial_rms_px = initial_rms;
        rep.final_rms_px = m > 0 ? (float)sqrt(lm.sq / (4.0 * m)) : 0.0f;
        rep.final_cost = (float)lm.cost;
        rep.lambda = (float)lm.lambda;
        *reinterpret_cast<sfm_refine_report *>(a.state + kStReport) = rep;
        s_cur = cur;
    }
    __syncthreads();
    if (s_cur) {                                          // the finish kernel reads the committed points from Xa
        for (int k = tid; k < m; k += kRefineThreads) a.Xa[k] = a.Xb[k];
    }
}

__device__ __forceinline__ void refine_finish_block(const RefineArgs &a, const int block)
{
    const int j = block * kFinishPoints + threadIdx.x;
    if (j >= a.n) return;
    const float *Po = a.state + kStPose;
    float Pm[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) Pm[k] = Po[k];
    const int k = a.slot[j];
    const float z1 = a.X0[2 * (size_t)a.ld + j], z2 = a.X1[2 * (size_t)a.ld + j];
    const float o[4] = { a.X0[j] / z1, a.X0[(size_t)a.ld + j] / z1, a.X1[j] / z2, a.X1[(size_t)a.ld + j] / z2 };
    float pt[4];
    if (k >= 0) {
        const float4 X = a.Xa[k];
        pt[0] = X.x; pt[1] = X.y; pt[2] = X.z; pt[3] = 1.0f;
    } else {
        triangulate_point(o[0], o[1], o[2], o[3], Pm, kRefineSweeps, pt);     // on the rays the error below is measured on
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) a.points[(size_t)c * a.n + j] = pt[c];
    RefinePose P;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) P.R[3 * r + c] = Pm[4 * r + c];
        P.t[r] = Pm[4 * r + 3];
        P.b1[r] = 0.0f; P.b2[r] = 0.0f;
    }
    const RefineCam K = { a.K[0], a.K[1], a.K[4] };
    float r[4], d1, d2;
    refine_residual(K, P, o, pt, r, d1, d2);
    const float e = fmaxf(sqrtf(r[0] * r[0] + r[1] * r[1]), sqrtf(r[2] * r[2] + r[3] * r[3]));
    a.reproj[j] = (d1 > 0.0f && d2 > 0.0f) ? e : __builtin_inff();
    reinterpret_cast<uint8_t *>(a.reproj + a.n)[j] = k >= 0 ? 1 : 0;
}

__global__ __launch_bounds__(256)
void refine_start_kernel(RefineArgs a) { refine_start_block(a, blockIdx.x); }

__global__ __launch_bounds__(kRefineThreads)
void refine_solve_kernel(RefineArgs a) { refine_solve_block(a); }

__global__ __launch_bounds__(kFinishPoints)
void refine_finish_kernel(RefineArgs a) { refine_finish_block(a, blockIdx.x); }

// ---- many pairs: job blockIdx.y (start, finish) / blockIdx.x (solve) of `jobs` ----
// the block's job, through a uniform address (scalar loads), every pointer marked global (global_ptr, block_ops.hpp)
__device__ __forceinline__ RefineArgs load_job(const RefineArgs *__restrict__ jobs, const unsigned int job)
{
    RefineArgs a = jobs[job];
    a.X0 = global_ptr(a.X0); a.X1 = global_ptr(a.X1); a.E = global_ptr(a.E); a.K = global_ptr(a.K); a.mask = global_ptr(a.mask);
    a.state = global_ptr(a.state); a.votes = global_ptr(a.votes); a.cand = global_ptr(a.cand);
    a.obs = global_ptr(a.obs); a.Xa = global_ptr(a.Xa); a.Xb = global_ptr(a.Xb);
    a.idx = global_ptr(a.idx); a.slot = global_ptr(a.slot); a.points = global_ptr(a.points); a.reproj = global_ptr(a.reproj);
    return a;
}

__global__ __launch_bounds__(256)
void refine_start_pairs_kernel(const RefineArgs *__restrict__ jobs)
{
    const RefineArgs a = load_job(jobs, blockIdx.y);
    if ((int)blockIdx.x * kStartPoints >= a.n) return;    // past this pair's blocks: the whole block, before the ballot and the barrier
    refine_start_block(a, blockIdx.x);
}

__global__ __launch_bounds__(kRefineThreads)
void refine_solve_pairs_kernel(const RefineArgs *__restrict__ jobs)
{
    const RefineArgs a = load_job(jobs, blockIdx.x);
    refine_solve_block(a);
}

__global__ __launch_bounds__(kFinishPoints)
void refine_finish_pairs_kernel(const RefineArgs *__restrict__ jobs)
{
    const RefineArgs a = load_job(jobs, blockIdx.y);
    if ((int)blockIdx.x * kFinishPoints >= a.n) return;
    refine_finish_block(a, blockIdx.x);
}

// pair->d_rwork for cap_points points: the arrays of `a` inside it; returns its size in bytes
static size_t refine_work_layout(void *buffer, int cap_points, RefineArgs &a)
{
    const size_t cap = (size_t)cap_points;
    Carver w(buffer);
    a.cand = w.take<float4>(4 * cap);
    a.obs = w.take<float4>(cap);
    a.Xa = w.take<float4>(cap);
    a.Xb = w.take<float4>(cap);
    a.votes = w.take<int>(4 * (size_t)((cap_points + kStartPoints - 1) / kStartPoints));
    a.idx = w.take<int>(cap);
    a.slot = w.take<int>(cap);
    return w.used;
}

static void refine_args(sfm_pair *pair, const sfm_refine_params &p, const uint8_t *d_mask, RefineArgs &a)
{
    a.X0 = pair->d_X[0]; a.X1 = pair->d_X[1]; a.ld = pair->ld; a.n = pair->n; a.cap = pair->cap_points;
    a.E = pair->d_E; a.K = pair->d_K;
    a.mask = d_mask ? d_mask : pair->d_mask;
    a.huber = p.huber_px; a.min_rel = p.min_rel_decrease; a.lambda0 = p.initial_lambda; a.max_iter = p.max_iterations;
    a.state = pair->d_rstate;
    a.points = pair->d_rpoints; a.reproj = pair->d_rreproj;
    refine_work_layout(pair->d_rwork, pair->cap_points, a);
}

int launch_refine(sfm_pair *pair, const sfm_refine_params &p)
{
    RefineArgs a;
    refine_args(pair, p, p.d_mask, a);
    hipStream_t st = pair->ctx->stream;
    const int nb = (pair->n + kStartPoints - 1) / kStartPoints;
    hipLaunchKernelGGL(refine_start_kernel, dim3(nb), dim3(256), 0, st, a);
    SFM_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(refine_solve_kernel, dim3(1), dim3(kRefineThreads), 0, st, a);
    SFM_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(refine_finish_kernel, dim3((pair->n + kFinishPoints - 1) / kFinishPoints), dim3(kFinishPoints), 0, st, a);
    SFM_HIP_TRY(hipGetLastError());
    return SFM_OK;
}

int launch_refine_pairs(sfm_ctx *ctx, sfm_pair *const *pairs, int num_pairs, const sfm_refine_params &p, const uint8_t *const *d_masks)
{
    hipStream_t st = ctx->stream;
    const RefineArgs *d_jobs = nullptr;
    int nmax = 0;                                         // long chains first: the solve blocks are dispatched in job order
    const int rc = job_array_stage(ctx->refine_jobs, num_pairs, st, [&](int i) { return pairs[i]->n; },
                                   [&](RefineArgs &job, int i) { refine_args(pairs[i], p, d_masks ? d_masks[i] : nullptr, job); }, &d_jobs, &nmax);
    if (rc != SFM_OK) return rc;
    hipLaunchKernelGGL(refine_start_pairs_kernel, dim3((nmax + kStartPoints - 1) / kStartPoints, num_pairs), dim3(256), 0, st, d_jobs);
    SFM_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(refine_solve_pairs_kernel, dim3(num_pairs), dim3(kRefineThreads), 0, st, d_jobs);
    SFM_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(refine_finish_pairs_kernel, dim3((nmax + kFinishPoints - 1) / kFinishPoints, num_pairs), dim3(kFinishPoints), 0, st, d_jobs);
    SFM_HIP_TRY(hipGetLastError());
    return SFM_OK;
}

size_t refine_work_bytes(int cap_points)
{
    RefineArgs a;
    return refine_work_layout(nullptr, cap_points, a);
}

int refine_state_words() { return kStWords; }
int refine_pose_offset() { return kStPose; }
int refine_report_offset() { return kStReport; }

} // namespace sfm
