// adjust.hip -- sfm_adjust_view / sfm_adjust_views (gfx950): Levenberg-Marquardt bundle adjustment of cameras 2 and 3 and of
// every used point over the pair's three views.  Per-point arithmetic: adjust_math.hpp (shared with the host build of the CPU
// tests); damping, accept test and stop rules: LmControl (refine_math.hpp).
//
// Three launches on the pair's stream, no host synchronisation:
//   adjust_gather_kernel   grid over records, one lane each: the record's 16 bytes at +32 (one vector load: match_xpos / _ypos),
//                          the observations of views 1 and 2, the input column; the view bits at the start poses (out.d_views),
//                          the six observation floats and the start point X / W into the pair's work buffer.
//   adjust_solve_kernel    ONE block of 512 threads: compacts the used records in record order (block_scan), runs the whole LM
//                          chain -- per iteration the reduced camera system (11 x 11), its Cholesky on one lane out of LDS, the
//                          back substitution and the cost of the tentative state -- and writes the poses and the report.
//   adjust_scatter_kernel  grid over records: the output column and the error at the final state.
// The 88 sums of the system.  A thread of refine_solve_kernel keeps its 25 sums as fp64 accumulators; 88 of them are 176 VGPRs
// before a Jacobian exists.  Here the accumulation is transposed: a wavefront takes 64 points at a time, every lane forms its
// point's 88 fp32 terms (adjust_schur's emit), and wave_transpose_sum adds them over the wavefront in fp64 by a halving exchange
// -- 63 + 55 shuffles per 64 points, those of one step independent of each other -- that leaves the sums of values q and q + 64
// in lane q, which adds them to its two accumulators: two fp64 registers per lane instead of 88.  A lane past the end of the
// used set contributes zeros.  The wavefronts' partials are added in wave order through LDS (no float atomics): the order of
// every sum depends only on the used set, so a call repeats bit for bit and a pair's bytes do not depend on its place in a
// batched list.  (One six-step butterfly per emitted value was the first form: 2.5x the time per call)
// Many pairs in one call (launch_adjust_views): the same three bodies over an array of AdjustArgs in device memory.
#include "common.hpp"
#include "device_math.hpp"
#include "block_ops.hpp"
#include "adjust_math.hpp"

namespace sfm {

constexpr int kAdjThreads = 512;
constexpr int kAdjWaves = kAdjThreads / 64;
constexpr int kAdjGrid = 256;             // records (= threads) per block of the gather and scatter kernels

struct AdjustArgs {
    const sfm_sift_point *sift;
    const float *X0, *X1;                 // 3 x ld
    const float *K, *Kinv;
    const float *points;                  // 4 x n
    const uint8_t *flags, *used2;         // n each
    const float *pose2, *pose3;           // pose_rows == 3: R (9) then t (3); 4: a 4 x 4 row-major matrix
    int pose_rows;
    int ld, n;
    float huber, min_rel, lambda0;
    int max_iter;
    // the pair's work buffer: per record (gather), then per used record in compact order (solve)
    float4 *obs12, *start;                // per record: views 1 and 2; X / W
    float2 *obs3;
    int *slot;                            // record -> compact index, -1 = not used
    float4 *cobs12, *Xa, *Xb;             // compact
    float2 *cobs3;
    uint8_t *cbits;
    float *out_poses;                     // 24
    float *out_points;                    // 4 x n
    uint8_t *out_views;                   // n
    float *out_err;                       // n, or null
    sfm_adjust_report *out_report;
};

typedef float adj_f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void adjust_gather_block(const AdjustArgs &a, const int block)
{
    const int j = block * kAdjGrid + threadIdx.x;
    if (j >= a.n) return;
    const char *rec = reinterpret_cast<const char *>(a.sift + j);
    const adj_f32x4 m = *reinterpret_cast<const adj_f32x4 *>(rec + 32);       // match, match_xpos, match_ypos, match_error
    float P2[12], P3[12], Kinv[9], Xin[4];
    view_points_pose(a.pose2, a.pose_rows, P2);
    view_points_pose(a.pose3, a.pose_rows, P3);
#pragma unroll
    for (int q = 0; q < 12; ++q) { P2[q] = uniform(P2[q]); P3[q] = uniform(P3[q]); }      // the same in every lane: scalar registers
#pragma unroll
    for (int q = 0; q < 9; ++q) Kinv[q] = uniform(a.Kinv[q]);
#pragma unroll
    for (int c = 0; c < 4; ++c) Xin[c] = a.points[(size_t)c * a.n + j];
    const int bits = adjust_view_bits(a.flags[j], a.used2[j] != 0, Xin, P2, P3);
    a.out_views[j] = (uint8_t)bits;
    const float z1 = a.X0[2 * (size_t)a.ld + j], z2 = a.X1[2 * (size_t)a.ld + j];
    a.obs12[j] = make_float4(a.X0[j] / z1, a.X0[(size_t)a.ld + j] / z1, a.X1[j] / z2, a.X1[(size_t)a.ld + j] / z2);
    float x[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) x[r] = fmaf(Kinv[3 * r + 2], 1.0f, fmaf(Kinv[3 * r + 1], m.z, Kinv[3 * r] * m.y));      // view_points_load's K^-1 u
    a.obs3[j] = make_float2(x[0] / x[2], x[1] / x[2]);
    a.start[j] = bits ? make_float4(Xin[0] / Xin[3], Xin[1] / Xin[3], Xin[2] / Xin[3], 1.0f) : make_float4(0.0f, 0.0f, 1.0f, 1.0f);
}

__device__ __forceinline__ void load_cams(const float *s, AdjustCams &c)
{
    float v[kAdjPoseWords];
#pragma unroll
    for (int k = 0; k < kAdjPoseWords; ++k) v[k] = uniform(s[k]);
    adjust_load_cams(v, c);
}

// one compact point of the solve: a lane past the end reads nothing and holds a harmless point seen by view 1 alone
struct AdjustPoint { float obs[6]; float X[3]; int bits; };

__device__ __forceinline__ AdjustPoint load_point(const AdjustArgs &a, const float4 *Xc, int k, bool live)
{
    AdjustPoint p = { { 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f }, { 0.0f, 0.0f, 1.0f }, kAdjView1 };
    if (live) {
        const float4 o = a.cobs12[k], X = Xc[k];
        const float2 o3 = a.cobs3[k];
        p.obs[0] = o.x; p.obs[1] = o.y; p.obs[2] = o.z; p.obs[3] = o.w; p.obs[4] = o3.x; p.obs[5] = o3.y;
        p.X[0] = X.x; p.X[1] = X.y; p.X[2] = X.z;
        p.bits = a.cbits[k];
    }
    return p;
}

// One lane: the damped 11 x 11 system from the totals, its Cholesky in place in LDS, the tentative state and the step as floats.
// False: not positive definite.  Inlined: as a called function it costs the kernel a stack in scratch (156 bytes); inlined, the
// unrolled factorisation is held in registers (the kernel reports 256 VGPRs, its whole budget at 512 threads, and no scratch).
__device__ __forceinline__ bool adjust_step_lane(double lambda, const double *s_tot, double *s_S, double *s_x, const float *s_pose, float *s_try, float *s_dc)
{
    for (int q = 0; q < kAdjS; ++q) s_S[q] = s_tot[q];
    for (int q = 0; q < kAdjCam; ++q) { s_S[symn<kAdjCam>(q, q)] += lambda * s_tot[kAdjU + q]; s_x[q] = -s_tot[kAdjB + q]; }
    if (!refine_cholesky<kAdjCam>(s_S, s_x)) return false;
    double dc[kAdjCam];
    float s[kAdjPoseWords], o[kAdjPoseWords];
#pragma unroll
    for (int q = 0; q < kAdjCam; ++q) { dc[q] = s_x[q]; s_dc[q] = (float)dc[q]; }
#pragma unroll
    for (int q = 0; q < kAdjPoseWords; ++q) s[q] = s_pose[q];
    adjust_camera_step(dc, s, o);
#pragma unroll
    for (int q = 0; q < kAdjPoseWords; ++q) s_try[q] = o[q];
    return true;
}

__device__ __forceinline__ void adjust_solve_block(const AdjustArgs &a)
{
    __shared__ double s_part[kAdjWaves * kAdjValues];
    __shared__ double s_tot[kAdjValues];
    __shared__ double s_S[kAdjS], s_x[kAdjCam];
    __shared__ float s_pose[kAdjPoseWords], s_try[kAdjPoseWords], s_dc[kAdjCam];
    __shared__ int s_scan[kAdjWaves + 1];
    __shared__ int s_go;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const RefineCam K = { uniform(a.K[0]), uniform(a.K[1]), uniform(a.K[4]) };

    if (tid == 0) {
        float P2[12], P3[12], s[kAdjPoseWords];
        view_points_pose(a.pose2, a.pose_rows, P2);
        view_points_pose(a.pose3, a.pose_rows, P3);
        adjust_start_state(P2, P3, s);
#pragma unroll
        for (int k = 0; k < kAdjPoseWords; ++k) s_pose[k] = s[k];
    }
    __syncthreads();

    // ---- used set, compacted in record order ----
    int m = 0;
    for (int base = 0; base < a.n; base += kAdjThreads) {
        const int j = base + tid;
        const int bits = j < a.n ? (int)a.out_views[j] : 0;
        const int k = m + block_scan<kAdjWaves>(bits ? 1 : 0, s_scan);
        m += s_scan[kAdjWaves];
        if (j < a.n) {
            a.slot[j] = bits ? k : -1;
            if (bits) { a.cobs12[k] = a.obs12[j]; a.cobs3[k] = a.obs3[j]; a.Xa[k] = a.start[j]; a.cbits[k] = (uint8_t)bits; }
        }
        __syncthreads();                                  // s_scan is read above and rewritten by the next round; orders the compact stores too
    }
    AdjustCams P;
    load_cams(s_pose, P);
    const float huber = a.huber;

    // ---- cost of the start, and how many records views 2 and 3 see ----
    {
        double v[4] = { 0.0, 0.0, 0.0, 0.0 };
        for (int k = tid; k < m; k += kAdjThreads) {
            const AdjustPoint p = load_point(a, a.Xa, k, true);
            float cost, sq;
            adjust_cost(K, P, p.obs, p.X, p.bits, huber, cost, sq);
            v[0] += (double)cost; v[1] += (double)sq;
            v[2] += (p.bits & kAdjView2) ? 1.0 : 0.0; v[3] += (p.bits & kAdjView3) ? 1.0 : 0.0;
        }
        block_sum<kAdjWaves>(v, s_part, s_tot);
    }
    const int n2 = (int)s_tot[2], n3 = (int)s_tot[3];
    const double terms = 2.0 * ((double)m + (double)n2 + (double)n3);
    LmControl lm(a.lambda0, s_tot[0], s_tot[1], n2 < kAdjMinView2 || n3 < kAdjMinView3);
    const float initial_rms = m > 0 ? (float)sqrt(lm.sq / terms) : 0.0f;
    int cur = 0;                                          // Xa (0) or Xb (1) holds the committed points
    __syncthreads();                                      // s_tot has been read

    while (lm.running(a.max_iter)) {
        const float lam = uniform((float)lm.lambda);
        const float4 *Xc = cur ? a.Xb : a.Xa;
        float4 *Xn = cur ? a.Xa : a.Xb;
        // ---- pass A: the reduced camera system, transposed: lane q keeps the wavefront's sums q and q + 64 ----
        double acc0 = 0.0, acc1 = 0.0;
        for (int base = wave * 64; base < m; base += kAdjThreads) {       // the same trip count in every lane of a wavefront
            const bool live = base + lane < m;
            const AdjustPoint p = load_point(a, Xc, base + lane, live);
            AdjustJac J;
            adjust_jacobian(K, P, p.obs, p.X, p.bits, J);
            float w[3], cost = 0.0f, sq = 0.0f, Vi[6], Wm[3 * kAdjCam], gp[3];
            adjust_weights(J.r, p.bits, huber, w, cost, sq);
            adjust_point_block(J, w, lam, Vi, Wm, gp);
            float vals[kAdjValues];
            adjust_schur(J, w, Vi, Wm, gp, [&](int q, float v) { vals[q] = live ? v : 0.0f; });
            acc0 += wave_transpose_sum<64>(vals, lane);
            acc1 += wave_transpose_sum<kAdjValues - 64>(vals + 64, lane);
        }
        s_part[wave * kAdjValues + lane] = acc0;
        if (lane < kAdjValues - 64) s_part[wave * kAdjValues + 64 + lane] = acc1;
        __syncthreads();
        if (tid < kAdjValues) {
            double s = s_part[tid];
            for (int w = 1; w < kAdjWaves; ++w) s += s_part[w * kAdjValues + tid];
            s_tot[tid] = s;
        }
        __syncthreads();
        // ---- the camera step on one lane, the system in LDS ----
        if (tid == 0) s_go = adjust_step_lane(lm.lambda, s_tot, s_S, s_x, s_pose, s_try, s_dc) ? 1 : 0;
        __syncthreads();
        if (!s_go) {                                      // not positive definite: more damping
            if (!lm.solve_failed()) break;
            continue;
        }
        // ---- pass B: point steps and the cost of the tentative state ----
        AdjustCams Pt;
        load_cams(s_try, Pt);
        float dc[kAdjCam];
#pragma unroll
        for (int q = 0; q < kAdjCam; ++q) dc[q] = uniform(s_dc[q]);
        double v[2] = { 0.0, 0.0 };
        for (int k = tid; k < m; k += kAdjThreads) {
            const AdjustPoint p = load_point(a, Xc, k, true);
            AdjustJac J;
            adjust_jacobian(K, P, p.obs, p.X, p.bits, J);
            float w[3], cost = 0.0f, sq = 0.0f, Vi[6], Wm[3 * kAdjCam], gp[3], dp[3];
            adjust_weights(J.r, p.bits, huber, w, cost, sq);
            adjust_point_block(J, w, lam, Vi, Wm, gp);
            adjust_point_step(Vi, Wm, gp, dc, dp);
            const float Xt[3] = { p.X[0] + dp[0], p.X[1] + dp[1], p.X[2] + dp[2] };
            Xn[k] = make_float4(Xt[0], Xt[1], Xt[2], 1.0f);
            adjust_cost(K, Pt, p.obs, Xt, p.bits, huber, cost, sq);
            v[0] += (double)cost; v[1] += (double)sq;
        }
        block_sum<kAdjWaves>(v, s_part, s_tot);
        const double nc = s_tot[0], nsq = s_tot[1];
        bool stop;
        const bool commit = lm.tentative(nc, nsq, (double)a.min_rel, stop);
        __syncthreads();                                  // every lane has read s_tot, s_pose and s_try for this iteration
        if (commit) {
            cur ^= 1;
            P = Pt;
            if (tid < kAdjPoseWords) s_pose[tid] = s_try[tid];
            __syncthreads();
        }
        if (stop) break;
    }

    // ---- the adjusted poses, the report; the committed points into Xa for the scatter kernel ----
    if (tid == 0) {
#pragma unroll
        for (int q = 0; q < 12; ++q) { a.out_poses[q] = s_pose[q]; a.out_poses[12 + q] = s_pose[18 + q]; }
        sfm_adjust_report rep;
        rep.status = lm.status; rep.iterations = lm.iters; rep.accepted = lm.accepted;
        rep.num_points = m; rep.num_view2 = n2; rep.num_view3 = n3;
        rep.initial_rms_px = initial_rms;
        rep.final_rms_px = m > 0 ? (float)sqrt(lm.sq / terms) : 0.0f;
        rep.final_cost = (float)lm.cost;
        rep.lambda = (float)lm.lambda;
        *a.out_report = rep;
    }
    if (cur) {
        for (int k = tid; k < m; k += kAdjThreads) a.Xa[k] = a.Xb[k];
    }
}

__device__ __forceinline__ void adjust_scatter_block(const AdjustArgs &a, const int block)
{
    const int j = block * kAdjGrid + threadIdx.x;
    if (j >= a.n) return;
    const int bits = a.out_views[j];
    const bool degenerate = a.out_report->status == SFM_REFINE_DEGENERATE;
    float out[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) out[c] = a.points[(size_t)c * a.n + j];
    float err = __builtin_inff();
    if (bits) {
        const float4 X4 = a.Xa[a.slot[j]];
        const float X[3] = { X4.x, X4.y, X4.z };
        if (!degenerate) { out[0] = X[0]; out[1] = X[1]; out[2] = X[2]; out[3] = 1.0f; }
        if (a.out_err) {
            const RefineCam K = { a.K[0], a.K[1], a.K[4] };
            const float4 o = a.obs12[j];
            const float2 o3 = a.obs3[j];
            const float obs[6] = { o.x, o.y, o.z, o.w, o3.x, o3.y };
            float P2[12], P3[12];
#pragma unroll
            for (int q = 0; q < 12; ++q) { P2[q] = a.out_poses[q]; P3[q] = a.out_poses[12 + q]; }      // (inside a divergent branch: plain loads)
            err = adjust_error(K, P2, P3, obs, X, bits);
        }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) a.out_points[(size_t)c * a.n + j] = out[c];
    if (a.out_err) a.out_err[j] = err;
}

__global__ __launch_bounds__(kAdjGrid)
void adjust_gather_kernel(AdjustArgs a) { adjust_gather_block(a, blockIdx.x); }

__global__ __launch_bounds__(kAdjThreads)
void adjust_solve_kernel(AdjustArgs a) { adjust_solve_block(a); }

__global__ __launch_bounds__(kAdjGrid)
void adjust_scatter_kernel(AdjustArgs a) { adjust_scatter_block(a, blockIdx.x); }

// ---- many pairs: job blockIdx.y (gather, scatter) / blockIdx.x (solve) of `jobs` ----
__device__ __forceinline__ AdjustArgs load_job(const AdjustArgs *__restrict__ jobs, const unsigned int job)
{
    AdjustArgs a = jobs[job];
    a.sift = global_ptr(a.sift); a.X0 = global_ptr(a.X0); a.X1 = global_ptr(a.X1); a.K = global_ptr(a.K); a.Kinv = global_ptr(a.Kinv);
    a.points = global_ptr(a.points); a.flags = global_ptr(a.flags); a.used2 = global_ptr(a.used2);
    a.pose2 = global_ptr(a.pose2); a.pose3 = global_ptr(a.pose3);
    a.obs12 = global_ptr(a.obs12); a.start = global_ptr(a.start); a.obs3 = global_ptr(a.obs3); a.slot = global_ptr(a.slot);
    a.cobs12 = global_ptr(a.cobs12); a.Xa = global_ptr(a.Xa); a.Xb = global_ptr(a.Xb); a.cobs3 = global_ptr(a.cobs3); a.cbits = global_ptr(a.cbits);
    a.out_poses = global_ptr(a.out_poses); a.out_points = global_ptr(a.out_points); a.out_views = global_ptr(a.out_views);
    a.out_err = global_ptr(a.out_err); a.out_report = global_ptr(a.out_report);
    return a;
}

__global__ __launch_bounds__(kAdjGrid)
void adjust_gather_views_kernel(const AdjustArgs *__restrict__ jobs)
{
    const AdjustArgs a = load_job(jobs, blockIdx.y);
    adjust_gather_block(a, blockIdx.x);                   // a block past the pair's records has no live lane (no barrier inside)
}

__global__ __launch_bounds__(kAdjThreads)
void adjust_solve_views_kernel(const AdjustArgs *__restrict__ jobs)
{
    const AdjustArgs a = load_job(jobs, blockIdx.x);
    adjust_solve_block(a);
}

__global__ __launch_bounds__(kAdjGrid)
void adjust_scatter_views_kernel(const AdjustArgs *__restrict__ jobs)
{
    const AdjustArgs a = load_job(jobs, blockIdx.y);
    adjust_scatter_block(a, blockIdx.x);
}

// pair->d_awork for cap_points records: the arrays of `a` inside it; returns its size in bytes
static size_t adjust_work_layout(void *buffer, int cap_points, AdjustArgs &a)
{
    const size_t cap = (size_t)cap_points;
    Carver w(buffer);
    a.obs12 = w.take<float4>(cap);
    a.start = w.take<float4>(cap);
    a.cobs12 = w.take<float4>(cap);
    a.Xa = w.take<float4>(cap);
    a.Xb = w.take<float4>(cap);
    a.obs3 = w.take<float2>(cap);
    a.cobs3 = w.take<float2>(cap);
    a.slot = w.take<int>(cap);
    a.cbits = w.take<uint8_t>(cap);
    return w.used;
}

size_t adjust_work_bytes(int cap_points)
{
    AdjustArgs a;
    return adjust_work_layout(nullptr, cap_points, a);
}

static void adjust_args(sfm_pair *pair, const AdjustInputs &in, const sfm_adjust_params &p, const sfm_adjust_out &out, AdjustArgs &a)
{
    a.sift = in.sift;
    a.X0 = pair->d_X[0]; a.X1 = pair->d_X[1];
    a.K = pair->d_K; a.Kinv = pair->d_Kinv;
    a.points = in.points; a.flags = in.flags; a.used2 = in.used2;
    a.pose2 = in.pose2; a.pose3 = in.pose3; a.pose_rows = in.pose_rows;
    a.ld = pair->ld; a.n = pair->n;
    a.huber = p.huber_px; a.min_rel = p.min_rel_decrease; a.lambda0 = p.initial_lambda; a.max_iter = p.max_iterations;
    adjust_work_layout(pair->d_awork, pair->cap_points, a);
    a.out_poses = out.d_poses; a.out_points = out.d_points; a.out_views = out.d_views; a.out_err = out.d_err; a.out_report = out.d_report;
}

int launch_adjust(sfm_pair *pair, const AdjustInputs &in, const sfm_adjust_params &p, const sfm_adjust_out &out)
{
    AdjustArgs a;
    adjust_args(pair, in, p, out, a);
    hipStream_t st = pair->ctx->stream;
    const int nb = (pair->n + kAdjGrid - 1) / kAdjGrid;
    if (nb > 0) {
        hipLaunchKernelGGL(adjust_gather_kernel, dim3(nb), dim3(kAdjGrid), 0, st, a);
        SFM_HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(adjust_solve_kernel, dim3(1), dim3(kAdjThreads), 0, st, a);
    SFM_HIP_TRY(hipGetLastError());
    if (nb > 0) {
        hipLaunchKernelGGL(adjust_scatter_kernel, dim3(nb), dim3(kAdjGrid), 0, st, a);
        SFM_HIP_TRY(hipGetLastError());
    }
    return SFM_OK;
}

int launch_adjust_views(sfm_ctx *ctx, sfm_pair *const *pairs, int num_pairs, const AdjustInputs *in, const sfm_adjust_params &p, const sfm_adjust_out *outs)
{
    hipStream_t st = ctx->stream;
    const AdjustArgs *d_jobs = nullptr;
    int nmax = 0;                                         // long chains first: the solve blocks are dispatched in job order
    const int rc = job_array_stage(ctx->adjust_jobs, num_pairs, st, [&](int i) { return pairs[i]->n; },
                                   [&](AdjustArgs &job, int i) { adjust_args(pairs[i], in[i], p, outs[i], job); }, &d_jobs, &nmax);
    if (rc != SFM_OK) return rc;
    const int nb = (nmax + kAdjGrid - 1) / kAdjGrid;
    if (nb > 0) {
        hipLaunchKernelGGL(adjust_gather_views_kernel, dim3(nb, num_pairs), dim3(kAdjGrid), 0, st, d_jobs);
        SFM_HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(adjust_solve_views_kernel, dim3(num_pairs), dim3(kAdjThreads), 0, st, d_jobs);
    SFM_HIP_TRY(hipGetLastError());
    if (nb > 0) {
        hipLaunchKernelGGL(adjust_scatter_views_kernel, dim3(nb, num_pairs), dim3(kAdjGrid), 0, st, d_jobs);
        SFM_HIP_TRY(hipGetLastError());
    }
    return SFM_OK;
}

} // namespace sfm
