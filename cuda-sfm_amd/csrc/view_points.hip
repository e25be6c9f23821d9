// view_points.hip -- sfm_triangulate_view / sfm_triangulate_views (gfx950): the pair's points triangulated and refined over the
// pair's two cameras and its registered view.  Arithmetic: view_points_math.hpp (shared with the host build of the CPU tests).
//
// One launch, one lane per point, blocks of 256: the lane reads its record (an 8-byte and a 16-byte load), its observations and
// its input column, classifies the point (SFM_VP_*), runs the DLT where the point is new, the point LM and the acceptance test,
// and writes its column, flag and error.  The class counts are reduced per block (a ballot per class and wavefront, the wave
// counts through LDS) and added with one integer atomic per block and class into a buffer the launcher zeroes on the stream: the
// counts do not depend on the order of arrival, and no float is ever added atomically.
//
// Divergence.  The DLT (eight Jacobi sweeps on a 4 x 4, about 4k instructions -- refine.hip) is needed by the new points only.  The
// block's new points are compacted with block_scan, their four observation values staged through LDS, the DLT runs on the dense
// lanes 0 .. count-1 and the start points go back through LDS to the lanes that own them.  The plain form -- the DLT in place on
// every lane with a new point, a wavefront paying for it when any of its lanes does -- was written too, gave the same bytes and
// was measured against this one (profiles/view_points_bench.txt): 19-24 % slower in the batched call, 3-4 % faster per single
// call on the synthetic scenes, 19 % slower per single call on the dino ring.  It is not kept.
//
// Many pairs in one call (launch_view_points_views): the same body over an array of ViewPointsArgs in device memory, grid
// (point blocks of the largest job, jobs).  A block past its job's points loads nothing and stores nothing but still runs to
// the last barrier.
#include "common.hpp"
#include "device_math.hpp"
#include "block_ops.hpp"
#include "view_points_math.hpp"
#include <math.h>

namespace sfm {

constexpr int kVpThreads = 256;
constexpr int kVpWaves = kVpThreads / 64;
constexpr int kVpClasses = 5;
// ONE register budget for the single-pair kernel and its batched twin: left alone, the batched kernel's job load costs it one more
// VGPR (107 against 106); under the same cap both come out at 106 (104 + the lanes that hold spilled SGPRs), no scratch
#define SFM_VP_KERNEL __global__ __launch_bounds__(kVpThreads) __attribute__((amdgpu_num_vgpr(104)))

__device__ __forceinline__ void view_points_block(const ViewPointsArgs &a)
{
    __shared__ int s_cnt[kVpWaves][kVpClasses];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = blockIdx.x * kVpThreads + tid;
    const bool live = j < a.n;

    ViewPointsCams c;
    c.K = RefineCam{ uniform(a.K[0]), uniform(a.K[1]), uniform(a.K[4]) };
#pragma unroll
    for (int q = 0; q < 9; ++q) c.Kinv[q] = uniform(a.Kinv[q]);
    {
        float P[12];
        view_points_pose(a.pose2, a.pose_rows, P);
#pragma unroll
        for (int q = 0; q < 12; ++q) c.P2[q] = uniform(P[q]);
        view_points_pose(a.pose3, a.pose_rows, P);
#pragma unroll
        for (int q = 0; q < 12; ++q) c.P3[q] = uniform(P[q]);
    }

    ViewPointsLane L;
    L.seen = false; L.usable = false;
#pragma unroll
    for (int q = 0; q < 6; ++q) L.obs[q] = 0.0f;
#pragma unroll
    for (int q = 0; q < 4; ++q) L.Xin[q] = 0.0f;
    if (live) view_points_load(a, c.Kinv, j, L);
    const bool fresh = live && L.seen && !L.usable;      // a new point: the DLT's

    float start[3] = { 0.0f, 0.0f, 0.0f };
    bool start_ok = false;
    {
        __shared__ int s_scan[kVpWaves + 1];
        __shared__ float4 s_obs[kVpThreads], s_start[kVpThreads];
        const int k = block_scan<kVpWaves>(fresh ? 1 : 0, s_scan);
        const int count = s_scan[kVpWaves];
        if (fresh) s_obs[k] = make_float4(L.obs[0], L.obs[1], L.obs[4], L.obs[5]);
        __syncthreads();
        if (tid < count) {
            const float4 o = s_obs[tid];
            float X[3];
            const bool ok = view_points_dlt(o.x, o.y, o.z, o.w, c.P3, X);
            s_start[tid] = make_float4(X[0], X[1], X[2], ok ? 1.0f : 0.0f);
        }
        __syncthreads();
        if (fresh) {
            const float4 s = s_start[k];
            start[0] = s.x; start[1] = s.y; start[2] = s.z;
            start_ok = s.w != 0.0f;
        }
    }

    int cls = -1;
    if (live) {
        float out[4], err;
        cls = view_points_finish(c, a, L, start_ok, start, out, err);
#pragma unroll
        for (int q = 0; q < 4; ++q) a.out_points[(size_t)q * a.n + j] = out[q];
        a.out_flags[j] = (uint8_t)cls;
        if (a.out_err) a.out_err[j] = err;
    }

    // ---- the class counts: per wavefront by ballot, per block through LDS, one integer atomic per block and class ----
#pragma unroll
    for (int q = 0; q < kVpClasses; ++q) {
        const int m = __popcll(__ballot(cls == q));
        if (lane == 0) s_cnt[wave][q] = m;
    }
    __syncthreads();
    if (tid < kVpClasses && a.out_counts) {
        int m = 0;
        for (int w = 0; w < kVpWaves; ++w) m += s_cnt[w][tid];
        if (m) atomicAdd(&a.out_counts[tid], m);
    }
}

SFM_VP_KERNEL
void view_points_kernel(ViewPointsArgs a) { view_points_block(a); }

// the block's job (blockIdx.y), through a uniform address, every pointer marked global (block_ops.hpp)
__device__ __forceinline__ ViewPointsArgs load_job(const ViewPointsArgs *__restrict__ jobs, const unsigned int job)
{
    ViewPointsArgs a = jobs[job];
    a.sift = global_ptr(a.sift); a.X0 = global_ptr(a.X0); a.X1 = global_ptr(a.X1); a.K = global_ptr(a.K); a.Kinv = global_ptr(a.Kinv);
    a.points = global_ptr(a.points); a.valid = global_ptr(a.valid); a.pose2 = global_ptr(a.pose2); a.pose3 = global_ptr(a.pose3);
    a.out_points = global_ptr(a.out_points); a.out_flags = global_ptr(a.out_flags); a.out_err = global_ptr(a.out_err);
    a.out_counts = global_ptr(a.out_counts);
    return a;
}

// Every block runs the body to its last barrier: one past its job's points has no live lane and leaves nothing behind.
SFM_VP_KERNEL
void view_points_views_kernel(const ViewPointsArgs *__restrict__ jobs)
{
    const ViewPointsArgs a = load_job(jobs, blockIdx.y);
    view_points_block(a);
}

static void view_points_args(sfm_pair *pair, const ViewPointsInputs &in, const sfm_view_points_params &p, const sfm_view_points_out &out, ViewPointsArgs &a)
{
    a.sift = in.sift;
    a.X0 = pair->d_X[0]; a.X1 = pair->d_X[1];
    a.K = pair->d_K; a.Kinv = pair->d_Kinv;
    a.points = in.points; a.valid = in.valid;
    a.pose2 = in.pose2; a.pose3 = in.pose3; a.pose_rows = in.pose_rows;
    a.ld = pair->ld; a.n = pair->n;
    a.min_score = p.min_score; a.max_ambiguity = p.max_ambiguity;
    a.thr = p.threshold_px;
    a.cos_min = view_points_cos_min(p.min_parallax_deg);
    a.max_iter = p.max_iterations; a.huber = p.huber_px; a.min_rel = p.min_rel_decrease; a.lambda0 = p.initial_lambda;
    a.out_points = out.d_points; a.out_flags = out.d_flags; a.out_err = out.d_err; a.out_counts = out.d_counts;
}

int launch_view_points(sfm_pair *pair, const ViewPointsInputs &in, const sfm_view_points_params &p, const sfm_view_points_out &out)
{
    ViewPointsArgs a;
    view_points_args(pair, in, p, out, a);
    hipStream_t st = pair->ctx->stream;
    if (out.d_counts) SFM_HIP_TRY(hipMemsetAsync(out.d_counts, 0, 8 * sizeof(int32_t), st));
    if (pair->n == 0) return SFM_OK;
    hipLaunchKernelGGL(view_points_kernel, dim3((pair->n + kVpThreads - 1) / kVpThreads), dim3(kVpThreads), 0, st, a);
    SFM_HIP_TRY(hipGetLastError());
    return SFM_OK;
}

int launch_view_points_views(sfm_ctx *ctx, sfm_pair *const *pairs, int num_pairs, const ViewPointsInputs *in, const sfm_view_points_params &p,
                             const sfm_view_points_out *outs)
{
    hipStream_t st = ctx->stream;
    const ViewPointsArgs *d_jobs = nullptr;
    int nmax = 0;                                         // large pairs first (the blocks of a job are dispatched in job order)
    const int rc = job_array_stage(ctx->view_points_jobs, num_pairs, st, [&](int i) { return pairs[i]->n; },
                                   [&](ViewPointsArgs &job, int i) { view_points_args(pairs[i], in[i], p, outs[i], job); }, &d_jobs, &nmax);
    if (rc != SFM_OK) return rc;
    // the count buffers: one memset per run of buffers that follow each other in memory (ONE when the caller keeps them in one array)
    for (int i = 0; i < num_pairs;) {
        int32_t *first = outs[i].d_counts;
        int run = 1;
        while (first && i + run < num_pairs && outs[i + run].d_counts == first + 8 * (size_t)run) ++run;
        if (first) SFM_HIP_TRY(hipMemsetAsync(first, 0, (size_t)run * 8 * sizeof(int32_t), st));
        i += run;
    }
    if (nmax == 0) return SFM_OK;
    hipLaunchKernelGGL(view_points_views_kernel, dim3((nmax + kVpThreads - 1) / kVpThreads, num_pairs), dim3(kVpThreads), 0, st, d_jobs);
    SFM_HIP_TRY(hipGetLastError());
    return SFM_OK;
}

} // namespace sfm
