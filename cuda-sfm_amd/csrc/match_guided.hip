// match_guided.hip -- sfm_match_guided: the exact fp32 MFMA matcher of match.hip behind an epipolar gate, and sfm_pair_fundamental.
//
// Every score is match.hip's (v_mfma_f32_32x32x2_f32, the d = 0..127 fused chain); what changes is which scores reach the running
// top-2: an accumulator element of query p1 and database row p2 is pushed as it is when the pair lies in the band of F
// (match_guided_math.hpp: guided_pass) and as -inf otherwise.  With top2_push's v_med3 form -inf leaves best, second and index
// alone (best >= second >= 0 > -inf, and -inf never wins), so the push stays branch-free.
//
// Per lane and column tile: the query's line F u1 and its limit lim1, formed once in the prologue (0 for a query past the end).
// Per staged database row: (x2, y2, lim2), formed ONCE per row per stage by the threads that stage the row's descriptor and kept
// in LDS next to the descriptor tile (64 rows x 16 bytes per buffer, 2 KiB for both); the epilogue reads it as a broadcast (all
// lanes of a k-parity half look at the same row).  The gate is then one residual (2 fma), its square, two compares and a select
// per element.
//
// Configurations: (1,4) and (1,8) of match.hip's plan.  The (2,8) configuration is NOT instantiated: the plain kernel takes 254
// of the 256 registers a wavefront can have there, and the gated fold needs its lines, rows and residuals on top -- every
// arrangement tried (lines parked in LDS, positions requested after the MFMA loop, descriptors stored before the fold, scheduling
// barriers in the fold) left 64 to 560 bytes of scratch per lane.  Calls with n1 > 11000 run (1,8), which the plan's table puts
// within 3 to 10 % of (2,8).
//
// The merge is the ticket merge only: no block ever waits for another one.
#include "match_guided_device.hpp"

namespace sfm {

// block (qblock, split) of grid (query blocks, database splits); the schedule is match_guided_body.inc, shared with the
// many-matches kernel of match_guided_pairs.hip
template <int CT, int W>
__global__ __launch_bounds__(W * 64)
void match_guided_kernel(sfm_sift_point *__restrict__ sift1, int nq, const sfm_sift_point *__restrict__ sift2, int ndb,
                         int rows_per_split, const float *__restrict__ d_F, float band,
                         float *__restrict__ ws_best, float *__restrict__ ws_second, int *__restrict__ ws_idx,
                         unsigned int *__restrict__ tickets)
{
    const int qblock = (int)blockIdx.x, split = (int)blockIdx.y, nsplit = (int)gridDim.y;
#include "match_guided_body.inc"
}

int launch_match_guided(sfm_ctx *ctx, sfm_sift_point *sift1, int n1, const sfm_sift_point *sift2, int n2, const float *d_F, float band_px)
{
    if (n1 <= 0 || n2 <= 0) return SFM_OK;
    const ExactMatchPlan plan = exact_match_plan(ctx->num_cus, n1, n2, 1);      // (no two-tile configuration: see the top of the file)
    unsigned int *tickets; float *wb, *wsnd; int *wi;
    const int wrc = match_partials_workspace(ctx, plan.qblocks, plan.nsplit, n1, &tickets, &wb, &wsnd, &wi);
    if (wrc != SFM_OK) return wrc;
    const dim3 grid(plan.qblocks, plan.nsplit);
#define SFM_GUIDED_LAUNCH(CT_, W_)                                                                                   \
    hipLaunchKernelGGL((match_guided_kernel<CT_, W_>), grid, dim3(W_ * 64), 0, ctx->stream,                          \
                       sift1, n1, sift2, n2, plan.rows_per_split, d_F, band_px, wb, wsnd, wi, tickets)
    if (plan.wv == 8) SFM_GUIDED_LAUNCH(1, 8);
    else SFM_GUIDED_LAUNCH(1, 4);
#undef SFM_GUIDED_LAUNCH
    SFM_HIP_TRY(hipGetLastError());
    return SFM_OK;
}

// sfm_pair_fundamental on one lane.  estimateE's E has X0^T E X1 = 0 with X0 = Kinv (xpos, ypos, 1) and X1 = Kinv (match_xpos,
// match_ypos, 1) (device_math.hpp: residual), so u2^T F u1 = 0 needs its transpose; the refined E = [t]x R has X1^T E X0 = 0
// (X1 = R X0 + t) and is taken as it is.
__global__ __launch_bounds__(64)
void pair_fundamental_kernel(const float *__restrict__ E, const float *__restrict__ Kinv, int transpose, float *__restrict__ F)
{
    if (threadIdx.x != 0) return;
    float e[9], k[9], f[9];
    for (int i = 0; i < 9; ++i) { e[i] = E[i]; k[i] = Kinv[i]; }
    guided_fundamental(e, k, transpose != 0, f);
    for (int i = 0; i < 9; ++i) F[i] = f[i];
}

int launch_pair_fundamental(sfm_pair *pair, int refined, float *d_F)
{
    const float *E = refined ? pair->d_rstate + refine_pose_offset() + 16 : pair->d_E;
    hipLaunchKernelGGL(pair_fundamental_kernel, dim3(1), dim3(64), 0, pair->ctx->stream, E, pair->d_Kinv, refined ? 0 : 1, d_F);
    SFM_HIP_TRY(hipGetLastError());
    return SFM_OK;
}

} // namespace sfm
