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
#include "match_mfma.hpp"
#include "match_guided_math.hpp"

namespace sfm {

struct GuidedRow { float x, y, lim, pad; };          // one staged database row's position and limit (16 bytes in LDS)

// positions of the rows stage_load<W> requests (same clamped rows, unconditional loads)
template <int W>
__device__ __forceinline__ void stage_load_pos(const sfm_sift_point *__restrict__ sift2, int row0, int nrows, float2 (&pos)[16 / W])
{
    const int rr = threadIdx.x >> 4;
#pragma unroll
    for (int pass = 0; pass < 16 / W; ++pass) {
        const int row = min(row0 + pass * (4 * W) + rr, nrows - 1);
        pos[pass] = *reinterpret_cast<const float2 *>(&sift2[row].xpos);        // xpos, ypos: the record's first eight bytes
    }
}

// (x2, y2, lim2) of the rows stage_store<W> writes; lim2 = 0 for rows past the end and under an F that is not finite.  Every
// thread of a row's sixteen forms the value, the one that stages the row's first descriptor chunk stores it.
template <int W>
__device__ __forceinline__ void stage_store_pos(GuidedRow *side, const float2 (&pos)[16 / W], int row0, int nrows,
                                                const float (&F)[9], const bool f_ok, const float band)
{
    const int c8 = threadIdx.x & 15;
    const int rr = threadIdx.x >> 4;
#pragma unroll
    for (int pass = 0; pass < 16 / W; ++pass) {
        const int slot = pass * (4 * W) + rr;
        const bool real = row0 + slot < nrows;
        float lt[3];
        guided_line_t(F, pos[pass].x, pos[pass].y, lt);
        const float lim2 = real && f_ok ? guided_limit(lt, band) : 0.0f;
        if (c8 == 0) side[slot] = GuidedRow{ pos[pass].x, pos[pass].y, lim2, 0.0f };
    }
}

// stage_scores' gate: the lane's lines and limits against the stage's rows
template <int CT>
struct EpipolarGate {
    typedef GuidedRow Row;
    const GuidedRow *side;
    float l[CT][3], lim1[CT];
    __device__ __forceinline__ Row row(int slot) const { return side[slot]; }
    __device__ __forceinline__ float score(int ct, float s, const Row &r) const
    {
        return guided_pass(guided_residual(l[ct], r.x, r.y), lim1[ct], r.lim) ? s : -__builtin_inff();
    }
};

// block (qblock, split) of grid (query blocks, database splits): match_body's schedule (match.hip) with the rows' positions
// staged beside their descriptors
template <int CT, int W>
__global__ __launch_bounds__(W * 64)
void match_guided_kernel(sfm_sift_point *__restrict__ sift1, int nq, const sfm_sift_point *__restrict__ sift2, int ndb,
                         int rows_per_split, const float *__restrict__ d_F, float band,
                         float *__restrict__ ws_best, float *__restrict__ ws_second, int *__restrict__ ws_idx,
                         unsigned int *__restrict__ tickets)
{
    __shared__ __attribute__((aligned(16))) float lds[2][kRowsPerStage * kLdsStride];
    __shared__ __attribute__((aligned(16))) GuidedRow side[2][kRowsPerStage];
    constexpr int ld = (int)(sizeof(sfm_sift_point) / sizeof(float));
    const float *q = sift1->data;
    const float *db = sift2->data;
    const int qblock = (int)blockIdx.x, split = (int)blockIdx.y, nsplit = (int)gridDim.y;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int col = lane & 31;
    const int half = lane >> 5;
    const int q0 = qblock * (CT * 32 * W);
    const int row_begin = split * rows_per_split;
    const int row_end = min(ndb, row_begin + rows_per_split);

    float F[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) F[i] = d_F[i];        // (a uniform address: scalar loads)
    const bool f_ok = guided_finite(F);

    // the first database stage is requested before the prologue, as in match_body
    const int nstage = (row_end - row_begin + kRowsPerStage - 1) / kRowsPerStage;
    float4 dbregs[16 / W][2];
    float2 dbpos[16 / W];
    if (nstage > 0) { stage_load<W>(db, ld, row_begin, row_end, dbregs); stage_load_pos<W>(sift2, row_begin, row_end, dbpos); }

    // ---- prologue: the queries' lines and limits, then their resident fragments -------------------
    EpipolarGate<CT> gate;
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
        const int p1 = q0 + (wave * CT + ct) * 32 + col;
        const float2 u1 = *reinterpret_cast<const float2 *>(&sift1[min(p1, nq - 1)].xpos);
        guided_line(F, u1.x, u1.y, gate.l[ct]);
        gate.lim1[ct] = p1 < nq && f_ok ? guided_limit(gate.l[ct], band) : 0.0f;
    }
    float bq[CT][64];
    load_queries<CT, W>(q, nq, ld, q0, lds, bq);

    Top2 top[CT];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) { top[ct].best = 0.0f; top[ct].second = 0.0f; top[ct].idx = -1; }

    // ---- main loop over database stages of 64 rows ------------------------------------------
    float4 regs[16 / W][2];
    float2 pos[16 / W];
    if (nstage > 0) { stage_store<W>(lds[0], dbregs, row_begin, row_end); stage_store_pos<W>(side[0], dbpos, row_begin, row_end, F, f_ok, band); }
    __syncthreads();
    for (int s = 0; s < nstage; ++s) {
        const float *cur = lds[s & 1];
        gate.side = side[s & 1];
        const int next_row0 = row_begin + (s + 1) * kRowsPerStage;
        if (s + 1 < nstage) { stage_load<W>(db, ld, next_row0, row_end, regs); stage_load_pos<W>(sift2, next_row0, row_end, pos); }

        // a split is a multiple of 32 rows: its last stage may hold one row tile only (wave-uniform)
        const int stage_row0 = row_begin + s * kRowsPerStage;
        if (row_end - stage_row0 > 32) stage_scores<CT, 2>(cur, bq, top, stage_row0, gate);
        else stage_scores<CT, 1>(cur, bq, top, stage_row0, gate);

        if (s + 1 < nstage) { stage_store<W>(lds[(s + 1) & 1], regs, next_row0, row_end); stage_store_pos<W>(side[(s + 1) & 1], pos, next_row0, row_end, F, f_ok, band); }
        __syncthreads();
    }

    // ---- the ticket merge into the records of sift1 ------------------------------------------
    float *const out_best = nullptr, *const out_second = nullptr;
    int *const out_idx = nullptr;
#include "match_ticket_merge.inc"
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
