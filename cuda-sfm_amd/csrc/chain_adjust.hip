// chain_adjust.hip -- sfm_adjust_chain (gfx950): Levenberg-Marquardt bundle adjustment of every camera and every used track of a
// fused chain.  Arithmetic: chain_adjust_math.hpp (shared with the host build of the CPU tests); damping, accept test and stop
// rules: LmControl, one per segment, kept in device memory (ChainSeg) between the launches.
//
// A fixed launch sequence on the context's stream, no host synchronisation, no cooperative launch, no block that waits for
// another, no float atomics and no atomic on global memory at all (integer atomics on LDS count a head pair's tracks):
//   chain_init_kernel     one lane per pair: its block's start state from slot 2p + 1 of d_cams, the first track whose head pair
//                         is >= p (binary search: tracks are numbered by head pair), the counters cleared.
//   chain_used_kernel     one lane per track: the used test at the unified start cameras, the start point X / W.
//   chain_cost_kernel     one block per head pair (mode 0): the cost of the start, summed per head pair, and the head pair's counts
//                         (used tracks, their observations per local block, over-long tracks) by integer atomics on LDS.  (One
//                         atomicAdd per track on its segment's counters in global memory cost the used kernel 589 us at 630 pairs.)
//   chain_open_kernel     one lane per root: the segment's end, its counts from its head pairs', the degenerate decision, its
//                         LmControl.
// then max_iterations times
//   chain_system_kernel   one block per head pair, its wavefronts (chain_system_waves(W): as many partial bands as fit 64 KiB of LDS,
//                         four at the most) taking rounds of 64 of its tracks in turn: every lane forms its track's 6 x 6 block
//                         for the local block pair (a, b) -- the same (a, b) in all lanes -- and wave_transpose_sum adds the 36
//                         values over the wavefront in fp64; lane q adds value q into the wavefront's partial band in LDS; the
//                         wavefronts' bands are added in wave order.  A lane whose track has no view a or b contributes zeros.
//                         No per-lane array sized by W: a view's Jacobian is formed again where it is needed.  (One wavefront
//                         per head pair was the first form: 1088 us per launch at 630 pairs of 600 tracks, whatever the chain.)
//   chain_solve_kernel    one block per segment (a block whose pair is no root leaves at once): the partials of the head pairs
//                         added in ascending order, the damping, the banded Cholesky with one row of the current column per
//                         thread (two barriers per column), both substitutions column by column, the camera steps.
//   chain_cost_kernel     (mode 1) per track the back substitution and the cost of the tentative state, summed per head pair.
//   chain_accept_kernel   one lane per root: the head pairs' costs in ascending order, LmControl's decision; a commit flips the
//                         segment's state and point buffers.
// and at the end
//   chain_finish_kernel   one lane per track (column, used flag, error) and one per pair (cameras, report).
// A segment that has stopped or is degenerate falls through at the top of every block.  The order of every sum depends only on the
// track table, so two calls give the same bytes and a segment's bytes do not depend on the other segments.
#include "chain_adjust_device.hpp"            // ChainArgs, ChainTrackViews, the work layout: shared with ring_adjust.hip

namespace sfm {

constexpr int kChainSolveThreads = 128;   // >= 6 * kChainMaxViews: one row of a column's band per thread

__global__ __launch_bounds__(64)
void chain_init_kernel(ChainArgs a)
{
    const int p = blockIdx.x * 64 + threadIdx.x;
    if (p > a.k) return;
    const int T = chain_tracks(a);
    {   // the first track whose head pair is >= p
        int lo = 0, hi = T;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if ((a.obs_cam[a.track_offset[mid]] >> 1) < p) lo = mid + 1; else hi = mid;
        }
        a.head[p] = lo;
    }
    if (p == a.k) return;
    float P[12], s[kChainState];
#pragma unroll
    for (int q = 0; q < 12; ++q) P[q] = a.cams[(size_t)kFuseCams * p + 12 + q];
    chain_start_state(a.root[p] == p ? kChainRoot : kChainFree, P, s);
#pragma unroll
    for (int q = 0; q < kChainState; ++q) a.state[0][(size_t)kChainState * p + q] = s[q];
    a.seg[p] = ChainSeg();
}

__global__ __launch_bounds__(kChainTrackBlock)
void chain_used_kernel(ChainArgs a)
{
    const int t = blockIdx.x * kChainTrackBlock + threadIdx.x;
    if (t >= chain_tracks(a)) return;
    const int o0 = a.track_offset[t], count = a.track_offset[t + 1] - o0;
    const ChainTrackViews view = { a, a.state[0], a.obs_cam + o0, a.obs_record + o0 };
    float Xin[4], X[3] = { 0.0f, 0.0f, 1.0f };
#pragma unroll
    for (int c = 0; c < 4; ++c) Xin[c] = a.points[(size_t)c * a.N + t];
    const bool used = chain_used(a.flags[t], count, a.W, Xin, view, X);
    a.out.d_used[t] = used ? 1 : 0;
    a.X[0][t] = make_float4(X[0], X[1], X[2], 1.0f);
}

// mode 0: the cost of the start points under the start states.  mode 1: the back substitution of this iteration's camera steps
// into the other point buffer and the cost of the tentative state.  One block per head pair, every thread its tracks in order.
__global__ __launch_bounds__(kChainTrackBlock)
void chain_cost_kernel(ChainArgs a, int mode)
{
    __shared__ double s_part[(kChainTrackBlock / 64) * 2], s_tot[2];
    __shared__ int s_cnt[kChainCounts];
    const int h = blockIdx.x;
    if (!mode) {
        if (threadIdx.x < kChainCounts) s_cnt[threadIdx.x] = 0;
        __syncthreads();
    }
    const ChainSeg &seg = a.seg[a.root[h]];
    int cur = 0;
    float lam = 0.0f;
    if (mode) {
        if (!chain_running(seg, a.p.max_iterations) || !seg.go) return;
        cur = seg.cur;
        lam = (float)seg.lm.lambda;
    }
    const float huber = a.p.huber_px;
    const float *S = a.state[cur], *St = a.state[cur ^ 1];
    double v[2] = { 0.0, 0.0 };
    const int first = a.root[h] == h ? 1 : 0;            // local block 0 of a root's tracks is the fixed camera
    for (int t = a.head[h] + (int)threadIdx.x; t < a.head[h + 1]; t += kChainTrackBlock) {
        const int o0 = a.track_offset[t], count = a.track_offset[t + 1] - o0;
        if (!mode && count > a.W) atomicAdd(&s_cnt[2], 1);
        if (!a.out.d_used[t]) continue;
        if (!mode) {
            atomicAdd(&s_cnt[0], 1);
            atomicAdd(&s_cnt[1], count);
            for (int o = first; o < count; ++o) atomicAdd(&s_cnt[3 + o], 1);
        }
        const float4 X4 = a.X[cur][t];
        float X[3] = { X4.x, X4.y, X4.z }, cost, sq;
        if (mode) {
            const ChainTrackViews view = { a, S, a.obs_cam + o0, a.obs_record + o0 };
            float Vi[6], gp[3], dp[3];
            chain_point_block(count, view, huber, lam, X, Vi, gp);
            chain_point_step(count, view, [&](int o) { return a.dc + 6 * (size_t)view.block(o); }, huber, X, Vi, gp, dp);
            X[0] += dp[0]; X[1] += dp[1]; X[2] += dp[2];
            a.X[cur ^ 1][t] = make_float4(X[0], X[1], X[2], 1.0f);
        }
        const ChainTrackViews trial = { a, mode ? St : S, a.obs_cam + o0, a.obs_record + o0 };
        chain_cost(count, trial, huber, X, cost, sq);
        v[0] += (double)cost; v[1] += (double)sq;
    }
    block_sum<kChainTrackBlock / 64>(v, s_part, s_tot);
    if (threadIdx.x < 2) a.pcost[2 * (size_t)h + threadIdx.x] = s_tot[threadIdx.x];
    if (!mode && threadIdx.x < kChainCounts) a.hcnt[kChainCounts * (size_t)h + threadIdx.x] = s_cnt[threadIdx.x];      // (behind block_sum's barriers)
}

__global__ __launch_bounds__(64)
void chain_open_kernel(ChainArgs a)
{
    const int p = blockIdx.x * 64 + threadIdx.x;
    if (p >= a.k || a.root[p] != p) return;
    ChainSeg seg = a.seg[p];
    int end = p + 1;
    while (end < a.k && a.root[end] == p) ++end;
    bool degenerate = false;
    for (int q = p; q < end; ++q) {                       // block q's used observations: local block v of head pair q + 1 - v
        int n = 0;
        for (int v = 0; v < a.W; ++v) {
            const int h = q + 1 - v;
            if (h >= p && h < end) n += a.hcnt[kChainCounts * (size_t)h + 3 + v];
        }
        degenerate = degenerate || n < (q == p ? kAdjMinView2 : kAdjMinView3);
    }
    double cost = 0.0, sq = 0.0;
    for (int h = p; h < end; ++h) {
        cost += a.pcost[2 * (size_t)h]; sq += a.pcost[2 * (size_t)h + 1];
        seg.tracks += a.hcnt[kChainCounts * (size_t)h]; seg.obs += a.hcnt[kChainCounts * (size_t)h + 1]; seg.over += a.hcnt[kChainCounts * (size_t)h + 2];
    }
    seg.end = end;
    seg.lm = LmControl((double)a.p.initial_lambda, cost, sq, degenerate);
    seg.initial_rms = seg.obs > 0 ? (float)sqrt(sq / (2.0 * (double)seg.obs)) : 0.0f;
    a.seg[p] = seg;
}

__global__ __launch_bounds__(256)
void chain_system_kernel(ChainArgs a)
{
    extern __shared__ double s_all[];                     // chain_system_waves(W) x chain_part_values(W)
    const int h = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
    const int r = a.root[h];
    const ChainSeg &seg = a.seg[r];
    if (!chain_running(seg, a.p.max_iterations)) return;
    const int W = a.W, values = chain_part_values(W);
    double *s_band = s_all + (size_t)values * wave;       // this wavefront's partial band
    for (int q = lane; q < values; q += 64) s_band[q] = 0.0;
    __syncthreads();                                      // a value is zeroed by lane q % 64 and added to by lane q % 36 or q % 12 (every thread of the block is here)
    const int cur = seg.cur;
    const float lam = (float)seg.lm.lambda, huber = a.p.huber_px;
    const float *S = a.state[cur];
    const int a0 = r == h ? 1 : 0;                        // local block 0 of a root's tracks is the fixed camera
    const int t0 = a.head[h], t1 = a.head[h + 1];
    for (int base = t0 + 64 * wave; base < t1; base += 64 * waves) {      // the same trip counts in every lane of a wavefront
        const int t = base + lane;
        const bool live = t < t1 && a.out.d_used[t] != 0;
        int o0 = 0, count = 0;
        float X[3] = { 0.0f, 0.0f, 1.0f }, Vi[6], gp[3];
        if (live) {
            o0 = a.track_offset[t]; count = a.track_offset[t + 1] - o0;
            const float4 X4 = a.X[cur][t];
            X[0] = X4.x; X[1] = X4.y; X[2] = X4.z;
        }
        const ChainTrackViews view = { a, S, a.obs_cam + o0, a.obs_record + o0 };
        if (live) chain_point_block(count, view, huber, lam, X, Vi, gp);
        int most = count;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) most = max(most, __shfl_xor(most, off));
        for (int va = a0; va < most; ++va) {
            ChainJac Ja;
            float wa = 0.0f, Wa[18], Ta[18], bu[12];
            const bool ina = va < count;
            if (ina) {
                chain_jacobian(view(va), X, Ja);
                wa = chain_view_w(Ja, huber, Wa);
                chain_row_terms(Ja, wa, Wa, Vi, gp, Ta, bu);
            } else {
#pragma unroll
                for (int q = 0; q < 12; ++q) bu[q] = 0.0f;
            }
            const double rows = wave_transpose_sum<12>(bu, lane);
            if (lane < 6) s_band[chain_part_b(W) + 6 * va + lane] += rows;
            else if (lane < 12) s_band[chain_part_u(W) + 6 * va + lane - 6] += rows;
            for (int vb = va; vb < most; ++vb) {
                float blk[36];
                if (ina && vb < count) {
                    if (vb == va) chain_block_terms(Ja, wa, Ta, Wa, true, blk);
                    else {
                        ChainJac Jb;
                        float Wb[18];
                        chain_jacobian(view(vb), X, Jb);
                        chain_view_w(Jb, huber, Wb);
                        chain_block_terms(Ja, wa, Ta, Wb, false, blk);
                    }
                } else {
#pragma unroll
                    for (int q = 0; q < 36; ++q) blk[q] = 0.0f;
                }
                const double sum = wave_transpose_sum<36>(blk, lane);
                if (lane < 36) s_band[chain_part_block(W, va, vb) + lane] += sum;
            }
        }
    }
    __syncthreads();
    double *part = a.part + (size_t)values * h;
    for (int q = threadIdx.x; q < values; q += blockDim.x) {
        double s = s_all[q];
        for (int w = 1; w < waves; ++w) s += s_all[(size_t)values * w + q];
        part[q] = s;
    }
}

__global__ __launch_bounds__(kChainSolveThreads)
void chain_solve_kernel(ChainArgs a)
{
    __shared__ double s_d;
    __shared__ int s_ok;
    const int p0 = blockIdx.x, tid = threadIdx.x;
    if (a.root[p0] != p0) return;
    ChainSeg seg = a.seg[p0];
    if (!chain_running(seg, a.p.max_iterations)) return;
    const int W = a.W, p1 = seg.end, nb = p1 - p0, N = 6 * nb;
    double *B = a.band + (size_t)36 * W * p0, *x = a.x + (size_t)6 * p0, *du = a.du + (size_t)6 * p0;
    // ---- the head pairs' partials in ascending order ----
    for (int idx = tid; idx < nb * W * 36; idx += kChainSolveThreads) {
        const int e = idx % 36, d = (idx / 36) % W, pl = idx / (36 * W);
        B[idx] = pl + d < nb ? chain_reduce_block(a.part, W, p0, p1, pl, d, e) : 0.0;
    }
    for (int idx = tid; idx < N; idx += kChainSolveThreads) {
        x[idx] = -chain_reduce_row(a.part, W, p0, p1, idx / 6, idx % 6, false);
        du[idx] = chain_reduce_row(a.part, W, p0, p1, idx / 6, idx % 6, true);
    }
    __syncthreads();
    for (int idx = tid; idx < N; idx += kChainSolveThreads) {             // row 5: the unit row of the 5-dof block (its other entries are zero)
        const size_t at = chain_band_at(W, idx, idx);
        B[at] = idx == 5 ? 1.0 : B[at] + seg.lm.lambda * du[idx];
    }
    if (tid == 0) s_ok = 1;
    __syncthreads();
    // ---- the banded Cholesky: thread i owns row j + i of column j ----
    for (int j = 0; j < N; ++j) {
        const int row = j + tid;
        const bool mine = row <= chain_band_last(W, N, j);
        const double s = mine ? chain_band_dot(B, W, row, j) : 0.0;
        if (tid == 0) {
            if (!(s > 0.0)) s_ok = 0;
            s_d = sqrt(s);
        }
        __syncthreads();
        if (!s_ok) break;
        if (mine) B[chain_band_at(W, row, j)] = tid == 0 ? s_d : s / s_d;
        __syncthreads();
    }
    const bool ok = s_ok != 0;
    if (ok) {
        // ---- L L^T x = -b: forward by ascending columns, backward by descending ones ----
        for (int j = 0; j < N; ++j) {
            if (tid == 0) x[j] /= B[chain_band_at(W, j, j)];
            __syncthreads();
            const int row = j + 1 + tid;
            if (row <= chain_band_last(W, N, j)) x[row] -= B[chain_band_at(W, row, j)] * x[j];
            __syncthreads();
        }
        for (int j = N - 1; j >= 0; --j) {
            if (tid == 0) x[j] /= B[chain_band_at(W, j, j)];
            __syncthreads();
            const int i = chain_band_first(W, j) + tid;
            if (i < j) x[i] -= B[chain_band_at(W, j, i)] * x[j];
            __syncthreads();
        }
        // ---- the camera steps into the other state buffer ----
        for (int pl = tid; pl < nb; pl += kChainSolveThreads) {
            double dc[6];
            float s[kChainState], o[kChainState];
#pragma unroll
            for (int q = 0; q < 6; ++q) { dc[q] = x[6 * pl + q]; a.dc[6 * (size_t)(p0 + pl) + q] = (float)dc[q]; }
#pragma unroll
            for (int q = 0; q < kChainState; ++q) s[q] = a.state[seg.cur][(size_t)kChainState * (p0 + pl) + q];
            chain_camera_step(pl == 0 ? kChainRoot : kChainFree, dc, s, o);
#pragma unroll
            for (int q = 0; q < kChainState; ++q) a.state[seg.cur ^ 1][(size_t)kChainState * (p0 + pl) + q] = o[q];
        }
    }
    if (tid == 0) {
        seg.go = ok ? 1 : 0;
        if (!ok && !seg.lm.solve_failed()) seg.stopped = 1;       // not positive definite: more damping, or the end
        a.seg[p0] = seg;
    }
}

__global__ __launch_bounds__(64)
void chain_accept_kernel(ChainArgs a)
{
    const int p = blockIdx.x * 64 + threadIdx.x;
    if (p >= a.k || a.root[p] != p) return;
    ChainSeg seg = a.seg[p];
    if (!chain_running(seg, a.p.max_iterations) || !seg.go) return;
    double cost = 0.0, sq = 0.0;
    for (int h = p; h < seg.end; ++h) { cost += a.pcost[2 * (size_t)h]; sq += a.pcost[2 * (size_t)h + 1]; }
    bool stop;
    if (seg.lm.tentative(cost, sq, (double)a.p.min_rel_decrease, stop)) seg.cur ^= 1;
    if (stop) seg.stopped = 1;
    seg.go = 0;
    a.seg[p] = seg;
}

__global__ __launch_bounds__(kChainTrackBlock)
void chain_finish_kernel(ChainArgs a, int track_blocks)
{
    if ((int)blockIdx.x >= track_blocks) {                // ---- one lane per pair: its cameras and its report ----
        const int p = ((int)blockIdx.x - track_blocks) * kChainTrackBlock + threadIdx.x;
        if (p >= a.k) return;
        const int r = a.root[p];
        const ChainSeg &seg = a.seg[r];
        const bool degenerate = seg.lm.status == SFM_REFINE_DEGENERATE;
        float *o = a.out.d_cams + (size_t)kFuseCams * p;
        const float *in = a.cams + (size_t)kFuseCams * p;
        const float *S = a.state[seg.cur];
#pragma unroll
        for (int q = 0; q < 12; ++q) {
            o[q] = (degenerate || r == p) ? in[q] : S[(size_t)kChainState * (p - 1) + q];
            o[12 + q] = degenerate ? in[12 + q] : S[(size_t)kChainState * p + q];
        }
        sfm_adjust_chain_report rep = {};
        rep.root = r;
        if (r == p) {
            rep.status = seg.lm.status; rep.iterations = seg.lm.iters; rep.accepted = seg.lm.accepted;
            rep.num_cameras = seg.end - p; rep.num_tracks = seg.tracks; rep.num_observations = seg.obs; rep.num_over_long = seg.over;
            rep.initial_rms_px = seg.initial_rms;
            rep.final_rms_px = seg.obs > 0 ? (float)sqrt(seg.lm.sq / (2.0 * (double)seg.obs)) : 0.0f;
            rep.final_cost = (float)seg.lm.cost;
            rep.lambda = (float)seg.lm.lambda;
        }
        a.out.d_reports[p] = rep;
        return;
    }
    const int t = blockIdx.x * kChainTrackBlock + threadIdx.x;
    if (t >= chain_tracks(a)) return;
    const int o0 = a.track_offset[t], count = a.track_offset[t + 1] - o0;
    const ChainSeg &seg = a.seg[a.root[a.obs_cam[o0] >> 1]];
    const bool degenerate = seg.lm.status == SFM_REFINE_DEGENERATE;
    float out[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) out[c] = a.points[(size_t)c * a.N + t];
    if (a.out.d_used[t] && !degenerate) {
        const float4 X4 = a.X[seg.cur][t];
        out[0] = X4.x; out[1] = X4.y; out[2] = X4.z; out[3] = 1.0f;
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) a.out.d_points[(size_t)c * a.N + t] = out[c];
    if (a.out.d_err) {
        const float X[3] = { out[0] / out[3], out[1] / out[3], out[2] / out[3] };
        const float *S = a.state[seg.cur];
        const ChainTrackViews view = { a, S, a.obs_cam + o0, a.obs_record + o0 };
        a.out.d_err[t] = chain_error(count, view, [&](int o) -> const float * {
            if (degenerate) return a.cams + 12 * (size_t)view.cam[o];          // the cameras as they are returned
            const int b = view.block(o);
            return b < 0 ? nullptr : S + (size_t)kChainState * b;
        }, X);
    }
}

int launch_adjust_chain(sfm_ctx *ctx, const FusePair *h_pairs, int num_pairs, const sfm_adjust_chain_in &in, const sfm_adjust_chain_params &p,
                        const sfm_adjust_chain_out &out)
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
    ChainArgs a;
    a.pairs = static_cast<const FusePair *>(ja.dev);
    a.k = num_pairs; a.N = N; a.W = p.max_track_views;
    a.p = p;
    a.root = in.d_root; a.track_offset = in.d_track_offset; a.obs_cam = in.d_obs_cam; a.obs_record = in.d_obs_record; a.counts = in.d_counts;
    a.cams = in.d_cams; a.points = in.d_points; a.flags = in.d_flags;
    a.out = out;
    const size_t need = chain_work_layout(nullptr, (size_t)num_pairs, (size_t)N, (size_t)a.W, (size_t)a.W, a);
    rc = grow(&ctx->chain_ws, &ctx->chain_ws_bytes, need, st);
    if (rc != SFM_OK) return rc;
    chain_work_layout(ctx->chain_ws, (size_t)num_pairs, (size_t)N, (size_t)a.W, (size_t)a.W, a);
    rc = job_array_upload(ja, (size_t)num_pairs, sizeof(FusePair), st);
    if (rc != SFM_OK) return rc;
    const int k = num_pairs, pair_blocks = (k + 63) / 64;
    const int track_blocks = (N + kChainTrackBlock - 1) / kChainTrackBlock;      // T <= N stays on the device
    const int waves = chain_system_waves(a.W);
    const size_t lds = (size_t)waves * chain_part_values(a.W) * sizeof(double);  // 40 KiB at W = 16 (one wavefront), 44 KiB at W = 8 (four)
    hipLaunchKernelGGL(chain_init_kernel, dim3(k / 64 + 1), dim3(64), 0, st, a);
    SFM_HIP_TRY(hipGetLastError());
    if (track_blocks > 0) {
        hipLaunchKernelGGL(chain_used_kernel, dim3(track_blocks), dim3(kChainTrackBlock), 0, st, a);
        SFM_HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(chain_cost_kernel, dim3(k), dim3(kChainTrackBlock), 0, st, a, 0);
    SFM_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(chain_open_kernel, dim3(pair_blocks), dim3(64), 0, st, a);
    SFM_HIP_TRY(hipGetLastError());
    for (int it = 0; it < p.max_iterations; ++it) {
        hipLaunchKernelGGL(chain_system_kernel, dim3(k), dim3(64 * waves), lds, st, a);
        SFM_HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(chain_solve_kernel, dim3(k), dim3(kChainSolveThreads), 0, st, a);
        SFM_HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(chain_cost_kernel, dim3(k), dim3(kChainTrackBlock), 0, st, a, 1);
        SFM_HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(chain_accept_kernel, dim3(pair_blocks), dim3(64), 0, st, a);
        SFM_HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(chain_finish_kernel, dim3(track_blocks + (k + kChainTrackBlock - 1) / kChainTrackBlock), dim3(kChainTrackBlock), 0, st, a,
                       track_blocks);
    SFM_HIP_TRY(hipGetLastError());
    return SFM_OK;
}

} // namespace sfm
