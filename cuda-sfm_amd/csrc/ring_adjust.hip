// ring_adjust.hip -- sfm_adjust_ring (gfx950): Levenberg-Marquardt bundle adjustment of a CLOSED ring as sfm_fuse_ring leaves it,
// one camera per view, view 0 fixed, the seam tracks used.  Arithmetic: ring_adjust_math.hpp over chain_adjust_math.hpp (shared
// with the host build of the CPU tests); damping, accept test and stop rules: LmControl, kept in device memory (RingSeg) between
// the launches.
//
// sfm_adjust_chain's fixed launch sequence (chain_adjust.hip) on the context's stream: no host synchronisation, no cooperative
// launch, no block that waits for another, no float atomics and no atomic on global memory (integer atomics on LDS count a head
// pair's tracks).  Every kernel reads sfm_fuse_ring's status from device memory at its top and leaves unless it is
// SFM_RING_CLOSED; the finish kernel then hands the inputs through.
//   ring_init_kernel      one lane per pair: block p's start state from slot 2p + 1 of d_cams (p < k - 1), the first track whose head
//                         pair is >= p, the ring's record cleared.
//   ring_used_kernel      one lane per track: the used test (REFINED or SEAM_REFINED) at the start cameras, the start point.
//   ring_cost_kernel      one block per head pair (mode 0): the cost of the start and the head pair's counts.
//   ring_open_kernel      one block: the blocks' used observations from the head pairs' counts (the degenerate decision), the sums
//                         in head-pair order, the LmControl.
// then max_iterations times
//   ring_system_kernel    chain_system_kernel's block per head pair; a local view v is ring view (h + v) mod k, and the fixed view
//                         (wherever it sits in the track) is passed over: its rows and blocks stay zero.
//   ring_solve_kernel     one block for the ring: the partials of the head pairs added in ascending order into the FOLDED band
//                         (ring_adjust_math.hpp), the damping, the banded Cholesky with one row of the current column per thread
//                         (up to 6 x 32 = 192 rows at W = 16: 256 threads), both substitutions, the camera steps.
//   ring_cost_kernel      (mode 1) per track the back substitution and the cost of the tentative state.
//   ring_accept_kernel    one lane: the head pairs' costs in ascending order, LmControl's decision.
// and at the end
//   ring_finish_kernel    one lane per track (column, used flag, error) and one per pair (cameras; lane 0 the report).
// Every loop over a track's views is a counted loop over its observation list.  The order of every sum depends only on the track
// table, so two calls give the same bytes.
#include "chain_adjust_device.hpp"
#include "ring_adjust_math.hpp"

namespace sfm {

constexpr int kRingSolveThreads = 256;    // >= 6 * 2 * kChainMaxViews: one row of a column's folded band per thread
constexpr int kRingOpenThreads = 256;

struct RingArgs {
    ChainArgs c;                          // (root, p, out and seg are not used; hcnt is rcnt's)
    sfm_adjust_ring_params p;
    sfm_adjust_ring_out out;
    const sfm_fuse_ring_report *ring;
    int Wf;                               // the folded band's block diagonals
    RingSeg *rs;                          // the ring's one record
    int *rcnt;                            // k x kRingCounts
};

// view o of a track under the states S: the modulo rule
struct RingTrackViews {
    const RingArgs &a;
    const float *S;
    const int32_t *cam, *rec;
    __device__ __forceinline__ int block(int o) const { return ring_block(cam[o], a.c.k); }
    __device__ __forceinline__ ChainView operator()(int o) const
    {
        const int c = cam[o], q = c >> 1;
        const FuseView f = fuse_view(a.c.pairs[q], a.c.cams, q, c & 1, rec[o]);
        const int b = ring_block(c, a.c.k);
        ChainView v;
        v.K = f.K; v.x = f.x; v.y = f.y;
        v.kind = ring_kind(b);
        v.S = S + (size_t)kChainState * (b < 0 ? 0 : b);
        return v;
    }
};

__device__ __forceinline__ bool ring_closed(const RingArgs &a) { return a.ring->status == SFM_RING_CLOSED; }
__device__ __forceinline__ bool ring_running(const RingArgs &a) { return chain_running(a.rs->s, a.p.max_iterations); }

__global__ __launch_bounds__(64)
void ring_init_kernel(RingArgs a)
{
    if (!ring_closed(a)) return;
    const int p = blockIdx.x * 64 + threadIdx.x, k = a.c.k;
    if (p > k) return;
    const int T = chain_tracks(a.c);
    {   // the first track whose head pair is >= p
        int lo = 0, hi = T;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if ((a.c.obs_cam[a.c.track_offset[mid]] >> 1) < p) lo = mid + 1; else hi = mid;
        }
        a.c.head[p] = lo;
    }
    if (p == 0) *a.rs = RingSeg();
    if (p >= k - 1) return;               // slot 2 (k - 1) + 1 is not read: that camera is view 0
    float P[12], s[kChainState];
#pragma unroll
    for (int q = 0; q < 12; ++q) P[q] = a.c.cams[(size_t)kFuseCams * p + 12 + q];
    chain_start_state(ring_kind(p), P, s);
#pragma unroll
    for (int q = 0; q < kChainState; ++q) a.c.state[0][(size_t)kChainState * p + q] = s[q];
}

__global__ __launch_bounds__(kChainTrackBlock)
void ring_used_kernel(RingArgs a)
{
    if (!ring_closed(a)) return;
    const int t = blockIdx.x * kChainTrackBlock + threadIdx.x;
    if (t >= chain_tracks(a.c)) return;
    const int o0 = a.c.track_offset[t], count = a.c.track_offset[t + 1] - o0;
    const RingTrackViews view = { a, a.c.state[0], a.c.obs_cam + o0, a.c.obs_record + o0 };
    float Xin[4], X[3] = { 0.0f, 0.0f, 1.0f };
#pragma unroll
    for (int c = 0; c < 4; ++c) Xin[c] = a.c.points[(size_t)c * a.c.N + t];
    const bool used = chain_used(ring_flag(a.c.flags[t]), count, a.c.W, Xin, view, X);
    a.out.d_used[t] = used ? 1 : 0;
    a.c.X[0][t] = make_float4(X[0], X[1], X[2], 1.0f);
}

// chain_cost_kernel over the ring's views; mode 0 also counts the head pair's used seam tracks
__global__ __launch_bounds__(kChainTrackBlock)
void ring_cost_kernel(RingArgs a, int mode)
{
    __shared__ double s_part[(kChainTrackBlock / 64) * 2], s_tot[2];
    __shared__ int s_cnt[kRingCounts];
    if (!ring_closed(a)) return;
    const int h = blockIdx.x;
    if (!mode) {
        if (threadIdx.x < kRingCounts) s_cnt[threadIdx.x] = 0;
        __syncthreads();
    }
    const ChainSeg &seg = a.rs->s;
    int cur = 0;
    float lam = 0.0f;
    if (mode) {
        if (!ring_running(a) || !seg.go) return;
        cur = seg.cur;
        lam = (float)seg.lm.lambda;
    }
    const float huber = a.p.huber_px;
    const float *S = a.c.state[cur], *St = a.c.state[cur ^ 1];
    double v[2] = { 0.0, 0.0 };
    for (int t = a.c.head[h] + (int)threadIdx.x; t < a.c.head[h + 1]; t += kChainTrackBlock) {
        const int o0 = a.c.track_offset[t], count = a.c.track_offset[t + 1] - o0;
        if (!mode && count > a.c.W) atomicAdd(&s_cnt[2], 1);
        if (!a.out.d_used[t]) continue;
        if (!mode) {
            atomicAdd(&s_cnt[0], 1);
            atomicAdd(&s_cnt[1], count);
            if (a.c.flags[t] == SFM_FUSE_SEAM_REFINED) atomicAdd(&s_cnt[3], 1);
            for (int o = 0; o < count; ++o) atomicAdd(&s_cnt[4 + o], 1);
        }
        const float4 X4 = a.c.X[cur][t];
        float X[3] = { X4.x, X4.y, X4.z }, cost, sq;
        if (mode) {
            const RingTrackViews view = { a, S, a.c.obs_cam + o0, a.c.obs_record + o0 };
            float Vi[6], gp[3], dp[3];
            chain_point_block(count, view, huber, lam, X, Vi, gp);
            chain_point_step(count, view, [&](int o) { return a.c.dc + 6 * (size_t)view.block(o); }, huber, X, Vi, gp, dp);
            X[0] += dp[0]; X[1] += dp[1]; X[2] += dp[2];
            a.c.X[cur ^ 1][t] = make_float4(X[0], X[1], X[2], 1.0f);
        }
        const RingTrackViews trial = { a, mode ? St : S, a.c.obs_cam + o0, a.c.obs_record + o0 };
        chain_cost(count, trial, huber, X, cost, sq);
        v[0] += (double)cost; v[1] += (double)sq;
    }
    block_sum<kChainTrackBlock / 64>(v, s_part, s_tot);
    if (threadIdx.x < 2) a.c.pcost[2 * (size_t)h + threadIdx.x] = s_tot[threadIdx.x];
    if (!mode && threadIdx.x < kRingCounts) a.rcnt[kRingCounts * (size_t)h + threadIdx.x] = s_cnt[threadIdx.x];      // (behind block_sum's barriers)
}

__global__ __launch_bounds__(kRingOpenThreads)
void ring_open_kernel(RingArgs a)
{
    __shared__ int s_deg;
    if (!ring_closed(a)) return;
    const int k = a.c.k, tid = threadIdx.x;
    if (tid == 0) s_deg = 0;
    __syncthreads();
    for (int P = tid; P < k - 1; P += kRingOpenThreads)
        if (ring_block_obs(a.rcnt, a.c.W, k, P) < (P == 0 ? kAdjMinView2 : kAdjMinView3)) atomicOr(&s_deg, 1);
    __syncthreads();
    if (tid != 0) return;
    RingSeg rs = *a.rs;
    double cost = 0.0, sq = 0.0;
    for (int h = 0; h < k; ++h) {
        const int *c = a.rcnt + kRingCounts * (size_t)h;
        cost += a.c.pcost[2 * (size_t)h]; sq += a.c.pcost[2 * (size_t)h + 1];
        rs.s.tracks += c[0]; rs.s.obs += c[1]; rs.s.over += c[2]; rs.seam += c[3];
    }
    rs.s.end = k - 1;
    rs.s.lm = LmControl((double)a.p.initial_lambda, cost, sq, s_deg != 0);
    rs.s.initial_rms = rs.s.obs > 0 ? (float)sqrt(sq / (2.0 * (double)rs.s.obs)) : 0.0f;
    *a.rs = rs;
}

__global__ __launch_bounds__(256)
void ring_system_kernel(RingArgs a)
{
    extern __shared__ double s_all[];                     // chain_system_waves(W) x chain_part_values(W)
    if (!ring_closed(a) || !ring_running(a)) return;
    const int h = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
    const ChainSeg &seg = a.rs->s;
    const int W = a.c.W, k = a.c.k, values = chain_part_values(W);
    double *s_band = s_all + (size_t)values * wave;       // this wavefront's partial band
    for (int q = lane; q < values; q += 64) s_band[q] = 0.0;
    __syncthreads();                                      // a value is zeroed by lane q % 64 and added to by lane q % 36 or q % 12 (every thread of the block is here)
    const int cur = seg.cur;
    const float lam = (float)seg.lm.lambda, huber = a.p.huber_px;
    const float *S = a.c.state[cur];
    const int t0 = a.c.head[h], t1 = a.c.head[h + 1];
    for (int base = t0 + 64 * wave; base < t1; base += 64 * waves) {      // the same trip counts in every lane of a wavefront
        const int t = base + lane;
        const bool live = t < t1 && a.out.d_used[t] != 0;
        int o0 = 0, count = 0;
        float X[3] = { 0.0f, 0.0f, 1.0f }, Vi[6], gp[3];
        if (live) {
            o0 = a.c.track_offset[t]; count = a.c.track_offset[t + 1] - o0;
            const float4 X4 = a.c.X[cur][t];
            X[0] = X4.x; X[1] = X4.y; X[2] = X4.z;
        }
        const RingTrackViews view = { a, S, a.c.obs_cam + o0, a.c.obs_record + o0 };
        if (live) chain_point_block(count, view, huber, lam, X, Vi, gp);
        int most = count;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) most = max(most, __shfl_xor(most, off));
        for (int va = 0; va < most; ++va) {
            if (ring_local_block(h, va, k) < 0) continue;                 // the fixed view: the same va in every lane of the block
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
                if (ring_local_block(h, vb, k) < 0) continue;
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
    double *part = a.c.part + (size_t)values * h;
    for (int q = threadIdx.x; q < values; q += blockDim.x) {
        double s = s_all[q];
        for (int w = 1; w < waves; ++w) s += s_all[(size_t)values * w + q];
        part[q] = s;
    }
}

__global__ __launch_bounds__(kRingSolveThreads)
void ring_solve_kernel(RingArgs a)
{
    __shared__ double s_d;
    __shared__ int s_ok;
    if (!ring_closed(a) || !ring_running(a)) return;
    const int tid = threadIdx.x;
    RingSeg rs = *a.rs;
    const int W = a.c.W, Wf = a.Wf, k = a.c.k, nb = k - 1, N = 6 * nb;
    double *B = a.c.band, *x = a.c.x, *du = a.c.du;
    // ---- the head pairs' partials in ascending order, into the folded positions ----
    for (int idx = tid; idx < nb * Wf * 36; idx += kRingSolveThreads) {
        const int e = idx % 36, d = (idx / 36) % Wf, pl = idx / (36 * Wf);
        B[idx] = pl + d < nb ? ring_reduce_block(a.c.part, W, k, ring_fold_block(pl, nb), ring_fold_block(pl + d, nb), e) : 0.0;
    }
    for (int idx = tid; idx < N; idx += kRingSolveThreads) {
        const int P = ring_fold_block(idx / 6, nb);
        x[idx] = -ring_reduce_row(a.c.part, W, k, P, idx % 6, false);
        du[idx] = ring_reduce_row(a.c.part, W, k, P, idx % 6, true);
    }
    __syncthreads();
    for (int idx = tid; idx < N; idx += kRingSolveThreads) {              // row 5: the unit row of the 5-dof block (block 0 is position 0)
        const size_t at = chain_band_at(Wf, idx, idx);
        B[at] = idx == 5 ? 1.0 : B[at] + rs.s.lm.lambda * du[idx];
    }
    if (tid == 0) s_ok = 1;
    __syncthreads();
    // ---- the banded Cholesky: thread i owns row j + i of column j ----
    for (int j = 0; j < N; ++j) {
        const int row = j + tid;
        const bool mine = row <= chain_band_last(Wf, N, j);
        const double s = mine ? chain_band_dot(B, Wf, row, j) : 0.0;
        if (tid == 0) {
            if (!(s > 0.0)) s_ok = 0;
            s_d = sqrt(s);
        }
        __syncthreads();
        if (!s_ok) break;
        if (mine) B[chain_band_at(Wf, row, j)] = tid == 0 ? s_d : s / s_d;
        __syncthreads();
    }
    const bool ok = s_ok != 0;
    if (ok) {
        // ---- L L^T x = -b: forward by ascending columns, backward by descending ones ----
        for (int j = 0; j < N; ++j) {
            if (tid == 0) x[j] /= B[chain_band_at(Wf, j, j)];
            __syncthreads();
            const int row = j + 1 + tid;
            if (row <= chain_band_last(Wf, N, j)) x[row] -= B[chain_band_at(Wf, row, j)] * x[j];
            __syncthreads();
        }
        for (int j = N - 1; j >= 0; --j) {
            if (tid == 0) x[j] /= B[chain_band_at(Wf, j, j)];
            __syncthreads();
            const int i = chain_band_first(Wf, j) + tid;
            if (i < j) x[i] -= B[chain_band_at(Wf, j, i)] * x[j];
            __syncthreads();
        }
        // ---- the camera steps into the other state buffer: block P's step sits at its folded position ----
        for (int P = tid; P < nb; P += kRingSolveThreads) {
            const int pos = ring_fold_pos(P, nb);
            double dc[6];
            float s[kChainState], o[kChainState];
#pragma unroll
            for (int q = 0; q < 6; ++q) { dc[q] = x[6 * pos + q]; a.c.dc[6 * (size_t)P + q] = (float)dc[q]; }
#pragma unroll
            for (int q = 0; q < kChainState; ++q) s[q] = a.c.state[rs.s.cur][(size_t)kChainState * P + q];
            chain_camera_step(ring_kind(P), dc, s, o);
#pragma unroll
            for (int q = 0; q < kChainState; ++q) a.c.state[rs.s.cur ^ 1][(size_t)kChainState * P + q] = o[q];
        }
    }
    if (tid == 0) {
        rs.s.go = ok ? 1 : 0;
        if (!ok && !rs.s.lm.solve_failed()) rs.s.stopped = 1;     // not positive definite: more damping, or the end
        *a.rs = rs;
    }
}

__global__ __launch_bounds__(64)
void ring_accept_kernel(RingArgs a)
{
    if (!ring_closed(a) || threadIdx.x != 0) return;
    RingSeg rs = *a.rs;
    if (!chain_running(rs.s, a.p.max_iterations) || !rs.s.go) return;
    double cost = 0.0, sq = 0.0;
    for (int h = 0; h < a.c.k; ++h) { cost += a.c.pcost[2 * (size_t)h]; sq += a.c.pcost[2 * (size_t)h + 1]; }
    bool stop;
    if (rs.s.lm.tentative(cost, sq, (double)a.p.min_rel_decrease, stop)) rs.s.cur ^= 1;
    if (stop) rs.s.stopped = 1;
    rs.s.go = 0;
    *a.rs = rs;
}

__global__ __launch_bounds__(kChainTrackBlock)
void ring_finish_kernel(RingArgs a, int track_blocks)
{
    const int ring_status = a.ring->status, k = a.c.k;
    const bool closed = ring_status == SFM_RING_CLOSED;
    // not CLOSED: the record was never written and is not read
    const bool through = !closed || a.rs->s.lm.status == SFM_REFINE_DEGENERATE;       // the inputs are handed through
    const int cur = closed ? a.rs->s.cur : 0;
    const float *S = a.c.state[cur];
    if ((int)blockIdx.x >= track_blocks) {                // ---- one lane per pair: its cameras; lane 0 the report ----
        const int p = ((int)blockIdx.x - track_blocks) * kChainTrackBlock + threadIdx.x;
        if (p >= k) return;
        float *o = a.out.d_cams + (size_t)kFuseCams * p;
        const float *in = a.c.cams + (size_t)kFuseCams * p;
#pragma unroll
        for (int q = 0; q < 12; ++q) {
            o[q] = (through || p == 0) ? in[q] : S[(size_t)kChainState * (p - 1) + q];
            o[12 + q] = through ? in[12 + q] : (p == k - 1 ? a.c.cams[q] : S[(size_t)kChainState * p + q]);     // view 0: camera 1 of pair 0
        }
        if (p != 0) return;
        sfm_adjust_ring_report rep = {};
        rep.ring_status = ring_status;
        if (closed) {
            const RingSeg &rs = *a.rs;
            rep.status = rs.s.lm.status; rep.iterations = rs.s.lm.iters; rep.accepted = rs.s.lm.accepted;
            rep.num_cameras = k - 1; rep.num_tracks = rs.s.tracks; rep.num_seam_tracks = rs.seam; rep.num_observations = rs.s.obs;
            rep.num_over_long = rs.s.over;
            rep.initial_rms_px = rs.s.initial_rms;
            rep.final_rms_px = rs.s.obs > 0 ? (float)sqrt(rs.s.lm.sq / (2.0 * (double)rs.s.obs)) : 0.0f;
            rep.final_cost = (float)rs.s.lm.cost;
            rep.lambda = (float)rs.s.lm.lambda;
        }
        *a.out.d_report = rep;
        return;
    }
    const int t = blockIdx.x * kChainTrackBlock + threadIdx.x;
    if (t >= chain_tracks(a.c)) return;
    const int o0 = a.c.track_offset[t], count = a.c.track_offset[t + 1] - o0;
    const bool used = closed && a.out.d_used[t] != 0;
    if (!closed) a.out.d_used[t] = 0;
    float out[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) out[c] = a.c.points[(size_t)c * a.c.N + t];
    if (used && !through) {
        const float4 X4 = a.c.X[cur][t];
        out[0] = X4.x; out[1] = X4.y; out[2] = X4.z; out[3] = 1.0f;
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) a.out.d_points[(size_t)c * a.c.N + t] = out[c];
    if (a.out.d_err) {
        const float X[3] = { out[0] / out[3], out[1] / out[3], out[2] / out[3] };
        const RingTrackViews view = { a, S, a.c.obs_cam + o0, a.c.obs_record + o0 };
        a.out.d_err[t] = chain_error(count, view, [&](int o) -> const float * {
            if (through) return a.c.cams + 12 * (size_t)view.cam[o];           // the cameras as they are returned
            const int b = view.block(o);
            return b < 0 ? nullptr : S + (size_t)kChainState * b;
        }, X);
    }
}

int launch_adjust_ring(sfm_ctx *ctx, const FusePair *h_pairs, int num_pairs, const sfm_adjust_ring_in &in, const sfm_adjust_ring_params &p,
                       const sfm_adjust_ring_out &out)
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
    const int k = num_pairs;
    RingArgs a = {};
    a.c.pairs = static_cast<const FusePair *>(ja.dev);
    a.c.k = k; a.c.N = N; a.c.W = p.max_track_views;
    a.c.track_offset = in.d_track_offset; a.c.obs_cam = in.d_obs_cam; a.c.obs_record = in.d_obs_record; a.c.counts = in.d_counts;
    a.c.cams = in.d_cams; a.c.points = in.d_points; a.c.flags = in.d_flags;
    a.p = p; a.out = out; a.ring = in.d_ring_report;
    a.Wf = ring_band_width(a.c.W, k - 1);
    // the chain's work buffer (its band Wf block diagonals wide), then the ring's counts and record
    auto layout = [&](void *buffer) {
        const size_t used = chain_work_layout(buffer, (size_t)k, (size_t)N, (size_t)a.c.W, (size_t)a.Wf, a.c);
        Carver w(buffer);
        w.used = used;
        a.rs = w.take<RingSeg>(1, 8);
        a.rcnt = w.take<int>((size_t)kRingCounts * k, 4);
        return w.used;
    };
    const size_t need = layout(nullptr);
    rc = grow(&ctx->chain_ws, &ctx->chain_ws_bytes, need, st);
    if (rc != SFM_OK) return rc;
    layout(ctx->chain_ws);
    rc = job_array_upload(ja, (size_t)num_pairs, sizeof(FusePair), st);
    if (rc != SFM_OK) return rc;
    const int track_blocks = (N + kChainTrackBlock - 1) / kChainTrackBlock;      // T <= N stays on the device
    const int waves = chain_system_waves(a.c.W);
    const size_t lds = (size_t)waves * chain_part_values(a.c.W) * sizeof(double);
    hipLaunchKernelGGL(ring_init_kernel, dim3(k / 64 + 1), dim3(64), 0, st, a);
    SFM_HIP_TRY(hipGetLastError());
    if (track_blocks > 0) {
        hipLaunchKernelGGL(ring_used_kernel, dim3(track_blocks), dim3(kChainTrackBlock), 0, st, a);
        SFM_HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(ring_cost_kernel, dim3(k), dim3(kChainTrackBlock), 0, st, a, 0);
    SFM_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(ring_open_kernel, dim3(1), dim3(kRingOpenThreads), 0, st, a);
    SFM_HIP_TRY(hipGetLastError());
    for (int it = 0; it < p.max_iterations; ++it) {
        hipLaunchKernelGGL(ring_system_kernel, dim3(k), dim3(64 * waves), lds, st, a);
        SFM_HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(ring_solve_kernel, dim3(1), dim3(kRingSolveThreads), 0, st, a);
        SFM_HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(ring_cost_kernel, dim3(k), dim3(kChainTrackBlock), 0, st, a, 1);
        SFM_HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(ring_accept_kernel, dim3(1), dim3(64), 0, st, a);
        SFM_HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(ring_finish_kernel, dim3(track_blocks + (k + kChainTrackBlock - 1) / kChainTrackBlock), dim3(kChainTrackBlock), 0, st, a,
                       track_blocks);
    SFM_HIP_TRY(hipGetLastError());
    return SFM_OK;
}

} // namespace sfm
