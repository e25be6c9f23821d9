// ring.hip -- sfm_close_ring (gfx950): the drift of a ring of aligned pairs measured, spread over the links, and seen at the seam.
// Arithmetic: ring_math.hpp (shared with the host build of the CPU tests), on top of fuse_math.hpp.
//
// Three launches on the context's stream, no host synchronisation.  The links are an array of RingLink in device memory (the
// context's JobArray); the fp64 frames, weights and sums live in the context's work buffer.
//   ring_walk_kernel     ONE block of 256 threads, 256 links at a time, fuse_frames_kernel's shape: every thread loads its link,
//                        tests it, inverts it in fp64 into LDS and stores its weight; wavefront 0 composes the inverses along the
//                        ring (restarting at an invalid link, as sfm_fuse_chain does), lane c < 13 holding element c of the
//                        running frame, and stores every F_i in fp64.  Then one lane forms D = F_k, the status, the drift
//                        numbers, the correction (sigma, w, t_c) and the alpha prefix: in link order, so serial like the walk
//                        (the weights come through LDS 256 at a time, the divisions by the total are taken by all threads).
//   ring_correct_kernel  one lane per link: B_i, B_{i+1}, F'_i, F'_{i+1}^-1 and L'_i in fp64, then the two 13-float stores (the
//                        input link and the open frame where the ring is not closed).
//   ring_seam_kernel     one lane per record of pair k - 1 in rounds of 256, block b taking the rounds b, b + blocks, ...: the three
//                        carries and tests, the errors; seven fp64 sums per block by block_sum.  The block partials go to the
//                        work buffer; an INTEGER ticket names the block that finishes last, which folds them in a fixed second
//                        stage -- thread t the partials t, t + 256, ... in block order, then block_sum -- and writes the report's
//                        seam block.  Which block folds varies, what it computes does not: no float atomics.
#include "common.hpp"
#include "device_math.hpp"
#include "block_ops.hpp"
#include "ring_math.hpp"
#include <string.h>

namespace sfm {

constexpr int kRingWaves = kRingBlock / 64;

struct RingArgs {
    const RingLink *links;
    int k, blocks;                        // links; blocks of the seam kernel
    int given;                            // the links' weights come from the caller, not from the reports
    float thr, max_rot, max_log;
    FusePair last;                        // pair k - 1: points, valid, X1, K, n, ld
    double *F;                            // (k + 1) x 13: the open frames, F[k] = D
    double *w, *alpha;                    // k weights; k + 1 running sums
    RingHead *head;
    double *partial;                      // blocks x kRingSums
    unsigned int *ticket;
    sfm_ring_out out;
};

__global__ __launch_bounds__(kRingBlock)
void ring_walk_kernel(RingArgs a)
{
    __shared__ double s_inv[kRingBlock][kFuseSim];
    __shared__ int s_valid[kRingBlock];
    __shared__ double s_w[kRingBlock], s_total;
    const int tid = threadIdx.x, lane = tid & 63;
    const int c = lane < kFuseSim ? lane : 0;
    const int row = fuse_compose_row(c);
    const int y0 = fuse_compose_operand(c, 0), y1 = fuse_compose_operand(c, 1), y2 = fuse_compose_operand(c, 2);
    double Fc = (c == 0 || c == 1 || c == 5 || c == 9) ? 1.0 : 0.0;                     // fuse_identity: F_0
    int first_invalid = -1;                                                              // the same in every lane of wavefront 0
    if (tid < kFuseSim) a.F[tid] = Fc;
    if (tid == 0) *a.ticket = 0u;
    for (int base = 0; base < a.k; base += kRingBlock) {
        const int i = base + tid;
        __syncthreads();
        // ---- every thread: its link's validity, inverse and weight (off the serial chain) ----
        s_valid[tid] = 0;
        if (i < a.k) {
            const RingLink &q = a.links[i];
            float link[kFuseSim];
            double inv[kFuseSim];
#pragma unroll
            for (int e = 0; e < kFuseSim; ++e) link[e] = q.sim[e];
            const bool ok = fuse_link_valid(q.report->status, link);
            s_valid[tid] = ok ? 1 : 0;
            if (ok) {
                fuse_invert(link, inv);
#pragma unroll
                for (int e = 0; e < kFuseSim; ++e) s_inv[tid][e] = inv[e];
            }
            a.w[i] = a.given ? q.weight : ring_weight(q.report->num_inliers);
        }
        __syncthreads();
        // ---- wavefront 0: F_{i+1} = F_i o L_i^-1, the identity behind an invalid link ----
        if (tid < 64) {
            const int cnt = min(kRingBlock, a.k - base);
            for (int l = 0; l < cnt; ++l) {
                if (!__builtin_amdgcn_readfirstlane(s_valid[l])) {
                    Fc = (c == 0 || c == 1 || c == 5 || c == 9) ? 1.0 : 0.0;
                    if (first_invalid < 0) first_invalid = base + l;
                } else {
                    const double x[3] = { __shfl(Fc, 1 + 3 * row), __shfl(Fc, 2 + 3 * row), __shfl(Fc, 3 + 3 * row) };
                    const double s0 = __shfl(Fc, 0), t0 = __shfl(Fc, 10 + row);
                    const double y[3] = { s_inv[l][y0], s_inv[l][y1], s_inv[l][y2] };
                    Fc = fuse_compose_element(c, s0, x, t0, y);
                }
                if (lane < kFuseSim) a.F[(size_t)kFuseSim * (base + l + 1) + c] = Fc;
            }
        }
    }
    __syncthreads();                                          // the block's stores to F before lane 0 reads them
    // ---- one lane: the drift, the status, the correction ----
    if (tid == 0) {
        RingHead h;
        float drift[3] = { 0.0f, 0.0f, 0.0f };
#pragma unroll
        for (int q = 0; q < 7; ++q) h.corr[q] = 0.0;
        fuse_identity(h.Dinv);
        h.status = SFM_RING_OPEN; h.pad = 0;
        if (first_invalid < 0) {
            double D[kFuseSim];
#pragma unroll
            for (int q = 0; q < kFuseSim; ++q) D[q] = a.F[(size_t)kFuseSim * a.k + q];
            ring_drift(D, a.max_rot, a.max_log, h, drift);
        }
        *a.head = h;
        sfm_ring_report *r = a.out.d_report;
        r->status = h.status; r->num_links = a.k; r->first_invalid = first_invalid;
        r->drift_log_scale = drift[0]; r->drift_rotation_rad = drift[1]; r->drift_t = drift[2];
        s_valid[0] = h.status;
    }
    __syncthreads();
    if (s_valid[0] != SFM_RING_CLOSED) return;
    // ---- the alpha prefix, ring_alphas' sums in link order: 256 weights per round through LDS (every thread reads the weight
    //      it stored), lane 0 adds them one after the other -- the total first, then the running sums of w_i / total ----
    double acc = 0.0;                                         // lane 0's: the total, then the running sum
    for (int base = 0; base < a.k; base += kRingBlock) {
        const int i = base + tid;
        s_w[tid] = i < a.k ? a.w[i] : 0.0;
        __syncthreads();
        if (tid == 0) {
            const int cnt = min(kRingBlock, a.k - base);
            for (int l = 0; l < cnt; ++l) acc += s_w[l];
        }
        __syncthreads();
    }
    if (tid == 0) { s_total = acc; acc = 0.0; a.alpha[0] = 0.0; }
    __syncthreads();
    const double total = s_total;
    for (int base = 0; base < a.k; base += kRingBlock) {
        const int i = base + tid;
        s_w[tid] = i < a.k ? a.w[i] / total : 0.0;
        __syncthreads();
        if (tid == 0) {
            const int cnt = min(kRingBlock, a.k - base);
            for (int l = 0; l < cnt; ++l) { acc += s_w[l]; s_w[l] = acc; }
        }
        __syncthreads();
        if (i < a.k) a.alpha[i + 1] = i + 1 == a.k ? 1.0 : s_w[tid];
        __syncthreads();
    }
}

__global__ __launch_bounds__(kRingBlock)
void ring_correct_kernel(RingArgs a)
{
    const int i = blockIdx.x * kRingBlock + threadIdx.x;
    if (i >= a.k) return;
    double F0[kFuseSim];
    float link[kFuseSim], frame[kFuseSim];
#pragma unroll
    for (int q = 0; q < kFuseSim; ++q) F0[q] = a.F[(size_t)kFuseSim * i + q];
    if (a.head->status != SFM_RING_CLOSED) {
        const float *sim = a.links[i].sim;
#pragma unroll
        for (int q = 0; q < kFuseSim; ++q) { link[q] = sim[q]; frame[q] = (float)F0[q]; }
    } else {
        double F1[kFuseSim];
#pragma unroll
        for (int q = 0; q < kFuseSim; ++q) F1[q] = a.F[(size_t)kFuseSim * (i + 1) + q];
        ring_correct(*a.head, a.alpha[i], a.alpha[i + 1], i + 1 == a.k, F0, F1, link, frame);
    }
#pragma unroll
    for (int q = 0; q < kFuseSim; ++q) {
        a.out.d_links[(size_t)kFuseSim * i + q] = link[q];
        a.out.d_frames[(size_t)kFuseSim * i + q] = frame[q];
    }
}

__global__ __launch_bounds__(kRingBlock)
void ring_seam_kernel(RingArgs a)
{
    __shared__ double s_part[kRingWaves * kRingSums], s_out[kRingSums];
    __shared__ unsigned int s_last;
    const int tid = threadIdx.x;
    const FusePair &p = a.last;
    // the three frames, the same in every lane: the measured closing link, the open F_{k-1}, the closed F'_{k-1} (ring_correct_kernel's)
    float link[kFuseSim], open[kFuseSim], closed[kFuseSim];
    const float *sim = a.links[a.k - 1].sim;
#pragma unroll
    for (int q = 0; q < kFuseSim; ++q) {
        link[q] = sim[q];
        open[q] = (float)a.F[(size_t)kFuseSim * (a.k - 1) + q];
        closed[q] = a.out.d_frames[(size_t)kFuseSim * (a.k - 1) + q];
    }
    const float *const frames[3] = { link, open, closed };
    double sums[kRingSums];
#pragma unroll
    for (int q = 0; q < kRingSums; ++q) sums[q] = 0.0;
    for (int base = (int)blockIdx.x * kRingBlock; base < p.n; base += a.blocks * kRingBlock) {
        const int j = base + tid;
        if (j >= p.n) continue;
        float err[3];
        double v[kRingSums];
        ring_seam_record(p, j, a.thr, frames, err, v);
#pragma unroll
        for (int q = 0; q < kRingSums; ++q) sums[q] += v[q];
        if (a.out.d_seam_err) {
#pragma unroll
            for (int f = 0; f < 3; ++f) a.out.d_seam_err[(size_t)f * p.n + j] = err[f];
        }
    }
    block_sum<kRingWaves, kRingSums>(sums, s_part, s_out);
    if (tid < kRingSums) a.partial[(size_t)kRingSums * blockIdx.x + tid] = s_out[tid];
    // ---- the ticket: the block that arrives last folds every block's partials.  The partials are published by ONE agent-scope
    //      release behind the block's stores (drained first, and again behind the fence: its own wait is not relied on) and taken
    //      by ONE agent-scope acquire in the folding block, whose loads below are vector loads ----
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        s_last = __hip_atomic_fetch_add(a.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    if (s_last != (unsigned int)(a.blocks - 1)) return;
    if (tid == 0) {
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < kRingSums; ++q) sums[q] = 0.0;
    for (int b = tid; b < a.blocks; b += kRingBlock) {
#pragma unroll
        for (int q = 0; q < kRingSums; ++q) sums[q] += a.partial[(size_t)kRingSums * b + q];
    }
    block_sum<kRingWaves, kRingSums>(sums, s_part, s_out);
    if (tid == 0) {
        double t[kRingSums];
#pragma unroll
        for (int q = 0; q < kRingSums; ++q) t[q] = s_out[q];
        sfm_ring_report r;
        ring_seam_report(t, r);
        sfm_ring_report *o = a.out.d_report;
        o->seam_count = r.seam_count; o->seam_lost_open = r.seam_lost_open; o->seam_lost_closed = r.seam_lost_closed;
        o->seam_rms_link_px = r.seam_rms_link_px; o->seam_rms_open_px = r.seam_rms_open_px; o->seam_rms_closed_px = r.seam_rms_closed_px;
    }
}

// the context's work buffer for k links and `blocks` seam blocks: the arrays of `a` inside it; returns its size in bytes
static size_t ring_work_layout(void *buffer, size_t k, size_t blocks, RingArgs &a)
{
    Carver w(buffer);
    a.F = w.take<double>((k + 1) * kFuseSim, 16);
    a.w = w.take<double>(k, 8);
    a.alpha = w.take<double>(k + 1, 8);
    a.partial = w.take<double>(blocks * kRingSums, 8);
    a.head = w.take<RingHead>(1, 8);
    a.ticket = w.take<unsigned int>(1, 4);
    return w.used;
}

int launch_close_ring(sfm_ctx *ctx, const RingLink *h_links, int num_links, const FusePair &last, const sfm_ring_params &p, const sfm_ring_out &out)
{
    hipStream_t st = ctx->stream;
    JobArray &ja = ctx->ring_jobs;
    int rc = job_array_reserve(ja, (size_t)num_links, sizeof(RingLink), st);
    if (rc != SFM_OK) return rc;
    memcpy(ja.pinned, h_links, (size_t)num_links * sizeof(RingLink));
    RingArgs a;
    a.links = static_cast<const RingLink *>(ja.dev);
    a.k = num_links; a.blocks = ring_seam_blocks(last.n);
    a.given = p.weights ? 1 : 0;
    a.thr = p.threshold_px; a.max_rot = p.max_rotation_rad; a.max_log = p.max_log_scale;
    a.last = last;
    a.out = out;
    const size_t need = ring_work_layout(nullptr, (size_t)num_links, (size_t)a.blocks, a);
    rc = grow(&ctx->ring_ws, &ctx->ring_ws_bytes, need, st);
    if (rc != SFM_OK) return rc;
    ring_work_layout(ctx->ring_ws, (size_t)num_links, (size_t)a.blocks, a);
    rc = job_array_upload(ja, (size_t)num_links, sizeof(RingLink), st);
    if (rc != SFM_OK) return rc;
    hipLaunchKernelGGL(ring_walk_kernel, dim3(1), dim3(kRingBlock), 0, st, a);
    SFM_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(ring_correct_kernel, dim3((num_links + kRingBlock - 1) / kRingBlock), dim3(kRingBlock), 0, st, a);
    SFM_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(ring_seam_kernel, dim3(a.blocks), dim3(kRingBlock), 0, st, a);
    SFM_HIP_TRY(hipGetLastError());
    return SFM_OK;
}

} // namespace sfm
