// fuse.hip -- sfm_fuse_chain (gfx950): a chain of aligned pairs fused into tracks and one refined point per track.
// Arithmetic: fuse_math.hpp (shared with the host build of the CPU tests); damping, accept test and stop rules: LmControl.
//
// One memset and seven launches on the context's stream, no host synchronisation.  The pairs and their links are an array of
// FusePair in device memory (the context's JobArray); node (i, j) has the global id pairs[i].offset + j, and a node block
// (256 nodes) never holds nodes of two pairs, so a block finds its pair once (binary search over block0) and the order of the
// blocks is the order of the nodes.
//   fuse_frames_kernel   ONE block of 256 threads, 256 links at a time: every thread loads its link, tests it and inverts it in fp64
//                        into LDS (the loads and the four divisions of an inverse need no other link); wavefront 0 composes the
//                        inverses along the chain, one link after the other (restarting at every cut), with lane c < 13
//                        holding element c of the running frame and computing that element alone (five shuffles and five fp64
//                        operations on the chain per link); rounded once to fp32, then every thread writes its pair's frame,
//                        root and two cameras.  Clears the counts.
//   fuse_edges_kernel    one lane per node of pairs 0 .. k-2: where record j proposes an edge, one 64-bit integer atomicMin of
//                        (bits(err) << 32) | j on the target's key (the keys are set to all ones by the memset in front).
//   fuse_links_kernel    one lane per node: its class (dead / live / head: live and nobody won it) and its successor (the target
//                        whose key is its own).  A launch of its own because a walk reads the successors of OTHER blocks' nodes.
//   fuse_count_kernel    one lane per node: a head walks its path; per block the number of heads and of observations (path
//                        length + 1 each) by block_scan's total, and the longest track that starts in the block.
//   fuse_scan_kernel     ONE block: exclusive scan of the block counts in rounds of 256 with a running carry: T, M, offset[T],
//                        the longest track; REFINED is set to T.
//   fuse_fill_kernel     one lane per node: block_scan of (heads, observations) inside the block on top of the block's base gives
//                        a head its track id and CSR offset; it walks its path again and writes d_track and d_obs_*.  Dead nodes
//                        write -1 into d_track themselves.
//   fuse_points_kernel   one lane per track: the mean start, the LM over the track's list (walked again for every trial cost:
//                        no per-lane array sized by the number of views), the acceptance test; a wavefront that keeps start
//                        points moves their number from REFINED to KEPT by two integer atomics.
#include "fuse_device.hpp"

namespace sfm {

__global__ __launch_bounds__(kFuseFrameThreads)
void fuse_frames_kernel(FuseArgs a)
{
    __shared__ double s_inv[kFuseFrameThreads][kFuseSim];     // the inverse of link i - 1 of pair i (the thread's pair)
    __shared__ float s_frame[kFuseFrameThreads][kFuseSim];    // the pair's rounded frame
    __shared__ int s_valid[kFuseFrameThreads], s_root[kFuseFrameThreads];
    const int tid = threadIdx.x, lane = tid & 63;
    if (tid < 8) a.out.d_counts[tid] = 0;
    // wavefront 0 walks the chain: lane c < 13 holds element c of the running frame
    const int c = lane < kFuseSim ? lane : 0;
    const int row = fuse_compose_row(c);
    const int y0 = fuse_compose_operand(c, 0), y1 = fuse_compose_operand(c, 1), y2 = fuse_compose_operand(c, 2);
    double Fc = 0.0;                                           // (pair 0 is a root: the first link visited restarts it)
    int root = 0, segs = 0;                                    // the same in every lane of wavefront 0
    for (int base = 0; base < a.k; base += kFuseFrameThreads) {
        const int i = base + tid;
        __syncthreads();
        // ---- every thread: its link's validity and inverse (the loads and the divisions are off the serial chain) ----
        s_valid[tid] = 0;
        if (i < a.k && i > 0) {
            const FusePair &q = a.pairs[i - 1];
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
        }
        __syncthreads();
        // ---- wavefront 0: the composition along the chain, restarted at every cut, rounded once: serial over the links, every
        //      lane computes its own element of the frame; what it needs of the others comes by shuffle ----
        if (tid < 64) {
            const int cnt = min(kFuseFrameThreads, a.k - base);
            for (int l = 0; l < cnt; ++l) {
                if (!__builtin_amdgcn_readfirstlane(s_valid[l])) {     // (the same in every lane: the shuffles below see all of them)
                    Fc = (c == 0 || c == 1 || c == 5 || c == 9) ? 1.0 : 0.0;              // fuse_identity
                    root = base + l;
                    ++segs;
                } else {
                    const double x[3] = { __shfl(Fc, 1 + 3 * row), __shfl(Fc, 2 + 3 * row), __shfl(Fc, 3 + 3 * row) };
                    const double s0 = __shfl(Fc, 0), t0 = __shfl(Fc, 10 + row);
                    const double y[3] = { s_inv[l][y0], s_inv[l][y1], s_inv[l][y2] };
                    Fc = fuse_compose_element(c, s0, x, t0, y);
                }
                if (lane < kFuseSim) s_frame[l][c] = (float)Fc;
                if (lane == 0) s_root[l] = root;
            }
        }
        __syncthreads();
        // ---- every thread: its pair's frame, root and cameras ----
        if (i < a.k) {
            const FusePair &q = a.pairs[i];
            float F[kFuseSim], P2[12], cams[kFuseCams];
#pragma unroll
            for (int e = 0; e < kFuseSim; ++e) { F[e] = s_frame[tid][e]; a.out.d_frames[(size_t)kFuseSim * i + e] = F[e]; }
            a.out.d_root[i] = s_root[tid];
            view_points_pose(q.pose, q.pose_rows, P2);
            fuse_cameras(F, P2, cams);
#pragma unroll
            for (int e = 0; e < kFuseCams; ++e) a.out.d_cams[(size_t)kFuseCams * i + e] = cams[e];
        }
    }
    if (tid == 0) a.out.d_counts[4] = segs;
}

__global__ __launch_bounds__(kFuseBlock)
void fuse_edges_kernel(FuseArgs a)
{
    const int i = fuse_locate(a.pairs, a.k, blockIdx.x);
    if (i >= a.k - 1) return;
    const FusePair p = load_pair(a.pairs, i), next = load_pair(a.pairs, i + 1);
    const int j = ((int)blockIdx.x - p.block0) * kFuseBlock + (int)threadIdx.x;
    if (j >= p.n) return;
    const bool link_ok = fuse_link_ok(p);
    unsigned long long key;
    const int m = fuse_edge(p, next, link_ok, j, key);
    if (m >= 0) atomicMin(&a.keys[(size_t)next.offset + m], key);
}

__global__ __launch_bounds__(kFuseBlock)
void fuse_links_kernel(FuseArgs a)
{
    const int i = fuse_locate(a.pairs, a.k, blockIdx.x);
    const FusePair p = load_pair(a.pairs, i), next = load_pair(a.pairs, min(i + 1, a.k - 1));     // (both before the lanes part)
    const int j = ((int)blockIdx.x - p.block0) * kFuseBlock + (int)threadIdx.x;
    if (j >= p.n) return;
    const size_t g = (size_t)p.offset + j;
    float X[4];
    const bool live = fuse_live(p, j, X);
    a.kind[g] = !live ? kFuseDead : (a.keys[g] == kFuseNoKey ? kFuseHead : kFuseLive);
    int succ = -1;
    if (i < a.k - 1) {
        unsigned long long key;
        const int m = fuse_edge(p, next, fuse_link_ok(p), j, key);
        if (m >= 0 && a.keys[(size_t)next.offset + m] == key) succ = next.offset + m;
    }
    a.succ[g] = succ;
}

__global__ __launch_bounds__(kFuseBlock)
void fuse_count_kernel(FuseArgs a)
{
    __shared__ unsigned long long s_scan[kFuseWaves + 1];
    __shared__ int s_max[kFuseWaves];
    const int i = fuse_locate(a.pairs, a.k, blockIdx.x);
    const int n = a.pairs[i].n, offset = a.pairs[i].offset, block0 = a.pairs[i].block0;
    const int j = ((int)blockIdx.x - block0) * kFuseBlock + (int)threadIdx.x;
    int L = 0;
    if (j < n && a.kind[(size_t)offset + j] == kFuseHead) {
        int g = offset + j;
        do { ++L; g = a.succ[g]; } while (g >= 0);
        a.len[(size_t)offset + j] = L;
    }
    const unsigned long long mine = L ? (((unsigned long long)(L + 1) << 32) | 1ull) : 0ull;
    block_scan<kFuseWaves>(mine, s_scan);
    int views = L ? L + 1 : 0;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) views = max(views, __shfl_xor(views, off));
    if ((threadIdx.x & 63) == 0) s_max[threadIdx.x >> 6] = views;
    __syncthreads();
    if (threadIdx.x == 0) {
        a.blk[blockIdx.x] = s_scan[kFuseWaves];
        int v = 0;
        for (int w = 0; w < kFuseWaves; ++w) v = max(v, s_max[w]);
        a.blkmax[blockIdx.x] = v;                         // (one atomicMax per block on one address cost 50 us at 5320 blocks)
    }
}

__global__ __launch_bounds__(kFuseScanThreads)
void fuse_scan_kernel(FuseArgs a)
{
    __shared__ unsigned long long s_scan[kFuseScanThreads / 64 + 1];
    __shared__ int s_max[kFuseScanThreads / 64];
    unsigned long long carry = 0ull;
    int views = 0;
    for (int base = 0; base < a.blocks; base += kFuseScanThreads) {
        const int b = base + (int)threadIdx.x;
        const unsigned long long v = b < a.blocks ? a.blk[b] : 0ull;
        if (b < a.blocks) views = max(views, a.blkmax[b]);
        const unsigned long long ex = block_scan<kFuseScanThreads / 64>(v, s_scan);
        if (b < a.blocks) a.blk[b] = carry + ex;
        carry += s_scan[kFuseScanThreads / 64];
        __syncthreads();                                  // s_scan is read above and rewritten by the next round
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) views = max(views, __shfl_xor(views, off));
    if ((threadIdx.x & 63) == 0) s_max[threadIdx.x >> 6] = views;
    __syncthreads();
    if (threadIdx.x == 0) {
        const int T = (int)(uint32_t)carry, M = (int)(carry >> 32);
        for (int w = 1; w < kFuseScanThreads / 64; ++w) views = max(views, s_max[w]);
        a.out.d_counts[0] = T;
        a.out.d_counts[1] = M;
        a.out.d_counts[2] = T;                            // REFINED: every track, less what the points kernel keeps
        a.out.d_counts[5] = views;
        a.out.d_track_offset[T] = M;
    }
}

__global__ __launch_bounds__(kFuseBlock)
void fuse_fill_kernel(FuseArgs a)
{
    __shared__ unsigned long long s_scan[kFuseWaves + 1];
    const int i = fuse_locate(a.pairs, a.k, blockIdx.x);
    const int n = a.pairs[i].n, offset = a.pairs[i].offset, block0 = a.pairs[i].block0;
    const int j = ((int)blockIdx.x - block0) * kFuseBlock + (int)threadIdx.x;
    uint8_t kind = kFuseLive;
    int L = 0;
    if (j < n) {
        kind = a.kind[(size_t)offset + j];
        if (kind == kFuseHead) L = a.len[(size_t)offset + j];
    }
    const unsigned long long mine = L ? (((unsigned long long)(L + 1) << 32) | 1ull) : 0ull;
    const unsigned long long at = a.blk[blockIdx.x] + block_scan<kFuseWaves>(mine, s_scan);
    if (j >= n) return;
    if (kind == kFuseDead) a.out.d_track[(size_t)offset + j] = -1;
    if (kind != kFuseHead) return;
    const int t = (int)(uint32_t)at;
    int o = (int)(at >> 32);
    a.out.d_track_offset[t] = o;
    int pair = i, g = offset + j, rec = j;
    for (;;) {
        a.out.d_track[g] = t;
        a.out.d_obs_cam[o] = 2 * pair; a.out.d_obs_record[o] = rec;
        ++o;
        const int nx = a.succ[g];
        if (nx < 0) break;
        ++pair;
        g = nx; rec = nx - a.pairs[pair].offset;
    }
    a.out.d_obs_cam[o] = 2 * pair + 1; a.out.d_obs_record[o] = rec;
}

__global__ __launch_bounds__(kFuseBlock)
void fuse_points_kernel(FuseArgs a)
{
    const int t = blockIdx.x * kFuseBlock + threadIdx.x;
    const int T = a.out.d_counts[0];
    uint8_t flag = 0;
    if (t < T) {
        const int o0 = a.out.d_track_offset[t], count = a.out.d_track_offset[t + 1] - o0;
        const int *cam = a.out.d_obs_cam + o0, *recs = a.out.d_obs_record + o0;
        // ---- the start: the mean of the path's points carried into the root frame, summed in path order ----
        float sum[3] = { 0.0f, 0.0f, 0.0f };
        for (int o = 0; o + 1 < count; ++o) {
            const int pair = cam[o] >> 1;
            const FusePair &q = a.pairs[pair];
            float F[kFuseSim], X[4], Y[3];
#pragma unroll
            for (int c = 0; c < kFuseSim; ++c) F[c] = a.out.d_frames[(size_t)kFuseSim * pair + c];
            fuse_live(q, recs[o], X);
            fuse_carry(F, X, Y);
            sum[0] += Y[0]; sum[1] += Y[1]; sum[2] += Y[2];
        }
        const float L = (float)(count - 1);
        const float start[3] = { sum[0] / L, sum[1] / L, sum[2] / L };
        auto view = [&](int o) {
            const int c = cam[o];
            const FusePair &q = a.pairs[c >> 1];
            return fuse_view(q, a.out.d_cams, c >> 1, c & 1, recs[o]);
        };
        float out[4], err;
        flag = fuse_point(count, view, start, a.p, out, err);
#pragma unroll
        for (int c = 0; c < 4; ++c) a.out.d_points[(size_t)c * a.N + t] = out[c];
        a.out.d_flags[t] = flag;
        if (a.out.d_err) a.out.d_err[t] = err;
    }
    // REFINED starts at T (the scan kernel): only the wavefronts that keep a start point -- few -- touch the two counters
    const unsigned long long kept = __ballot(flag == SFM_FUSE_KEPT);
    if ((threadIdx.x & 63) == 0 && kept) {
        atomicSub(&a.out.d_counts[2], __popcll(kept));
        atomicAdd(&a.out.d_counts[3], __popcll(kept));
    }
}

int fuse_prepare(sfm_ctx *ctx, const FusePair *h_pairs, int num_pairs, const sfm_fuse_params &p, const sfm_fuse_out &out, FuseArgs &a,
                 size_t seam, int **seam_head)
{
    hipStream_t st = ctx->stream;
    JobArray &ja = ctx->fuse_jobs;
    int rc = job_array_reserve(ja, (size_t)num_pairs, sizeof(FusePair), st);
    if (rc != SFM_OK) return rc;
    FusePair *jobs = static_cast<FusePair *>(ja.pinned);
    int N = 0, blocks = 0;
    for (int i = 0; i < num_pairs; ++i) {
        jobs[i] = h_pairs[i];
        jobs[i].offset = N; jobs[i].block0 = blocks;
        N += h_pairs[i].n; blocks += fuse_blocks(h_pairs[i].n);
    }
    a.pairs = static_cast<const FusePair *>(ja.dev);
    a.k = num_pairs; a.N = N; a.blocks = blocks;
    a.p = p;
    a.out = out;
    const size_t need = fuse_work_layout(nullptr, (size_t)N, (size_t)blocks, a, seam, seam_head);
    rc = grow(&ctx->fuse_ws, &ctx->fuse_ws_bytes, need, st);
    if (rc != SFM_OK) return rc;
    fuse_work_layout(ctx->fuse_ws, (size_t)N, (size_t)blocks, a, seam, seam_head);
    return job_array_upload(ja, (size_t)num_pairs, sizeof(FusePair), st);
}

int fuse_enqueue_front(hipStream_t st, const FuseArgs &a)
{
    hipLaunchKernelGGL(fuse_frames_kernel, dim3(1), dim3(kFuseFrameThreads), 0, st, a);
    SFM_HIP_TRY(hipGetLastError());
    if (a.blocks == 0) return SFM_OK;                     // no records anywhere
    SFM_HIP_TRY(hipMemsetAsync(a.keys, 0xFF, (size_t)a.N * sizeof(unsigned long long), st));
    if (a.k > 1) {
        hipLaunchKernelGGL(fuse_edges_kernel, dim3(a.blocks), dim3(kFuseBlock), 0, st, a);
        SFM_HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(fuse_links_kernel, dim3(a.blocks), dim3(kFuseBlock), 0, st, a);
    SFM_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(fuse_count_kernel, dim3(a.blocks), dim3(kFuseBlock), 0, st, a);
    SFM_HIP_TRY(hipGetLastError());
    return SFM_OK;
}

int fuse_enqueue_scan(hipStream_t st, const FuseArgs &a)
{
    hipLaunchKernelGGL(fuse_scan_kernel, dim3(1), dim3(kFuseScanThreads), 0, st, a);
    SFM_HIP_TRY(hipGetLastError());
    return SFM_OK;
}

int launch_fuse_chain(sfm_ctx *ctx, const FusePair *h_pairs, int num_pairs, const sfm_fuse_params &p, const sfm_fuse_out &out)
{
    hipStream_t st = ctx->stream;
    FuseArgs a;
    int rc = fuse_prepare(ctx, h_pairs, num_pairs, p, out, a);
    if (rc == SFM_OK) rc = fuse_enqueue_front(st, a);
    if (rc != SFM_OK) return rc;
    if (a.blocks == 0) {                                  // no records anywhere: no tracks
        SFM_HIP_TRY(hipMemsetAsync(out.d_track_offset, 0, sizeof(int32_t), st));
        return SFM_OK;
    }
    rc = fuse_enqueue_scan(st, a);
    if (rc != SFM_OK) return rc;
    hipLaunchKernelGGL(fuse_fill_kernel, dim3(a.blocks), dim3(kFuseBlock), 0, st, a);
    SFM_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(fuse_points_kernel, dim3((a.N + kFuseBlock - 1) / kFuseBlock), dim3(kFuseBlock), 0, st, a);
    SFM_HIP_TRY(hipGetLastError());
    return SFM_OK;
}

} // namespace sfm
