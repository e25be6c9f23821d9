// fuse_ring.hip -- sfm_fuse_ring (gfx950): sfm_fuse_chain's fusion over a closed ring, the tracks that cross the seam joined.
// Arithmetic: fuse_ring_math.hpp on top of fuse_math.hpp and ring_math.hpp (shared with the host build of the CPU tests).
//
// On the context's stream, no host synchronisation.  The front is fuse.hip's own (fuse_enqueue_front: frames, key memset, edges,
// links, count over pairs 0 .. k - 1 and links 0 .. k - 2), which leaves the chain tracks: successors, classes, and `len` in every
// head.  Then
//   fuse_ring_closure_kernel  ONE block: every thread tests links tid, tid + 256, ... (an integer atomicMin in LDS gives the first
//                             invalid one); thread 0 composes the closure from pair k - 1's stored frame, puts it through
//                             ring_drift and writes the report's head; the seam counters are cleared.
//   fuse_ring_edges_kernel    one lane per record of pair k - 1, nothing unless CLOSED: the edge test, the head of its own chain
//                             track by a walk back along the winning keys (counted by the pair index), the eligibility test
//                             against `len` of its target, one 64-bit atomicMin on pair 0's key (all ones since the memset: no
//                             chain edge ends in pair 0).  The head (or -1) is kept per record for the next kernel.
//   fuse_ring_links_kernel    one lane per record of pair k - 1, nothing unless CLOSED: the winner sets its successor, turns its
//                             target from head to live and adds the target's length to its own head's.  A and B are joined at
//                             most once each, heads lie in pairs >= 2 and targets in pair 0: no two lanes meet on an address.
//   fuse_ring_count_kernel    one lane per node: heads and observations per block from `kind` and `len`, no walks.
// fuse.hip's scan (fuse_enqueue_scan), and the ring's variants of the chain's last two kernels:
//   fuse_ring_fill_kernel     fuse_fill_kernel with the walk counted by the stored length and the pair index stepping modulo k.
//   fuse_ring_points_kernel   fuse_points_kernel with the seam flags and the report's seam_refined / seam_kept.
// Where the ring is not CLOSED the two seam kernels leave at once and the rest writes what sfm_fuse_chain writes.
// Integer atomics only; counters take one atomic per wavefront through a ballot.
#include "fuse_device.hpp"
#include "fuse_ring_math.hpp"

namespace sfm {

constexpr int kFuseRingClosureThreads = 256;

struct FuseRingArgs {
    FuseArgs f;
    int *seam_head;                       // n of pair k - 1: the head of the record's chain track where it proposes an eligible join, else -1
    float max_rotation_rad, max_log_scale;
    sfm_fuse_ring_report *report;
};

__global__ __launch_bounds__(kFuseRingClosureThreads)
void fuse_ring_closure_kernel(FuseRingArgs r)
{
    __shared__ int s_first;
    const FuseArgs &a = r.f;
    if (threadIdx.x == 0) s_first = a.k;
    __syncthreads();
    const int mine = fuse_ring_first_invalid(a.pairs, a.k, (int)threadIdx.x, kFuseRingClosureThreads);
    if (mine < a.k) atomicMin(&s_first, mine);
    __syncthreads();
    if (threadIdx.x != 0) return;
    sfm_fuse_ring_report rep;
    rep.status = SFM_RING_OPEN;
    rep.first_invalid = s_first < a.k ? s_first : -1;
    float closure[3] = { 0.0f, 0.0f, 0.0f };
    if (s_first == a.k) {
        float frame[kFuseSim], link[kFuseSim];
#pragma unroll
        for (int q = 0; q < kFuseSim; ++q) {
            frame[q] = a.out.d_frames[(size_t)kFuseSim * (a.k - 1) + q];
            link[q] = a.pairs[a.k - 1].sim[q];
        }
        rep.status = fuse_ring_closure(frame, link, r.max_rotation_rad, r.max_log_scale, closure);
    }
    rep.closure_log_scale = closure[0]; rep.closure_rotation_rad = closure[1]; rep.closure_t = closure[2];
    rep.seam_proposals = 0; rep.seam_ineligible = 0; rep.seam_tracks = 0; rep.seam_refined = 0; rep.seam_kept = 0;
    *r.report = rep;
}

__global__ __launch_bounds__(kFuseBlock)
void fuse_ring_edges_kernel(FuseRingArgs r)
{
    if (r.report->status != SFM_RING_CLOSED) return;
    const FuseArgs &a = r.f;
    const FusePair last = load_pair(a.pairs, a.k - 1), first = load_pair(a.pairs, 0);
    const int j = (int)blockIdx.x * kFuseBlock + (int)threadIdx.x;
    bool proposes = false, ineligible = false;
    if (j < last.n) {
        unsigned long long key;
        int head;
        bool eligible;
        const int m = fuse_ring_proposal(a.pairs, a.k, last, first, fuse_link_ok(last), a.keys, a.len, j, key, head, eligible);
        proposes = m >= 0;
        ineligible = proposes && !eligible;
        if (proposes && eligible) atomicMin(&a.keys[(size_t)first.offset + m], key);
        r.seam_head[j] = proposes && eligible ? head : kFuseRingNoHead;
    }
    const unsigned long long bp = __ballot(proposes), bi = __ballot(ineligible);
    if ((threadIdx.x & 63) == 0) {
        if (bp) atomicAdd(&r.report->seam_proposals, __popcll(bp));
        if (bi) atomicAdd(&r.report->seam_ineligible, __popcll(bi));
    }
}

__global__ __launch_bounds__(kFuseBlock)
void fuse_ring_links_kernel(FuseRingArgs r)
{
    if (r.report->status != SFM_RING_CLOSED) return;
    const FuseArgs &a = r.f;
    const FusePair last = load_pair(a.pairs, a.k - 1), first = load_pair(a.pairs, 0);
    const int j = (int)blockIdx.x * kFuseBlock + (int)threadIdx.x;
    bool won = false;
    if (j < last.n) {
        const int head = r.seam_head[j];
        if (head != kFuseRingNoHead) {                        // an eligible proposal: its index is in range (fuse_edge)
            const size_t target = (size_t)first.offset + last.index[j];
            won = a.keys[target] == fuse_key(last.err[j], j);
            if (won) {
                a.succ[(size_t)last.offset + j] = (int)target;
                a.kind[target] = kFuseLive;
                a.len[head] += a.len[target];
            }
        }
    }
    const unsigned long long bw = __ballot(won);
    if ((threadIdx.x & 63) == 0 && bw) atomicAdd(&r.report->seam_tracks, __popcll(bw));
}

__global__ __launch_bounds__(kFuseBlock)
void fuse_ring_count_kernel(FuseArgs a)
{
    __shared__ unsigned long long s_scan[kFuseWaves + 1];
    __shared__ int s_max[kFuseWaves];
    const int i = fuse_locate(a.pairs, a.k, blockIdx.x);
    const int n = a.pairs[i].n, offset = a.pairs[i].offset, block0 = a.pairs[i].block0;
    const int j = ((int)blockIdx.x - block0) * kFuseBlock + (int)threadIdx.x;
    int L = 0;
    if (j < n && a.kind[(size_t)offset + j] == kFuseHead) L = a.len[(size_t)offset + j];
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
        a.blkmax[blockIdx.x] = v;
    }
}

__global__ __launch_bounds__(kFuseBlock)
void fuse_ring_fill_kernel(FuseArgs a)
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
    for (int s = 0; s < L; ++s) {                             // counted by the stored length: L pairs, L + 1 observations
        a.out.d_track[g] = t;
        a.out.d_obs_cam[o] = 2 * pair; a.out.d_obs_record[o] = rec;
        ++o;
        if (s + 1 == L) break;
        const int nx = a.succ[g];
        // Not reached: `len` of a head is the number of nodes on its path (the count kernel's walk, plus B's for a joined track),
        // so a node with s + 1 < L has a successor.  The test only keeps a damaged work buffer from becoming a store through
        // index -1; the slots `len` promised would then stay unwritten.
        if (nx < 0) break;
        pair = fuse_ring_next(pair, a.k);
        g = nx; rec = nx - a.pairs[pair].offset;
    }
    a.out.d_obs_cam[o] = 2 * pair + 1; a.out.d_obs_record[o] = rec;
}

__global__ __launch_bounds__(kFuseBlock)
void fuse_ring_points_kernel(FuseRingArgs r)
{
    const FuseArgs &a = r.f;
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
        flag = fuse_ring_flag(fuse_point(count, view, start, a.p, out, err), cam[0], cam[count - 1]);
#pragma unroll
        for (int c = 0; c < 4; ++c) a.out.d_points[(size_t)c * a.N + t] = out[c];
        a.out.d_flags[t] = flag;
        if (a.out.d_err) a.out.d_err[t] = err;
    }
    // REFINED starts at T (the scan kernel): only the wavefronts that keep a start point, or hold a seam track, touch the counters
    const unsigned long long kept = __ballot(flag == SFM_FUSE_KEPT || flag == SFM_FUSE_SEAM_KEPT);
    const unsigned long long sr = __ballot(flag == SFM_FUSE_SEAM_REFINED), sk = __ballot(flag == SFM_FUSE_SEAM_KEPT);
    if ((threadIdx.x & 63) == 0) {
        if (kept) {
            atomicSub(&a.out.d_counts[2], __popcll(kept));
            atomicAdd(&a.out.d_counts[3], __popcll(kept));
        }
        if (sr) atomicAdd(&r.report->seam_refined, __popcll(sr));
        if (sk) atomicAdd(&r.report->seam_kept, __popcll(sk));
    }
}

int launch_fuse_ring(sfm_ctx *ctx, const FusePair *h_pairs, int num_pairs, const sfm_fuse_ring_params &p, const sfm_fuse_out &out,
                     sfm_fuse_ring_report *d_report)
{
    hipStream_t st = ctx->stream;
    FuseRingArgs r;
    const int n_last = h_pairs[num_pairs - 1].n;
    int rc = fuse_prepare(ctx, h_pairs, num_pairs, p.fuse, out, r.f, (size_t)n_last, &r.seam_head);
    if (rc == SFM_OK) rc = fuse_enqueue_front(st, r.f);
    if (rc != SFM_OK) return rc;
    r.max_rotation_rad = p.max_closure_rotation_rad; r.max_log_scale = p.max_closure_log_scale;
    r.report = d_report;
    const FuseArgs &a = r.f;
    hipLaunchKernelGGL(fuse_ring_closure_kernel, dim3(1), dim3(kFuseRingClosureThreads), 0, st, r);
    SFM_HIP_TRY(hipGetLastError());
    if (a.blocks == 0) {                                  // no records anywhere: no tracks
        SFM_HIP_TRY(hipMemsetAsync(out.d_track_offset, 0, sizeof(int32_t), st));
        return SFM_OK;
    }
    if (n_last > 0) {
        hipLaunchKernelGGL(fuse_ring_edges_kernel, dim3(fuse_blocks(n_last)), dim3(kFuseBlock), 0, st, r);
        SFM_HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(fuse_ring_links_kernel, dim3(fuse_blocks(n_last)), dim3(kFuseBlock), 0, st, r);
        SFM_HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(fuse_ring_count_kernel, dim3(a.blocks), dim3(kFuseBlock), 0, st, a);
    SFM_HIP_TRY(hipGetLastError());
    rc = fuse_enqueue_scan(st, a);
    if (rc != SFM_OK) return rc;
    hipLaunchKernelGGL(fuse_ring_fill_kernel, dim3(a.blocks), dim3(kFuseBlock), 0, st, a);
    SFM_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(fuse_ring_points_kernel, dim3((a.N + kFuseBlock - 1) / kFuseBlock), dim3(kFuseBlock), 0, st, r);
    SFM_HIP_TRY(hipGetLastError());
    return SFM_OK;
}

} // namespace sfm
