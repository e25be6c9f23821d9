// fuse_device.hpp -- what the two translation units of the fusion share on the device side: fuse.hip (sfm_fuse_chain) and
// fuse_ring.hip (sfm_fuse_ring).  The kernels' argument block, the classes of a node, how a node block finds its pair, the work
// buffer's layout, and the host functions by which fuse_ring.hip enqueues fuse.hip's kernels (it runs the chain's front stages
// and its scan as they are: the seven kernels stay in fuse.hip).
#pragma once
#include "common.hpp"
#include "device_math.hpp"
#include "block_ops.hpp"
#include "fuse_math.hpp"

namespace sfm {

constexpr int kFuseWaves = kFuseBlock / 64;
constexpr int kFuseScanThreads = 256;     // block counts per round of the scan kernel
constexpr int kFuseFrameThreads = 256;    // links per round of the frames kernel (40 KiB of LDS)

struct FuseArgs {
    const FusePair *pairs;
    int k, N, blocks;                     // pairs, nodes, node blocks
    sfm_fuse_params p;
    unsigned long long *keys;             // N: the winning key of every node's incoming edges
    int *succ;                            // N: the node behind this one on its path, or -1
    int *len;                             // N: pairs on the path that starts here (heads only)
    uint8_t *kind;                        // N: 0 dead, 1 live, 2 head
    unsigned long long *blk;              // blocks: (observations << 32) | heads per block, then its exclusive scan
    int *blkmax;                          // blocks: the longest track (views) that starts in the block
    sfm_fuse_out out;
};

constexpr uint8_t kFuseDead = 0, kFuseLive = 1, kFuseHead = 2;

// the pair of node block b: the last pair whose block0 is <= b (pairs without records own no block)
__device__ __forceinline__ int fuse_locate(const FusePair *__restrict__ pairs, int k, int b)
{
    int lo = 0, hi = k - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (pairs[mid].block0 <= b) lo = mid; else hi = mid - 1;
    }
    return __builtin_amdgcn_readfirstlane(lo);
}

// pair i of the chain where i is the same in every lane of the wavefront: its pointers are global ones in scalar registers.  Where
// every lane has a pair of its own (the frames kernel's lanes, a track's views) the struct is read as it is.
__device__ __forceinline__ FusePair load_pair(const FusePair *__restrict__ pairs, int i)
{
    FusePair p = pairs[i];
    p.points = global_ptr(p.points); p.valid = global_ptr(p.valid); p.X0 = global_ptr(p.X0); p.X1 = global_ptr(p.X1);
    p.K = global_ptr(p.K); p.pose = global_ptr(p.pose);
    p.index = global_ptr(p.index); p.sim = global_ptr(p.sim); p.inlier = global_ptr(p.inlier); p.err = global_ptr(p.err);
    p.report = global_ptr(p.report);
    return p;
}

// the context's work buffer for N nodes in `blocks` node blocks: the arrays of `a` inside it, and behind them `seam` ints for the
// caller (sfm_fuse_ring: the head of every record of pair k - 1); returns its size in bytes
inline size_t fuse_work_layout(void *buffer, size_t N, size_t blocks, FuseArgs &a, size_t seam = 0, int **seam_head = nullptr)
{
    Carver w(buffer);
    a.keys = w.take<unsigned long long>(N, 16);
    a.blk = w.take<unsigned long long>(blocks, 8);
    a.succ = w.take<int>(N, 4);
    a.len = w.take<int>(N, 4);
    a.blkmax = w.take<int>(blocks, 4);
    a.kind = w.take<uint8_t>(N);
    int *s = w.take<int>(seam, 4);
    if (seam_head) *seam_head = s;
    return w.used;
}

// fuse.hip.  fuse_prepare: the pairs into the context's job array (offsets and block numbers filled in), the work buffer grown and
// carved, the upload enqueued: `a` is ready for the launches.  fuse_enqueue_front: the frames kernel and, where there are records,
// the key memset, the edges (more than one pair), the links and the count.  fuse_enqueue_scan: the scan of the block counts.
int fuse_prepare(sfm_ctx *ctx, const FusePair *h_pairs, int num_pairs, const sfm_fuse_params &p, const sfm_fuse_out &out, FuseArgs &a,
                 size_t seam = 0, int **seam_head = nullptr);
int fuse_enqueue_front(hipStream_t st, const FuseArgs &a);
int fuse_enqueue_scan(hipStream_t st, const FuseArgs &a);

} // namespace sfm
