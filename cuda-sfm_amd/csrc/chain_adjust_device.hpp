// chain_adjust_device.hpp -- what chain_adjust.hip (sfm_adjust_chain) and ring_adjust.hip (sfm_adjust_ring) share on the device
// side: the kernels' argument block, the views of a chain's track, the number of tracks and the work buffer's layout.
#pragma once
#include "common.hpp"
#include "device_math.hpp"
#include "block_ops.hpp"
#include "chain_adjust_math.hpp"

namespace sfm {

constexpr int kChainTrackBlock = 256;     // tracks per block of the per-track kernels; threads of the cost kernel
constexpr int kChainCounts = 3 + kChainMaxViews;

struct ChainArgs {
    const FusePair *pairs;
    int k, N, W;
    sfm_adjust_chain_params p;
    const int32_t *root, *track_offset, *obs_cam, *obs_record, *counts;
    const float *cams, *points;
    const uint8_t *flags;
    sfm_adjust_chain_out out;
    // the context's work buffer
    float *state[2];                      // 18 k each: the committed states are state[seg.cur]
    float4 *X[2];                         // N each: the committed points are X[seg.cur]
    ChainSeg *seg;                        // k, entry p meaningful where root[p] == p
    int *head;                            // k + 1: the first track of every head pair, T at the end
    int *hcnt;                            // k x kChainCounts: per head pair used tracks, their observations, over-long tracks, then
                                          // the used observations of its local blocks 0 .. W - 1
    double *part;                         // k x chain_part_values(W): the head pairs' partial bands
    double *pcost;                        // k x 2: the head pairs' cost and squared error
    double *band;                         // k x W x 36
    double *x, *du;                       // 6 k each
    float *dc;                            // 6 k: the camera steps as floats
};

// view o of a track whose observations start at `cam` / `rec`, under the states S
struct ChainTrackViews {
    const ChainArgs &a;
    const float *S;
    const int32_t *cam, *rec;
    __device__ __forceinline__ int block(int o) const { return chain_block(cam[o], a.root[cam[o] >> 1]); }
    __device__ __forceinline__ ChainView operator()(int o) const
    {
        const int c = cam[o], q = c >> 1;
        const FuseView f = fuse_view(a.pairs[q], a.cams, q, c & 1, rec[o]);
        const int b = chain_block(c, a.root[q]);
        ChainView v;
        v.K = f.K; v.x = f.x; v.y = f.y;
        v.kind = b < 0 ? kChainFixed : (a.root[b] == b ? kChainRoot : kChainFree);
        v.S = S + (size_t)kChainState * (b < 0 ? 0 : b);
        return v;
    }
};

// the number of tracks: d_counts[0], never more than the nodes the buffers were sized for
__device__ __forceinline__ int chain_tracks(const ChainArgs &a) { return min(a.counts[0], a.N); }

// the context's work buffer for k pairs, N nodes, tracks of at most W views and a band of band_W block diagonals (the chain: W;
// the folded ring: ring_band_width); returns its size in bytes
inline size_t chain_work_layout(void *buffer, size_t k, size_t N, size_t W, size_t band_W, ChainArgs &a)
{
    Carver w(buffer);
    a.X[0] = w.take<float4>(N, 16);
    a.X[1] = w.take<float4>(N, 16);
    a.part = w.take<double>(k * (size_t)chain_part_values((int)W), 8);
    a.band = w.take<double>(k * band_W * 36, 8);
    a.pcost = w.take<double>(2 * k, 8);
    a.x = w.take<double>(6 * k, 8);
    a.du = w.take<double>(6 * k, 8);
    a.seg = w.take<ChainSeg>(k, 8);
    a.state[0] = w.take<float>(kChainState * k, 4);
    a.state[1] = w.take<float>(kChainState * k, 4);
    a.dc = w.take<float>(6 * k, 4);
    a.head = w.take<int>(k + 1, 4);
    a.hcnt = w.take<int>(kChainCounts * k, 4);
    return w.used;
}

} // namespace sfm
